"""Traffic field maps on the GPU (copo_field_*, copo_amd/fields.py) against the restatement of their rules (tests/field_numpy.py): the hand
cases, random poses at the full slot count and at odd sizes on grids that are no multiple of the tile, a rollout of the reference's CoPO
population with terminations, slot reuse and scene resets at two cell sizes and strides; bit-for-bit repeatability, no effect on the
simulation, forget / reset / close, the dict env and `vis --heatmap`, and the C entry points' argument checks.

Comparisons (field_numpy.compare).  Every accumulator is an integer.  Visits, speed_q, the three event layers, critical and scene_records
are EQUAL: centre cells and speed_q are restated in float32 with the kernel's individually rounded operations.  Occupancy and wreck lie
within [lo, hi] per cell, lo counting the (body, cell) pairs whose cell centre is more than 1e-3 m inside the rectangle and hi also those
within 1e-3 m of an edge (an fp32 ulp is 3e-5 m below 300 m); at most 1 % of a case's pairs may be of the second kind
(tests/test_fields_cpu.py measures 0.24 % on the rollout).  vx_q / vy_q are within one quantisation step per sample of the float64 sums:
|d| <= visits per cell (the fp32 sincos error is ~1e-6 x 22 m/s x 256, far below a step)."""
import ctypes as C
import os

import numpy as np
import pytest

import field_cases as fc
import field_numpy as fn
import interact_cases as ic
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _read(fm):
    m, r = fm.maps()
    return m.cpu().numpy(), r.cpu().numpy()


def test_hand_set_states():
    """Every hand case of tests/test_fields_cpu.py in a 2 x 5 simulator: the cells counted by hand, on the GPU."""
    from copo_amd.fields import FieldMaps
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="intersection", num_envs=2, num_agents=5)
    sim = VecSim(cfg)
    fm = FieldMaps(sim, **fc.HAND_GRID)
    grid = fn.Grid(**fc.HAND_GRID)
    try:
        sim.reset()
        st0, env = _np_state(sim)
        for case in fc.HAND_CASES:
            _set_state(sim, fc.hand_state(st0, case), env)
            fm.reset()
            fm.record()
            fm.record()
            maps, rec = _read(fm)
            want = fc.expected_maps(case, grid, scale=2)
            assert rec.tolist() == [4], (case, rec)                      # two scenes, two records
            assert np.array_equal(maps[0], want), (case, {fn.LAYERS[k]: (np.argwhere(maps[0, k] != want[k])[:6].tolist()) for k in range(10)})
    finally:
        fm.close()
        sim.close()


@pytest.mark.parametrize("N", [64, 7])
def test_random_poses(N):
    """E = 5 (no multiple of a scene block), G = 3 with one scene switched off and one naming a group that does not exist; a 40 x 24
    grid (neither side a multiple of the 32-cell tile) and a 33 x 65 one (tile borders crossed both ways; 0.5 m cells at 7 slots)."""
    from copo_amd.fields import FieldMaps
    from copo_amd.sim import VecSim
    if N == 64:
        cfg, seeds = SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=5, num_agents=64), ic.RANDOM_SEEDS_64
    else:
        cfg, seeds = SimConfig(map="intersection", num_envs=5, num_agents=7), ic.RANDOM_SEEDS_7
    sim = VecSim(cfg)
    fms = [FieldMaps(sim, groups=3, **gk) for gk in fc.RANDOM_GRIDS[N]]
    try:
        sim.reset()
        st0, env = _np_state(sim)
        for seed, aligned in seeds:
            st = ic.random_state(st0, seed, aligned)
            _set_state(sim, st, env)
            for fm, gk in zip(fms, fc.RANDOM_GRIDS[N]):
                fm.reset()
                fm.set_groups(fc.RANDOM_GROUPS)
                fm.record()
                ref = fn.Recorder(fn.Grid(**gk), 5, N, cfg.veh_half_len, cfg.veh_half_wid, groups=3)
                ref.set_groups(fc.RANDOM_GROUPS)
                ref.record(st)
                maps, rec = _read(fm)
                worst = fn.compare(maps, rec, ref)
                print("N %d seed %d%s grid %dx%d: pairs %d sure / %d ambiguous, visits %d, largest velocity deviation %d steps"
                      % (N, seed, " aligned" if aligned else "", gk["W"], gk["H"], ref.sure_pairs, ref.ambiguous_pairs, int(maps[:, 2].sum()), worst))
                assert ref.ambiguous_pairs <= 0.01 * ref.sure_pairs and rec.tolist() == [1, 1, 1]
                assert maps[:, 0].sum() > 0 and maps[:, 1].sum() > 0 and maps[:, 2].sum() > 0
    finally:
        for fm in fms:
            fm.close()
        sim.close()


def _rollout(golden_dir, with_refs=False, with_fields=True):
    """120 steps of the rollout case with both recorders of field_cases.rollout_grids attached (and the meter, whose ttc feeds the
    critical layer).  Returns ([(maps, scene_records)] per recorder, refs, the last step's outputs as bits, the final state)."""
    import torch
    from copo_amd.fields import FieldMaps
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    cfg = fc.rollout_config()
    sim = VecSim(cfg)
    meter = InteractionMeter(sim) if with_fields else None
    fms, refs = [], []
    act = ic.rollout_policy(golden_dir)
    try:
        if with_fields:
            for gk, groups, stride in fc.rollout_grids(cfg):
                fm = FieldMaps(sim, groups=groups, ttc_below=fc.TTC_BELOW, stride=stride, **gk)
                groups_of = fc.ROLLOUT_GROUPS if groups > 1 else np.zeros(sim.E, np.int32)
                fm.set_groups(groups_of)
                fms.append(fm)
                if with_refs:
                    refs.append(fn.Recorder(fn.Grid(**gk), sim.E, sim.N, cfg.veh_half_len, cfg.veh_half_wid, groups=groups, ttc_below=fc.TTC_BELOW,
                                            stride=stride))
                    refs[-1].set_groups(groups_of)

        def record(flags):
            if not with_fields:
                return
            _, ttc = meter.record()
            for fm in fms:
                fm.record(flags=flags, ttc=ttc)
            if with_refs:
                st, f, t = sim.get_state()[0].cpu().numpy(), None if flags is None else flags.cpu().numpy(), ttc.cpu().numpy()
                for r in refs:
                    r.record(st, f, t)
        out = sim.reset()
        record(None)
        trace = []
        for t in range(fc.ROLLOUT_STEPS):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            record(out["flags"])
            trace.append(int(out["flags"].to(torch.int64).sum()) * 31 + int(out["rew"].view(torch.int32).to(torch.int64).sum()))
        final = [x.cpu().numpy().view(np.int32).copy() for x in sim.get_state()]
        return [_read(fm) for fm in fms], refs, trace, final
    finally:
        for fm in fms:
            fm.close()
        if meter is not None:
            meter.close()
        sim.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    return _rollout(golden_dir, with_refs=True)


def test_rollout_against_the_restatement(rollout):
    got, refs, _, _ = rollout
    for (maps, rec), ref in zip(got, refs):
        worst = fn.compare(maps, rec, ref)
        print("rollout %.1f m cells, stride %d, %d groups: pairs %d sure / %d ambiguous (%.2f %%); visits %d, crash %d, out %d, arrive %d, critical %d; "
              "scene_records %s; largest velocity deviation %d steps" % (float(ref.grid.cell), ref.stride, ref.G, ref.sure_pairs, ref.ambiguous_pairs,
                                                                       100.0 * ref.ambiguous_pairs / ref.sure_pairs, int(maps[:, 2].sum()), int(maps[:, 6].sum()),
                                                                       int(maps[:, 7].sum()), int(maps[:, 8].sum()), int(maps[:, 9].sum()), rec.tolist(), worst))
        assert ref.ambiguous_pairs <= 0.01 * ref.sure_pairs
        assert maps[:, 6].sum() > 0 and maps[:, 1].sum() > 0 and maps[:, 9].sum() > 0         # crashes, wrecks and critical steps occurred
    # every record accumulates at stride 1 (six scenes each), every third at stride 3 (groups 0, 1, 2 hold 2, 2, 1 scenes)
    assert got[0][1].tolist() == [6 * 121] and got[1][1].tolist() == [2 * 41, 2 * 41, 41]
    # events count in every record whatever the stride: the 0.5 m recorder holds the events of its five routed scenes
    assert 0 < got[1][0][:, 6].sum() <= got[0][0][:, 6].sum()


def test_two_identical_runs_give_identical_bits(golden_dir, rollout):
    again, _, trace, final = _rollout(golden_dir)
    for (ma, ra), (mb, rb) in zip(rollout[0], again):
        assert np.array_equal(ma, mb) and np.array_equal(ra, rb)
    assert trace == rollout[2] and all(np.array_equal(a, b) for a, b in zip(final, rollout[3]))


def test_recording_does_not_perturb_the_simulation(golden_dir, rollout):
    _, _, trace, final = _rollout(golden_dir, with_fields=False)
    assert trace == rollout[2] and all(np.array_equal(a, b) for a, b in zip(final, rollout[3]))


def test_forget_reset_close_and_argument_errors_leave_everything_usable():
    import torch
    from copo_amd import _capi
    from copo_amd.fields import FieldMaps
    from copo_amd.sim import VecSim
    lib = _capi.lib
    sim = VecSim(SimConfig(map="intersection", num_envs=4))
    act = torch.zeros(4, sim.N, 2, device="cuda")
    act[..., 1] = 0.5
    h = C.c_void_p()
    try:
        sim.reset()
        for bad in ((0.0, 0.0, 1.0, 0, 8, 1, 0.0), (0.0, 0.0, 1.0, 8, 1025, 1, 0.0), (0.0, 0.0, 1.0, 8, 8, 0, 0.0), (0.0, 0.0, 1.0, 8, 8, 65, 0.0),
                    (0.0, 0.0, 0.0, 8, 8, 1, 0.0), (0.0, 0.0, -1.0, 8, 8, 1, 0.0), (0.0, 0.0, float("nan"), 8, 8, 1, 0.0)):
            cfg = _capi.FieldCfg(*bad)
            assert lib.copo_field_create(sim._h, C.byref(cfg), C.byref(h)) == -2 and b"copo_field_create" in lib.copo_last_error(), bad
        for bad in ((float("inf"), 0.0, 1.0, 8, 8, 1, 0.0), (0.0, 0.0, 1.0, 8, 8, 1, -1.0), (0.0, 0.0, 1.0, 8, 8, 1, float("nan"))):
            cfg = _capi.FieldCfg(*bad)
            assert lib.copo_field_create(sim._h, C.byref(cfg), C.byref(h)) == -5, bad
        good = _capi.FieldCfg(0.0, 0.0, 1.0, 8, 8, 1, 0.0)
        assert lib.copo_field_create(sim._h, None, C.byref(h)) == -1 and lib.copo_field_create(sim._h, C.byref(good), None) == -1
        with pytest.raises(_capi.CopoError):
            FieldMaps(sim, 0.0, 0.0, 2000, 8)
        with pytest.raises(ValueError):
            FieldMaps(sim, 0.0, 0.0, 8, 8, stride=0)
        fm = FieldMaps.for_map(sim, cell=1.0, ttc_below=1.0)
        with pytest.raises(ValueError):
            fm.record()                                                  # the critical layer needs the meter's ttc
        fm.close()
        fm = FieldMaps.for_map(sim, cell=2.0, groups=2)
        st = _capi.current_stream()
        fm.record()
        flags = torch.full((4, sim.N), 1 | 2 | 8, dtype=torch.uint8, device="cuda")          # every slot: DONE and CRASH
        before = _read(fm)
        assert lib.copo_field_record(fm._h, flags.data_ptr(), None, 2, st) == -2 and b"copo_field_record" in lib.copo_last_error()
        assert lib.copo_field_set_groups(fm._h, None, st) == -1 and lib.copo_field_read(fm._h, None, None, st) == -1
        with pytest.raises(ValueError):
            fm.set_groups([0, 1])
        with pytest.raises(ValueError):
            fm.record(flags=flags[:2])
        after = _read(fm)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])   # a refused call launched nothing
        alive = int(before[0][0, 2].sum())
        assert alive > 0 and before[1].tolist() == [4, 0] and before[0][1].sum() == 0
        # forget: the flags find no remembered cell; without it every ALIVE slot of the record before counts once
        fm.forget()
        fm.record(flags=flags)
        assert _read(fm)[0][:, 6].sum() == 0
        fm.record(flags=flags)
        assert _read(fm)[0][0, 6].sum() == alive
        # either output of read may be left out
        only = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        assert lib.copo_field_read(fm._h, None, only.data_ptr(), st) == 0 and only.cpu().tolist() == [12, 0]
        fm.set_groups(torch.tensor([1, 1, -1, 7], dtype=torch.int32, device="cuda"))
        fm.record()
        assert _read(fm)[1].tolist() == [12, 2]
        fm.reset()
        m0, r0 = _read(fm)
        assert (m0 == 0).all() and (r0 == 0).all() and fm.n_records == 0
        fm.record(flags=flags)                                           # reset forgot the cells as well; the groups stayed
        m1, r1 = _read(fm)
        assert m1[:, 6].sum() == 0 and r1.tolist() == [0, 2] and m1[0].sum() == 0 and m1[1, 2].sum() > 0
        data = fm.read()
        assert data["mean_speed"].shape == (2, fm.H, fm.W) and data["meta"]["groups"] == 2 and np.isnan(data["occupancy_frac"][0]).all()
        fm.close()
        fm.close()                                                       # closing twice is harmless
        out = sim.step(act)
        assert torch.isfinite(out["rew"]).all()
        again = FieldMaps.for_map(sim)
        again.record(flags=out["flags"])
        assert _read(again)[1].tolist() == [4]
        again.close()
    finally:
        sim.close()


def test_dict_env_key_and_vis_heatmap(tmp_path, golden_dir):
    from copo_amd import vis
    from copo_amd.fields import load
    from copo_amd.render import read_ppm
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    with pytest.raises(ValueError):
        MultiAgentIntersectionEnv(dict(num_agents=10, field_maps=dict(ttc_below=1.5)))
    env = MultiAgentIntersectionEnv(dict(num_agents=10, horizon=30, delay_done=2, interaction_metrics=True, field_maps=dict(cell=1.0, ttc_below=1.5)))
    try:
        o = env.reset()
        ended = 0
        for _ in range(40):
            o, r, d, i = env.step({k: np.array([0.0, 0.3 + 0.07 * ((int(k[5:]) * 7) % 10)]) for k in o})
            ended += sum(1 for k, v in d.items() if k != "__all__" and v and (i[k]["crash"] or i[k]["out_of_road"] or i[k]["arrive_dest"]))
            if d["__all__"]:
                o = env.reset()
        fm = env.field_maps()
        data = fm.read()
        assert fm.n_records >= 41 and data["scene_records"].tolist() == [fm.n_records]
        assert data["visits"].sum() > 0 and np.nanmax(data["mean_speed"]) > 1.0
        assert data["crash"].sum() + data["out"].sum() + data["arrive"].sum() >= ended
        path = fm.save(str(tmp_path / "maps.npz"))
        back = load(path)
        assert np.array_equal(back["occupancy"], data["occupancy"]) and back["meta"]["W"] == fm.W
    finally:
        env.close()
    out = str(tmp_path / "frames")
    vis.main(["--env", "inter", "--algo", "copo", "--weights", os.path.join(golden_dir, "eval_policy_function.npz"), "--key", "copo_inter",
              "--steps", "12", "--out", out, "--size", "128", "128", "--heatmap", "occupancy"])
    img = read_ppm(os.path.join(out, "heatmap_occupancy.ppm"))
    plain = read_ppm(os.path.join(out, "frame_00011.ppm"))
    assert img.shape == (128, 128, 3) and (img != plain).any()
