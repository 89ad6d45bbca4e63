"""Traffic gates on the GPU (copo_gate_*, copo_amd/gates.py) against the restatement of their rules (tests/gate_numpy.py): the hand-made
sequence at 7 and 64 slots with 1 and 32 gates, 0 and 64 sections and 1 and 3 groups, a rollout of the reference's CoPO population, the
launch shapes, forget / reset / scene resets / repeatability / no effect on the simulation, the argument checks, the dict env and the
`.npz` file.  Every comparison is on raw int64 accumulators and exact: the restatement does the side and extent tests in float32 with
the kernel's individually rounded operations."""
import ctypes as C

import numpy as np
import pytest

import gate_cases as gc
import gate_numpy as gn
import interact_cases as ic
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _read(tg):
    return {k: v.cpu().numpy() for k, v in tg.counters().items()}


@pytest.mark.parametrize("N,L,S,G", [(7, 2, 3, 3), (7, 1, 0, 1), (7, 32, 64, 3), (64, 32, 64, 3), (64, 1, 64, 1), (64, 32, 0, 1)])
def test_hand_sequence(N, L, S, G):
    """E = 5: one full workgroup of four scenes and a partial one.  (7, 2, 3, 3) is the case tests/test_gates_cpu.py works out by hand."""
    from copo_amd.gates import TrafficGates
    from copo_amd.sim import VecSim
    kw = dict(map="intersection", num_envs=gc.HAND_E, num_agents=N)
    sim = VecSim(SimConfig(map_kwargs=dict(exit_length=80.0), **kw) if N == 64 else SimConfig(**kw))
    hand = (L, S) == (2, 3)
    g = gc.HAND_GATES if hand else gc.padded_gates(L)
    sections = gc.HAND_SECTIONS if hand else gc.padded_sections(S, L)
    cfg = dict(gc.HAND_KW, groups=G)
    tg = TrafficGates(sim, g, sections, **cfg)
    ref = gn.Recorder(g, sections, gc.HAND_E, N, **cfg)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        for r in range(gc.HAND_RECORDS):
            st, env = gc.hand_record(st0, env0, r)
            _set_state(sim, st, env)
            tg.set_groups(gc.hand_groups(G, r))
            ref.set_groups(gc.hand_groups(G, r))
            tg.record()
            ref.record(st, env)
            gn.compare(_read(tg), ref)
        got = _read(tg)
        print("N %d L %d S %d G %d: forward %d backward %d, sections %d, headway %s" % (N, L, S, G, got["count"][..., 0].sum(), got["count"][..., 1].sum(),
                                                                                     got["sec_count"].sum(), got["headway"].sum((0, 1)).tolist()))
        assert got["count"].sum() > 0 and tg.n_records == gc.HAND_RECORDS
        if hand:
            for k in gn.RAW:
                assert np.array_equal(got[k], gc.HAND_EXPECTED[k]), k
    finally:
        tg.close()
        sim.close()


def _rollout(golden_dir, with_ref=False, with_gates=True, steps=gc.ROLLOUT_STEPS):
    """The rollout case with `for_map` gates.  Returns (counters at the end, counters after record ROLLOUT_MID, the restatement and a
    copy of its accumulators at ROLLOUT_MID, a trace of the step outputs, the final state)."""
    import copy
    import torch
    from copo_amd.gates import TrafficGates
    from copo_amd.sim import VecSim
    cfg = gc.rollout_config()
    sim = VecSim(cfg)
    tg = ref = mid = ref_mid = None
    act = ic.rollout_policy(golden_dir)
    try:
        if with_gates:
            tg = TrafficGates.for_map(sim, inset=gc.ROLLOUT_INSET, **gc.ROLLOUT_KW)
            tg.set_groups(gc.ROLLOUT_GROUPS)
            assert np.array_equal(tg.gates, gc.rollout_gates(cfg)[0])
        if with_ref:
            ref = gn.Recorder(tg.gates, tg.sections, sim.E, sim.N, **gc.ROLLOUT_KW)
            ref.set_groups(gc.ROLLOUT_GROUPS)

        def record():
            if with_gates:
                before = [x.clone() for x in sim.get_state()] if with_ref and tg.n_records == 3 else None
                tg.record()
                if before is not None:       # simulator memory is only read
                    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, sim.get_state()))
            if with_ref:
                ref.record(*_np_state(sim))
        out = sim.reset()
        record()
        trace = []
        for t in range(steps):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            record()
            trace.append(int(out["flags"].to(torch.int64).sum()) * 31 + int(out["rew"].view(torch.int32).to(torch.int64).sum()))
            if with_gates and t + 1 == gc.ROLLOUT_MID:
                mid, ref_mid = _read(tg), copy.deepcopy(ref)
        final = [x.cpu().numpy().view(np.int32).copy() for x in sim.get_state()]
        return (_read(tg) if with_gates else None), mid, ref, ref_mid, trace, final
    finally:
        if tg is not None:
            tg.close()
        sim.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    return _rollout(golden_dir, with_ref=True)


def test_rollout_against_the_restatement(rollout):
    got, mid, ref, ref_mid, _, _ = rollout
    gn.compare(mid, ref_mid)
    gn.compare(got, ref)
    gc.check_invariants(ref)
    gc.check_premises(ref)
    print("forward %s backward %s; sections %s; headway %s; most crossings of a gate in a scene-record %d"
          % (got["count"][:, :, 0].sum(0).tolist(), got["count"][:, :, 1].sum(0).tolist(), got["sec_count"].sum(0).tolist(),
             got["headway"].sum((0, 1)).tolist(), ref.max_crossings_of_a_gate_in_a_scene_record))
    assert (got["count"][:, :, 0].sum(0) >= 1).all() and got["sec_count"].sum() >= 1 and got["headway"][:, :, 1:].sum() >= 1
    assert got["scene_records"].tolist() == [3 * (gc.ROLLOUT_STEPS + 1), 2 * (gc.ROLLOUT_STEPS + 1)]


def test_two_identical_runs_give_identical_bits_and_recording_does_not_perturb(golden_dir, rollout):
    short = 60
    a = _rollout(golden_dir, steps=short)
    b = _rollout(golden_dir, steps=short)
    plain = _rollout(golden_dir, with_gates=False, steps=short)
    assert all(np.array_equal(a[0][k], b[0][k]) for k in gn.RAW) and a[0]["count"].sum() > 0
    assert a[4] == b[4] == plain[4] == rollout[4][:short] and all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[5], b[5], plain[5]))


@pytest.mark.parametrize("E", [1, 4, 5, 1030, 4100])
def test_launch_shapes(E):
    """The same seeded state in every scene count: one partial workgroup, one full, one and a bit, 258 workgroups, and (4 100: 1 025 batches
    of four scenes for at most 1 024 workgroups) a workgroup that walks two batches.  Scene e holds scene e % 5 of the hand sequence at 64 slots."""
    import torch
    from copo_amd.gates import TrafficGates
    from copo_amd.sim import VecSim
    N, G = 64, 3
    sim = VecSim(SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=E, num_agents=N))
    g, sections = gc.padded_gates(8), gc.padded_sections(6, 8)
    tg = TrafficGates(sim, g, sections, **dict(gc.HAND_KW, groups=G))
    ref = gn.Recorder(g, sections, gc.HAND_E, N, **dict(gc.HAND_KW, groups=1))
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        base_st, base_env = np.zeros((16, gc.HAND_E, N), np.float32), np.zeros((gc.HAND_E, 4), np.int32)
        idx = np.arange(E) % gc.HAND_E
        groups = (np.arange(E) % (G + 1)).astype(np.int32)                # group 3 does not exist
        tg.set_groups(groups)
        per_scene = []
        for r in range(4):
            hs, he = gc.hand_record(base_st, base_env, r)
            st, env = st0.copy(), env0.copy()
            st[:4], st[13:15], env[:, 1] = hs[:4][:, idx], hs[13:15][:, idx], he[idx, 1]
            _set_state(sim, st, env)
            tg.record()
            ref.record(hs, he)
        # the restatement ran the five distinct scenes once, all in one group; scene e of the device run adds scene e % 5's part to its group
        solo = []
        for k in range(gc.HAND_E):
            one = gn.Recorder(g, sections, gc.HAND_E, N, **dict(gc.HAND_KW, groups=1))
            one.set_groups([0 if j == k else -1 for j in range(gc.HAND_E)])
            for r in range(4):
                one.record(*gc.hand_record(base_st, base_env, r))
            solo.append(one)
        got = _read(tg)
        for key in gn.RAW:
            want = np.zeros_like(got[key])
            for e in range(E):
                if groups[e] < G:
                    want[groups[e]] += getattr(solo[idx[e]], key)[0]
            assert np.array_equal(got[key], want), (E, key)
        assert got["count"].sum() > 0 and sum(getattr(s, "count").sum() for s in solo) == ref.count.sum()
    finally:
        tg.close()
        sim.close()


def test_scene_reset_inside_a_rollout_produces_no_crossing(golden_dir):
    """Intersection, 3 scenes x 10 slots, agents end after 55 steps at the latest: the scenes are reset inside 120 steps.  One group per
    scene: in the record after a scene's episode word changed, that scene's counts do not move, although every slot holds a new agent far
    from where the slot was."""
    import torch
    from copo_amd.gates import TrafficGates
    from copo_amd.sim import VecSim
    cfg = ic.rollout_config()
    sim = VecSim(cfg)
    tg = TrafficGates.for_map(sim, inset=30.0, groups=3)
    ref = gn.Recorder(tg.gates, tg.sections, sim.E, sim.N, groups=3)
    act = ic.rollout_policy(golden_dir)
    try:
        tg.set_groups([0, 1, 2])
        ref.set_groups([0, 1, 2])
        out = sim.reset()
        tg.record()
        ref.record(*_np_state(sim))
        resets = 0
        for t in range(ic.ROLLOUT_STEPS):
            ep0 = _np_state(sim)[1][:, 1].copy()
            before = _read(tg)
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            tg.record()
            st, env = _np_state(sim)
            ref.record(st, env)
            after = _read(tg)
            for e in np.nonzero(env[:, 1] != ep0)[0]:
                resets += 1
                assert np.array_equal(before["count"][e], after["count"][e]) and np.array_equal(before["sec_count"][e], after["sec_count"][e])
                assert after["scene_records"][e] == before["scene_records"][e] + 1
        gn.compare(_read(tg), ref)
        assert resets >= 3 and ref.count.sum() > 0
    finally:
        tg.close()
        sim.close()


def test_forget_reset_close_and_argument_errors_leave_everything_usable():
    import torch
    from copo_amd import _capi
    from copo_amd.gates import TrafficGates
    from copo_amd.sim import VecSim
    lib = _capi.lib
    sim = VecSim(SimConfig(map="intersection", num_envs=gc.HAND_E, num_agents=7))
    h = C.c_void_p()
    g2, sec = np.ascontiguousarray(gc.HAND_GATES), np.array(gc.HAND_SECTIONS, np.int32)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        good = (2, 3, 3, 2, 3, 3, 2, 2)
        for i, v in ((0, 0), (0, 33), (1, -1), (1, 65), (2, 0), (2, 65), (3, 0), (3, 257), (4, 0), (5, 0), (5, 65), (6, 0), (6, 65), (7, 0)):
            bad = list(good)
            bad[i] = v
            if i == 0 and v == 33:
                gates_, sec_ = gc.padded_gates(33), sec
            else:
                gates_, sec_ = g2, (np.zeros((65, 2), np.int32) if (i, v) == (1, 65) else sec)
            cfg = _capi.GateCfg(*bad)
            assert lib.copo_gate_create(sim._h, C.byref(cfg), gates_.ctypes.data, sec_.ctypes.data, C.byref(h)) == -2, bad
            assert b"copo_gate_create" in lib.copo_last_error()
        cfg = _capi.GateCfg(*good)
        for bad_sec in ([(0, 2), (0, 0), (0, 0)], [(0, 0), (-1, 0), (0, 0)]):
            s_ = np.array(bad_sec, np.int32)
            assert lib.copo_gate_create(sim._h, C.byref(cfg), g2.ctypes.data, s_.ctypes.data, C.byref(h)) == -2
        for bad_gate in ((100.0, 50.0, 100.0, 50.0), (float("nan"), 50.0, 100.0, 40.0), (100.0, 50.0, float("inf"), 40.0)):
            g_ = g2.copy()
            g_[1] = bad_gate
            assert lib.copo_gate_create(sim._h, C.byref(cfg), g_.ctypes.data, sec.ctypes.data, C.byref(h)) == -5, bad_gate
        assert lib.copo_gate_create(sim._h, None, g2.ctypes.data, sec.ctypes.data, C.byref(h)) == -1
        assert lib.copo_gate_create(sim._h, C.byref(cfg), None, sec.ctypes.data, C.byref(h)) == -1
        assert lib.copo_gate_create(sim._h, C.byref(cfg), g2.ctypes.data, None, C.byref(h)) == -1       # S > 0 needs the sections
        with pytest.raises(_capi.CopoError):
            TrafficGates(sim, gc.padded_gates(33))
        tg = TrafficGates(sim, gc.HAND_GATES, gc.HAND_SECTIONS, **gc.HAND_KW)
        stream = _capi.current_stream()
        tg.set_groups(gc.hand_groups(3, 0))

        def put(r):
            _set_state(sim, *gc.hand_record(st0, env0, r))
        put(0)
        tg.record()
        before = _read(tg)
        assert lib.copo_gate_set_groups(tg._h, None, stream) == -1 and lib.copo_gate_read(tg._h, None, None, stream) == -1
        with pytest.raises(ValueError):
            tg.set_groups([0, 1])
        assert all(np.array_equal(before[k], v) for k, v in _read(tg).items())            # a refused call launched nothing
        # forget() after set_state fires nothing; without it record 1 counts the hand sequence's crossings
        put(1)
        tg.forget()
        tg.record()
        got = _read(tg)
        assert got["count"].sum() == 0 and got["scene_records"].tolist() == [4, 2, 2] and tg.n_records == 2
        put(2)
        tg.record()
        assert _read(tg)["count"][1:, 0, 1].tolist() == [1, 1] and _read(tg)["count"].sum() == 2
        n = C.c_int32(-1)
        assert lib.copo_gate_read(tg._h, None, C.byref(n), stream) == 0 and n.value == 3
        tg.reset()
        assert all((v == 0).all() for v in _read(tg).values()) and tg.n_records == 0
        # reset forgot the memory as well and the groups stayed: the whole sequence again gives the hand values
        for r in range(gc.HAND_RECORDS):
            put(r)
            tg.set_groups(gc.hand_groups(3, r))
            tg.record()
        got = _read(tg)
        assert all(np.array_equal(got[k], gc.HAND_EXPECTED[k]) for k in gn.RAW)
        data = tg.read()
        assert data["flow_per_hour"].shape == (3, 2, 2) and data["meta"]["sections"] == [list(s) for s in gc.HAND_SECTIONS]
        assert data["mean_travel_s"][0, 0] == 8 / 3 * sim.cfg.dt and data["density"][0] == 7.0
        tg.close()
        tg.close()                                                       # closing twice is harmless
        out = sim.step(torch.zeros(gc.HAND_E, sim.N, 2, device="cuda"))
        assert torch.isfinite(out["rew"]).all()
    finally:
        sim.close()


def test_dict_env_key_and_file(tmp_path):
    """The dict env with `traffic_gates` on for 20 steps at 2 scenes against a hand-driven `TrafficGates` on the same seeds."""
    import torch
    from copo_amd.gates import TrafficGates, load
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    kw = dict(inset=30.0, bins=(4, 8))
    env = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2, traffic_gates=kw))
    other = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2))
    tg = TrafficGates.for_map(other.sim, **kw)
    try:
        act = torch.zeros(2, env.sim.N, 2, device="cuda")
        act[..., 1] = torch.linspace(0.3, 1.0, env.sim.N, device="cuda")
        env.vec_reset()
        other.vec_reset()
        tg.forget()
        tg.record()
        for _ in range(20):
            env.vec_step(act)
            other.vec_step(act)
            tg.record()
        mine = env.traffic_gates()
        a, b = _read(mine), _read(tg)
        assert mine.n_records == 21 and all(np.array_equal(a[k], b[k]) for k in gn.RAW)
        assert a["count"][:, :, 0].sum() > 0 and a["scene_records"].tolist() == [42]
        path = mine.save(str(tmp_path / "gates.npz"))
        back = load(path)
        assert all(np.array_equal(back[k], a[k]) for k in gn.RAW) and back["meta"]["bins"] == [4, 8] and len(back["meta"]["gates"]) == mine.L
        assert np.array_equal(back["flow_per_hour"], mine.read()["flow_per_hour"], equal_nan=True)
    finally:
        tg.close()
        other.close()
        env.close()
