"""Interaction meter on the GPU (copo_interact_*, copo_amd/interact.py) against the float64 restatement of its rules
(tests/interact_numpy.py): hand-set scenes, random poses at the full slot count and at odd sizes, a rollout of the reference's CoPO
population with terminations, slot reuse and scene resets; bit-for-bit repeatability, no effect on the simulation, the dict env and
`RecorderEnv` surface, reset / close, and the C entry points' argument checks.

Tolerances.  The gap is compared absolutely, the TTC as |d| <= TTC_TOL (1 + ttc), on every sample the restatement does not mark
ambiguous (at most 1 % of a case's ALIVE samples may be marked; tests/test_interact_cpu.py checks the chosen seeds on the CPU).
Largest deviation of the kernel's arithmetic from the restatement over the cases of this file: gap 2.93e-5 m (the 200 m gaps of the
hand-set scenes, two ulps there; 1.5e-6 m on the random poses), TTC 3.4e-7 (relative to 1 + ttc); each tolerance is 4 x that, for
fp32 re-association across compiler versions: 1.172e-4 m and 1.36e-6.  The figures come from the kernel's pair arithmetic compiled
for the host (the same individually rounded fp32 operations and fused multiply-adds, -ffp-contract=off); every comparison prints what
it meets on the GPU."""
import ctypes as C

import numpy as np
import pytest

import interact_cases as ic
import interact_numpy as im
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu

MEASURED_GAP, MEASURED_TTC = 2.93e-5, 3.4e-7
GAP_TOL, TTC_TOL = 4 * MEASURED_GAP, 4 * MEASURED_TTC
SEEN = dict(gap=0.0, ttc=0.0)          # largest deviations met so far in this session (printed by every comparison)


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _compare(tag, gap, ttc, ref_gap, ref_ttc, amb, alive):
    """GPU outputs of one record against the restatement's; returns (ALIVE samples, ambiguous ones)"""
    g, t = gap.cpu().numpy().astype(np.float64), ttc.cpu().numpy().astype(np.float64)
    assert np.isposinf(g[~alive]).all() and np.isposinf(t[~alive]).all(), tag            # slots that do not drive own nothing
    assert (np.isinf(g) == np.isinf(ref_gap)).all(), (tag, np.argwhere(np.isinf(g) != np.isinf(ref_gap))[:5].tolist())
    fin = np.isfinite(ref_gap)
    dg = float(np.abs(g[fin] - ref_gap[fin]).max()) if fin.any() else 0.0
    sure = alive & ~amb
    bad_inf = sure & (np.isinf(t) != np.isinf(ref_ttc))
    fin_t = sure & np.isfinite(ref_ttc) & np.isfinite(t)
    dt = float((np.abs(t[fin_t] - ref_ttc[fin_t]) / (1.0 + ref_ttc[fin_t])).max()) if fin_t.any() else 0.0
    SEEN["gap"], SEEN["ttc"] = max(SEEN["gap"], dg), max(SEEN["ttc"], dt)
    print("%s: gap deviation %.3e m, TTC deviation %.3e (x (1 + ttc)); session maxima %.3e / %.3e; ambiguous %d of %d"
          % (tag, dg, dt, SEEN["gap"], SEEN["ttc"], int((amb & alive).sum()), int(alive.sum())))
    assert not bad_inf.any(), (tag, np.argwhere(bad_inf)[:5].tolist(), t[bad_inf][:5].tolist(), ref_ttc[bad_inf][:5].tolist())
    assert dg < 1e-3, (tag, dg)                     # beyond a millimetre on coordinates below 300 m is a bug, whatever the tolerance
    assert dg <= GAP_TOL and dt <= TTC_TOL, (tag, dg, GAP_TOL, dt, TTC_TOL)
    return int(alive.sum()), int((amb & alive).sum())


def _check_totals(tag, meter, tracker, flush):
    counts, sums = (x.cpu().numpy() for x in meter.totals(flush_open=flush))
    ref = tracker.totals(flush_open=flush)
    print(tag, "flush" if flush else "closed", "counts", counts.tolist(), "restatement", ref["counts"].tolist(), "sums", sums.tolist(),
          "restatement", ref["sums"].tolist(), "slack", ref["slack"].tolist())
    assert (counts >= ref["lo"]).all() and (counts <= ref["hi"]).all(), (tag, counts.tolist(), ref["lo"].tolist(), ref["hi"].tolist())
    fin = np.isfinite(ref["sums"])           # (+inf: an agent that never had a partner -- the same on both sides)
    assert (np.isposinf(sums) == ~fin).all()
    assert (np.abs(sums - ref["sums"])[fin] <= (1e-6 * np.abs(ref["sums"]) + ref["slack"])[fin]).all(), (tag, sums.tolist(), ref["sums"].tolist(), ref["slack"].tolist())
    return counts, sums


def test_hand_set_states():
    """Every hand case of tests/test_interact_cpu.py in a 2 x 5 simulator, with EMPTY slots lying on top of the bodies."""
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="intersection", num_envs=2, num_agents=5)
    sim = VecSim(cfg)
    meter = InteractionMeter(sim)
    P = im.Params.of(cfg)
    try:
        sim.reset()
        st0, env = _np_state(sim)
        for case, (_, (want_gap, want_ttc)) in ic.HAND_CASES.items():
            st = ic.hand_state(st0, case)
            _set_state(sim, st, env)
            meter.reset()
            gap, ttc = meter.record()
            ref_gap, ref_ttc, amb, alive = im.measure(st, P)
            assert not amb.any() and alive.sum() == (3 if case == "wreck ahead" else 5)
            _compare(case, gap, ttc, ref_gap, ref_ttc, amb, alive)
            g, t = gap.cpu().numpy(), ttc.cpu().numpy()
            for e, n in ((0, 1), (1, 4)):              # body i of the case, in both scenes
                assert abs(g[e, n] - want_gap) < 1e-4, (case, e, g[e, n], want_gap)
                assert (np.isinf(t[e, n]) and np.isinf(want_ttc)) or abs(t[e, n] - want_ttc) < 1e-4, (case, e, t[e, n], want_ttc)
            if case == "cross-shaped overlap":
                assert g[0, 1] == 0.0 and t[0, 1] == 0.0
            assert np.isposinf(g[0, [0, 2, 4]]).all()                                     # EMPTY slots
            counts, _ = meter.totals(flush_open=True)
            assert counts.cpu().numpy()[:, 0].tolist() == [int(alive[0].sum()), int(alive[1].sum())]
    finally:
        meter.close()
        sim.close()


@pytest.mark.parametrize("shape", ["1x64", "3x7"])
def test_random_poses(shape):
    """1 x 64: every slot in use, 2016 pairs less the EMPTY ones, the LDS lists at their bound (an Intersection with 80 m arms: the
    default map has 48 spawn places); 3 x 7: odd sizes, a partly filled wave.  Totals after one record: every ALIVE slot is an agent."""
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    if shape == "1x64":
        cfg, seeds = SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=1, num_agents=64), ic.RANDOM_SEEDS_64
    else:
        cfg, seeds = SimConfig(map="intersection", num_envs=3, num_agents=7), ic.RANDOM_SEEDS_7
    sim = VecSim(cfg)
    meter = InteractionMeter(sim)
    P = im.Params.of(cfg)
    try:
        sim.reset()
        st0, env = _np_state(sim)
        for seed, aligned in seeds:
            st = ic.random_state(st0, seed, aligned)
            _set_state(sim, st, env)
            meter.reset()
            gap, ttc = meter.record()
            tr = im.Tracker(P, sim.E, sim.N)
            ref_gap, ref_ttc, amb, alive = tr.record(st, env)
            n_alive, n_amb = _compare("%s seed %d%s" % (shape, seed, " aligned" if aligned else ""), gap, ttc, ref_gap, ref_ttc, amb, alive)
            assert tr.ambiguous_samples <= 0.01 * n_alive and n_amb <= 0.01 * n_alive
            assert (ref_gap[alive] == 0).any() and np.isfinite(ref_ttc[alive]).any() and np.isinf(ref_ttc[alive]).any()
            _check_totals(shape, meter, tr, True)
            assert (meter.totals()[0].cpu().numpy() == 0).all()
    finally:
        meter.close()
        sim.close()


def _rollout(golden_dir, tracker=None, check=None):
    """120 steps of the rollout case; returns the meter's (closed, flushed) totals as numpy arrays"""
    import torch
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    cfg = ic.rollout_config()
    sim = VecSim(cfg)
    meter = InteractionMeter(sim)
    act = ic.rollout_policy(golden_dir)
    try:
        out = sim.reset()
        gap, ttc = meter.record()
        if check:
            check(0, sim, gap, ttc)
        for t in range(ic.ROLLOUT_STEPS):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            gap, ttc = meter.record()
            if check:
                check(t + 1, sim, gap, ttc)
        res = [tuple(x.cpu().numpy() for x in meter.totals(flush_open=f)) for f in (False, True)]
        if tracker is not None:
            for f in (False, True):
                _check_totals("rollout", meter, tracker, f)
        return res
    finally:
        meter.close()
        sim.close()


def test_rollout_against_the_restatement(golden_dir):
    cfg = ic.rollout_config()
    tr = im.Tracker(im.Params.of(cfg), cfg.num_envs, 10)
    stat = dict(alive=0, amb=0, resets=0, episodes=None)

    def check(t, sim, gap, ttc):
        st, env = _np_state(sim)
        ref_gap, ref_ttc, amb, alive = tr.record(st, env)
        a, b = _compare("rollout step %d" % t, gap, ttc, ref_gap, ref_ttc, amb, alive)
        stat["alive"] += a
        stat["amb"] += b
        stat["resets"] += 0 if stat["episodes"] is None else int((env[:, 1] != stat["episodes"]).sum())
        stat["episodes"] = env[:, 1].copy()
    (closed, _), (flushed, _) = _rollout(golden_dir, tracker=tr, check=check)
    print("rollout:", stat, "ambiguous by the tracker:", tr.ambiguous_samples, "of", tr.alive_samples)
    assert tr.ambiguous_samples <= 0.01 * tr.alive_samples and stat["amb"] <= 0.01 * stat["alive"]
    assert stat["resets"] >= 1 and (closed[:, 0] > 10).all()       # more agents than slots ended: resets and respawns happened
    assert (flushed[:, 0] >= closed[:, 0]).all() and (flushed[:, 1] > closed[:, 1]).any()
    assert (flushed[:, 2] > 0).any() and (flushed[:, 3] > 0).any() and (flushed[:, 4] > 0).any()      # every counter is exercised


def test_two_identical_runs_give_identical_bits(golden_dir):
    a, b = _rollout(golden_dir), _rollout(golden_dir)
    for (ca, sa), (cb, sb) in zip(a, b):
        assert np.array_equal(ca, cb) and np.array_equal(sa.view(np.int64), sb.view(np.int64))
    assert a[1][0][:, 0].sum() > 30


def test_metering_does_not_perturb_the_simulation():
    import torch
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="roundabout", num_envs=8)
    a, b = VecSim(cfg), VecSim(cfg)
    meter = InteractionMeter(a)
    rng = np.random.RandomState(3)
    keys = ("obs", "rew", "nei_rew", "flags", "nbr_idx", "lcf")

    def bits(t):
        t = t.cpu()
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    try:
        a.reset()
        b.reset()
        for t in range(50):
            act = np.zeros((8, a.N, 2), np.float32)
            act[..., 0], act[..., 1] = rng.uniform(-1.0, 1.0, (8, a.N)), rng.uniform(-0.3, 1.0, (8, a.N))
            act = torch.from_numpy(act).cuda()
            oa = a.step(act)
            meter.record()
            meter.totals(flush_open=True)
            ob = b.step(act)
            for k in keys:
                assert torch.equal(bits(oa[k]), bits(ob[k])), (t, k)
        for x, y in zip(a.get_state(), b.get_state()):
            assert torch.equal(bits(x), bits(y))
        assert meter.summary(flush_open=True)["steps"] > 0
    finally:
        meter.close()
        a.close()
        b.close()


TODAY_KEYS = {
    "velocity_step_mean_episode_min", "velocity_step_mean_episode_mean", "velocity_step_mean_episode_max", "energy_step_mean_episode_min",
    "energy_step_mean_episode_mean", "energy_step_mean_episode_max", "num_neighbours_mean_episode_mean", "num_neighbours_mean_episode_max",
    "num_agents_total", "num_agents_total_per_300_steps", "success_rate", "num_agents_success", "num_agents_success_per_300_steps",
    "num_agents_failed_per_300_steps", "episode_reward_mean", "episode_reward_min", "episode_reward_max", "episode_cost_mean",
    "episode_cost_min", "episode_cost_max", "episode_cost_sum", "crash_rate", "num_agents_crash", "out_rate", "num_agents_out",
    "episode_length_mean", "success_episode_length_mean", "svo_estimate_deg_mean", "svo_estimate_deg_min", "svo_estimate_deg_max", "svo_reward"}


def _throttles(obs):
    """Straight ahead, a throttle of its own per agent (0.30 .. 0.93 by agent number): followers catch up with slower leaders, so finite
    TTCs occur; with one throttle for all, vehicles of a lane keep their spacing and no pair ever closes inside the TTC horizon."""
    return {k: np.array([0.0, 0.3 + 0.07 * ((int(k[5:]) * 7) % 10)]) for k in obs}


def _episode(on):
    from copo_amd.eval.recoder import RecorderEnv
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    env = RecorderEnv(MultiAgentIntersectionEnv(dict(num_agents=10, horizon=30, delay_done=2, interaction_metrics=on)))
    infos = []
    try:
        o, d = env.reset(), {"__all__": False}
        for _ in range(200):
            o, r, d, i = env.step(_throttles(o))
            infos.append(i)
            if d["__all__"]:
                break
        assert d["__all__"]
        res = env.get_episode_result()
        o = env.reset()
        env.step(_throttles(o))           # the env goes on after an episode
        return res, infos
    finally:
        env.close()


def test_dict_env_and_recorder():
    off, infos_off = _episode(False)
    assert set(off) == TODAY_KEYS
    assert not any("min_gap" in v or "ttc" in v for i in infos_off for v in i.values())
    on, infos = _episode(True)
    acted = [v for i in infos for v in i.values() if "step_reward" in v]
    assert acted and all(v["min_gap"] >= 0.0 and v["ttc"] >= 0.0 for v in acted)
    assert any(np.isfinite(v["min_gap"]) for v in acted) and any(np.isfinite(v["ttc"]) for v in acted)
    assert all(np.isposinf(v["min_gap"]) for i in infos for v in i.values() if v.get("crash") or v.get("arrive_dest"))
    extra = {"interaction_" + k for k in ("agents", "steps", "min_gap_mean", "min_ttc_mean", "ttc_finite_frac", "tet_frac", "tit_mean",
                                         "near_events_per_agent", "brake_events_per_agent")}
    assert set(on) == TODAY_KEYS | extra
    assert {k: on[k] for k in TODAY_KEYS} == off                      # the metering changes no existing figure
    assert on["interaction_agents"] == on["num_agents_total"] and on["interaction_steps"] > 0 and np.isfinite(on["interaction_min_gap_mean"])
    print({k: on[k] for k in sorted(extra)})


def test_reset_close_and_argument_errors_leave_everything_usable():
    import torch
    from copo_amd import _capi
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    lib = _capi.lib
    sim = VecSim(SimConfig(map="intersection", num_envs=4))
    act = torch.zeros(4, sim.N, 2, device="cuda")
    act[..., 1] = 0.5
    h = C.c_void_p()
    try:
        sim.reset()
        for bad in ((0.0, 1.5, 0.5, 4.0), (-1.0, 1.5, 0.5, 4.0), (6.0, -0.1, 0.5, 4.0), (6.0, 1.5, -1.0, 4.0), (6.0, 1.5, 0.5, 0.0),
                    (float("inf"), 1.5, 0.5, 4.0), (6.0, float("nan"), 0.5, 4.0)):
            cfg = _capi.InteractCfg(*bad)
            assert lib.copo_interact_create(sim._h, C.byref(cfg), C.byref(h)) == -5, bad
        good = _capi.InteractCfg(6.0, 1.5, 0.5, 4.0)
        assert lib.copo_interact_create(sim._h, None, C.byref(h)) == -1
        assert lib.copo_interact_create(sim._h, C.byref(good), None) == -1
        with pytest.raises(_capi.CopoError):
            InteractionMeter(sim, horizon=0.0)
        meter = InteractionMeter(sim, horizon=4.0, ttc_crit=2.0, gap_near=1.0, brake=3.0)
        for _ in range(5):
            sim.step(act)
            gap, ttc = meter.record()
        st = _capi.current_stream()
        counts = torch.full((4, 6), -7, dtype=torch.int64, device="cuda")
        sums = torch.full((4, 3), -7.0, dtype=torch.float64, device="cuda")
        assert lib.copo_interact_totals(meter._h, None, sums.data_ptr(), 1, st) == -1
        assert lib.copo_interact_totals(meter._h, counts.data_ptr(), None, 1, st) == -1
        assert lib.copo_interact_totals(meter._h, counts.data_ptr(), sums.data_ptr(), 2, st) == -2
        torch.cuda.synchronize()
        assert (counts.cpu() == -7).all() and (sums.cpu() == -7.0).all()            # nothing was launched
        # either per-step output may be left out
        g2 = torch.full_like(gap, -1.0)
        before = meter.totals(flush_open=True)[0].cpu()
        assert lib.copo_interact_record(meter._h, g2.data_ptr(), None, st) == 0
        assert lib.copo_interact_record(meter._h, None, None, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(g2.cpu().view(torch.int32), gap.cpu().view(torch.int32))
        after = meter.totals(flush_open=True)[0].cpu()
        assert (after[:, 1] == before[:, 1] + 2 * before[:, 0]).all() and (after[:, 0] == before[:, 0]).all()
        s = meter.summary(flush_open=True)
        assert s["agents"] == int(after[:, 0].sum()) and s["steps"] == 7 * s["agents"]
        meter.reset()
        c0, s0 = meter.totals(flush_open=True)
        assert (c0.cpu() == 0).all() and (s0.cpu() == 0).all()
        meter.record()
        assert meter.summary(flush_open=True)["steps"] == s["agents"]
        meter.close()
        meter.close()                                                                   # closing twice is harmless
        out = sim.step(act)
        assert torch.isfinite(out["rew"]).all()
        again = InteractionMeter(sim)
        again.record()
        assert again.summary(flush_open=True)["agents"] == s["agents"]
        again.close()
    finally:
        sim.close()
