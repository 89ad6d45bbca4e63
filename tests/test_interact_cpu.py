"""CPU: the float64 restatement of the interaction meter (tests/interact_numpy.py) on cases worked out by hand, its per-agent
tracker on a hand-made sequence, and the library surface of `copo_interact_*` (exports, ctypes binding, NULL-argument codes)."""
import ctypes as C

import numpy as np

import interact_numpy as im

HL, HW, DT = 2.2575, 0.926, 0.1
P = im.Params(HL, HW, DT)
ALIVE, WRECK, EMPTY = im.ST_ALIVE, im.ST_WRECK, im.ST_EMPTY


def _scene(bodies):
    """bodies: (x, y, heading, speed, status) per slot"""
    b = np.array([r[:4] for r in bodies], np.float32)
    return im.scene(b[:, 0], b[:, 1], b[:, 2], b[:, 3], np.array([r[4] for r in bodies]), P)


def test_head_on():
    """Centres 20 m apart on one line, 5 m/s each: gap = 20 - 2 x 2.2575 = 15.485 m, closing at 10 m/s: TTC = 1.5485 s."""
    gap, ttc, amb = _scene([(0, 0, 0, 5, ALIVE), (20, 0, np.pi, 5, ALIVE)])
    np.testing.assert_allclose(gap, [15.485, 15.485], atol=1e-5)
    np.testing.assert_allclose(ttc, [1.5485, 1.5485], atol=1e-5)
    assert not amb.any()


def test_side_by_side_same_velocity():
    """Same heading and speed, 3.5 m apart laterally: the relative velocity is zero and the bodies are apart on the lateral axis, so they
    never meet; the gap is the lateral clearance 3.5 - 2 x 0.926 = 1.648 m."""
    gap, ttc, amb = _scene([(50, 10, 0.3, 7, ALIVE), (50 - 3.5 * np.sin(0.3), 10 + 3.5 * np.cos(0.3), 0.3, 7, ALIVE)])
    np.testing.assert_allclose(gap, [1.648, 1.648], atol=1e-5)
    assert np.isinf(ttc).all() and not amb.any()


def test_perpendicular_crossing():
    """i at the origin heading +x, j at (20, -15) heading +y, 10 m/s each; relative velocity w = (-10, 10).
    Along x the extents add to hl + hw = 3.1835 and the offset 20 closes at 10 m/s: overlap for t in [1.68165, 2.31835];
    along y the same extents, offset -15 closing at 10 m/s: overlap for t in [1.18165, 1.81835].
    t_in = 1.68165 <= t_out = 1.81835: TTC = 1.68165 s.  At t = 0 the nearest corners are (2.2575, -0.926) and (19.074, -12.7425):
    gap = hypot(16.8165, 11.8165) = 20.55296 m."""
    gap, ttc, amb = _scene([(0, 0, 0, 10, ALIVE), (20, -15, np.pi / 2, 10, ALIVE)])
    np.testing.assert_allclose(gap, [np.hypot(16.8165, 11.8165)] * 2, atol=1e-5)
    np.testing.assert_allclose(ttc, [1.68165, 1.68165], atol=1e-5)
    assert not amb.any()
    # j at 6 m/s: the y window becomes [11.8165 / 6, 18.1835 / 6] = [1.96942, 3.03058], entered inside the x window: TTC = 1.96942 s;
    # at 4 m/s it is [2.954, 4.546], after the x window has closed: they never meet
    _, slower, _ = _scene([(0, 0, 0, 10, ALIVE), (20, -15, np.pi / 2, 6, ALIVE)])
    np.testing.assert_allclose(slower, [11.8165 / 6] * 2, atol=1e-5)
    _, slowest, _ = _scene([(0, 0, 0, 10, ALIVE), (20, -15, np.pi / 2, 4, ALIVE)])
    assert np.isinf(slowest).all()


def test_cross_shaped_overlap_without_a_vertex_inside():
    """Two bodies at right angles over each other's middle: no corner of either lies inside the other (|2.2575| > 0.926 across), the
    separating-axis test still finds the overlap: gap 0, TTC 0."""
    gap, ttc, amb = _scene([(0, 0, 0, 3, ALIVE), (0.3, 0.2, np.pi / 2, 2, ALIVE)])
    corners_j = im._corners(0.3, 0.2, float(np.float32(np.pi / 2)), P.hl, P.hw)
    assert all(im._point_to_body(c, 0.0, 0.0, 0.0, P.hl, P.hw) > 0.5 for c in corners_j)
    assert (gap == 0).all() and (ttc == 0).all() and not amb.any()


def test_wreck_ahead_is_a_standing_obstacle():
    """A wreck 15 m ahead whose state still holds 5 m/s counts as standing: gap = 15 - 4.515 = 10.485 m, TTC = 10.485 / 8 s; the
    wreck owns no measurement; an EMPTY slot in between takes no part."""
    gap, ttc, amb = _scene([(0, 0, 0, 8, ALIVE), (7, 0, 0, 0, EMPTY), (15, 0, 0, 5, WRECK)])
    np.testing.assert_allclose([gap[0], ttc[0]], [10.485, 10.485 / 8], atol=1e-5)
    assert np.isinf(gap[1:]).all() and np.isinf(ttc[1:]).all() and not amb.any()


def test_horizon_and_grazing_marks():
    """TTC beyond the horizon is +inf; within 1e-3 s of it the sample is marked; so is a pair whose overlap window is shorter than 1e-3 s."""
    for v, inf, marked in ((1.6, True, False), (10.485 / 6.0005, True, True), (10.485 / 5.9995, False, True), (2.0, False, False)):
        gap, ttc, amb = _scene([(0, 0, 0, v, ALIVE), (15, 0, 0, 0, WRECK)])
        assert bool(np.isinf(ttc[0])) == inf and bool(amb[0]) == marked, (v, ttc, amb)
    # the crossing above with j further on: it leaves i's lane just as i arrives (the x window opens at 1.68165 s)
    hit = _scene([(0, 0, 0, 10, ALIVE), (20, -13.6335, np.pi / 2, 10, ALIVE)])      # y window ends at 1.68170 s: 0.05 ms of overlap
    assert np.isfinite(hit[1]).all() and hit[2].all()
    miss = _scene([(0, 0, 0, 10, ALIVE), (20, -13.63, np.pi / 2, 10, ALIVE)])       # y window ends at 1.68135 s: missed by 0.3 ms
    assert np.isinf(miss[1]).all() and miss[2].all()


def _state(E, N, rows):
    """State block [16][E][N] from {(e, n): (x, y, heading, speed, status, agent id)}"""
    st = np.zeros((16, E, N), np.float32)
    si = st.view(np.int32)
    for (e, n), (x, y, th, v, status, aid) in rows.items():
        st[0, e, n], st[1, e, n], st[2, e, n], st[3, e, n] = x, y, th, v
        si[13, e, n], si[14, e, n] = status | (3 << 8) | (7 << 16), aid
    return st


def test_tracker_follows_agents_through_slot_reuse_and_scene_reset():
    """One scene, two slots.  Agent 0 closes in on a wreck at TTC 2.0, 1.4, 0.8, 0.2 s: 4 steps, three of them critical (< 1.5 s),
    tit (0.1 + 0.7 + 1.3) x 0.1, ONE near event (it stays near), and 8 -> 7 m/s in the last step (10 m/s^2 > 4): one brake event.  Then
    the slot holds agent 5 (fold), then the episode counter moves (fold), then the slot is empty (fold)."""
    tr = im.Tracker(P, 1, 2)
    env = np.array([[0, 3, 0, 1]], np.int32)
    W = (100.0, 0.0, 0.0, 0.0, WRECK, 9)

    def at(ttc, v, aid):
        return (100.0 - 2 * HL - ttc * v, 0.0, 0.0, v, ALIVE, aid)
    for ttc, v in ((2.0, 8.0), (1.4, 8.0), (0.8, 8.0)):
        tr.record(_state(1, 2, {(0, 0): at(ttc, v, 0), (0, 1): W}), env)
    tr.record(_state(1, 2, {(0, 0): at(0.2, 7.0, 0), (0, 1): W}), env)
    t = tr.totals(flush_open=True)
    assert t["counts"][0].tolist() == [1, 4, 3, 1, 1, 1]
    np.testing.assert_allclose(t["sums"][0], [0.2 * 7.0, 0.2, (0.1 + 0.7 + 1.3) * DT], rtol=1e-4)
    assert (t["lo"] == t["counts"]).all() and (t["hi"] == t["counts"]).all() and (t["slack"] == 0).all()
    assert tr.totals()["counts"][0].tolist() == [0] * 6                       # nobody has ended yet
    tr.record(_state(1, 2, {(0, 0): at(3.0, 5.0, 5), (0, 1): W}), env)         # another agent in the slot
    assert tr.totals()["counts"][0].tolist() == [1, 4, 3, 1, 1, 1]
    env2 = env.copy()
    env2[0, 1] = 4
    tr.record(_state(1, 2, {(0, 0): at(3.0, 5.0, 5), (0, 1): W}), env2)        # same id, next episode: a new agent
    assert tr.totals()["counts"][0].tolist() == [2, 5, 3, 1, 1, 2]
    tr.record(_state(1, 2, {(0, 1): W}), env2)
    assert tr.totals()["counts"][0].tolist() == [3, 6, 3, 1, 1, 3] and tr.totals(True)["counts"][0].tolist() == [3, 6, 3, 1, 1, 3]
    assert tr.alive_samples == 6 and tr.ambiguous_samples == 0


def test_library_exports_and_binds_the_interaction_entries():
    from copo_amd import _capi
    names = ["copo_interact_create", "copo_interact_record", "copo_interact_totals", "copo_interact_reset", "copo_interact_destroy"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS and getattr(_capi.lib, name).restype is C.c_int
    assert C.sizeof(_capi.InteractCfg) == 16 and [f[0] for f in _capi.InteractCfg._fields_] == ["horizon_s", "ttc_crit_s", "gap_near_m", "brake_mps2"]
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    # NULL arguments are refused before any device call
    h, cfg = C.c_void_p(), _capi.InteractCfg(6.0, 1.5, 0.5, 4.0)
    assert _capi.lib.copo_interact_create(None, C.byref(cfg), C.byref(h)) == -1
    assert b"copo_interact_create" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_interact_record(None, None, None, None) == -1
    assert _capi.lib.copo_interact_totals(None, None, None, 0, None) == -1
    assert _capi.lib.copo_interact_reset(None, None) == -1
    assert _capi.lib.copo_interact_destroy(None) == -1


def test_summary_reduces_over_scenes():
    from copo_amd.interact import COUNT_KEYS, SUM_KEYS, summarise
    assert COUNT_KEYS == im.COUNT_KEYS and SUM_KEYS == im.SUM_KEYS
    s = summarise(np.array([[2, 30, 6, 3, 1, 1], [2, 10, 0, 1, 1, 2]]), np.array([[4.0, 1.0, 0.3], [2.0, 5.0, 0.1]]))
    assert s == dict(agents=4, steps=40, min_gap_mean=1.5, min_ttc_mean=2.0, ttc_finite_frac=0.75, tet_frac=0.15, tit_mean=0.1,
                     near_events_per_agent=1.0, brake_events_per_agent=0.5)
    empty = summarise(np.zeros((3, 6), np.int64), np.zeros((3, 3)))
    assert empty["agents"] == 0 and all(np.isnan(v) for k, v in empty.items() if k not in ("agents", "steps"))


def test_chosen_cases_stay_under_the_ambiguity_cap(golden_dir):
    """The seeds of the GPU comparison (tests/test_gpu_interact.py), by the restatement alone: ambiguous samples stay under 1 % of the
    ALIVE samples of every case, and the rollout (here on the CPU oracle, which the HIP simulator matches bit for bit) has what it is
    meant to have: slots taken over by new agents inside an episode and scene resets."""
    import interact_cases as ic
    import oracle_lib as ol
    cfg = ic.rollout_config()
    Pc = im.Params.of(cfg)
    for shape, seeds in (((1, 64), ic.RANDOM_SEEDS_64), ((3, 7), ic.RANDOM_SEEDS_7)):
        for seed, aligned in seeds:
            alive, amb = ic.ambiguous_samples(ic.random_state(np.zeros((16,) + shape, np.float32), seed, aligned), Pc)
            assert alive >= 0.5 * shape[0] * shape[1] and amb <= 0.01 * alive, (shape, seed, aligned, alive, amb)
    o = ol.OracleSim(cfg)
    try:
        out, act = o.reset(), ic.rollout_policy(golden_dir)
        tr = im.Tracker(Pc, o.E, o.N)
        tr.record(*o.get_state())
        agents_of = {}
        for t in range(ic.ROLLOUT_STEPS):
            out = o.step(act(out["obs"]))
            st, env = o.get_state()
            tr.record(st, env)
            si = st.view(np.int32)
            for e, n in zip(*np.nonzero((si[13] & 0xFF) == ALIVE)):
                agents_of.setdefault((e, int(env[e, 1]), n), set()).add(int(si[14, e, n]))
        assert tr.ambiguous_samples <= 0.01 * tr.alive_samples, (tr.ambiguous_samples, tr.alive_samples)
        assert sum(len(v) > 1 for v in agents_of.values()) >= 1, "no slot was taken over inside an episode"
        assert len({(e, ep) for e, ep, _ in agents_of}) > o.E, "no scene was reset"
        t = tr.totals(flush_open=True)
        assert (t["counts"][:, 2] > 0).any() and (t["counts"][:, 3] > 0).any() and (t["counts"][:, 4] > 0).any(), t["counts"]
    finally:
        o.close()
