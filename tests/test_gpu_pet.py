"""Encroachment log on the GPU (copo_pet_*, copo_amd/encroach.py) against the restatement of its rules (tests/pet_numpy.py): the sequences
worked out by hand at 3 scenes x 7 slots and 5 scenes x 64 slots, two short rollouts of the reference's population on the maps where paths
cross, scene groups, overflow inside a scene with a `clear`, 4 100 scenes (more than one pass of the scene grid and of the assign
workgroup), `reset`, the refused configurations and the lifetime of the handle.  Every comparison is exact: the rows word for word,
`count()`, the whole stamp grid, the `met` masks, the histogram and the map."""
import ctypes as C

import numpy as np
import pytest

import pet_cases as pc
import pet_numpy as pn
from rowlog_gpu import _np_state, _set_state, _sim64

pytestmark = pytest.mark.gpu


def _hand_log(sim, **kwargs):
    from copo_amd.encroach import EncroachmentLog
    kw = dict(cell=1.0, window=pc.HAND_WINDOW, critical_s=pc.HAND_CRITICAL * float(sim.cfg.dt), max_rows=256)
    kw.update(kwargs)
    return EncroachmentLog(sim, 0.0, 0.0, pc.HAND_W, pc.HAND_H, **kw)


def _run_hand(N, log_kwargs=None, ref_kwargs=None, groups=None, after=None):
    """the hand sequence through a device log and the restatement next to it, compared after every record; `after(r, log, ref)` runs
    after record r's comparison"""
    sim = _sim64(pc.hand_scenes(N), N)
    log = None
    try:
        log = _hand_log(sim, **(log_kwargs or {}))
        ref = pc.hand_log(N, **(ref_kwargs or {}))
        assert log.critical_records == pc.HAND_CRITICAL and (sim.cfg.veh_half_len, sim.cfg.veh_half_wid) == (pc.HL, pc.HW)
        if groups is not None:
            log.set_groups(groups)
            ref.set_groups(groups)
        sim.reset()
        st0, env0 = _np_state(sim)

        def record(r, st, env):
            _set_state(sim, st, env)
            log.record()
            ref.record(st, env)
            pn.compare_all(log, ref)
            if after is not None:
                after(r, log, ref)

        def forget():
            log.forget()
            ref.forget()
        pc.run_hand(N, record, forget, st0, env0)
        return log.rows().cpu().numpy().view(np.uint32), log.count(), log.aggregates(), ref
    finally:
        if log is not None:
            log.close()
        sim.close()


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence(N):
    """3 and 5 scenes: the last workgroup is partial.  The rows are the ones tests/pet_cases.py writes out by hand"""
    rows, count, agg, ref = _run_hand(N)
    want = pc.hand_expected(N)
    assert count == (len(want), 0) and rows.shape == want.shape and np.array_equal(rows, want), np.argwhere(rows != want).tolist()
    if N == 7:
        assert agg["hist"][0].tolist() == pc.HAND_HIST
        assert {(int(x), int(y)): int(agg["critical"][0, y, x]) for y, x in np.argwhere(agg["critical"][0])} == pc.HAND_CRITICAL_MAP
    assert ref.second_touches >= 3 and ref.turnovers_in_window >= 1
    assert agg["meta"]["n_records"] == pc.HAND_RECORDS and agg["pet_s"].tolist() == [(k + 1) * agg["meta"]["dt"] for k in range(pc.HAND_WINDOW)]


def test_groups_two_groups_and_one_scene_routed_nowhere():
    rows, count, agg, ref = _run_hand(7, dict(groups=2), dict(groups=2), groups=[1, 0, -1])
    want = pc.hand_expected(7)
    assert np.array_equal(rows, want) and count == (len(want), 0)          # the rows of a scene that is routed nowhere are written
    per_scene = [int((want[:, 0] == e).sum()) for e in range(3)]
    assert agg["hist"].shape == (2, 3, pc.HAND_WINDOW) and agg["hist"][1].sum() == per_scene[0] and agg["hist"][0].sum() == per_scene[1] and per_scene[2] > 0
    assert agg["critical"][0, 25, 14] == 2 and agg["critical"][1, 26, 4] == 1 and agg["critical"][:, 5, 18].sum() == 0


def test_overflow_inside_scene_2_then_clear():
    """a pool of 9: record 6 has two rows in scene 2, ids 8 and 9; the second one and everything after it is dropped, the aggregates
    are complete; after a `clear` that follows record 7 the later rows are stored"""
    def after(r, log, ref):
        if r == 6:
            assert log.count() == (9, 1) and np.array_equal(log.rows().cpu().numpy().view(np.uint32), pc.hand_expected(7, upto=7)[:9])
        if r == 7:
            assert log.count() == (9, 2)
            t = log.table()
            assert t.meta["dropped"] == 2 and len(t) == 9
            log.clear()
            ref.clear()
    rows, count, agg, ref = _run_hand(7, dict(max_rows=9), dict(max_rows=9), after=after)
    want = pc.hand_expected(7)
    assert count == (2, 0) and np.array_equal(rows, want[-2:])
    assert agg["hist"][0].tolist() == pc.HAND_HIST and agg["critical"].sum() == sum(pc.HAND_CRITICAL_MAP.values())


def test_4100_scenes_tile_the_hand_sequence():
    """the 5-scene hand state tiled 820 times: more scenes than one pass of the scene grid (4 096) and of the assign workgroup (1 024); the
    5 scenes are restated once and the rows expected with their scene ids"""
    from copo_amd.encroach import state_bytes
    N, T = 64, 820
    E = 5 * T
    sim = _sim64(E, N)
    log = None
    try:
        log = _hand_log(sim, max_rows=1 << 15)
        assert log.state_bytes == state_bytes(E, N, 32, 32, pc.HAND_WINDOW, 1, 1 << 15) == 8 * E * 1024 + 20 * E * N + 16 * E + 8 * (12 + 1024) + (64 << 15) + 16
        ref = pc.hand_log(N)
        sim.reset()
        st0, env0 = _np_state(sim)
        want = []

        def record(r, st, env):
            _set_state(sim, np.tile(st, (1, T, 1)), np.tile(env, (T, 1)))
            log.record()
            before = ref.n_rows
            ref.record(st, env)
            new = ref.rows()[before:]
            for t in range(T):
                rows = new.copy()
                rows[:, 0] += 5 * t
                want.append(rows)

        def forget():
            log.forget()
            ref.forget()
        sim_st0 = st0[:, :5].copy()
        pc.run_hand(N, record, forget, sim_st0, env0[:5].copy())
        want = np.concatenate(want)
        rows = log.rows().cpu().numpy().view(np.uint32)
        assert log.count() == (len(want), 0) and len(want) == 15 * T and np.array_equal(rows, want), np.argwhere(rows != want)[:8].tolist()
        grid, met = log.memory()
        assert np.array_equal(grid.reshape(T, 5, -1), np.broadcast_to(ref.stamps, (T, 5, 1024)))
        assert np.array_equal(met.reshape(T, 5, N), np.broadcast_to(ref.met, (T, 5, N)))
        agg = log.aggregates()
        assert np.array_equal(agg["hist"], ref.hist * T) and np.array_equal(agg["critical"], ref.critical * T)
    finally:
        if log is not None:
            log.close()
        sim.close()


@pytest.mark.parametrize("name", ["intersection", "roundabout"])
def test_rollout_against_the_restatement(golden_dir, name):
    """6 x 40, the shipped population: the states are read back each step and fed to the restatement; the simulator's memory is only read"""
    import torch
    from copo_amd.encroach import EncroachmentLog
    from copo_amd.sim import VecSim
    cfg = pc.rollout_config(name)
    sim = VecSim(cfg)
    log = None
    act = pc.rollout_policy(golden_dir, name)
    try:
        log = EncroachmentLog.for_map(sim, window=pc.ROLLOUT_WINDOW, critical_s=1.0)
        g = pc.rollout_grid(cfg)
        assert (log.x0, log.y0, log.W, log.H, log.critical_records) == (float(g.x0), float(g.y0), g.W, g.H, pc.ROLLOUT_CRITICAL)
        ref = pn.EncroachmentLog(sim.E, sim.N, g, pc.HL, pc.HW, window=pc.ROLLOUT_WINDOW, critical_records=pc.ROLLOUT_CRITICAL)
        out = sim.reset()
        for t in range(pc.GPU_ROLLOUT_STEPS + 1):
            before = [x.clone() for x in sim.get_state()] if t == 3 else None
            log.record()
            if before is not None:
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, sim.get_state()))
            ref.record(*_np_state(sim))
            if t % 20 == 0 or t == pc.GPU_ROLLOUT_STEPS:
                pn.compare_all(log, ref)
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
        pc.check_invariants(ref)
        t = log.table()
        print("%s: %d rows %s, hist sum %d, critical %d, second touches %d" % (name, len(t), {k: int((t.type == k).sum()) for k in ("following", "crossing", "opposing")},
                                                                           ref.hist.sum(), ref.critical.sum(), ref.second_touches))
        assert len(t) == ref.n_rows >= 1 and (t.pet_s <= pc.ROLLOUT_WINDOW * float(cfg.dt) + 1e-9).all()
    finally:
        if log is not None:
            log.close()
        sim.close()


def test_reset_read_bounds_and_refused_configs():
    import torch
    from copo_amd import _capi
    from copo_amd.encroach import EncroachmentLog
    lib = _capi.lib
    N = 7
    sim = _sim64(pc.hand_scenes(N), N)
    h = C.c_void_p()
    log = None
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        for cfg, code in pc.refused_configs(_capi):
            assert lib.copo_pet_create(sim._h, C.byref(cfg), C.byref(h)) == code and b"copo_pet_create" in lib.copo_last_error() and not h.value
        ok = _capi.PetCfg(0.0, 0.0, 1.0, 32, 32, 1, 4, 2, 16)
        assert lib.copo_pet_create(sim._h, None, C.byref(h)) == -1 and lib.copo_pet_create(sim._h, C.byref(ok), None) == -1
        with pytest.raises(_capi.CopoError) as err:                  # 1.31 m is wider than 2 x 0.926 / sqrt(2) = 1.3096 m; 1.30 m is not
            EncroachmentLog(sim, 0.0, 0.0, 32, 32, cell=1.31)
        assert err.value.code == -5
        EncroachmentLog(sim, 0.0, 0.0, 32, 32, cell=1.30).close()
        log = _hand_log(sim, max_rows=64)
        stream = _capi.current_stream()

        def run(upto):
            for r in range(upto):
                st, env = pc.hand_record(st0, env0, r)
                _set_state(sim, st, env)
                log.record()
        run(5)
        want = pc.hand_expected(N, upto=5)
        first = log.rows().cpu().numpy().view(np.uint32)
        assert np.array_equal(first, want) and log.count() == (len(want), 0)
        out = torch.empty(65, 16, dtype=torch.int32, device="cuda")
        for a, n in ((0, 65), (64, 1), (-1, 1), (0, -1), (2 ** 31 - 1, 2)):
            assert lib.copo_pet_read(log._h, a, n, out.data_ptr(), stream) == -2 and b"copo_pet_read" in lib.copo_last_error()
        assert lib.copo_pet_read(log._h, 0, 4, None, stream) == -1 and lib.copo_pet_count(log._h, None, stream) == -1
        assert lib.copo_pet_aggregates(log._h, None, None, stream) == -1 and lib.copo_pet_memory(log._h, None, None, stream) == -1
        assert lib.copo_pet_set_groups(log._h, None, stream) == -1
        with pytest.raises(ValueError):
            log.set_groups([0, 0])
        log.flush()                                      # a no-op: nothing is ever open
        assert log.count() == (len(want), 0)
        # reset: rows, stamps, masks and aggregates are gone and records count from 0: the hand sequence gives its rows again
        log.reset()
        grid, met = log.memory()
        assert log.count() == (0, 0) and log.n_records == 0 and not grid.any() and not met.any() and not log.aggregates()["hist"].any()
        run(5)
        assert np.array_equal(log.rows().cpu().numpy().view(np.uint32), want)
        out = sim.step(torch.zeros(sim.E, sim.N, 2, device="cuda"))
        assert torch.isfinite(out["rew"]).all()
    finally:
        if log is not None:
            log.close()
        sim.close()


def test_lifecycle_closed_twice_and_after_its_simulator():
    """tests/test_gpu_handles.py's checks for this handle"""
    import torch
    sim = _sim64(2, 7)
    sim.reset()
    try:
        obs = _hand_log(sim, max_rows=8)
        assert obs._h.value and obs.sim is sim
        obs.record()
        obs.reset()
        obs.close()
        assert not obs._h.value
        obs.close()                                    # a no-op
    finally:
        sim.close()
    sim = _sim64(2, 7)
    sim.reset()
    obs = _hand_log(sim, max_rows=8)
    obs.record()
    torch.cuda.synchronize()
    sim.close()
    obs.close()                                        # reads the handle alone, not the simulator that is gone
    assert not obs._h.value
