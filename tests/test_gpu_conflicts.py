"""Conflict log on the GPU (copo_conflict_*, copo_amd/conflicts.py) against the restatement of its rules (tests/conflict_numpy.py): the
sequence worked out by hand at 7 and 64 slots, two rollouts of the reference's CoPO population (one with a `clear` in the middle, one with
a small horizon and a reset by hand), overflow inside a scene at 1, 3 and 1 030 scenes of 2 016 pairs each, `flush`, `read` bounds, the
refused configurations, the lifetime of the handle and `env.conflict_log()`.  Every comparison is on raw 32-bit words and exact."""
import ctypes as C

import numpy as np
import pytest

import conflict_cases as cc
import conflict_numpy as cn
import interact_cases as ic
from rowlog_gpu import Both, _dev, _np_state, _read, _set_state, _sim64
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence(N):
    """E = 4: one workgroup.  The rows are the ones tests/conflict_cases.py writes out by hand; the restatement runs next to the device"""
    from copo_amd.conflicts import ConflictLog, state_bytes
    sim = _sim64(cc.HAND_E, N)
    log = ConflictLog(sim, max_rows=64, radius=cc.RADIUS, leave_radius=cc.LEAVE)
    ref = cn.ConflictLog(cc.HAND_E, N, max_rows=64, radius=cc.RADIUS, leave_radius=cc.LEAVE)
    try:
        assert log.state_bytes == state_bytes(cc.HAND_E, N, 64) == 48 * cc.HAND_E * N * (N - 1) // 2 + 20 * cc.HAND_E * N + 12 * cc.HAND_E + 64 * 64 + 16
        sim.reset()
        st0, env0 = _np_state(sim)

        def record(r, st, env, flags):
            _set_state(sim, st, env)
            log.record(_dev(flags))
            ref.record(st, env, flags)
            cn.compare(*_read(log), ref)
        mid, end = cc.run_hand(Both(log, ref), N, record, lambda: _read(log), st0, env0)
        before, after = cc.hand_expected(N)
        for (got, count), want in ((mid, before), (end, after)):
            assert count == (len(want), 0) and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want).tolist()
        assert log.n_records == cc.HAND_RECORDS
        log.flush()                                      # nothing stayed open
        assert log.count() == (len(after), 0)
    finally:
        log.close()
        sim.close()


def _rollout(golden_dir, cfg, steps, reset_after=None, clear_after=None):
    """A rollout of the reference's population with a `ConflictLog` and the restatement next to it; the simulator's memory is only read."""
    import torch
    from copo_amd.conflicts import ConflictLog
    from copo_amd.sim import VecSim
    sim = VecSim(cfg)
    log = None
    act = ic.rollout_policy(golden_dir)
    try:
        log = ConflictLog(sim)
        ref = cn.ConflictLog(sim.E, sim.N)
        drained = 0

        def record(out):
            flags = None if out is None else out["flags"]
            before = [x.clone() for x in sim.get_state()] if log.n_records == 3 else None
            log.record(flags)
            if before is not None:
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, sim.get_state()))
            ref.record(*_np_state(sim), None if flags is None else flags.cpu().numpy())
        out = sim.reset()
        record(None)
        for t in range(steps):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            record(out)
            if reset_after is not None and t + 1 == reset_after:
                out = sim.reset(cc.short_seeds(sim.E))
                record(None)
            if clear_after is not None and t + 1 == clear_after:
                t_mid = log.drain()
                cn.compare(t_mid.raw, (len(t_mid), t_mid.meta["dropped"]), ref)
                ref.clear()
                drained = len(t_mid)
        rows, count = _read(log)
        cn.compare(rows, count, ref)
        cc.check_invariants(ref)
        log.flush()
        ref.flush()
        cn.compare(*_read(log), ref)
        return rows, count, ref, drained
    finally:
        if log is not None:
            log.close()
        sim.close()


def test_rollout_with_a_clear_in_the_middle_against_the_restatement(golden_dir):
    """6 x 40, 200 steps: 586 rows on the CPU oracle (121 of kind 1, 14 of them with CRASH on both sides; 465 parted), 109 scene-records with
    two or more closes, up to four encounters of one slot at once"""
    from copo_amd import conflicts
    rows, count, ref, drained = _rollout(golden_dir, cc.rollout_config(), cc.ROLLOUT_STEPS, clear_after=cc.ROLLOUT_CLEAR_AFTER)
    d = conflicts.decode(rows, 0.1, ic.HL, ic.HW)
    print("drained %d, then %s rows; kinds %s; scene-records with two closes %d, most encounters of one slot %d"
          % (drained, count, np.bincount(d["kind"], minlength=5).tolist(), ref.scene_records_with_two_closes, ref.max_encounters_of_one_slot))
    assert drained > 0 and count[0] > 0 and count[1] == 0 and drained + count[0] == 586
    assert ref.scene_records_with_two_closes >= 1 and ref.max_encounters_of_one_slot >= 2 and (d["outcome"] == "both_crashed").any()


def test_short_rollout_with_a_reset_by_hand_against_the_restatement(golden_dir):
    from copo_amd import conflicts
    rows, count, ref, _ = _rollout(golden_dir, cc.short_config(), cc.SHORT_STEPS, reset_after=cc.SHORT_RESET_AFTER)
    d = conflicts.decode(rows, 0.1, ic.HL, ic.HW)
    print("rows %s kinds %s" % (count, np.bincount(d["kind"], minlength=5).tolist()))
    assert (d["kind"] == cn.KIND_VANISHED).sum() >= 1 and (d["kind"] == cn.KIND_DONE).sum() >= 1


@pytest.mark.parametrize("E", [1, 3, 1030])
def test_overflow_inside_a_scene(E):
    """64 slots, every one ALIVE within `radius` of every other: 2 016 open pairs per scene, which all end in one record (DONE on every
    slot), into a pool that overflows inside a scene: the last scene at 1 and 3 scenes, scene 2 at 1 030 (the 2 M pairs of that size take
    seconds of python in the restatement as it is; the rows it would take to fill a pool up to scene 1 025 would double them).  At 1 030
    scenes a second round -- three slots in each of the scenes 1 020 .. 1 029 -- puts rows on both sides of the assign walk's second pass."""
    from copo_amd.conflicts import ConflictLog
    N, P = 64, 2016
    sim = _sim64(E, N)
    max_rows = (E - 1) * P + 1000 if E < 1000 else 2 * P + 1000
    log = ConflictLog(sim, max_rows=max_rows)
    ref = cn.ConflictLog(E, N, max_rows=max_rows)
    rng = np.random.RandomState(E)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)

        def record(status, flags):
            st = st0.copy()
            su = st.view(np.uint32)
            st[0], st[1] = rng.uniform(0.0, 4.0, (E, N)).astype(np.float32), rng.uniform(0.0, 4.0, (E, N)).astype(np.float32)
            st[2], st[3] = rng.uniform(-3.0, 3.0, (E, N)).astype(np.float32), rng.uniform(0.0, 9.0, (E, N)).astype(np.float32)
            su[13] = (su[13] & ~np.uint32(0xFF)) | status.astype(np.uint32)
            su[14] = np.arange(E * N, dtype=np.uint32).reshape(E, N)
            _set_state(sim, st, env0)
            log.record(_dev(flags))
            ref.record(st, env0, flags)
        alive = np.full((E, N), cn.ST_ALIVE)
        record(alive, None)
        assert ref.n_open() == E * P
        ends = (cn.F_ACTED | cn.F_DONE | rng.choice([cn.F_ARRIVE, cn.F_CRASH, cn.F_OUT], size=(E, N))).astype(np.uint8)
        record(np.full((E, N), cn.ST_EMPTY), ends)
        rows, count = _read(log)
        cn.compare(rows, count, ref)
        print("E %d: %d rows, %d dropped" % (E, count[0], count[1]))
        assert count == (max_rows, E * P - max_rows) and ref.n_open() == 0 and count[1] > 0
        log.flush()
        cn.compare(*_read(log), ref)                     # nothing was open
        if E > 1024:
            log.clear()
            ref.clear()
            some = np.full((E, N), cn.ST_EMPTY)
            some[1020:, [5, 40, 63]] = cn.ST_ALIVE
            record(some, np.zeros((E, N), np.uint8))
            record(np.full((E, N), cn.ST_EMPTY), np.where(some == cn.ST_ALIVE, cn.F_ACTED | cn.F_DONE | cn.F_CRASH, 0).astype(np.uint8))
            rows, count = _read(log)
            cn.compare(rows, count, ref)
            assert count == (30, 0) and rows[:, 0].tolist() == [e for e in range(1020, 1030) for _ in range(3)]
    finally:
        log.close()
        sim.close()


def test_flush_read_bounds_reset_and_refused_configs():
    import torch
    from copo_amd import _capi
    from copo_amd.conflicts import ConflictLog
    from copo_amd.sim import VecSim
    lib = _capi.lib
    N = 7
    sim = VecSim(SimConfig(map="intersection", num_envs=cc.HAND_E, num_agents=N))
    h = C.c_void_p()
    log = None
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        for cfg, code in cc.refused_configs(_capi):
            assert lib.copo_conflict_create(sim._h, C.byref(cfg), C.byref(h)) == code and b"copo_conflict_create" in lib.copo_last_error() and not h.value
        assert lib.copo_conflict_create(sim._h, None, C.byref(h)) == -1 and lib.copo_conflict_create(sim._h, C.byref(_capi.ConflictCfg(8, 8.0, 10.0)), None) == -1
        with pytest.raises(_capi.CopoError):
            ConflictLog(sim, max_rows=0)
        with pytest.raises(_capi.CopoError):
            ConflictLog(sim, radius=8.0, leave_radius=7.0)
        log = ConflictLog(sim, max_rows=64, radius=cc.RADIUS, leave_radius=cc.LEAVE)
        stream = _capi.current_stream()

        def run(upto, first=0):
            for r in range(first, upto):
                st, env, flags = cc.hand_record(st0, env0, r)
                _set_state(sim, st, env)
                log.record(_dev(flags))
        run(4)
        before = _read(log)
        assert before[1] == (6, 0) and np.array_equal(before[0], cc.hand_expected(N)[0])
        # refused calls launch nothing and leave the handle usable
        out = torch.empty(65, 16, dtype=torch.int32, device="cuda")
        for first, n in ((0, 65), (64, 1), (-1, 1), (0, -1), (2 ** 31 - 1, 2)):
            assert lib.copo_conflict_read(log._h, first, n, out.data_ptr(), stream) == -2 and b"copo_conflict_read" in lib.copo_last_error()
        assert lib.copo_conflict_read(log._h, 0, 4, None, stream) == -1 and lib.copo_conflict_count(log._h, None, stream) == -1
        assert lib.copo_conflict_read(log._h, 0, 0, None, stream) == 0 and lib.copo_conflict_read(log._h, 60, 4, out.data_ptr(), stream) == 0
        E = cc.HAND_E
        for bad in (torch.zeros(E, N, dtype=torch.int32, device="cuda"), torch.zeros(E, N + 1, dtype=torch.uint8, device="cuda"),
                    torch.zeros(E, N, dtype=torch.uint8), torch.zeros(N, E, dtype=torch.uint8, device="cuda").t()):
            with pytest.raises(ValueError):
                log.record(bad)
        after = _read(log)
        assert after[1] == before[1] and np.array_equal(after[0], before[0]) and log.n_records == 4
        # flush in the middle: the open encounters leave with kind 4 in (scene, slot_a, slot_b) order, and whoever is still close opens again
        log.flush()
        rows, count = _read(log)
        assert count[0] > 6 and ((rows[6:, 1] >> 12) & 15 == cn.KIND_FLUSHED).all()
        order = [(int(s), int(w & 63), int((w >> 6) & 63)) for s, w in rows[6:, :2]]
        assert order == sorted(order)
        # reset: every row, counter and open encounter is gone and records count from 0: the hand sequence gives its rows again
        log.reset()
        assert log.count() == (0, 0) and log.n_records == 0
        log.flush()
        assert log.count() == (0, 0)                     # nothing was open
        run(4)
        again = _read(log)
        assert again[1] == (6, 0) and np.array_equal(again[0], before[0])
        log.clear()
        run(cc.HAND_RECORDS, first=4)
        log.flush()
        rows, count = _read(log)
        assert count == (11, 0) and np.array_equal(rows, cc.hand_expected(N)[1])
        t = log.table()
        assert len(t) == 11 and t.meta["n_records"] == cc.HAND_RECORDS and t.meta["dt"] == float(sim.cfg.dt) and t.outcome[0] == "parted"
        out = sim.step(torch.zeros(cc.HAND_E, sim.N, 2, device="cuda"))
        assert torch.isfinite(out["rew"]).all()
    finally:
        if log is not None:
            log.close()
        sim.close()


def _lifecycle_sim():
    import sim_config_cases as scc
    from copo_amd.sim import VecSim
    sim = VecSim(scc.sim_config("intersection", 2, 12))
    sim.reset()
    return sim


def test_lifecycle_closed_twice_and_after_its_simulator():
    """tests/test_gpu_handles.py's checks for this handle"""
    import torch
    from copo_amd.conflicts import ConflictLog
    sim = _lifecycle_sim()
    try:
        obs = ConflictLog(sim, max_rows=8)
        assert obs._h.value and obs.sim is sim
        obs.record()
        obs.reset()
        obs.close()
        assert not obs._h.value
        obs.close()                                    # a no-op
        assert not obs._h.value
    finally:
        sim.close()
    sim.close()
    assert not sim._h.value
    sim = _lifecycle_sim()
    obs = ConflictLog(sim, max_rows=8)
    obs.record()
    torch.cuda.synchronize()
    sim.close()
    obs.close()                                        # reads the handle alone, not the simulator that is gone
    assert not obs._h.value
    sim = _lifecycle_sim()
    try:
        obs = ConflictLog(sim, max_rows=8)
        obs.record()
        torch.cuda.synchronize()
        assert obs.n_records == 1 and obs.count() == (0, 0)      # the one record: counted, and no encounter has ended in it
        obs.close()
    finally:
        sim.close()


def test_env_conflict_log_attaches_late_and_matches_a_log_by_hand():
    """`env.conflict_log()` after five steps: one record at once, then one per reset and step (its count follows the list's); a log driven
    by hand over a second env on the same seeds, fed the same states, has the same rows"""
    import torch
    from copo_amd.conflicts import ConflictLog
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    assert "conflict_log" not in MultiAgentIntersectionEnv.default_config()
    env = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2, trip_log={}))
    other = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2))
    log = None
    try:
        act = torch.zeros(2, env.sim.N, 2, device="cuda")
        act[..., 1] = torch.linspace(0.3, 1.0, env.sim.N, device="cuda")
        env.vec_reset()
        other.vec_reset()
        for _ in range(5):
            env.vec_step(act)
            other.vec_step(act)
        assert env.observer("conflict_log") is None
        mine = env.conflict_log(max_rows=4096, radius=9.0, leave_radius=12.0)
        log = ConflictLog(other.sim, max_rows=4096, radius=9.0, leave_radius=12.0)
        log.record()
        at = env.observers.records
        assert mine.n_records == 1 and env.conflict_log() is mine and env.observers.names() == ["trip_log", "conflict_log"]
        for k in range(2):
            for _ in range(12):
                env.vec_step(act)
                log.record(other.vec_step(act)["flags"])
            assert mine.n_records == 1 + env.observers.records - at
            if k == 0:
                env.vec_reset()
                other.vec_reset()
                log.record()
        assert mine.n_records == log.n_records == 26
        mine.flush()
        log.flush()
        a, b = mine.table(), log.table()
        assert len(a) > 0 and a.meta["dropped"] == 0 and np.array_equal(a.raw, b.raw) and (a.kind == cn.KIND_FLUSHED).any()
        assert a.meta["radius"] == 9.0 and (a.min_dist < 9.0).all()
        # the join with the trip log of the same env
        env.trip_log().flush()
        m = a.route_matrix(env.trip_log().table())
        assert m["all"].sum() > 0 and m["missing"] < 2 * len(a)
        # arguments make a new log, which replaces (and closes) the first
        new = env.conflict_log(max_rows=16)
        assert new is not mine and not mine._h.value and env.conflict_log() is new and new.n_records == 1
    finally:
        if log is not None:
            log.close()
        other.close()
        env.close()
    assert env.observer("conflict_log") is None
