"""Trip log on the GPU (copo_trip_*, copo_amd/trips.py) against the restatement of its rules (tests/trip_numpy.py): the sequence worked out
by hand at 7 and 64 slots, two rollouts of the reference's CoPO population (one fed by the interaction meter, one with a small horizon
and a reset by hand), the launch shapes, overflow with `clear` / `drain`, `reset`, repeatability and no effect on the simulation, the
argument checks, close after the simulator, the dict env and the `.npz` file.  Every comparison is on raw 32-bit words and exact."""
import ctypes as C

import numpy as np
import pytest

import interact_cases as ic
import trip_cases as tc
import trip_numpy as tn
from rowlog_gpu import Both, _dev, _np_state, _read, _set_state, _sim64
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence(N):
    """E = 4: one workgroup.  The rows are the ones tests/trip_cases.py writes out by hand; the restatement runs next to the device"""
    from copo_amd.trips import TripLog
    sim = _sim64(tc.HAND_E, N)
    log = TripLog(sim, max_rows=64, stop_speed=tc.STOP_SPEED)
    ref = tn.TripLog(tc.HAND_E, N, max_rows=64, stop_speed=tc.STOP_SPEED)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)

        def record(r, st, env, flags, rew, gap, ttc):
            _set_state(sim, st, env)
            log.record(_dev(flags), _dev(rew), _dev(gap), _dev(ttc))
            ref.record(st, env, flags, rew, gap, ttc)
            tn.compare(*_read(log), ref)
        mid, end = tc.run_hand(Both(log, ref), N, record, lambda: _read(log), st0, env0)
        before, after = tc.hand_expected(N)
        for (got, count), want in ((mid, before), (end, after)):
            assert count == (len(want), 0) and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want).tolist()
        tn.compare(*_read(log), ref)
        assert log.n_records == tc.HAND_RECORDS
        log.flush()                                      # nothing stayed open
        assert log.count() == (len(after), 0)
    finally:
        log.close()
        sim.close()


def _rollout(golden_dir, cfg, steps, with_log=True, with_ref=False, meter=False, reset_after=None, max_rows=65536, clear_after=None):
    """A rollout of the reference's population with a `TripLog` next to it.  Returns (rows, count, the restatement, a trace of the step
    outputs, the final state, what `drain` gave at `clear_after`)."""
    import torch
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import VecSim
    from copo_amd.trips import TripLog
    sim = VecSim(cfg)
    log = m = ref = drained = None
    act = ic.rollout_policy(golden_dir)
    try:
        if with_log:
            log = TripLog(sim, max_rows=max_rows)
        if meter:
            m = InteractionMeter(sim)
        if with_ref:
            ref = tn.TripLog(sim.E, sim.N, max_rows=max_rows)

        def record(out):
            flags, rew = (None, None) if out is None else (out["flags"], out["rew"])
            gap, ttc = m.record() if m is not None else (None, None)
            if with_log:
                before = [x.clone() for x in sim.get_state()] if with_ref and log.n_records == 3 else None
                log.record(flags, rew, gap, ttc)
                if before is not None:       # simulator memory is only read
                    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, sim.get_state()))
            if with_ref:
                ref.record(*_np_state(sim), *(None if x is None else x.cpu().numpy() for x in (flags, rew, gap, ttc)))
        out = sim.reset()
        record(None)
        trace = []
        for t in range(steps):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            record(out)
            trace.append(int(out["flags"].to(torch.int64).sum()) * 31 + int(out["rew"].view(torch.int32).to(torch.int64).sum()))
            if reset_after is not None and t + 1 == reset_after:
                out = sim.reset(tc.short_seeds(sim.E))
                record(None)
            if clear_after is not None and t + 1 == clear_after:
                drained = log.drain()
                if with_ref:
                    tn.compare(drained.raw, (len(drained), drained.meta["dropped"]), ref)
                    ref.clear()
        final = [x.cpu().numpy().view(np.int32).copy() for x in sim.get_state()]
        rows, count = _read(log) if with_log else (None, None)
        return rows, count, ref, trace, final, drained
    finally:
        for h in (log, m):
            if h is not None:
                h.close()
        sim.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    return _rollout(golden_dir, tc.rollout_config(), tc.ROLLOUT_STEPS, with_ref=True, meter=True)


def test_rollout_against_the_restatement(rollout):
    from copo_amd import trips
    rows, count, ref, _, _, _ = rollout
    tn.compare(rows, count, ref)
    tc.check_invariants(ref)
    d = trips.decode(rows, 0.1)
    counts = {k: int((d["outcome"] == k).sum()) for k in trips.OUTCOMES}
    print("rows %s %s; scene-records with two closes %d, records with closes in two scenes %d; finite min_ttc %d, min_gap %d"
          % (count, counts, ref.scene_records_with_two_closes, ref.records_with_closes_in_two_scenes, int(np.isfinite(d["min_ttc"]).sum()),
             int(np.isfinite(d["min_gap"]).sum())))
    assert count == (120, 0) and (counts["arrive"], counts["crash"], counts["out"]) == (58, 28, 34)
    assert ref.scene_records_with_two_closes >= 1 and ref.records_with_closes_in_two_scenes >= 1
    assert np.isfinite(d["min_ttc"]).sum() >= 1 and np.isfinite(d["min_gap"]).sum() >= 100 and (d["reward"] != 0).any()


def test_short_rollout_with_a_reset_by_hand_against_the_restatement(golden_dir):
    from copo_amd import trips
    rows, count, ref, _, _, _ = _rollout(golden_dir, tc.short_config(), tc.SHORT_STEPS, with_ref=True, reset_after=tc.SHORT_RESET_AFTER)
    tn.compare(rows, count, ref)
    tc.check_invariants(ref, resets_by_hand=(tc.SHORT_RESET_AFTER + 1,))
    d = trips.decode(rows, 0.1)
    print("rows %s kinds %s ENV_RESET rows %d" % (count, np.bincount(d["kind"], minlength=4).tolist(), int(((d["flags"] & trips.F_ENV_RESET) != 0).sum())))
    assert (d["outcome"] == "maxstep").sum() >= 1 and ((d["flags"] & trips.F_ENV_RESET) != 0).sum() >= 1 and (d["kind"] == tn.KIND_VANISHED).sum() >= 1
    assert np.isinf(d["min_ttc"]).all()                  # never fed


def test_two_identical_runs_give_identical_bits_and_recording_does_not_perturb(golden_dir, rollout):
    short = 60
    cfg = tc.rollout_config()
    a = _rollout(golden_dir, cfg, short, meter=True)
    b = _rollout(golden_dir, cfg, short, meter=True)
    plain = _rollout(golden_dir, cfg, short, with_log=False)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1][0] > 0
    assert np.array_equal(a[0], rollout[0][:a[1][0]])    # (rows come in the order of their close record)
    assert a[3] == b[3] == plain[3] == rollout[3][:short] and all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[4], b[4], plain[4]))


def test_overflow_clear_and_drain_mid_run(golden_dir, rollout):
    """a pool of 64 rows on the 120-row rollout: the first 64 unchanged, the rest counted; a pool of 80 with a `drain` after step 120 (41
    rows by then on the CPU oracle, 79 after) loses nothing"""
    rows, count, _, _, _, _ = _rollout(golden_dir, tc.rollout_config(), tc.ROLLOUT_STEPS, meter=True, max_rows=64)
    full = rollout[0]
    assert count == (64, len(full) - 64) and np.array_equal(rows, full[:64])
    rows, count, ref, _, _, drained = _rollout(golden_dir, tc.rollout_config(), tc.ROLLOUT_STEPS, with_ref=True, meter=True, max_rows=80, clear_after=120)
    tn.compare(rows, count, ref)
    n = len(drained)
    print("drained %d rows after step 120 (dropped %d), %s after" % (n, drained.meta["dropped"], count))
    assert 0 < n <= 80 and drained.meta["dropped"] == 0 and count[1] == 0 and n + count[0] == len(full)
    assert np.array_equal(np.concatenate([drained.raw, rows]), full)      # trips open at the drain arrive later with their full history


@pytest.mark.parametrize("E", [1, 3, 1030])
def test_launch_shapes(E):
    """Synthetic states at 64 slots: one partial workgroup (1, 3 scenes) and 258 workgroups with a partial last one (1 030 scenes: the assign
    walk takes a second pass of its 1 024 threads).  Three records; in the last EVERY open trip ends (a cause drawn at random, half of
    the slots taken over at once), so the order of some forty rows per scene is decided by the prefix alone.  At 1 030 scenes the pool is
    smaller than the rows, so the overflow falls inside a scene."""
    from copo_amd.trips import TripLog
    N = 64
    sim = _sim64(E, N)
    rng = np.random.RandomState(E)
    status = rng.choice([tn.ST_ALIVE, tn.ST_WRECK, tn.ST_EMPTY], p=[0.65, 0.15, 0.2], size=(E, N))
    alive = status == tn.ST_ALIVE
    max_rows = int(alive.sum()) + 7 if E < 1000 else int(alive.sum()) - 1000 - 13
    log = TripLog(sim, max_rows=max_rows, stop_speed=1.0)
    ref = tn.TripLog(E, N, max_rows=max_rows, stop_speed=1.0)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        aid = rng.randint(0, 5000, (E, N))
        for r in range(3):
            st, env = st0.copy(), env0.copy()
            su = st.view(np.uint32)
            flags = np.where(alive, tn.F_ACTED, 0).astype(np.uint8)
            if r == 2:
                flags = np.where(alive, tn.F_ACTED | tn.F_DONE | rng.choice([tn.F_ARRIVE, tn.F_CRASH, tn.F_OUT, tn.F_MAXSTEP], size=(E, N)), 0).astype(np.uint8)
                taken = alive & (rng.rand(E, N) < 0.5)
                status, aid = np.where(alive, np.where(taken, tn.ST_ALIVE, tn.ST_EMPTY), status), np.where(taken, aid + 5000, aid)
                flags |= np.where(taken, tn.F_SPAWNED, 0).astype(np.uint8)
            st[3] = rng.uniform(-1.0, 20.0, (E, N)).astype(np.float32)
            st[9], st[10] = rng.uniform(0.0, 200.0, (E, N)), rng.uniform(-1.0, 1.0, (E, N))
            su[12] = rng.randint(0, 12, (E, N)) | (rng.randint(0, 9, (E, N)) << 16)
            su[13] = (su[13] & ~np.uint32(0xFF)) | status.astype(np.uint32)
            su[14] = aid.astype(np.uint32)
            rew = rng.uniform(-1.0, 1.0, (E, N)).astype(np.float32)
            gap, ttc = rng.uniform(0.0, 30.0, (E, N)).astype(np.float32), np.where(rng.rand(E, N) < 0.5, np.inf, rng.uniform(0.0, 6.0, (E, N))).astype(np.float32)
            _set_state(sim, st, env)
            args = (None,) * 4 if r == 0 else (flags, rew, gap, ttc)
            log.record(*(_dev(x) for x in args))
            ref.record(st, env, *args)
        rows, count = _read(log)
        tn.compare(rows, count, ref)
        print("E %d: %d rows, %d dropped, %d trips open" % (E, count[0], count[1], ref.n_open()))
        assert ref.total_closed == int(alive.sum()) > 0 and count[0] == min(max_rows, ref.total_closed) and (count[1] > 0) == (E > 1000)
        assert ref.n_open() > 0 or E == 1
        log.flush()
        ref.flush()
        tn.compare(*_read(log), ref)
    finally:
        log.close()
        sim.close()


def test_reset_refused_arguments_and_close_after_the_simulator():
    import torch
    from copo_amd import _capi
    from copo_amd.sim import VecSim
    from copo_amd.trips import TripLog
    lib = _capi.lib
    N = 7
    sim = VecSim(SimConfig(map="intersection", num_envs=tc.HAND_E, num_agents=N))
    h = C.c_void_p()
    log = None
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        for cfg, code in ((_capi.TripCfg(0, 0.5), -2), (_capi.TripCfg(-1, 0.5), -2), (_capi.TripCfg(8, -1.0), -5), (_capi.TripCfg(8, float("nan")), -5),
                          (_capi.TripCfg(8, float("inf")), -5)):
            assert lib.copo_trip_create(sim._h, C.byref(cfg), C.byref(h)) == code and b"copo_trip_create" in lib.copo_last_error() and not h.value
        assert lib.copo_trip_create(sim._h, None, C.byref(h)) == -1 and lib.copo_trip_create(sim._h, C.byref(_capi.TripCfg(8, 0.5)), None) == -1
        with pytest.raises(_capi.CopoError):
            TripLog(sim, max_rows=0)
        log = TripLog(sim, max_rows=64, stop_speed=tc.STOP_SPEED)
        stream = _capi.current_stream()

        def run(upto, first=0):
            for r in range(first, upto):
                st, env, *arrays = tc.hand_record(st0, env0, r)
                _set_state(sim, st, env)
                log.record(*(_dev(x) for x in arrays))
        run(4)
        before = _read(log)
        assert before[1] == (4, 0) and np.array_equal(before[0], tc.hand_expected(N)[0])
        # refused calls launch nothing and leave the handle usable
        out = torch.empty(65, 16, dtype=torch.int32, device="cuda")
        for first, n in ((0, 65), (64, 1), (-1, 1), (0, -1), (2 ** 31 - 1, 2)):
            assert lib.copo_trip_read(log._h, first, n, out.data_ptr(), stream) == -2 and b"copo_trip_read" in lib.copo_last_error()
        assert lib.copo_trip_read(log._h, 0, 4, None, stream) == -1 and lib.copo_trip_count(log._h, None, stream) == -1
        assert lib.copo_trip_read(log._h, 0, 0, None, stream) == 0 and lib.copo_trip_read(log._h, 60, 4, out.data_ptr(), stream) == 0
        E = tc.HAND_E
        for bad in (dict(flags=torch.zeros(E, N, dtype=torch.int32, device="cuda")), dict(rew=torch.zeros(E, N, dtype=torch.float64, device="cuda")),
                    dict(gap=torch.zeros(E, N + 1, device="cuda")), dict(ttc=torch.zeros(E, N)), dict(rew=torch.zeros(N, E, device="cuda").t())):
            with pytest.raises(ValueError):
                log.record(**bad)
        after = _read(log)
        assert after[1] == before[1] and np.array_equal(after[0], before[0]) and log.n_records == 4
        # reset: every row, counter and open trip is gone and records count from 0: the hand sequence gives its rows again
        log.reset()
        assert log.count() == (0, 0) and log.n_records == 0
        log.flush()
        assert log.count() == (0, 0)                     # nothing was open
        run(4)
        again = _read(log)
        assert again[1] == (4, 0) and np.array_equal(again[0], before[0])
        log.clear()
        run(tc.HAND_RECORDS, first=4)
        log.flush()
        rows, count = _read(log)
        assert count == (12, 0) and np.array_equal(rows, tc.hand_expected(N)[1])
        t = log.table()
        assert len(t) == 12 and t.meta["n_records"] == tc.HAND_RECORDS and t.meta["dt"] == float(sim.cfg.dt) and t.outcome[0] == "arrive"
        out = sim.step(torch.zeros(tc.HAND_E, sim.N, 2, device="cuda"))
        assert torch.isfinite(out["rew"]).all()
        # the simulator goes first
        sim.close()
        log.close()
        log.close()                                      # closing twice is harmless
    finally:
        if log is not None:
            log.close()
        sim.close()


def test_dict_env_key_and_file(tmp_path):
    """The env with `trip_log` and `interaction_metrics` on for 30 steps at 2 scenes against a hand-driven `TripLog` and meter on the same
    seeds; then the one-scene dict API."""
    import torch
    from copo_amd.interact import InteractionMeter
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    from copo_amd.trips import TripLog, TripTable
    assert MultiAgentIntersectionEnv.default_config()["trip_log"] is None
    env = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2, interaction_metrics=True, trip_log=dict(max_rows=512, stop_speed=1.0)))
    other = MultiAgentIntersectionEnv(dict(num_agents=20, num_envs=2))
    log, meter = TripLog(other.sim, max_rows=512, stop_speed=1.0), InteractionMeter(other.sim)
    try:
        with pytest.raises(AssertionError):
            other.trip_log()
        act = torch.zeros(2, env.sim.N, 2, device="cuda")
        act[..., 1] = torch.linspace(0.3, 1.0, env.sim.N, device="cuda")
        mine = env.trip_log()
        for k in range(2):                               # the rows are kept over a reset by hand
            env.vec_reset()
            other.vec_reset()
            log.record(None, None, *meter.record())
            for _ in range(15):
                env.vec_step(act)
                out = other.vec_step(act)
                log.record(out["flags"], out["rew"], *meter.record())
            # a reset with the same seeds gives every slot its agent id and episode word again, which continues the trips: whoever wants
            # them cut at a reset by hand flushes first
            mine.flush()
            log.flush()
            assert mine.count() == log.count() and mine.count()[0] >= 40 * (k + 1)      # all 40 slots drive after a reset
        assert mine.n_records == 32
        a, b = mine.table(), log.table()
        assert np.array_equal(a.raw, b.raw) and (a.kind == 3).sum() >= 40 and np.isfinite(a.min_gap).all()
        assert set(a.first_rec[a.kind == 3].tolist()) >= {0, 16} and (a.first_rec + a.steps <= 32).all()
        path = a.save(str(tmp_path / "trips.npz"))
        back = TripTable.load(path)
        assert np.array_equal(back.raw, a.raw) and back.meta["stop_speed"] == 1.0 and back.meta["n_records"] == 32 and back.meta["num_agents"] == 20
        assert back.meta["sim_config"]["map"] == "intersection" and np.array_equal(back.mean_speed, a.mean_speed, equal_nan=True)
        assert back.summary("outcome")[-1]["bucket"] == "open" and len(back.of(int(a.scene[0]), int(a.aid[0]), int(a.episode[0]))) >= 1
    finally:
        log.close()
        meter.close()
        other.close()
        env.close()
    one = MultiAgentIntersectionEnv(dict(num_agents=8, trip_log={}))
    try:
        o, ended = one.reset(), 0
        for _ in range(5):
            o, _, d, _ = one.step({a: np.array([0.0, 1.0], np.float32) for a in o})
            ended += sum(1 for k, v in d.items() if k != "__all__" and v)
        one.trip_log().flush()
        t = one.trip_log().table()
        assert len(t) >= 8 and (t.first_rec + t.steps <= 6).all() and (t.kind == 1).sum() == ended and np.isinf(t.min_ttc).all()
    finally:
        one.close()
    assert one.observer("trip_log") is None
