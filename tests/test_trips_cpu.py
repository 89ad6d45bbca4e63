"""CPU: the restatement of the trip log (tests/trip_numpy.py) on the sequence worked out by hand, on two rollouts of the reference's CoPO
Intersection population on the CPU oracle with the premises the GPU comparison rests on, the overflow rule, `decode` / `summary` / `of` /
the `.npz` round trip of `TripTable`, and the library surface of `copo_trip_*` (exports, ctypes binding, NULL / DIM / CONFIG codes)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import interact_cases as ic
import interact_numpy as im
import trip_cases as tc
import trip_numpy as tn
from copo_amd import trips
from copo_amd.sim import SimConfig


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence_gives_the_rows_written_out_by_hand(N):
    """ARRIVE, CRASH that stays a WRECK, DONE with a new occupant in the same record, an agent-id change without DONE, an episode-word
    change, an EMPTY slot, no arrays in record 0, speed 300 / exactly `stop_speed` / one fp32 step below, NaN and +inf in gap and ttc,
    rew without ACTED, two closes in one scene and closes in two scenes of one record, `clear` in the middle, `flush` at the end; N = 64
    adds lane 63"""
    ref = tn.TripLog(tc.HAND_E, N, stop_speed=tc.STOP_SPEED)
    mid, end = tc.run_hand(ref, N, lambda r, *a: ref.record(*a), lambda: (ref.rows(), (ref.n_rows, ref.dropped)))
    before, after = tc.hand_expected(N)
    for (got, count), want in ((mid, before), (end, after)):
        assert count == (len(want), 0) and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want).tolist()
    assert ref.n_open() == 0 and ref.r == tc.HAND_RECORDS
    assert ref.scene_records_with_two_closes >= 2 and ref.records_with_closes_in_two_scenes >= 1 and ref.close_and_open_in_one_record >= 3
    d = trips.decode(after, 0.1)
    assert d["outcome"][:4].tolist() == ["arrive", "vanished", "vanished", "maxstep"] and (d["outcome"][-1] == "open")
    assert d["max_speed"][0] == 255.0 and d["stop_frac"][0] == 0.25 and d["min_gap"][0] == 3.0 and d["min_ttc"][0] == 2.0
    assert trips.decode(before, 0.1)["outcome"].tolist() == ["crash", "out", "vanished"] + ["arrive"] * (len(before) - 3)


def _oracle_rollout(golden_dir, cfg, steps, logs, reset_after=None, meter=False):
    """records of a rollout on the CPU oracle into every restatement of `logs`; returns the records made"""
    import oracle_lib as ol
    o = ol.OracleSim(cfg)
    P = im.Params.of(cfg)
    try:
        act = ic.rollout_policy(golden_dir)

        def record(out):
            st, env = o.get_state()
            kw = {} if out is None else dict(flags=out["flags"], rew=out["rew"])
            if meter:
                gap, ttc, _, _ = im.measure(st, P)
                kw.update(gap=gap.astype(np.float32), ttc=ttc.astype(np.float32))
            for log in logs:
                log.record(st, env, **kw)
        out = o.reset()
        record(None)
        for t in range(steps):
            out = o.step(act(out["obs"]))
            record(out)
            if reset_after is not None and t + 1 == reset_after:
                out = o.reset(tc.short_seeds(o.E))
                record(None)
    finally:
        o.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    cfg = tc.rollout_config()
    full, small = tn.TripLog(cfg.num_envs, 40), tn.TripLog(cfg.num_envs, 40, max_rows=64)
    _oracle_rollout(golden_dir, cfg, tc.ROLLOUT_STEPS, (full, small))
    return full, small


@pytest.fixture(scope="module")
def short_rollout(golden_dir):
    cfg = tc.short_config()
    ref = tn.TripLog(cfg.num_envs, cfg.num_agents)
    _oracle_rollout(golden_dir, cfg, tc.SHORT_STEPS, (ref,), reset_after=tc.SHORT_RESET_AFTER, meter=True)
    return ref


def test_rollout_invariants_and_premises(rollout):
    ref, _ = rollout
    tc.check_invariants(ref)
    d = trips.decode(ref.rows(), 0.1)
    counts = {k: int((d["outcome"] == k).sum()) for k in trips.OUTCOMES}
    print("rows %d %s; scene-records with two closes %d, records with closes in two scenes %d, close and open in one record %d, still open %d"
          % (ref.n_rows, counts, ref.scene_records_with_two_closes, ref.records_with_closes_in_two_scenes, ref.close_and_open_in_one_record, ref.n_open()))
    # the premises of the GPU comparison: without them it could pass vacuously
    assert counts["arrive"] >= 1 and counts["crash"] >= 1 and counts["out"] >= 1
    assert ref.scene_records_with_two_closes >= 1 and ref.records_with_closes_in_two_scenes >= 1
    # what the oracle gives for this case
    assert (ref.n_rows, counts["arrive"], counts["crash"], counts["out"]) == (120, 58, 28, 34) and ref.dropped == 0 and ref.r == tc.ROLLOUT_STEPS + 1
    assert (ref.scene_records_with_two_closes, ref.records_with_closes_in_two_scenes) == (19, 21)
    assert (d["kind"] == tn.KIND_DONE).all() and (d["distance"][d["outcome"] == "arrive"] > 50.0).all() and (d["mean_speed"] > 0.5).all()
    assert set(np.unique(d["route"]).tolist()) <= set(range(SimConfig(map="intersection").tables().n_routes)) and len(np.unique(d["route"])) > 4
    assert ((d["lcf"] >= -1.0) & (d["lcf"] <= 1.0)).all() and len(np.unique(d["lcf"])) > 50


def test_short_rollout_has_maxstep_env_reset_vanished_and_a_finite_ttc(short_rollout):
    ref = short_rollout
    tc.check_invariants(ref, resets_by_hand=(tc.SHORT_RESET_AFTER + 1,))
    d = trips.decode(ref.rows(), 0.1)
    print("rows %d, kinds %s, outcomes %s, ENV_RESET rows %d, finite min_ttc %d, finite min_gap %d"
          % (ref.n_rows, np.bincount(d["kind"], minlength=4).tolist(), {k: int((d["outcome"] == k).sum()) for k in trips.OUTCOMES},
             int(((d["flags"] & trips.F_ENV_RESET) != 0).sum()), int(np.isfinite(d["min_ttc"]).sum()), int(np.isfinite(d["min_gap"]).sum())))
    assert (d["outcome"] == "maxstep").sum() >= 1 and ((d["flags"] & trips.F_ENV_RESET) != 0).sum() >= 1
    assert (d["kind"] == tn.KIND_VANISHED).sum() >= 1 and ((d["kind"] == tn.KIND_VANISHED) == (d["outcome"] == "vanished")).all()
    assert np.isfinite(d["min_ttc"]).sum() >= 1 and np.isfinite(d["min_gap"]).sum() >= 1
    # a reset by hand ends every trip that was open, and only by kind 2: their last step is the record before it
    van = d["kind"] == tn.KIND_VANISHED
    assert ((d["first_rec"] + d["steps"])[van] == tc.SHORT_RESET_AFTER + 1).all() and (d["flags"][van] == 0).all()
    assert (d["steps"][d["outcome"] == "maxstep"] <= tc.SHORT_HORIZON + 1).all()


def test_overflow_keeps_the_first_rows_and_counts_the_rest(rollout):
    full, small = rollout
    assert small.n_rows == 64 and small.dropped == full.n_rows - 64 > 0 and np.array_equal(small.rows(), full.rows()[:64])
    assert small.total_closed == full.total_closed and small.n_open() == full.n_open()      # a dropped trip is closed all the same


def _table():
    """twelve rows by hand: the hand sequence's rows after the flush"""
    _, after = tc.hand_expected(7)
    return trips.TripTable(after, trips.trip_meta(SimConfig(map="roundabout", num_envs=4, num_agents=7), 7, 100, tc.STOP_SPEED, dropped=3, n_records=8))


def test_decode_columns():
    t = _table()
    assert len(t) == 12 and set(t.columns) == set(trips.RAW) | set(trips.DERIVED) | {"outcome"}
    assert t.scene.tolist() == [0, 2, 1, 1, 0, 0, 0, 0, 1, 1, 2, 3] and t.slot.tolist() == [0, 6, 0, 1, 2, 3, 5, 6, 0, 1, 0, 3]
    assert t.aid.tolist() == [10, 36, 20, 21, 17, 18, 15, 16, 20, 22, 31, 40] and t.route.tolist() == [a % 5 + 1 for a in t.aid.tolist()]
    assert t.episode.tolist() == [0, 7, 0, 0, 0, 0, 0, 0, 1, 1, 7, 0] and t.kind.tolist() == [1, 2, 2, 1] + [3] * 8
    assert t.outcome.tolist() == ["arrive", "vanished", "vanished", "maxstep"] + ["open"] * 8 and t["flags"][3] == 0xE3
    assert np.array_equal(t.lcf, t.aid / 64.0) and t.distance.tolist() == [3.0, 2.0, 4.0, 4.0, 4.0, 4.0, 7.0, 7.0, 2.0, 2.0, 1.0, 7.0]
    assert np.allclose(t.duration_s, t.steps * 0.1) and t.mean_speed[0] == 68096 / 256.0 / 4 and t.mean_speed[-1] == 4.5 and t.max_speed[-1] == 8.0
    assert t.stop_frac[7] == 7 / 8 and t.reward[0] == 3.75 and t.min_gap[6] == 6.5 and np.isinf(t.min_ttc[6]) and t.min_ttc[-1] == 0.0
    assert np.signbit(t.min_gap[-1]) and t.min_gap[-1] == 0.0
    # precedence arrive > out > crash > maxstep, and the kinds
    mk = lambda end, kind: [0, 0, 0, 0, 0, 1, end | (kind << 8)] + [0] * 9      # noqa: E731
    raw = np.array([mk(0x02 | b, 1) for b in (0x04 | 0x10 | 0x08, 0x10 | 0x08 | 0x20, 0x08 | 0x20, 0x20, 0x00)] + [mk(0, 2), mk(0, 3)], np.uint32)
    assert trips.decode(raw, 0.1)["outcome"].tolist() == ["arrive", "out", "crash", "maxstep", "vanished", "vanished", "open"]
    assert len(trips.decode(np.zeros((0, 16), np.uint32), 0.1)["outcome"]) == 0
    f = t.frame()
    assert len(f) == 12 and list(f.columns) == list(trips.RAW + ("outcome",) + trips.DERIVED) and f["aid"].tolist() == t.aid.tolist()


def test_summary_of_and_npz_round_trip(tmp_path):
    t = _table()
    by = {r["bucket"]: r for r in t.summary("outcome")}
    assert list(by) == ["arrive", "maxstep", "vanished", "open"] and [by[k]["count"] for k in by] == [1, 1, 2, 8]
    assert by["arrive"]["success_rate"] == 1.0 and by["open"]["success_rate"] == 0.0 and by["vanished"]["distance"] == 3.0
    assert by["arrive"]["min_ttc"] == 2.0 and np.isnan(by["vanished"]["min_ttc"]) and by["open"]["min_gap"] == (6.5 + 0.0) / 2
    assert [(r["bucket"], r["count"]) for r in t.summary("scene")] == [(0, 5), (1, 4), (2, 2), (3, 1)]
    routes = t.summary("route")
    assert [r["bucket"] for r in routes] == [1, 2, 3, 4] and sum(r["count"] for r in routes) == 12 and routes[0]["success_rate"] == 1 / 5
    bins = t.summary([0.0, 0.25, 0.5, 1.0])       # lcf = aid / 64: 10, 15 | 16 .. 31 | 36, 40 (the last bin is closed)
    assert [r["count"] for r in bins] == [2, 8, 2] and bins[0]["bucket"] == (0.0, 0.25) and bins[0]["success_rate"] == 0.5
    assert t.summary([0.5, 0.625])[0]["count"] == 2 and "arrive" in t.text("outcome")
    with pytest.raises(ValueError):
        t.summary("colour")
    with pytest.raises(ValueError):
        t.summary([1.0, 0.0])
    # the join with a clip header: (scene, trig_aid, episode)
    assert t.of(1, 20, 0).tolist() == [2] and t.of(1, 20, 1).tolist() == [8] and t.of(1, 20, 2).tolist() == [] and t.of(0, 20, 0).tolist() == []
    path = t.save(str(tmp_path / "trips.npz"))
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["meta", "rows"] and f["rows"].dtype == np.uint32
    back = trips.TripTable.load(path)
    assert np.array_equal(back.raw, t.raw) and back.meta == t.meta and back.meta["dropped"] == 3
    assert SimConfig(**back.meta["sim_config"]).map == "roundabout" and back.meta["sim_config"] == dataclasses.asdict(SimConfig(map="roundabout", num_envs=4, num_agents=7))
    for k in trips.RAW + trips.DERIVED + ("outcome",):
        assert np.array_equal(back[k], t[k]), k


def test_library_exports_and_binds_the_trip_entries():
    from copo_amd import _capi
    names = ["copo_trip_create", "copo_trip_record", "copo_trip_flush", "copo_trip_count", "copo_trip_read", "copo_trip_clear", "copo_trip_reset",
             "copo_trip_destroy"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    assert C.sizeof(_capi.TripCfg) == 8 and [f[0] for f in _capi.TripCfg._fields_] == ["max_rows", "stop_speed"]
    assert (_capi.TRIP_WORDS, _capi.TRIP_DONE, _capi.TRIP_VANISHED, _capi.TRIP_FLUSHED) == (tn.WORDS, tn.KIND_DONE, tn.KIND_VANISHED, tn.KIND_FLUSHED)
    assert len(trips.ROW_KEYS) == trips.WORDS == 16
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    # NULL arguments are refused before any device call
    lib, h, cfg = _capi.lib, C.c_void_p(), _capi.TripCfg(16, 0.5)
    assert lib.copo_trip_create(None, C.byref(cfg), C.byref(h)) == -1 and b"copo_trip_create" in lib.copo_last_error()
    out = (C.c_int64 * 2)()
    for fn, args in (("copo_trip_record", (None,) * 6), ("copo_trip_flush", (None, None)), ("copo_trip_count", (None, out, None)),
                     ("copo_trip_read", (None, 0, 0, None, None)), ("copo_trip_clear", (None, None)), ("copo_trip_reset", (None, None)),
                     ("copo_trip_destroy", (None,))):
        assert getattr(lib, fn)(*args) == -1 and fn.encode() in lib.copo_last_error(), fn
    # the configuration is checked before any device call as well: a handle that is not NULL is enough to get there
    fake = C.create_string_buffer(1 << 16)
    for bad, code in ((_capi.TripCfg(0, 0.5), -2), (_capi.TripCfg(-5, 0.5), -2), (_capi.TripCfg(16, -0.5), -5), (_capi.TripCfg(16, float("nan")), -5),
                      (_capi.TripCfg(16, float("inf")), -5)):
        assert lib.copo_trip_create(C.cast(fake, C.c_void_p), C.byref(bad), C.byref(h)) == code and b"copo_trip_create" in lib.copo_last_error(), (bad.max_rows, bad.stop_speed)
        assert not h.value
    assert lib.copo_trip_create(C.cast(fake, C.c_void_p), None, C.byref(h)) == -1
