"""CPU: the restatement of the conflict log (tests/conflict_numpy.py) on the sequence worked out by hand, on two rollouts of the reference's
CoPO Intersection population on the CPU oracle with the premises the GPU comparison rests on, the overflow rule, `decode` on hand poses,
`route_matrix` against a hand-made `TripTable`, `summary` / `of` / the `.npz` round trip of `ConflictTable`, `ObserverList.add` with fakes
and the library surface of `copo_conflict_*` (exports, ctypes binding, NULL / DIM / CONFIG codes)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import conflict_cases as cc
import conflict_numpy as cn
import interact_cases as ic
from copo_amd import conflicts, trips
from copo_amd.sim import SimConfig

HL, HW = 2.0, 1.0      # of the decode cases: exact in binary


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence_gives_the_rows_written_out_by_hand(N):
    """a pair that parts at exactly `leave_radius` and stays one fp32 step below, does not open at exactly `radius` and opens one step below,
    stays open between the radii but does not open there; DONE on one party, on both with CRASH, with a new occupant that opens a new
    encounter in the same record; an agent-id change without DONE and an episode-word change; a NaN position; one slot in three
    encounters; two closes in one scene and closes in three scenes of one record; no flags in record 0; a tie of the minimum; `clear` in
    the middle, `flush` at the end; N = 64 adds pair (62, 63) and pair (1, 63)"""
    ref = cn.ConflictLog(cc.HAND_E, N, radius=cc.RADIUS, leave_radius=cc.LEAVE)
    mid, end = cc.run_hand(ref, N, lambda r, *a: ref.record(*a), lambda: (ref.rows(), (ref.n_rows, ref.dropped)))
    before, after = cc.hand_expected(N)
    for (got, count), want in ((mid, before), (end, after)):
        assert count == (len(want), 0) and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want).tolist()
    assert ref.n_open() == 0 and ref.r == cc.HAND_RECORDS
    assert ref.scene_records_with_two_closes >= 2 and ref.records_with_closes_in_two_scenes >= 1 and ref.close_and_open_in_one_record == 5
    assert ref.max_encounters_of_one_slot == 3
    cc.check_invariants(ref)
    d = conflicts.decode(before, 0.1, ic.HL, ic.HW)
    assert d["outcome"].tolist() == ["parted", "one_left", "vanished", "vanished", "parted", "both_crashed"]
    assert d["kind"].tolist() == [3, 1, 2, 2, 3, 1] and d["end_b"].tolist() == [0, 7, 0, 0, 0, 11] and d["end_a"].tolist() == [0, 0, 0, 0, 0, 11]
    assert d["min_dist"].tolist() == [3.0, 3.0, 7.0, 7.0, 2.0, 1.0] and d["min_off"].tolist() == [0, 0, 0, 0, 1, 1]
    d = conflicts.decode(after, 0.1, ic.HL, ic.HW)
    assert d["outcome"][:5].tolist() == ["parted", "one_left", "vanished", "vanished", "vanished"] and (d["outcome"][5:] == "open").all()
    assert d["min_dist"][0] == np.sqrt(np.float64(np.float32(cc.D2_BELOW_IN))) < 8.0 and d["steps"][0] == 3 and d["first_rec"][0] == 1


def _raw(pa, pb, kind=3, ends=(0, 0), d2=25.0, steps=4, min_off=2):
    b = cn.bits
    return [3, 1 | (5 << 6) | (kind << 12) | (ends[0] << 16) | (ends[1] << 24), 70, 71, 2, 9, steps | (min_off << 16), b(d2)] + [b(v) for v in pa + pb]


def test_decode_on_hand_poses():
    P = np.float32(np.pi)
    raw = np.array([
        _raw((0.0, 0.0, 0.0, 5.0), (5.0, 0.0, 0.0, 3.0)),                                  # following, b one metre ahead of a's bumper
        _raw((0.0, 0.0, 0.0, 5.0), (4.0, 0.0, 0.0, 5.0), d2=16.0),                         # bumper to bumper
        _raw((5.0, 0.0, 0.0, 3.0), (0.0, 0.0, 0.0, 5.0)),                                  # the same pair, a ahead
        _raw((0.0, 0.0, 0.0, 10.0), (10.0, -10.0, float(P / 2), 10.0), d2=200.0),          # perpendicular
        _raw((0.0, 0.0, 0.0, 5.0), (20.0, 0.0, float(P), 5.0), d2=400.0),                  # head on
        _raw((0.0, 0.0, 3.0, 1.0), (0.0, 9.0, -3.0, 1.0), d2=81.0),                        # -6 wraps to 2 pi - 6 = 16 degrees
    ], np.uint32)
    d = conflicts.decode(raw, 0.1, HL, HW)
    assert d["scene"].tolist() == [3] * 6 and d["slot_a"].tolist() == [1] * 6 and d["slot_b"].tolist() == [5] * 6 and d["kind"].tolist() == [3] * 6
    assert d["aid_a"].tolist() == [70] * 6 and d["aid_b"].tolist() == [71] * 6 and d["episode"].tolist() == [2] * 6 and d["first_rec"].tolist() == [9] * 6
    assert d["steps"].tolist() == [4] * 6 and d["min_off"].tolist() == [2] * 6 and np.allclose(d["duration_s"], 0.4)
    assert d["type"].tolist() == ["following", "following", "following", "crossing", "opposing", "following"]
    assert d["leader"].tolist() == ["b", "b", "a", "", "", "b"]      # (the last: a heads (cos 3, sin 3), b is 9 sin 3 = 1.27 m ahead along it)
    assert d["min_dist"][:3].tolist() == [5.0, 4.0, 5.0] and d["gap"][:3].tolist() == [1.0, 0.0, 1.0] and d["rel_speed"][:3].tolist() == [2.0, 0.0, 2.0]
    assert d["rel_heading"][:3].tolist() == [0.0, 0.0, 0.0]
    # the perpendicular pair: a covers [-2, 2] x [-1, 1], b (heading up) [9, 11] x [-12, -8]: the corners (2, -1) and (9, -8)
    assert abs(d["gap"][3] - np.hypot(7.0, 7.0)) < 1e-6 and abs(d["rel_heading"][3] - np.pi / 2) < 1e-7 and abs(d["rel_speed"][3] - np.hypot(10.0, 10.0)) < 1e-6
    assert abs(d["gap"][4] - 16.0) < 1e-6 and abs(abs(d["rel_heading"][4]) - np.pi) < 1e-6 and abs(d["rel_speed"][4] - 10.0) < 1e-6
    assert abs(d["rel_heading"][5] - (2 * np.pi - 6.0)) < 1e-12 and -np.pi < d["rel_heading"].min() and d["rel_heading"].max() <= np.pi
    # the boundaries: |rel| < 30 degrees is following, > 150 degrees opposing; the float32 headings next to them on either side
    for edge, inside, outside in ((np.pi / 6, "following", "crossing"), (5 * np.pi / 6, "crossing", "opposing")):
        lo = np.float32(edge)
        lo = lo if float(lo) < edge else np.nextafter(lo, np.float32(0))
        hi = np.nextafter(lo, np.float32(4))
        assert float(lo) < edge < float(hi)
        for sign in (1.0, -1.0):
            pair = np.array([_raw((0.0, 0.0, 0.0, 1.0), (6.0, 0.0, sign * float(h), 1.0)) for h in (lo, hi)], np.uint32)
            assert conflicts.decode(pair, 0.1, HL, HW)["type"].tolist() == [inside, outside], (edge, sign)
            pair = np.array([_raw((0.0, 0.0, -sign * float(h), 1.0), (6.0, 0.0, 0.0, 1.0)) for h in (lo, hi)], np.uint32)
            assert conflicts.decode(pair, 0.1, HL, HW)["type"].tolist() == [inside, outside], (edge, sign)
    # outcomes: the ends that carry CRASH decide among the kind-1 rows
    A, D, ARR, CR = cc.A, cc.D, cc.ARR, cc.CR
    p = ((0.0, 0.0, 0.0, 1.0), (6.0, 0.0, 0.0, 1.0))
    raw = np.array([_raw(*p, kind=1, ends=(A | D | CR, A | D | CR)), _raw(*p, kind=1, ends=(0, A | D | CR)), _raw(*p, kind=1, ends=(A | D | CR, A | D | ARR)),
                    _raw(*p, kind=1, ends=(A | D | ARR, 0)), _raw(*p, kind=2), _raw(*p, kind=3), _raw(*p, kind=4)], np.uint32)
    d = conflicts.decode(raw, 0.1, HL, HW)
    assert d["outcome"].tolist() == ["both_crashed", "one_crashed", "one_crashed", "one_left", "vanished", "parted", "open"]
    assert d["end_a"].tolist() == [11, 0, 11, 7, 0, 0, 0] and d["end_b"].tolist() == [11, 11, 7, 0, 0, 0, 0]
    assert len(conflicts.decode(np.zeros((0, 16), np.uint32), 0.1, HL, HW)["outcome"]) == 0
    assert len(conflicts.ROW_KEYS) == conflicts.WORDS == 16


def _tables():
    """the six rows of the hand sequence before its `clear`, and a hand-made trip table: (scene, aid, episode) -> route"""
    before, _ = cc.hand_expected(7)
    cfg = SimConfig(map="roundabout", num_envs=4, num_agents=7)
    t = conflicts.ConflictTable(before, conflicts.conflict_meta(cfg, 7, 100, cc.RADIUS, cc.LEAVE, dropped=3, n_records=4))
    who = [(0, 14, 0, 1), (0, 15, 0, 2), (1, 20, 0, 1), (1, 21, 0, 1), (2, 30, 7, 3), (2, 31, 7, 1), (1, 22, 0, 2), (1, 23, 0, 3), (3, 41, 0, 2),
           (2, 30, 8, 2), (0, 30, 7, 2)]          # (the last two: agent 30 in another episode and in another scene, which join nothing)
    raw = np.zeros((len(who), 16), np.uint32)
    for k, (scene, aid, ep, route) in enumerate(who):
        raw[k, :4] = scene, k % 7 | (route << 16), aid, ep
    return t, trips.TripTable(raw, dict(dt=0.1))


def test_route_matrix_against_a_hand_made_trip_table():
    t, tr = _tables()
    m = t.route_matrix(tr)
    # scene 0 (14, 15): routes 1-2; scene 1 (20, 21): 1-1; scene 2 (30, 31): 3-1; scene 2 (30, 33) and scene 3 (41, 44): agents 33 and 44 have
    # no trip; scene 1 (22, 23): 2-3, both crashed
    assert m["routes"] == [1, 2, 3] and m["missing"] == 2
    assert m["all"].tolist() == [[1, 1, 1], [1, 0, 1], [1, 1, 0]] and m["both_crashed"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]]
    empty = conflicts.ConflictTable(np.zeros((0, 16), np.uint32), t.meta).route_matrix(tr)
    assert empty["routes"] == [] and empty["all"].shape == (0, 0) and empty["missing"] == 0


def test_summary_of_and_npz_round_trip(tmp_path):
    t, _ = _tables()
    assert len(t) == 6 and set(t.columns) == set(conflicts.RAW) | set(conflicts.DERIVED) | {"type", "leader", "outcome", "pose_a", "pose_b"}
    by = {r["bucket"]: r for r in t.summary("outcome")}
    assert list(by) == ["both_crashed", "one_left", "parted", "vanished"] and [by[k]["count"] for k in by] == [1, 1, 2, 2]
    assert by["parted"]["min_dist"] == 2.5 and by["vanished"]["duration_s"] == pytest.approx(0.2) and by["parted"]["share"] == 2 / 6
    ty = t.summary("type")                         # headings differ by (slot_b - slot_a) / 8 rad: 7 to 21 degrees
    assert [(r["bucket"], r["count"]) for r in ty] == [("following", 6)] and "following" in t.text("type") and "parted" in t.text("outcome")
    with pytest.raises(ValueError):
        t.summary("colour")
    # the join with a clip header / a trip row: (scene, aid, episode), either party
    assert t.of(2, 30, 7).tolist() == [2, 3] and t.of(2, 33, 7).tolist() == [3] and t.of(2, 30, 8).tolist() == [] and t.of(0, 30, 7).tolist() == []
    assert t.of(1, 23, 0).tolist() == [5]
    path = t.save(str(tmp_path / "conflicts.npz"))
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["meta", "rows"] and f["rows"].dtype == np.uint32
    back = conflicts.ConflictTable.load(path)
    assert np.array_equal(back.raw, t.raw) and back.meta == t.meta and back.meta["dropped"] == 3 and back.meta["radius"] == 8.0
    assert back.meta["sim_config"] == dataclasses.asdict(SimConfig(map="roundabout", num_envs=4, num_agents=7))
    for k in t.columns:
        assert np.array_equal(back[k], t[k]), k
    f = t.frame()
    assert len(f) == 6 and list(f.columns) == list(conflicts.RAW + ("type", "leader", "outcome") + conflicts.DERIVED)


def test_observer_list_add_appends_and_replaces():
    from copo_amd import observers as ob
    log = []

    class Fake:
        def __init__(self, name):
            self.name = name

        def env_record(self, feed):
            log.append((self.name, "env_record", feed.flags))

        def close(self):
            log.append((self.name, "close", None))
    lst = ob.ObserverList("sim", {})
    first, a, b = Fake("first"), Fake("a"), Fake("b")
    lst.add("x", a)
    lst.add_first("renderer", first)
    lst.add("y", Fake("y"))
    assert lst.names() == ["renderer", "x", "y"] and lst.get("x") is a
    lst.after_step(dict(flags="F", rew="R"))
    assert log == [("first", "env_record", "F"), ("a", "env_record", "F"), ("y", "env_record", "F")]
    del log[:]
    lst.add("x", b)                                  # closes the one of that name; the new one goes to the end
    assert log == [("a", "close", None)] and lst.names() == ["renderer", "y", "x"] and lst.get("x") is b
    lst.close()
    assert sorted(n for n, c, _ in log if c == "close") == ["a", "b", "first", "y"]


def _oracle_rollout(golden_dir, cfg, steps, logs, reset_after=None):
    """records of a rollout on the CPU oracle into every restatement of `logs`"""
    import oracle_lib as ol
    o = ol.OracleSim(cfg)
    try:
        act = ic.rollout_policy(golden_dir)

        def record(out):
            st, env = o.get_state()
            for log in logs:
                log.record(st, env, None if out is None else out["flags"])
        out = o.reset()
        record(None)
        for t in range(steps):
            out = o.step(act(out["obs"]))
            record(out)
            if reset_after is not None and t + 1 == reset_after:
                out = o.reset(cc.short_seeds(o.E))
                record(None)
    finally:
        o.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    cfg = cc.rollout_config()
    full, small = cn.ConflictLog(cfg.num_envs, 40), cn.ConflictLog(cfg.num_envs, 40, max_rows=64)
    _oracle_rollout(golden_dir, cfg, cc.ROLLOUT_STEPS, (full, small))
    return full, small


def _counts(ref):
    d = conflicts.decode(ref.rows(), 0.1, ic.HL, ic.HW)
    return d, np.bincount(d["kind"], minlength=5).tolist(), {k: int((d["outcome"] == k).sum()) for k in conflicts.OUTCOMES}, \
        {k: int((d["type"] == k).sum()) for k in conflicts.TYPES}


def test_rollout_invariants_and_premises(rollout):
    ref, _ = rollout
    cc.check_invariants(ref)
    d, kinds, outcomes, types = _counts(ref)
    print("rows %d kinds %s %s %s; scene-records with two closes %d, records with closes in two scenes %d, close and open in one record %d, "
          "most encounters of one slot at once %d, still open %d"
          % (ref.n_rows, kinds, outcomes, types, ref.scene_records_with_two_closes, ref.records_with_closes_in_two_scenes, ref.close_and_open_in_one_record,
             ref.max_encounters_of_one_slot, ref.n_open()))
    # the premises of the GPU comparison: without them it could pass vacuously
    assert kinds[cn.KIND_DONE] >= 1 and kinds[cn.KIND_PARTED] >= 1 and outcomes["both_crashed"] >= 1
    assert ref.scene_records_with_two_closes >= 1 and ref.max_encounters_of_one_slot >= 2
    # what the oracle gives for this case at the default radii
    assert (ref.n_rows, kinds, ref.dropped, ref.r) == (ROLLOUT_ROWS, ROLLOUT_KINDS, 0, cc.ROLLOUT_STEPS + 1)
    assert (outcomes["both_crashed"], outcomes["one_crashed"], outcomes["one_left"], outcomes["parted"]) == ROLLOUT_OUTCOMES
    assert (ref.scene_records_with_two_closes, ref.records_with_closes_in_two_scenes, ref.max_encounters_of_one_slot) == ROLLOUT_ORDER
    assert (d["gap"] <= d["min_dist"]).all() and (d["min_dist"] < 8.0).all() and set(types) == set(conflicts.TYPES) and min(types.values()) >= 1


# observed on the CPU oracle
ROLLOUT_ROWS, ROLLOUT_KINDS, ROLLOUT_OUTCOMES, ROLLOUT_ORDER = 586, [0, 121, 0, 465, 0], (14, 21, 86, 465), (109, 134, 4)
SHORT_ROWS, SHORT_KINDS = 11, [0, 9, 2, 0, 0]


def test_short_rollout_with_a_reset_by_hand_has_vanished_rows(golden_dir):
    cfg = cc.short_config()
    ref = cn.ConflictLog(cfg.num_envs, cfg.num_agents)
    _oracle_rollout(golden_dir, cfg, cc.SHORT_STEPS, (ref,), reset_after=cc.SHORT_RESET_AFTER)
    cc.check_invariants(ref)
    d, kinds, outcomes, _ = _counts(ref)
    print("rows %d kinds %s %s" % (ref.n_rows, kinds, outcomes))
    assert kinds[cn.KIND_VANISHED] >= 1 and kinds[cn.KIND_DONE] >= 1
    assert (ref.n_rows, kinds) == (SHORT_ROWS, SHORT_KINDS)
    # the reset by hand ends every encounter that was open, by kind 2 (the scenes' own resets come with DONE flags: kind 1)
    van = d["kind"] == cn.KIND_VANISHED
    assert ((d["first_rec"] + d["steps"])[van] == cc.SHORT_RESET_AFTER + 1).all() and (d["end_a"][van] == 0).all()


def test_overflow_keeps_the_first_rows_and_counts_the_rest(rollout):
    full, small = rollout
    assert small.n_rows == 64 and small.dropped == full.n_rows - 64 > 0 and np.array_equal(small.rows(), full.rows()[:64])
    assert small.total_closed == full.total_closed and small.n_open() == full.n_open()      # a dropped encounter is closed all the same


def test_library_exports_and_binds_the_conflict_entries():
    from copo_amd import _capi
    names = ["copo_conflict_create", "copo_conflict_record", "copo_conflict_flush", "copo_conflict_count", "copo_conflict_read", "copo_conflict_clear",
             "copo_conflict_reset", "copo_conflict_destroy"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    assert C.sizeof(_capi.ConflictCfg) == 12 and [f[0] for f in _capi.ConflictCfg._fields_] == ["max_rows", "radius", "leave_radius"]
    assert (_capi.CONFLICT_WORDS, _capi.CONFLICT_DONE, _capi.CONFLICT_VANISHED, _capi.CONFLICT_PARTED, _capi.CONFLICT_FLUSHED) == \
        (cn.WORDS, cn.KIND_DONE, cn.KIND_VANISHED, cn.KIND_PARTED, cn.KIND_FLUSHED)
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    # NULL arguments are refused before any device call
    lib, h, cfg = _capi.lib, C.c_void_p(), _capi.ConflictCfg(16, 8.0, 10.0)
    assert lib.copo_conflict_create(None, C.byref(cfg), C.byref(h)) == -1 and b"copo_conflict_create" in lib.copo_last_error()
    out = (C.c_int64 * 2)()
    for fn, args in (("copo_conflict_record", (None,) * 3), ("copo_conflict_flush", (None, None)), ("copo_conflict_count", (None, out, None)),
                     ("copo_conflict_read", (None, 0, 0, None, None)), ("copo_conflict_clear", (None, None)), ("copo_conflict_reset", (None, None)),
                     ("copo_conflict_destroy", (None,))):
        assert getattr(lib, fn)(*args) == -1 and fn.encode() in lib.copo_last_error(), fn
    # the configuration is checked before any device call as well: a handle that is not NULL is enough to get there
    fake = C.create_string_buffer(1 << 16)
    for bad, code in cc.refused_configs(_capi):
        assert lib.copo_conflict_create(C.cast(fake, C.c_void_p), C.byref(bad), C.byref(h)) == code and b"copo_conflict_create" in lib.copo_last_error(), \
            (bad.max_rows, bad.radius, bad.leave_radius)
        assert not h.value
    assert lib.copo_conflict_create(C.cast(fake, C.c_void_p), None, C.byref(h)) == -1
    assert conflicts.state_bytes(1, 40, 1) == 48 * 780 + 20 * 40 + 12 + 64 + 16 and conflicts.state_bytes(16384, 40, 65536) > 0.6e9
