"""Cases shared by the conflict log's tests (test_conflicts_cpu.py, test_gpu_conflicts.py): a hand-made sequence of eight records in four
scenes whose rows are written out by hand, and the two rollouts of the reference's CoPO Intersection population that tests/trip_cases.py
drives.  States are the simulator's blocks [16][E][N] of 32-bit words, env [E][4] int32."""
import numpy as np

import conflict_numpy as cn
import interact_cases as ic
import trip_cases as tc

ALIVE, WRECK, EMPTY = cn.ST_ALIVE, cn.ST_WRECK, cn.ST_EMPTY
NAN = float("nan")
A, D, ARR, CR, OUT, MX, SP, ER = (1 << i for i in range(8))      # the step's flag bits
RADIUS, LEAVE = 8.0, 10.0                                        # r2_in = 64, r2_out = 100

HAND_E, HAND_RECORDS, HAND_CLEAR_AFTER = 4, 8, 3      # `clear` follows record 3, `flush` record 7
HAND_EPISODES = ((0,) * 8, (0,) * 8, (7, 7, 7, 7, 7, 7, 8, 8), (0,) * 8)

# fp32 steps around the two radii.  (8 - 2^-21)^2 = 64 - 2^-17 + 2^-42 rounds to 64 - 2^-17 (the spacing below 64 is 2^-18), so
#   (8 - 2^-21, 2^-9):  d2 = (64 - 2^-17) + 2^-18 = 64 - 2^-18, ONE step below r2_in
#   (6, 8 - 2^-21):     d2 = 36 + (64 - 2^-17) = 100 - 2^-17, ONE step below r2_out (the spacing below 128 is 2^-17)
BELOW8 = 8.0 - 2.0 ** -21
D2_BELOW_IN, D2_BELOW_OUT = 64.0 - 2.0 ** -18, 100.0 - 2.0 ** -17
assert cn.dist2(0, 0, np.float32(BELOW8), np.float32(2.0 ** -9)) == np.nextafter(np.float32(64), np.float32(0)) == np.float32(D2_BELOW_IN)
assert cn.dist2(0, 0, np.float32(6), np.float32(BELOW8)) == np.nextafter(np.float32(100), np.float32(0)) == np.float32(D2_BELOW_OUT)
assert cn.dist2(0, 0, np.float32(8), np.float32(0)) == cn.r2(RADIUS) == 64 and cn.dist2(0, 0, np.float32(6), np.float32(8)) == cn.r2(LEAVE) == 100

# Defaults of every slot and record, so that only what a case is about is written down: heading = slot % 16 / 8, speed = record + slot % 16 /
# 4 (the pose words differ from record to record, so a row shows WHICH record its poses are from), flags = ACTED where the slot is ALIVE in
# this record and held the same agent in the one before, else 0.  Record 0 has no flags.  A slot that is not listed is EMPTY at (0, 0), on
# top of the bodies there: it must not count.
# (scene, slot) -> dict: `who` = per record (status, agent id); `pos` = {record: (x, y)}, kept until the next entry; `flags` = {record: byte}


def _who(*spans):
    """[(status, aid)] * 8 from (status, aid, records) spans"""
    out = []
    for status, aid, n in spans:
        out += [(status, aid)] * n
    assert len(out) == HAND_RECORDS
    return out


HAND_SLOTS = {
    # scene 0: the radii.  (0, 1): exactly `radius` does not open, one step below opens, between the radii it stays, one step below
    # `leave_radius` it stays, exactly `leave_radius` it parts, between the radii it does not open again
    (0, 0): dict(who=_who((ALIVE, 10, 8)), pos={0: (0.0, 0.0)}),
    (0, 1): dict(who=_who((ALIVE, 11, 8)), pos={0: (8.0, 0.0), 1: (BELOW8, 2.0 ** -9), 2: (9.0, 0.0), 3: (6.0, BELOW8), 4: (6.0, 8.0), 5: (9.0, 0.0)}),
    # (2, 3): d2 = 25, 16, 16 (a tie: the first record keeps the poses), then 25
    (0, 2): dict(who=_who((ALIVE, 12, 8)), pos={0: (100.0, 0.0)}),
    (0, 3): dict(who=_who((ALIVE, 13, 8)), pos={0: (105.0, 0.0), 1: (104.0, 0.0), 2: (100.0, 4.0), 3: (105.0, 0.0)}),
    # (4, 5): a NaN position in records 1 and 2 parts the pair and keeps it from opening; it opens again in record 3
    (0, 4): dict(who=_who((ALIVE, 14, 8)), pos={0: (200.0, 0.0)}),
    (0, 5): dict(who=_who((ALIVE, 15, 8)), pos={0: (203.0, 0.0), 1: (NAN, 0.0), 3: (203.0, 0.0)}),
    # scene 1: DONE.  (0, 1): on one party, which leaves its slot EMPTY
    (1, 0): dict(who=_who((ALIVE, 20, 8)), pos={0: (0.0, 0.0)}),
    (1, 1): dict(who=_who((ALIVE, 21, 2), (EMPTY, 21, 6)), pos={0: (3.0, 0.0)}, flags={2: A | D | ARR}),
    # (2, 3): on both parties with CRASH in the same record; they stay as WRECKs, which is no encounter
    (1, 2): dict(who=_who((ALIVE, 22, 3), (WRECK, 22, 5)), pos={0: (100.0, 0.0)}, flags={3: A | D | CR}),
    (1, 3): dict(who=_who((ALIVE, 23, 3), (WRECK, 23, 5)), pos={0: (102.0, 0.0), 1: (101.0, 0.0)}, flags={3: A | D | CR}),
    # (4, 5): DONE with a new occupant that opens a new encounter with the same partner slot in that same record
    (1, 4): dict(who=_who((ALIVE, 24, 8)), pos={0: (200.0, 0.0)}),
    (1, 5): dict(who=_who((ALIVE, 25, 5), (ALIVE, 26, 3)), pos={0: (204.0, 0.0), 5: (205.0, 0.0)}, flags={5: A | D | OUT | SP}),
    # scene 2: slot 0 in three encounters at once.  Record 2: slot 1's agent id changes without DONE and slot 3 is gone without DONE (two
    # closes in one scene; scenes 1 and 3 close in that record too).  Record 6: the episode word changes, everything closes and opens again
    (2, 0): dict(who=_who((ALIVE, 30, 8)), pos={0: (0.0, 0.0)}),
    (2, 1): dict(who=_who((ALIVE, 31, 2), (ALIVE, 39, 6)), pos={0: (7.0, 0.0)}),
    (2, 2): dict(who=_who((ALIVE, 32, 8)), pos={0: (0.0, 7.0)}),
    (2, 3): dict(who=_who((ALIVE, 33, 2), (EMPTY, 33, 6)), pos={0: (-7.0, 0.0)}),
    (2, 5): dict(who=_who((ALIVE, 35, 8)), pos={0: (300.0, 0.0)}),
    (2, 6): dict(who=_who((ALIVE, 36, 8)), pos={0: (300.0, 6.0)}),                          # the last lane of N = 7
    # scene 3: a pair that closes in, then parts well beyond `leave_radius`
    (3, 1): dict(who=_who((ALIVE, 41, 8)), pos={0: (0.0, 0.0)}),
    (3, 4): dict(who=_who((ALIVE, 44, 8)), pos={0: (3.0, 0.0), 1: (2.0, 0.0), 2: (12.0, 0.0)}),
}
# N = 64 only: pair (62, 63), and a pair of lane 63 with a low lane (d2 = 36; slot 4 of that scene is never closer to it than 8 m)
HAND_SLOTS_64 = {
    (0, 62): dict(who=_who((ALIVE, 962, 8)), pos={0: (500.0, 0.0)}),
    (0, 63): dict(who=_who((ALIVE, 963, 8)), pos={0: (503.0, 0.0)}),
    (3, 63): dict(who=_who((ALIVE, 973, 8)), pos={0: (-6.0, 0.0)}),
}


def hand_slots(N):
    assert N in (7, 64)
    return {**HAND_SLOTS, **HAND_SLOTS_64} if N == 64 else HAND_SLOTS


def _heading(slot):
    return (slot % 16) / 8.0


def _speed(slot, r):
    return r + (slot % 16) / 4.0


def hand_record(st0, env0, r):
    """(state, env, flags) of record r on the base arrays [16, 4, N] / [4, 4] (N = 7 or 64); flags is None at record 0."""
    st, env = st0.copy(), env0.copy()
    _, E, N = st.shape
    assert E == HAND_E
    flags = np.zeros((E, N), np.uint8)
    slots = hand_slots(N)
    for e in range(E):
        env[e, 1] = HAND_EPISODES[e][r]
        for n in range(N):
            c = slots.get((e, n))
            if c is None:
                ic.put(st, e, n, (0.0, 0.0, 0.0, 0.0, EMPTY), 60 + n)
                continue
            status, aid = c["who"][r]
            x, y = c["pos"][max(k for k in c["pos"] if k <= r)]
            ic.put(st, e, n, (x, y, _heading(n), _speed(n, r), status), aid)
            if r:
                flags[e, n] = c.get("flags", {}).get(r, A if status == ALIVE and c["who"][r - 1] == (ALIVE, aid) else 0)
    return st, env, (flags if r else None)


def _row(scene, a, b, kind, aids, episode, first_rec, steps, min_off, d2min, pos_a, pos_b, ends=(0, 0)):
    """the poses are those of record first_rec + min_off"""
    bt, rec = cn.bits, first_rec + min_off
    pose = lambda n, p: [bt(p[0]), bt(p[1]), bt(_heading(n)), bt(_speed(n, rec))]      # noqa: E731
    return [scene, a | (b << 6) | (kind << 12) | (ends[0] << 16) | (ends[1] << 24), aids[0], aids[1], episode, first_rec, steps | (min_off << 16),
            bt(d2min)] + pose(a, pos_a) + pose(b, pos_b)


# The rows, worked out by hand.  Records 0..3, before the `clear`:
#   record 1: scene 0: slot 5's x is NaN: (4, 5), open since record 0 at 3 m, parts
#   record 2: scene 1: agent 21 arrives: (0, 1) ends with its flags byte on the b side; scene 2: slot 1 holds agent 39 instead of 31 and slot 3
#             is EMPTY, both without DONE: (0, 1) and (0, 3) vanish; scene 3: (1, 4), closest (2 m) in record 1, is 12 m apart
#   record 3: scene 1: agents 22 and 23 crash into each other: (2, 3), closest (1 m) in record 1, ends with CRASH on both sides
_BEFORE = [
    _row(0, 4, 5, 3, (14, 15), 0, 0, 1, 0, 9.0, (200.0, 0.0), (203.0, 0.0)),
    _row(1, 0, 1, 1, (20, 21), 0, 0, 2, 0, 9.0, (0.0, 0.0), (3.0, 0.0), ends=(0, A | D | ARR)),
    _row(2, 0, 1, 2, (30, 31), 7, 0, 2, 0, 49.0, (0.0, 0.0), (7.0, 0.0)),
    _row(2, 0, 3, 2, (30, 33), 7, 0, 2, 0, 49.0, (0.0, 0.0), (-7.0, 0.0)),
    _row(3, 1, 4, 3, (41, 44), 0, 0, 2, 1, 4.0, (0.0, 0.0), (2.0, 0.0)),
    _row(1, 2, 3, 1, (22, 23), 0, 0, 3, 1, 1.0, (100.0, 0.0), (101.0, 0.0), ends=(A | D | CR, A | D | CR)),
]
# Records 4..7 and the `flush`, after the `clear`:
#   record 4: scene 0: (0, 1) -- not opened at exactly 8 m in record 0, opened one fp32 step below in record 1, kept at 9 m and one step below
#             10 m -- parts at exactly 10 m: three records, the minimum in its first
#   record 5: scene 1: agent 25 leaves the road and agent 26 takes slot 5 at once: (4, 5) ends with the flags byte on the b side and the ids
#             it remembers; the new pair opens in this record (flushed below)
#   record 6: scene 2: the episode word goes from 7 to 8: (0, 1) (open since record 2 with agent 39), (0, 2) and (5, 6) vanish with episode 7
#             and open again with episode 8
#   flush:    everything still open, in (scene, slot_a, slot_b) order.  Scene 0's (2, 3) has d2 = 25, 16, 16, 25 ...: the tie in record 2 does
#             not move the poses; its (4, 5) opened again in record 3, after the NaN; (9 m apart, (0, 1) did not open again)
_AFTER = [
    _row(0, 0, 1, 3, (10, 11), 0, 1, 3, 0, D2_BELOW_IN, (0.0, 0.0), (BELOW8, 2.0 ** -9)),
    _row(1, 4, 5, 1, (24, 25), 0, 0, 5, 0, 16.0, (200.0, 0.0), (204.0, 0.0), ends=(0, A | D | OUT | SP)),
    _row(2, 0, 1, 2, (30, 39), 7, 2, 4, 0, 49.0, (0.0, 0.0), (7.0, 0.0)),
    _row(2, 0, 2, 2, (30, 32), 7, 0, 6, 0, 49.0, (0.0, 0.0), (0.0, 7.0)),
    _row(2, 5, 6, 2, (35, 36), 7, 0, 6, 0, 36.0, (300.0, 0.0), (300.0, 6.0)),
]
_FLUSH = {
    0: [_row(0, 2, 3, 4, (12, 13), 0, 0, 8, 1, 16.0, (100.0, 0.0), (104.0, 0.0)), _row(0, 4, 5, 4, (14, 15), 0, 3, 5, 0, 9.0, (200.0, 0.0), (203.0, 0.0))],
    1: [_row(1, 4, 5, 4, (24, 26), 0, 5, 3, 0, 25.0, (200.0, 0.0), (205.0, 0.0))],
    2: [_row(2, 0, 1, 4, (30, 39), 8, 6, 2, 0, 49.0, (0.0, 0.0), (7.0, 0.0)), _row(2, 0, 2, 4, (30, 32), 8, 6, 2, 0, 49.0, (0.0, 0.0), (0.0, 7.0)),
        _row(2, 5, 6, 4, (35, 36), 8, 6, 2, 0, 36.0, (300.0, 0.0), (300.0, 6.0))],
    3: [],
}
_FLUSH_64 = {0: [_row(0, 62, 63, 4, (962, 963), 0, 0, 8, 0, 9.0, (500.0, 0.0), (503.0, 0.0))], 1: [], 2: [],
             3: [_row(3, 1, 63, 4, (41, 973), 0, 0, 8, 0, 36.0, (0.0, 0.0), (-6.0, 0.0))]}


def hand_expected(N):
    """(rows after record 3, rows after the flush that follows record 7) uint32 [n, 16]; the pool is cleared in between"""
    before, after = list(_BEFORE), list(_AFTER)
    for e in range(HAND_E):
        after += _FLUSH[e] + (_FLUSH_64[e] if N == 64 else [])
    u = lambda rows: np.array([[w & 0xFFFFFFFF for w in row] for row in rows], np.uint32)      # noqa: E731
    return u(before), u(after)


def run_hand(log, N, record, read, st0=None, env0=None):
    """Drive the hand sequence through `log` (the restatement or a `ConflictLog`): `record(r, st, env, flags)` makes record r, `read()`
    returns (rows, (n_rows, dropped)).  Returns what `read` gave after record 3 and after the flush."""
    st0 = np.zeros((16, HAND_E, N), np.float32) if st0 is None else st0
    env0 = np.zeros((HAND_E, 4), np.int32) if env0 is None else env0
    mid = None
    for r in range(HAND_RECORDS):
        record(r, *hand_record(st0, env0, r))
        if r == HAND_CLEAR_AFTER:
            mid = read()
            log.clear()
    log.flush()
    return mid, read()


# ---- the rollouts of tests/trip_cases.py: Intersection, 6 x 40, 200 steps of the reference's CoPO population, and 3 x 10 with horizon 30, 80
# steps and a reset by hand (other seeds, a record without flags) after step 50 ----
ROLLOUT_STEPS, rollout_config = tc.ROLLOUT_STEPS, tc.rollout_config
SHORT_STEPS, SHORT_RESET_AFTER, short_config, short_seeds = tc.SHORT_STEPS, tc.SHORT_RESET_AFTER, tc.short_config, tc.short_seeds
ROLLOUT_CLEAR_AFTER = 100


def check_invariants(ref):
    """what holds for every run on a restatement: the order rule, and what a row says about itself"""
    rows = ref.rows().astype(np.int64)
    a, b = rows[:, 1] & 63, (rows[:, 1] >> 6) & 63
    assert (a < b).all() and (b < ref.N).all()
    steps, off = rows[:, 6] & 0xFFFF, rows[:, 6] >> 16
    assert (steps >= 1).all() and (off < steps).all() and (rows[:, 5] + steps <= ref.r).all()
    order = [(c, int(s), int(x), int(y)) for c, s, x, y in zip(ref.close_rec, rows[:, 0], a, b)]
    assert order == sorted(order) and len(set(order)) == len(order)
    d2 = rows[:, 7].astype(np.uint32).view(np.float32)
    assert (d2 < ref.r2_in).all()                        # an encounter opens below `radius`, so its minimum is below it


def refused_configs(_capi):
    """the configurations `copo_conflict_create` refuses, with their codes"""
    nan, inf = float("nan"), float("inf")
    K = _capi.ConflictCfg
    return ((K(0, 8.0, 10.0), -2), (K(-5, 8.0, 10.0), -2), (K(16, 0.0, 10.0), -5), (K(16, -1.0, 10.0), -5), (K(16, 8.0, 7.5), -5), (K(16, nan, 10.0), -5),
            (K(16, 8.0, nan), -5), (K(16, 8.0, inf), -5), (K(16, inf, inf), -5))
