"""Cases shared by the trip log's tests (test_trips_cpu.py, test_gpu_trips.py): a hand-made sequence of eight records in four scenes whose
rows are written out by hand, the 200-step rollout of the reference's CoPO Intersection population, and a short rollout with a small
horizon and a reset by hand.  States are the simulator's blocks [16][E][N] of 32-bit words, env [E][4] int32."""
import dataclasses

import numpy as np

import gate_cases as gc
import interact_cases as ic
import trip_numpy as tn

ALIVE, WRECK, EMPTY = tn.ST_ALIVE, tn.ST_WRECK, tn.ST_EMPTY
NAN, INF = float("nan"), float("inf")
A, D, ARR, CR, OUT, MX, SP, ER = (1 << i for i in range(8))      # the step's flag bits
STOP_SPEED = 0.5
BELOW_STOP = float(np.nextafter(np.float32(STOP_SPEED), np.float32(0.0)))      # one fp32 step below: a stop, and q = 128 all the same

HAND_E, HAND_RECORDS, HAND_CLEAR_AFTER = 4, 8, 3      # `clear` follows record 3, `flush` record 7
HAND_EPISODES = ((0,) * 8, (0, 0, 0, 0, 0, 1, 1, 1), (7,) * 8, (0,) * 8)

# Defaults of every slot and record, so that only what a case is about is written down: speed 2.0 (q = 512), route progress (field 9) =
# agent id + r, LCF (field 10) = agent id / 64, field 12 = (agent id % 5 + 1) | 9 << 16 (route = agent id % 5 + 1), flags = ACTED where the
# slot is ALIVE in this record and was in the one before, else 0, rew = 0.125, gap = ttc = +inf.  Record 0 has no arrays at all.
# (scene, slot) -> dict: `who` = per record (status, agent id); optional per-record overrides v, flags, rew, gap, ttc as {record: value}


def _who(*spans):
    """[(status, aid)] * 8 from (status, aid, records) spans"""
    out = []
    for status, aid, n in spans:
        out += [(status, aid)] * n
    assert len(out) == HAND_RECORDS
    return out


HAND_SLOTS = {
    # scene 0
    (0, 0): dict(who=_who((ALIVE, 10, 4), (EMPTY, 10, 4)), v={0: 10.0, 1: 300.0, 2: STOP_SPEED, 3: BELOW_STOP}, flags={4: A | D | ARR},
                 rew={1: 1.0, 2: 0.5, 3: 0.25, 4: 2.0}, gap={1: 5.0, 2: NAN, 3: 3.0}, ttc={1: INF, 2: 2.0, 3: NAN}),     # ends by ARRIVE after the clear
    (0, 1): dict(who=_who((ALIVE, 11, 2), (WRECK, 11, 3), (EMPTY, 11, 3)), flags={2: A | D | CR}, rew={1: 0.5, 2: -1.0}),  # CRASH, stays a WRECK
    (0, 2): dict(who=_who((ALIVE, 12, 3), (ALIVE, 17, 5)), flags={3: A | D | OUT | SP}),                                   # DONE and a new occupant at once
    (0, 3): dict(who=_who((ALIVE, 13, 3), (ALIVE, 18, 5)), flags={3: A}),                                                  # the agent id changes without DONE
    (0, 4): dict(who=_who((EMPTY, 14, 8)), rew={r: 9.0 for r in range(8)}),                                                # an EMPTY slot
    (0, 5): dict(who=_who((ALIVE, 15, 8)), flags={2: 0}, rew={2: 100.0}, gap={1: 7.0, 5: 6.5}),                            # rew without ACTED is ignored
    (0, 6): dict(who=_who((ALIVE, 16, 8)), v={r: (NAN if r == 4 else -3.0) for r in range(8)}),                            # negative speed: q = 0, a stop; NaN: neither
    # scene 1: the episode word changes at record 5
    (1, 0): dict(who=_who((ALIVE, 20, 8)), flags={5: A}),
    (1, 1): dict(who=_who((ALIVE, 21, 5), (ALIVE, 22, 3)), flags={5: A | D | MX | SP | ER}),
    # scene 2
    (2, 0): dict(who=_who((ALIVE, 30, 3), (EMPTY, 30, 3), (ALIVE, 31, 2)), flags={3: A | D | ARR | CR, 6: SP}),            # two causes; a later occupant
    (2, 6): dict(who=_who((EMPTY, 36, 1), (ALIVE, 36, 3), (WRECK, 36, 4)), flags={1: SP}),                                 # the last lane of N = 7; gone without DONE
    # scene 3
    (3, 3): dict(who=_who((ALIVE, 40, 8)), v={r: float(r + 1) for r in range(8)}, gap={2: -0.0, 3: 0.0}, ttc={3: 0.0, 4: 1.0}),
}
# N = 64 only: lane 63, the top bit of the masks.  Scene 0's ends at record 3 with a new occupant at once: three closes in that scene-record
HAND_SLOTS_64 = {
    (0, 63): dict(who=_who((ALIVE, 900, 3), (ALIVE, 950, 5)), flags={3: A | D | ARR | SP}),
    (1, 63): dict(who=_who((ALIVE, 901, 8)), flags={5: A}),
    (2, 63): dict(who=_who((ALIVE, 902, 8))),
    (3, 63): dict(who=_who((ALIVE, 903, 8))),
}


def hand_slots(N):
    assert N in (7, 64)
    return {**HAND_SLOTS, **HAND_SLOTS_64} if N == 64 else HAND_SLOTS


def hand_record(st0, env0, r):
    """(state, env, flags, rew, gap, ttc) of record r on the base arrays [16, 4, N] / [4, 4] (N = 7 or 64); the four arrays are None at
    record 0.  Every slot that is not listed is EMPTY."""
    st, env = st0.copy(), env0.copy()
    _, E, N = st.shape
    assert E == HAND_E
    su = st.view(np.uint32)
    flags, rew = np.zeros((E, N), np.uint8), np.full((E, N), 0.125, np.float32)
    gap, ttc = np.full((E, N), np.inf, np.float32), np.full((E, N), np.inf, np.float32)
    slots = hand_slots(N)
    for e in range(E):
        env[e, 1] = HAND_EPISODES[e][r]
        for n in range(N):
            c = slots.get((e, n))
            status, aid = c["who"][r] if c else (EMPTY, 60 + n)
            v = c.get("v", {}).get(r, 2.0) if c else 0.0
            ic.put(st, e, n, (float(n), float(e), 0.0, v, status), aid)
            st[9, e, n], st[10, e, n] = float(aid + r), aid / 64.0
            su[12, e, n] = (aid % 5 + 1) | (9 << 16)
            if c and r:
                was = c["who"][r - 1]
                flags[e, n] = c.get("flags", {}).get(r, A if status == ALIVE and was == (ALIVE, aid) else 0)
                for arr, key in ((rew, "rew"), (gap, "gap"), (ttc, "ttc")):
                    if r in c.get(key, {}):
                        arr[e, n] = c[key][r]
    return (st, env) + ((flags, rew, gap, ttc) if r else (None, None, None, None))


def _row(scene, slot, aid, episode, first_rec, steps, end, kind, prog0, prog1, speed_sum, speed_max, stops, reward, min_gap=INF, min_ttc=INF):
    b = tn.bits
    return [scene, slot | ((aid % 5 + 1) << 16), aid, episode, first_rec, steps, end | (kind << 8), b(aid / 64.0), b(prog0), b(prog1), speed_sum, speed_max,
            stops, b(reward), b(min_gap), b(min_ttc)]


# The rows, worked out by hand (q: 10 -> 2560, 300 -> 65280, 0.5 and the step below -> 128, 2 -> 512, n -> 256 n).
# Records 0..3, before the `clear`:
#   record 2: agent 11 crashes: two records driven, rewards 0.5 - 1.0
#   record 3: scene 0: agent 12 leaves the road (three records, 3 x 0.125) and agent 13 is replaced without DONE (kind 2, the reward of
#             record 3 still added); [N = 64: agent 900 arrives in lane 63;] scene 2: agent 30 arrives and crashes at once
_BEFORE = [
    _row(0, 1, 11, 0, 0, 2, A | D | CR, 1, 11.0, 12.0, 1024, 512, 0, -0.5),
    _row(0, 2, 12, 0, 0, 3, A | D | OUT | SP, 1, 12.0, 14.0, 1536, 512, 0, 0.375),
    _row(0, 3, 13, 0, 0, 3, 0, 2, 13.0, 15.0, 1536, 512, 0, 0.375),
    _row(2, 0, 30, 7, 0, 3, A | D | ARR | CR, 1, 30.0, 32.0, 1536, 512, 0, 0.375),
]
_BEFORE_63 = _row(0, 63, 900, 0, 0, 3, A | D | ARR | SP, 1, 900.0, 902.0, 1536, 512, 0, 0.375)
# Records 4..7 and the `flush`, after the `clear`:
#   record 4: agent 10 arrives with its whole history: records 0..3, speeds 10, 300 (clamped), 0.5 (no stop), one step below (a stop),
#             rewards 1 + 0.5 + 0.25 + 2, gaps 5, NaN, 3, TTCs inf, 2, NaN; agent 36 (driving since record 1) is a wreck without DONE
#   record 5: scene 1's episode word changes: agent 20 vanishes (five records, the reward of record 5 added) and agent 21 ends with the flags
#             byte of the scene reset; [N = 64: agent 901 vanishes as well]
#   flush:    everything still open, in (scene, slot) order
_AFTER = [
    _row(0, 0, 10, 0, 0, 4, A | D | ARR, 1, 10.0, 13.0, 2560 + 65280 + 128 + 128, 65280, 1, 3.75, 3.0, 2.0),
    _row(2, 6, 36, 7, 1, 3, 0, 2, 37.0, 39.0, 1536, 512, 0, 0.25),
    _row(1, 0, 20, 0, 0, 5, 0, 2, 20.0, 24.0, 2560, 512, 0, 0.625),
    _row(1, 1, 21, 0, 0, 5, A | D | MX | SP | ER, 1, 21.0, 25.0, 2560, 512, 0, 0.625),
]
_AFTER_63 = _row(1, 63, 901, 0, 0, 5, 0, 2, 901.0, 905.0, 2560, 512, 0, 0.625)
_FLUSH = {
    0: [_row(0, 2, 17, 0, 3, 5, 0, 3, 20.0, 24.0, 2560, 512, 0, 0.5), _row(0, 3, 18, 0, 3, 5, 0, 3, 21.0, 25.0, 2560, 512, 0, 0.5),
        _row(0, 5, 15, 0, 0, 8, 0, 3, 15.0, 22.0, 4096, 512, 0, 0.75, 6.5), _row(0, 6, 16, 0, 0, 8, 0, 3, 16.0, 23.0, 0, 0, 7, 0.875)],
    1: [_row(1, 0, 20, 1, 5, 3, 0, 3, 25.0, 27.0, 1536, 512, 0, 0.25), _row(1, 1, 22, 1, 5, 3, 0, 3, 27.0, 29.0, 1536, 512, 0, 0.25)],
    2: [_row(2, 0, 31, 7, 6, 2, 0, 3, 37.0, 38.0, 1024, 512, 0, 0.125)],
    3: [_row(3, 3, 40, 0, 0, 8, 0, 3, 40.0, 47.0, 256 * 36, 2048, 0, 0.875, -0.0, 0.0)],
}
_FLUSH_63 = {0: _row(0, 63, 950, 0, 3, 5, 0, 3, 953.0, 957.0, 2560, 512, 0, 0.5), 1: _row(1, 63, 901, 1, 5, 3, 0, 3, 906.0, 908.0, 1536, 512, 0, 0.25),
             2: _row(2, 63, 902, 7, 0, 8, 0, 3, 902.0, 909.0, 4096, 512, 0, 0.875), 3: _row(3, 63, 903, 0, 0, 8, 0, 3, 903.0, 910.0, 4096, 512, 0, 0.875)}


def hand_expected(N):
    """(rows after record 3, rows after the flush that follows record 7) uint32 [n, 16]; the pool is cleared in between"""
    before, after = list(_BEFORE), list(_AFTER)
    if N == 64:
        before.insert(3, _BEFORE_63)
        after.append(_AFTER_63)
    for e in range(HAND_E):
        after += _FLUSH[e] + ([_FLUSH_63[e]] if N == 64 else [])
    u = lambda rows: np.array([[w & 0xFFFFFFFF for w in row] for row in rows], np.uint32)      # noqa: E731
    return u(before), u(after)


def run_hand(log, N, record, read, st0=None, env0=None):
    """Drive the hand sequence through `log` (the restatement or a `TripLog`): `record(r, st, env, flags, rew, gap, ttc)` makes record r,
    `read()` returns (rows, (n_rows, dropped)).  Returns what `read` gave after record 3 and after the flush."""
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


# ---- rollout (b): Intersection, 6 scenes x 40 slots, 200 steps of the reference's CoPO population (the gates' rollout).  On the CPU oracle:
# 120 finished agents (58 arrive, 28 crash, 34 out), 19 scene-records with two or more closes, 21 records with closes in two or more scenes,
# no slot that ends and respawns in one step (the hand sequence has that) ----
ROLLOUT_STEPS = 200
rollout_config = gc.rollout_config

# ---- rollout (c): Intersection, 3 scenes x 10 slots, every agent ends after 30 steps of driving at the latest, 80 steps with a reset by hand
# (other seeds, a record without flags) after step 50.  On the CPU oracle: 82 rows -- 58 MAXSTEP (50 of them with ENV_RESET), 2 crashes and
# 22 of kind 2 from the reset by hand ----
SHORT_STEPS, SHORT_RESET_AFTER, SHORT_HORIZON, SHORT_RESEED = 80, 50, 30, 99


def short_config():
    return dataclasses.replace(ic.rollout_config(), horizon=SHORT_HORIZON)


def short_seeds(E):
    return np.arange(E, dtype=np.uint64) + np.uint64(SHORT_RESEED)


def check_invariants(ref, resets_by_hand=()):
    """what holds for every run that records every step and does not `flush`, on a restatement.  `resets_by_hand`: the records that follow
    a reset by hand, which starts the episode words and agent ids again"""
    rows = ref.rows().astype(np.int64)
    keys = [(sum(f >= r for r in resets_by_hand),) + tuple(k) for f, k in zip(rows[:, 4].tolist(), rows[:, [0, 2, 3]].tolist())]
    assert len(set(keys)) == len(keys), "a (scene, aid, episode) appears twice"
    assert (rows[:, 5] >= 1).all() and (rows[:, 4] + rows[:, 5] <= ref.r).all()
    order = [(c, int(s), int(w & 0xFFFF)) for c, s, w in zip(ref.close_rec, rows[:, 0], rows[:, 1])]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert all(c == f + n for c, f, n in zip(ref.close_rec, rows[:, 4], rows[:, 5])), "a trip that is followed ends the record after its last step"
