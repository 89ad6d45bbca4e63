"""The rules of the conflict log (include/copo_hip.h) restated: a python loop over records, scenes and pairs, the
squared distance in numpy.float32 one operation at a time, a dict as the pair memory.  Equality with the kernels is by construction:
every comparison is on raw 32-bit words, there is no tolerance.

Rules.  Records count from 0 since creation / `reset`.  State fields 0..3 (x, y, heading, speed) are read as raw bits, the status byte of
field 13, field 14 (agent id), env word 1 (episode); `flags` u8 [E][N] is optional (None = absent).  A party's identity is (agent id,
episode word).  For slots a < b, both ALIVE now: dx = x_b - x_a, dy = y_b - y_a, d2 = dx dx + dy dy, every operation fp32 and rounded by
itself; r2_in = radius^2 and r2_out = leave_radius^2 rounded once to fp32; comparisons are plain `<`, so a NaN is never close.  The
handle remembers per slot the agent id of the previous record, per scene the episode word, per open pair {first_rec, steps, d2min,
min_off, the poses of a and b at the minimum}.  At record r, per scene:
  1 close, every open pair: with flags given and DONE on a or b: kind 1, end_a = the flags byte of a if it carries DONE else 0, end_b
    likewise; otherwise, if either slot is not ALIVE now with its remembered identity: kind 2, ends 0; otherwise, if not d2 < r2_out:
    kind 3, ends 0
  2 open, every pair a < b, both ALIVE now, not open after 1 (also one that closed in this record), d2 < r2_in: first_rec = r, steps = 0,
    d2min = +inf, min_off = 0
  3 accumulate, every pair open after 1 and 2: steps = min(steps + 1, 65535); if d2 < d2min: d2min = d2, min_off = min(r - first_rec,
    65535), the eight pose words are copied as raw bits
  4 the slot and scene memory is overwritten from the current state
Row: {scene, slot_a | slot_b << 6 | kind << 12 | end_a << 16 | end_b << 24, aid_a, aid_b, episode, first_rec, steps | min_off << 16, d2min
bits, pose_a[4], pose_b[4]}, identities as remembered.  The rows closed in one record take the ids n_rows, n_rows + 1, ... in ascending
(scene, slot_a, slot_b) order; an id >= max_rows is dropped, the encounter is closed all the same.  `flush` closes every open encounter
with kind 4 and ends 0 under the same order rule; `clear` empties the pool and the dropped count only.  ALIVE-WRECK pairs are out of
scope."""
import struct

import numpy as np

from rowlog_numpy import (F_ACTED, F_ARRIVE, F_CRASH, F_DONE, F_ENV_RESET, F_MAXSTEP, F_OUT, F_SPAWNED, M32, ST_ALIVE, ST_EMPTY, ST_WRECK,  # noqa: F401
                          WORDS, RowPool, compare, f32)

KIND_DONE, KIND_VANISHED, KIND_PARTED, KIND_FLUSHED = 1, 2, 3, 4
CAP = 65535
INF = float("inf")


def bits(x):
    """the 32-bit word of the float32 nearest to x"""
    return struct.unpack("<I", struct.pack("<f", x))[0]


def r2(radius):
    """radius^2 rounded once to fp32 (the product of two fp32 values is exact in float64)"""
    return f32(np.float64(f32(radius)) * np.float64(f32(radius)))


def dist2(xa, ya, xb, yb):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = f32(xb - xa), f32(yb - ya)
        px, py = f32(dx * dx), f32(dy * dy)
        return f32(px + py)


FIRST_REC, STEPS, D2MIN, MIN_OFF, POSE_A, POSE_B = range(6)      # the pair memory: a list per open pair


class ConflictLog(RowPool):
    def __init__(self, E, N, max_rows=65536, radius=8.0, leave_radius=10.0):
        self.E, self.N, self.max_rows = E, N, int(max_rows)
        self.r2_in, self.r2_out = float(r2(radius)), float(r2(leave_radius))
        self.reset()

    def reset(self):
        self.r = 0
        self.open = [dict() for _ in range(self.E)]            # (a, b) -> the pair memory
        self.aid = np.zeros((self.E, self.N), np.int64)
        self.episode = np.zeros(self.E, np.int64)
        self.clear()
        # what the tests' premises need (not part of the rules)
        self.total_closed = 0
        self.scene_records_with_two_closes = 0
        self.records_with_closes_in_two_scenes = 0
        self.close_and_open_in_one_record = 0
        self.max_encounters_of_one_slot = 0

    def n_open(self):
        return sum(len(d) for d in self.open)

    def _commit(self, e, a, b, p, kind, end_a, end_b):
        self._store([e, a | (b << 6) | (kind << 12) | (end_a << 16) | (end_b << 24), int(self.aid[e, a]) & M32, int(self.aid[e, b]) & M32,
                     int(self.episode[e]) & M32, p[FIRST_REC], p[STEPS] | (p[MIN_OFF] << 16), bits(p[D2MIN])] + p[POSE_A] + p[POSE_B], self.r)

    def record(self, state, env, flags=None):
        """state [16][E][N] float32 words, env [E][4] int32 of the simulator after a step / reset / set_state"""
        st = np.ascontiguousarray(state, np.float32)
        su, si = st.view(np.uint32), st.view(np.int32)
        flags = None if flags is None else np.asarray(flags, np.uint8).reshape(self.E, self.N)
        r, scenes_closing = self.r, 0
        for e in range(self.E):
            ep = int(env[e, 1])
            alive = [(int(si[13, e, n]) & 0xFF) == ST_ALIVE for n in range(self.N)]
            aid = [int(si[14, e, n]) for n in range(self.N)]
            same = [alive[n] and aid[n] == int(self.aid[e, n]) and ep == int(self.episode[e]) for n in range(self.N)]
            end = [int(flags[e, n]) if flags is not None and (int(flags[e, n]) & F_DONE) else 0 for n in range(self.N)]
            x, y = st[0, e], st[1, e]
            D = dist2(x[:, None], y[:, None], x[None, :], y[None, :])                      # [a][b], float32, every operation by itself
            am = np.array(alive, bool)
            with np.errstate(invalid="ignore"):
                near = np.argwhere(np.triu((D < f32(self.r2_in)) & am[:, None] & am[None, :], 1)).tolist()
            D, pose = D.tolist(), su[:4, e, :].T.tolist()      # (python floats hold a float32 exactly, so `<` decides the same)
            mem = self.open[e]
            closed = set()
            for (a, b) in sorted(mem):                                                    # 1 close
                if end[a] or end[b]:
                    self._commit(e, a, b, mem[(a, b)], KIND_DONE, end[a], end[b])
                elif not (same[a] and same[b]):
                    self._commit(e, a, b, mem[(a, b)], KIND_VANISHED, 0, 0)
                elif not D[a][b] < self.r2_out:
                    self._commit(e, a, b, mem[(a, b)], KIND_PARTED, 0, 0)
                else:
                    continue
                closed.add((a, b))
            for k in closed:
                del mem[k]
            # `near`: the pairs a < b, both ALIVE now, with d2 < r2_in, in order.  Only they and the open pairs can open or accumulate: the
            # loop over all a < b, cut down to them
            keys = [tuple(k) for k in near]
            if mem:
                keys = sorted(set(keys) | set(mem))
            for k in keys:
                a, b = k
                d = D[a][b]
                p = mem.get(k)
                if p is None:                                                             # 2 open
                    p = mem[k] = [r, 0, INF, 0, None, None]
                    self.close_and_open_in_one_record += 1 if k in closed else 0
                p[STEPS] = min(p[STEPS] + 1, CAP)                                         # 3 accumulate
                if d < p[D2MIN]:
                    p[D2MIN], p[MIN_OFF], p[POSE_A], p[POSE_B] = d, min(r - p[FIRST_REC], CAP), pose[a], pose[b]
            self.aid[e, :] = aid                                                          # 4 the memory
            self.episode[e] = ep
            per_slot = np.zeros(self.N, np.int64)
            for (a, b) in self.open[e]:
                per_slot[a] += 1
                per_slot[b] += 1
            self.max_encounters_of_one_slot = max(self.max_encounters_of_one_slot, int(per_slot.max()) if self.N else 0)
            self.scene_records_with_two_closes += 1 if len(closed) >= 2 else 0
            scenes_closing += 1 if closed else 0
        self.records_with_closes_in_two_scenes += 1 if scenes_closing >= 2 else 0
        self.r += 1

    def flush(self):
        for e in range(self.E):
            for (a, b) in sorted(self.open[e]):
                self._commit(e, a, b, self.open[e][(a, b)], KIND_FLUSHED, 0, 0)
            self.open[e] = dict()
