"""The rules of the trip log (include/copo_hip.h) restated: a python loop over records, scenes and slots, the fp32
steps (the reward add, the speed quantisation, the `<` of speed, gap and TTC) in numpy.float32 in the order the rules give them.  Equality
with the kernels is by construction: every comparison is on raw 32-bit words, there is no tolerance.

Rules.  Records count from 0 since creation / `reset`.  State fields: 3 speed, 9 route progress, 10 LCF, 12 route | road << 16, 13 status
| timer << 8 | age << 16, 14 agent id; env word 1 is the scene's episode.  A slot's identity is (agent id, episode word).  At record r
with the optional arrays flags u8, rew, gap, ttc fp32 [E][N] (None = absent), for every slot:
  1 close, when a trip is open: with flags & ACTED and rew given, reward = reward + rew (fp32); with flags & DONE the trip closes with
    kind 1 and end = the flags byte; otherwise, if the slot is not ALIVE now with the same identity, with kind 2 and end = 0
  2 open, when the slot is ALIVE and no trip is open (also after a close in this record): first_rec = r, route = field 12 & 0xffff, lcf and
    prog0 the raw bits of fields 10 and 9, steps = speed_sum = speed_max = stops = 0, reward = +0.0, min_gap = min_ttc = +inf
  3 accumulate, when a trip is open now: steps += 1, prog1 = bits of field 9, q = rint(min(max(v, 0), 255) * 256), speed_sum += q (uint32),
    speed_max = max(speed_max, q), stops += (v < stop_speed), min_gap = gap if gap < min_gap, min_ttc likewise
Row: {scene, slot | route << 16, aid, episode, first_rec, steps, end | kind << 8, lcf, prog0, prog1, speed_sum, speed_max, stops, reward,
min_gap, min_ttc}.  The rows closed in one record take the ids n_rows, n_rows + 1, ... in ascending (scene, slot) order; an id >= max_rows
is dropped.  `flush` closes every open trip with kind 3 and end = 0 under the same order rule; `clear` empties the pool and the dropped
count only."""
import numpy as np

from rowlog_numpy import (F_ACTED, F_ARRIVE, F_CRASH, F_DONE, F_ENV_RESET, F_MAXSTEP, F_OUT, F_SPAWNED, M32, ST_ALIVE, ST_EMPTY, ST_WRECK,  # noqa: F401
                          WORDS, RowPool, compare, f32)

KIND_DONE, KIND_VANISHED, KIND_FLUSHED = 1, 2, 3
INF_BITS = 0x7F800000


def bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def speed_q(v):
    """rint(min(max(v, 0), 255) x 256) in float32, half to even (the field maps' quantisation; fmaxf(NaN, 0) = 0)"""
    v = f32(v)
    v = f32(0.0) if not v >= f32(0.0) else v
    v = min(v, f32(255.0))
    return int(np.rint(f32(v * f32(256.0))))


class _Trip:
    __slots__ = ("aid", "episode", "first_rec", "route", "lcf", "prog0", "prog1", "steps", "speed_sum", "speed_max", "stops", "reward", "min_gap",
                 "min_ttc")


class TripLog(RowPool):
    def __init__(self, E, N, max_rows=65536, stop_speed=0.5):
        self.E, self.N, self.max_rows, self.stop_speed = E, N, int(max_rows), f32(stop_speed)
        self.reset()

    def reset(self):
        self.r = 0
        self.open = [[None] * self.N for _ in range(self.E)]
        self.clear()
        # what the tests' premises need (not part of the rules)
        self.total_closed = 0
        self.scene_records_with_two_closes = 0
        self.records_with_closes_in_two_scenes = 0
        self.close_and_open_in_one_record = 0

    def _commit(self, e, n, t, end, kind, close_rec):
        self._store([e, n | (t.route << 16), t.aid & M32, t.episode & M32, t.first_rec, t.steps & M32, end | (kind << 8), t.lcf, t.prog0, t.prog1,
                     t.speed_sum & M32, t.speed_max, t.stops & M32, bits(t.reward), bits(t.min_gap), bits(t.min_ttc)], close_rec)

    def record(self, state, env, flags=None, rew=None, gap=None, ttc=None):
        """state [16][E][N] float32 words, env [E][4] int32 of the simulator after a step / reset / set_state"""
        st = np.ascontiguousarray(state, np.float32)
        su = st.view(np.uint32)
        si = st.view(np.int32)
        opt = lambda a, dt: None if a is None else np.asarray(a, dt).reshape(self.E, self.N)      # noqa: E731
        flags, rew, gap, ttc = opt(flags, np.uint8), opt(rew, np.float32), opt(gap, np.float32), opt(ttc, np.float32)
        r, scenes_closing = self.r, 0
        for e in range(self.E):
            ep, closes = int(env[e, 1]), 0
            for n in range(self.N):
                alive = (int(si[13, e, n]) & 0xFF) == ST_ALIVE
                aid = int(si[14, e, n])
                t = self.open[e][n]
                closed = False
                if t is not None:                                                           # 1 close
                    f = int(flags[e, n]) if flags is not None else 0
                    if (f & F_ACTED) and rew is not None:
                        with np.errstate(invalid="ignore", over="ignore"):
                            t.reward = f32(t.reward + rew[e, n])
                    if f & F_DONE:
                        self._commit(e, n, t, f, KIND_DONE, r)
                        closed = True
                    elif not (alive and aid == t.aid and ep == t.episode):
                        self._commit(e, n, t, 0, KIND_VANISHED, r)
                        closed = True
                    if closed:
                        t = self.open[e][n] = None
                        closes += 1
                if alive and t is None:                                                     # 2 open
                    t = self.open[e][n] = _Trip()
                    t.aid, t.episode, t.first_rec = aid, ep, r
                    t.route, t.lcf, t.prog0, t.prog1 = int(su[12, e, n]) & 0xFFFF, int(su[10, e, n]), int(su[9, e, n]), 0
                    t.steps = t.speed_sum = t.speed_max = t.stops = 0
                    t.reward, t.min_gap, t.min_ttc = f32(0.0), f32(np.inf), f32(np.inf)
                    self.close_and_open_in_one_record += 1 if closed else 0
                if t is not None:                                                           # 3 accumulate
                    v = st[3, e, n]
                    q = speed_q(v)
                    t.steps += 1
                    t.prog1 = int(su[9, e, n])
                    t.speed_sum = (t.speed_sum + q) & M32
                    t.speed_max = max(t.speed_max, q)
                    t.stops += 1 if v < self.stop_speed else 0
                    if gap is not None and gap[e, n] < t.min_gap:
                        t.min_gap = gap[e, n]
                    if ttc is not None and ttc[e, n] < t.min_ttc:
                        t.min_ttc = ttc[e, n]
            self.scene_records_with_two_closes += 1 if closes >= 2 else 0
            scenes_closing += 1 if closes else 0
        self.records_with_closes_in_two_scenes += 1 if scenes_closing >= 2 else 0
        self.r += 1

    def flush(self):
        for e in range(self.E):
            for n in range(self.N):
                if self.open[e][n] is not None:
                    self._commit(e, n, self.open[e][n], 0, KIND_FLUSHED, self.r)
                    self.open[e][n] = None

    def n_open(self):
        return sum(t is not None for row in self.open for t in row)
