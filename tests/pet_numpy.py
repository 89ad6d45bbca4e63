"""The rules of the encroachment log (include/copo_hip.h) restated: a python loop over records, scenes and slots, a
numpy array of 64-bit stamps per scene.  Equality with the kernels is by construction: every comparison is on raw words, there is no
tolerance.

Rules.  Records count from 0 since creation / `reset`.
  1 Footprint.  C(n): the grid cells whose centre lies in the body of slot n, the field maps' rule: sincos_det of the heading, u = fm(dx, c,
    dy s), w = fm(dy, c, -(dx s)), |u| <= hl && |w| <= hw, cell centres at x0 + (ix + 0.5) cell, every operation fp32 (`fm` = one fused
    multiply-add).  Cells outside the grid do not exist.  tests/field_numpy.py's float64 footprint gives the candidates (its sure and its
    ambiguous cells); the fp32 rule, restated here operation for operation, decides among them.
  2 Stamp.  (q + 1) << 32 | (aid & 0xffff) << 16 | hq << 8 | slot for a stamp written in record q; hq = rint(heading * fp32(128 / pi)) &
    255, one fp32 product.  0 = empty.
  3 Identity.  Per slot the remembered aid and a 64-bit `met` mask, per scene the remembered episode word and `epoch`.  Slot n turns over in
    record r when it is not ALIVE, its aid differs from the remembered one, or the scene's episode word changed: it clears its `met`, and
    every slot of the scene clears bit n of its own.  An episode change sets epoch = r; `forget()` sets epoch = the next record's number
    in every scene and clears every `met`.
  4 Valid stamp.  {q + 1, a16, hq, s} under C(n) is valid for ALIVE slot n in record r iff s != n, slot s is ALIVE now with (aid[s] &
    0xffff) == a16, q + 1 > epoch, and 1 <= r - q <= window.
  5 Encounter.  P(n): the slots with a valid stamp under C(n).  For every s of P(n) & ~met[n], ascending, ONE row: pet = the smallest r - q
    over the valid stamps of s under C(n), cell = the lowest cell index that attains it, that stamp's hq, n_cells = the cells under C(n)
    with valid stamps of s.  Then met[n] |= P(n).  Row: {scene, slot_b | slot_a << 6, aid_b, aid_a, episode, r, pet, cell, n_cells, speed_a
    bits, x_b, y_b, heading_b, speed_b bits, hq_a, hq_b}, b = n, a = s.  Rows leave in (scene, slot_b, slot_a) order.
  6 Aggregates, with g = group[e] in 0..G-1: hist[g][type][pet - 1] += 1, type from d = min(rel, 256 - rel), rel = (hq_b - hq_a) & 255: 0
    following d <= 21, 2 opposing d >= 107, else 1 crossing; critical[g][cell] += 1 when pet <= critical_records.  Dropped rows count.
  7 Stamping, after every read of the record: every ALIVE slot writes max(old, its stamp) into each cell of C(n)."""
import numpy as np

import field_numpy as fn
from rowlog_numpy import M32, ST_ALIVE, ST_EMPTY, ST_WRECK, WORDS, RowPool, compare, f32  # noqa: F401

f64 = np.float64
FOLLOW_Q, OPPOSE_Q = 21, 107
HQ_SCALE = f32(128 / np.pi)


def fm(a, b, c):
    """fp32 fused multiply-add, exactly: the product of two fp32 values is exact in float64; the sum is rounded to odd in float64 (two-sum
    gives the error's sign), which then rounds to fp32 as the exact sum would"""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    p = np.asarray(a * b, f64)
    s = np.asarray(p + c, f64)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def sincos_det(x):
    """sim_math.h's sincos_det on a float32 scalar: (s, c)"""
    x = f32(x)
    kf = np.floor(fm(x, f32(0.636619772), f32(0.5)))
    k = int(kf)
    r = fm(-kf, f32(1.5703125), x)
    r = fm(-kf, f32(4.83751297e-4), r)
    r = fm(-kf, f32(7.54978996e-8), r)
    z = f32(r * r)
    sp = fm(f32(fm(fm(f32(-1.9515295891e-4), z, f32(8.3321608736e-3)), z, f32(-1.6666654611e-1)) * z), r, r)
    cp = fm(z, fm(z, fm(fm(f32(2.443315711809948e-5), z, f32(-1.388731625493765e-3)), z, f32(4.166664568298827e-2)), f32(-0.5)), f32(1.0))
    q = k & 3
    a, b = (cp, sp) if q & 1 else (sp, cp)
    return f32(-a if q & 2 else a), f32(-b if q in (1, 2) else b)


def heading_q(th):
    with np.errstate(invalid="ignore"):
        return int(np.rint(f32(th) * HQ_SCALE).astype(np.int64) & 255)


def stamp(rec, aid, hq, slot):
    """the stamp of record `rec`"""
    return ((rec + 1) << 32) | ((aid & 0xFFFF) << 16) | (hq << 8) | slot


def cells(x, y, th, grid, hl, hw):
    """C(n) of one body: the ascending cell indices iy * W + ix"""
    x, y = f32(x), f32(y)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(f32(th))):
        return np.zeros(0, np.int64)
    sure, amb = fn.footprint(x, y, th, grid, hl, hw)
    iy, ix = np.concatenate([sure[0], amb[0]]), np.concatenate([sure[1], amb[1]])
    if iy.size == 0:
        return np.zeros(0, np.int64)
    s, c = sincos_det(th)
    hl, hw = f32(hl), f32(hw)
    px = (grid.x0 + ((ix.astype(f32) + f32(0.5)) * grid.cell).astype(f32)).astype(f32)
    py = (grid.y0 + ((iy.astype(f32) + f32(0.5)) * grid.cell).astype(f32)).astype(f32)
    dx, dy = (px - x).astype(f32), (py - y).astype(f32)
    u = fm(dx, c, (dy * s).astype(f32))
    w = fm(dy, c, -((dx * s).astype(f32)))
    inside = (np.abs(u) <= hl) & (np.abs(w) <= hw)
    return np.sort(iy[inside] * grid.W + ix[inside])


def type_index(hq_a, hq_b):
    rel = (hq_b - hq_a) & 255
    d = min(rel, 256 - rel)
    return 0 if d <= FOLLOW_Q else (2 if d >= OPPOSE_Q else 1)


class EncroachmentLog(RowPool):
    def __init__(self, E, N, grid, hl, hw, window=50, critical_records=10, groups=1, max_rows=65536):
        if not float(grid.cell) <= 2.0 * float(f32(hw)) / np.sqrt(2.0):
            raise ValueError("cell=%g m is wider than 2 hw / sqrt(2): a body could pass between cell centres" % float(grid.cell))
        self.E, self.N, self.grid, self.hl, self.hw = E, N, grid, hl, hw
        self.window, self.critical_records, self.G, self.max_rows = int(window), int(critical_records), int(groups), int(max_rows)
        self.group = np.zeros(E, np.int64)
        self.reset()

    def reset(self):
        g = self.grid
        self.r = 0
        self.stamps = np.zeros((self.E, g.H * g.W), np.uint64)
        self.aid = np.zeros((self.E, self.N), np.int64)
        self.met = np.zeros((self.E, self.N), np.uint64)
        self.episode = np.zeros(self.E, np.int64)
        self.epoch = np.zeros(self.E, np.int64)
        self.hist = np.zeros((self.G, 3, self.window), np.int64)
        self.critical = np.zeros((self.G, g.H, g.W), np.int64)
        self.clear()
        # what the tests' premises need (not part of the rules)
        self.total_closed = 0
        self.turnovers_in_window = 0           # a slot turned over while a stamp of its last agent was young enough to count
        self.second_touches = 0                # valid stamps of a partner that is already in `met`

    def set_groups(self, group):
        self.group = np.asarray(group, np.int64).reshape(self.E).copy()

    def forget(self):
        self.epoch[:] = self.r
        self.met[:] = 0

    def flush(self):
        pass

    def record(self, state, env):
        """state [16][E][N] float32 words, env [E][4] int32 of the simulator after a step / reset / set_state"""
        st = np.ascontiguousarray(state, np.float32)
        su, si = st.view(np.uint32), st.view(np.int32)
        r, W = self.r, self.grid.W
        for e in range(self.E):
            ep = int(env[e, 1])
            alive = [(int(si[13, e, n]) & 0xFF) == ST_ALIVE for n in range(self.N)]
            aid = [int(si[14, e, n]) for n in range(self.N)]
            changed = ep != int(self.episode[e])
            if changed:                                                                   # 3 identity
                self.epoch[e] = r
                self.episode[e] = ep
            turned = 0
            for n in range(self.N):
                if not alive[n] or aid[n] != int(self.aid[e, n]) or changed:
                    turned |= 1 << n
                    self.met[e, n] = 0
                    if alive[n] and not changed and r:                                    # (a premise: a new agent over live stamps of the last)
                        mine = self.stamps[e][(self.stamps[e] & np.uint64(0xFF)) == np.uint64(n)] >> np.uint64(32)
                        self.turnovers_in_window += 1 if mine.size and r - (int(mine.max()) - 1) <= self.window and int(mine.max()) > int(self.epoch[e]) else 0
            self.met[e] &= np.uint64(~turned & 0xFFFFFFFFFFFFFFFF)
            self.aid[e, :] = aid
            epoch = int(self.epoch[e])
            G = self.stamps[e]
            g = int(self.group[e])
            foot = {}
            for n in range(self.N):
                if not alive[n]:
                    continue
                C = foot[n] = cells(st[0, e, n], st[1, e, n], st[2, e, n], self.grid, self.hl, self.hw)
                best = {}                                                                 # s -> [pet, cell, hq, n_cells]
                for c, word in zip(C.tolist(), G[C].tolist()):
                    q1, a16, hq, s = word >> 32, (word >> 16) & 0xFFFF, (word >> 8) & 0xFF, word & 0xFF
                    if q1 == 0 or s == n or not (s < self.N and alive[s] and (aid[s] & 0xFFFF) == a16):      # 4 valid
                        continue
                    pet = r - (q1 - 1)
                    if not (q1 > epoch and 1 <= pet <= self.window):
                        continue
                    b = best.setdefault(s, [pet, c, hq, 0])
                    b[3] += 1
                    if pet < b[0]:
                        b[0], b[1], b[2] = pet, c, hq
                met = int(self.met[e, n])
                hq_b = heading_q(st[2, e, n])
                for s in sorted(best):                                                    # 5 encounter
                    if (met >> s) & 1:
                        self.second_touches += 1
                        continue
                    pet, c, hq_a, n_cells = best[s]
                    self._store([e, n | (s << 6), aid[n] & M32, aid[s] & M32, ep & M32, r, pet, c, n_cells, int(su[3, e, s]), int(su[0, e, n]),
                                 int(su[1, e, n]), int(su[2, e, n]), int(su[3, e, n]), hq_a, hq_b], r)
                    if 0 <= g < self.G:                                                   # 6 aggregates
                        self.hist[g, type_index(hq_a, hq_b), pet - 1] += 1
                        if pet <= self.critical_records:
                            self.critical[g, c // W, c % W] += 1
                    met |= 1 << s
                self.met[e, n] = met
            for n, C in foot.items():                                                     # 7 stamping
                w = np.uint64(stamp(r, aid[n], heading_q(st[2, e, n]), n))
                G[C] = np.maximum(G[C], w)
        self.r += 1


def compare_all(log, ref):
    """the device's rows, count, stamps, `met` masks, histogram and critical map equal the restatement's"""
    compare(log.rows().cpu().numpy(), log.count(), ref)
    grid, met = log.memory()
    g = ref.grid
    assert np.array_equal(grid.reshape(ref.E, -1), ref.stamps), np.argwhere(grid.reshape(ref.E, -1) != ref.stamps)[:8].tolist()
    assert np.array_equal(met, ref.met), np.argwhere(met != ref.met)[:8].tolist()
    agg = log.aggregates()
    assert np.array_equal(agg["hist"], ref.hist), np.argwhere(agg["hist"] != ref.hist)[:8].tolist()
    assert np.array_equal(agg["critical"], ref.critical) and agg["critical"].shape == (ref.G, g.H, g.W)
