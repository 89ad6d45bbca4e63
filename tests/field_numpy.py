"""numpy restatement of the traffic field maps' rules (copo_amd/csrc/field_kernels.hip) on `get_state()` blocks
[16][E][N] of 32-bit words.

Centre cells and `speed_q` are computed in float32 with the kernel's individually rounded operations: they are exact by construction.
Footprints and `vx_q` / `vy_q` are computed in float64.  A (body, cell) pair whose cell centre lies within `EDGE` = 1e-3 m of an edge of
the body's rectangle is AMBIGUOUS (coordinates below 300 m have an fp32 ulp of 3e-5 m): the footprint layers come back as `lo` (the
sure pairs) and `hi` (sure + ambiguous ones), and the recorder counts both kinds of pairs."""
import numpy as np

ST_EMPTY, ST_ALIVE, ST_WRECK = 0, 1, 2
F_DONE, F_ARRIVE, F_CRASH, F_OUT = 0x02, 0x04, 0x08, 0x10
LAYERS = ("occupancy", "wreck", "visits", "speed_q", "vx_q", "vy_q", "crash", "out", "arrive", "critical")
L = {k: i for i, k in enumerate(LAYERS)}
EDGE = 1e-3
f32 = np.float32


class Grid:
    def __init__(self, x0, y0, W, H, cell=1.0):
        self.x0, self.y0, self.cell = f32(x0), f32(y0), f32(cell)
        self.inv = f32(1.0 / np.float64(self.cell))          # rounded once
        self.W, self.H = int(W), int(H)

    def centres(self):
        """float64 cell centres: (px [W], py [H])"""
        c = np.float64(self.cell)
        return np.float64(self.x0) + (np.arange(self.W) + 0.5) * c, np.float64(self.y0) + (np.arange(self.H) + 0.5) * c


def centre_cells(x, y, grid):
    """(ix, iy, inside) of float32 positions: floor((x - x0) * inv) with every operation rounded to float32"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    fx = np.floor((x - grid.x0).astype(f32) * grid.inv).astype(f32)
    fy = np.floor((y - grid.y0).astype(f32) * grid.inv).astype(f32)
    inside = (fx >= 0) & (fx < grid.W) & (fy >= 0) & (fy < grid.H)
    return np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64), inside


def speed_q(v):
    """rint(min(max(v, 0), 255) * 256): a float32 product, round half to even"""
    v = np.asarray(v, f32)
    return np.rint(np.fmin(np.fmax(v, f32(0)), f32(255)) * f32(256)).astype(np.int64)


def velocity_q(v, th):
    """float64: rint(clamp(v, -255, 255) cos(th) 256), the same with sin"""
    v, th = np.asarray(v, np.float64), np.asarray(th, np.float64)
    vc = np.clip(v, -255.0, 255.0)
    return np.rint(vc * np.cos(th) * 256.0).astype(np.int64), np.rint(vc * np.sin(th) * 256.0).astype(np.int64)


def footprint(x, y, th, grid, hl, hw):
    """Cells of one body's footprint, float64: (iy, ix) index arrays of the sure cells and of the ambiguous ones"""
    x, y, th = np.float64(x), np.float64(y), np.float64(th)
    hl, hw = np.float64(f32(hl)), np.float64(f32(hw))
    px, py = grid.centres()
    reach = np.hypot(hl, hw) + 2 * EDGE
    jx, jy = np.nonzero(np.abs(px - x) <= reach)[0], np.nonzero(np.abs(py - y) <= reach)[0]
    if jx.size == 0 or jy.size == 0:
        z = np.zeros(0, np.int64)
        return (z, z), (z, z)
    dx, dy = px[jx][None, :] - x, py[jy][:, None] - y
    c, s = np.cos(th), np.sin(th)
    u, w = np.abs(dx * c + dy * s), np.abs(dy * c - dx * s)
    sure = (u <= hl - EDGE) & (w <= hw - EDGE)
    amb = (u <= hl + EDGE) & (w <= hw + EDGE) & ~sure
    a, b = np.nonzero(sure)
    p, q = np.nonzero(amb)
    return (jy[a], jx[b]), (jy[p], jx[q])


class Recorder:
    """The handle's whole behaviour: maps, scene_records, last-seen memory, stride and groups."""

    def __init__(self, grid, E, N, hl, hw, groups=1, ttc_below=0.0, stride=1):
        self.grid, self.E, self.N, self.hl, self.hw = grid, E, N, hl, hw
        self.G, self.ttc_below, self.stride = int(groups), f32(ttc_below), int(stride)
        self.group = np.zeros(E, np.int64)
        self.clear()

    def clear(self):
        g = self.grid
        self.lo = np.zeros((self.G, len(LAYERS), g.H, g.W), np.int64)       # every layer; the footprint layers: sure pairs only
        self.hi = np.zeros((self.G, 2, g.H, g.W), np.int64)                 # footprint layers: sure + ambiguous pairs
        self.scene_records = np.zeros(self.G, np.int64)
        self.n_records = 0
        self.sure_pairs = self.ambiguous_pairs = 0
        self.forget()

    reset = clear

    def forget(self):
        self.last = np.full((self.E, self.N, 2), -1, np.int64)             # (iy, ix) where the slot was ALIVE inside the grid, else -1

    def set_groups(self, group):
        self.group = np.asarray(group, np.int64).reshape(self.E).copy()

    def record(self, st, flags=None, ttc=None):
        st = np.asarray(st, f32)
        status = st.view(np.int32)[13] & 0xFF
        accumulate = self.n_records % self.stride == 0
        self.n_records += 1
        x, y, th, v = st[0], st[1], st[2], st[3]
        ix, iy, inside = centre_cells(x, y, self.grid)
        sq = speed_q(v)
        vxq, vyq = velocity_q(v, th)
        for e in range(self.E):
            g = int(self.group[e])
            routed = 0 <= g < self.G
            if routed and flags is not None:
                for n in range(self.N):
                    f = int(flags[e, n])
                    if (f & F_DONE) and self.last[e, n, 0] >= 0:
                        cy, cx = self.last[e, n]
                        for bit, name in ((F_CRASH, "crash"), (F_OUT, "out"), (F_ARRIVE, "arrive")):
                            if f & bit:
                                self.lo[g, L[name], cy, cx] += 1
            alive = status[e] == ST_ALIVE
            self.last[e, :, 0] = np.where(alive & inside[e], iy[e], -1)
            self.last[e, :, 1] = np.where(alive & inside[e], ix[e], -1)
            if not (accumulate and routed):
                continue
            self.scene_records[g] += 1
            for n in range(self.N):
                if status[e, n] not in (ST_ALIVE, ST_WRECK):
                    continue
                k = 0 if status[e, n] == ST_ALIVE else 1
                sure, amb = footprint(x[e, n], y[e, n], th[e, n], self.grid, self.hl, self.hw)
                np.add.at(self.lo[g, k], sure, 1)
                np.add.at(self.hi[g, k], sure, 1)
                np.add.at(self.hi[g, k], amb, 1)
                self.sure_pairs += len(sure[0])
                self.ambiguous_pairs += len(amb[0])
                if k == 0 and inside[e, n]:
                    c = (iy[e, n], ix[e, n])
                    self.lo[g, L["visits"]][c] += 1
                    self.lo[g, L["speed_q"]][c] += sq[e, n]
                    self.lo[g, L["vx_q"]][c] += vxq[e, n]
                    self.lo[g, L["vy_q"]][c] += vyq[e, n]
                    if ttc is not None and self.ttc_below > 0 and f32(ttc[e, n]) < self.ttc_below:
                        self.lo[g, L["critical"]][c] += 1


def compare(maps, scene_records, ref):
    """GPU maps int64 [G, 10, H, W] and scene_records [G] against a `Recorder`: layers 2, 3, 6..9 and scene_records equal, 0 and 1
    within [lo, hi] per cell, 4 and 5 within one quantisation step per sample (|d| <= visits).  Returns the largest |d| of 4 / 5."""
    maps, scene_records = np.asarray(maps, np.int64), np.asarray(scene_records, np.int64)
    assert maps.shape == ref.lo.shape, (maps.shape, ref.lo.shape)
    assert np.array_equal(scene_records, ref.scene_records), (scene_records.tolist(), ref.scene_records.tolist())
    for k in (2, 3, 6, 7, 8, 9):
        bad = np.argwhere(maps[:, k] != ref.lo[:, k])
        assert bad.size == 0, (LAYERS[k], bad[:5].tolist(), [int(maps[:, k][tuple(b)]) for b in bad[:5]], [int(ref.lo[:, k][tuple(b)]) for b in bad[:5]])
    for k in (0, 1):
        bad = np.argwhere((maps[:, k] < ref.lo[:, k]) | (maps[:, k] > ref.hi[:, k]))
        assert bad.size == 0, (LAYERS[k], bad[:5].tolist(), [int(maps[:, k][tuple(b)]) for b in bad[:5]], [int(ref.lo[:, k][tuple(b)]) for b in bad[:5]],
                               [int(ref.hi[:, k][tuple(b)]) for b in bad[:5]])
    worst = 0
    for k in (4, 5):
        d = np.abs(maps[:, k] - ref.lo[:, k])
        worst = max(worst, int(d.max()))
        assert (d <= ref.lo[:, 2]).all(), (LAYERS[k], np.argwhere(d > ref.lo[:, 2])[:5].tolist(), worst)
    return worst
