"""numpy (float64) restatement of the top-down render rules (copo_amd/csrc/render_kernels.hip).

`render_frames(...)` returns the RGB frames and, per pixel, whether its colour is AMBIGUOUS: decided by a test whose boundary lies
within EPS metres of the pixel centre (road limits, line width and ends, dash ends, box and vehicle edges, the heading marker).  Every
test is evaluated three times -- exact, shrunk by EPS, grown by EPS -- and the layers are composed with three-valued membership: a
pixel is ambiguous when some layer that still shows in the final colour might or might not have painted it.
"""
import math

import numpy as np

from copo_amd import maps as M
from copo_amd.render import BACKGROUND, BOX_HIDDEN, BOX_SEEN, LINE, PALETTE, ROAD, WRECK
from copo_amd.sim import line_table

EPS = 2e-3
ST_ALIVE, ST_WRECK = 1, 2


def road_records(tables):
    """[n, 16] float64: the road records of every route (terminal records excluded), duplicates dropped."""
    rows = []
    for r in range(tables.n_routes):
        for k in range(int(tables.route_meta[r, 1])):
            rows.append(np.asarray(tables.route_segs[r, k], np.float32))
    return np.unique(np.stack(rows), axis=0).astype(np.float64)


def line_records(tables):
    return line_table(tables.lines).astype(np.float64)


def box_records(cfg, tables):
    if cfg.toll_buildings and tables.boxes is not None:
        return np.asarray(tables.boxes, np.float32).astype(np.float64)
    return np.zeros((0, 6))


def _tri(x, lo, hi):
    """(exact, strict, loose) membership of lo <= x <= hi, strict / loose with the interval shrunk / grown by EPS (arrays lo, hi ok)."""
    return (x >= lo) & (x <= hi), (x >= lo + EPS) & (x <= hi - EPS), (x >= lo - EPS) & (x <= hi + EPS)


def _and(a, b):
    return a[0] & b[0], a[1] & b[1], a[2] & b[2]


def _project_arc(ex, ey, sg, R, umx, umy, length):
    rho = np.sqrt(ex * ex + ey * ey)
    ang = np.arctan2(sg * (umx * ey - umy * ex), umx * ex + umy * ey)
    return ang * R + 0.5 * length, sg * (R - rho), R / np.maximum(rho, 1e-9)


def funnel_extra(g, sl, w):
    R = g[12]
    if g[5] != 0.0 or R == 0.0:
        return np.zeros_like(sl)
    L, Ds, u1 = g[4], g[14], g[15]
    D = abs(Ds)
    u = np.clip(sl if Ds > 0 else L - sl, 0.0, L)
    R1, R2 = R + 0.5 * w, R - 0.5 * w
    v = L - u
    return np.where(u <= u1, D - (R1 - np.sqrt(np.maximum(R1 * R1 - u * u, 0.0))), R2 - np.sqrt(np.maximum(R2 * R2 - v * v, 0.0)))


def road_test(g, x, y, w):
    """(exact, strict, loose) of the road rule of record g at points (x, y)."""
    if g[5] == 0.0:
        dx, dy = x - g[0], y - g[1]
        sl, lat, ks = dx * g[2] + dy * g[3], dy * g[2] - dx * g[3], 1.0
    else:
        sg, R = (1.0 if g[5] > 0 else -1.0), g[12]
        cx, cy = g[0] - sg * R * g[3], g[1] + sg * R * g[2]
        sl, lat, ks = _project_arc(x - cx, y - cy, sg, R, g[14], g[15], g[4])
    right = (math.floor(g[M.SEG_LANES]) - 0.5) * w + funnel_extra(g, sl, w)
    s_in = ((sl >= 0) & (sl <= g[4]), (sl >= EPS * ks) & (sl <= g[4] - EPS * ks), (sl >= -EPS * ks) & (sl <= g[4] + EPS * ks))
    return _and(s_in, _tri(lat, -right, 0.5 * w))


def line_test(L, x, y, h):
    kind = L[0]
    if kind not in (1.0, 2.0):
        z = np.zeros(np.shape(x), bool)
        return z, z, z
    if L[6] == 0.0:
        dx, dy = x - L[1], y - L[2]
        sl, lat, ks = dx * L[3] + dy * L[4], dy * L[3] - dx * L[4], 1.0
    else:
        sg = 1.0 if L[6] > 0 else -1.0
        sl, lat, ks = _project_arc(x - L[7], y - L[8], sg, 1.0 / abs(L[6]), L[9], L[10], L[5])
    e = EPS * ks
    base = ((sl >= 0) & (sl <= L[5]), (sl >= e) & (sl <= L[5] - e), (sl >= -e) & (sl <= L[5] + e))
    base = _and(base, _tri(np.abs(lat), -np.inf, h))
    if kind == 2.0:
        return base
    md = np.fmod(sl, 6.0)
    dash = (md < 3.0, (md >= e) & (md < 3.0 - e), (md < 3.0 + e) | (md > 6.0 - e))
    return _and(base, dash)


def obb_test(x, y, bx, by, c, s, hl, hw):
    dx, dy = x - bx, y - by
    u, v = dx * c + dy * s, dy * c - dx * s
    return _and(_tri(np.abs(u), -np.inf, hl), _tri(np.abs(v), -np.inf, hw)), u


def prim_bbox(x0, y0, c, s, length, kap, lat0, lat1, pad=0.5):
    sl = np.linspace(0.0, length, 129)
    if kap == 0.0:
        px, py, hc, hs = x0 + c * sl, y0 + s * sl, np.full_like(sl, c), np.full_like(sl, s)
    else:
        a = kap * sl
        hc, hs = c * np.cos(a) - s * np.sin(a), s * np.cos(a) + c * np.sin(a)
        px, py = x0 + (hs - s) / kap, y0 - (hc - c) / kap
    qx = np.concatenate([px - hs * lat0, px - hs * lat1])
    qy = np.concatenate([py + hc * lat0, py + hc * lat1])
    return qx.min() - pad, qx.max() + pad, qy.min() - pad, qy.max() + pad


def spawn_poses(tables, w):
    """[n_spawns, 2] positions of the spawn slots (copo_sim_create's respawn-place pose)."""
    out = []
    for sp in range(tables.n_spawns):
        g = tables.route_segs[tables.spawn_tab[sp, 0], 0].astype(np.float32)
        s0, off = np.float32(tables.spawn_s[sp]), np.float32(tables.spawn_tab[sp, 2] * w)
        out.append((float(g[0] + g[2] * s0 + g[3] * off), float(g[1] + g[3] * s0 - g[2] * off)))
    return np.array(out)


class Map:
    """The static part of a scene: deduplicated roads, lane lines and boxes (float64) with their world boxes."""

    def __init__(self, cfg):
        t, _ = cfg.resolved()
        self.w = float(np.float32(cfg.lane_width))
        self.hl, self.hw = float(np.float32(cfg.veh_half_len)), float(np.float32(cfg.veh_half_wid))
        self.roads, self.lines, self.boxes = road_records(t), line_records(t), box_records(cfg, t)
        self.box_rgb = np.array(BOX_HIDDEN if int(cfg.toll_buildings) == 2 else BOX_SEEN, np.int64)
        self.road_bb = []
        for g in self.roads:
            funnel = abs(g[14]) if (g[5] == 0.0 and g[12] != 0.0) else 0.0
            self.road_bb.append(prim_bbox(g[0], g[1], g[2], g[3], g[4], g[5], 0.5 * self.w,
                                          -((math.floor(g[M.SEG_LANES]) - 0.5) * self.w + funnel)))
        self.line_bb = [prim_bbox(L[1], L[2], L[3], L[4], L[5], L[6], 0.0, 0.0) for L in self.lines]

    def on_road(self, x, y):
        """Exact road membership of points (x, y)."""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        on = np.zeros(x.shape, bool)
        for g in self.roads:
            on |= road_test(g, x, y, self.w)[0]
        return on


def _window(bb, X, Y, pad):
    """index ranges of the pixel columns / rows whose centres may fall in the world box bb grown by pad"""
    jx = np.nonzero((X >= bb[0] - pad) & (X <= bb[1] + pad))[0]
    iy = np.nonzero((Y >= bb[2] - pad) & (Y <= bb[3] + pad))[0]
    if jx.size == 0 or iy.size == 0:
        return None
    return slice(iy[0], iy[-1] + 1), slice(jx[0], jx[-1] + 1)


def _paint(col, amb, win, tri, rgb):
    """opaque layer: definitely in -> rgb, settled; maybe in -> ambiguous"""
    ex, strict, loose = tri
    c, a = col[win], amb[win]
    c[ex] = rgb
    a[strict] = False
    a[loose & ~strict] = True


def blend(below, c, w):
    return (below * (256 - w) + c * w) >> 8


def marker(c):
    return (np.asarray(c, np.int64) * 3) >> 2


def render_frame(mp, state, env, e, view, W, H, trail_snaps=(), K=0):
    """(rgb uint8 [H, W, 3], ambiguous bool [H, W]) of scene e.  state: [16, E, N] float32, env [E, 4] int32 (get_state());
    trail_snaps: the (state, env) snapshots drawn, oldest first (at most K; the newest has age 1)."""
    cx, cy, m = (float(v) for v in np.asarray(view, np.float32))
    X = cx + ((np.arange(W) + 0.5) - W / 2.0) * m
    Y = cy - ((np.arange(H) + 0.5) - H / 2.0) * m
    col = np.empty((H, W, 3), np.int64)
    col[:] = BACKGROUND
    amb = np.zeros((H, W), bool)
    # 1 roads (a union)
    on = [np.zeros((H, W), bool) for _ in range(3)]
    for g, bb in zip(mp.roads, mp.road_bb):
        win = _window(bb, X, Y, m)
        if win is None:
            continue
        xx, yy = np.meshgrid(X[win[1]], Y[win[0]])
        for k, t in enumerate(road_test(g, xx, yy, mp.w)):
            on[k][win] |= t
    _paint(col, amb, (slice(None), slice(None)), on, ROAD)
    # 2 lane lines (a union)
    h = max(0.1, m / 2.0)
    on = [np.zeros((H, W), bool) for _ in range(3)]
    for L, bb in zip(mp.lines, mp.line_bb):
        win = _window(bb, X, Y, h + m)
        if win is None:
            continue
        xx, yy = np.meshgrid(X[win[1]], Y[win[0]])
        for k, t in enumerate(line_test(L, xx, yy, h)):
            on[k][win] |= t
    _paint(col, amb, (slice(None), slice(None)), on, LINE)
    # 3 static boxes
    for B in mp.boxes:
        ext = B[4] + B[5]
        win = _window((B[0] - ext, B[0] + ext, B[1] - ext, B[1] + ext), X, Y, m)
        if win is None:
            continue
        xx, yy = np.meshgrid(X[win[1]], Y[win[0]])
        _paint(col, amb, win, obb_test(xx, yy, B[0], B[1], B[2], B[3], B[4], B[5])[0], mp.box_rgb)
    ext = mp.hl + mp.hw

    def bodies(st):
        si = st.view(np.int32)
        return st[0, e], st[1, e], st[2, e], si[13, e] & 0xFF, si[14, e]

    # 4 trail: snapshots of age Kd .. 1 of the current episode, slots in order, blended
    ep_now = int(env[e, 1])
    Kd = len(trail_snaps)
    for q, (sst, senv) in enumerate(trail_snaps):
        age = Kd - q
        if int(senv[e, 1]) != ep_now:
            continue
        wgt = 160 * (K + 1 - age) // (K + 1)
        for x, y, th, st, aid in zip(*bodies(sst)):
            if st not in (ST_ALIVE, ST_WRECK):
                continue
            c = np.array(WRECK if st == ST_WRECK else PALETTE[aid % 12], np.int64)
            win = _window((x - ext, x + ext, y - ext, y + ext), X, Y, m)
            if win is None:
                continue
            xx, yy = np.meshgrid(X[win[1]], Y[win[0]])
            (ex, strict, loose), _ = obb_test(xx, yy, float(x), float(y), math.cos(th), math.sin(th), mp.hl, mp.hw)
            cc, a = col[win], amb[win]
            cc[ex] = blend(cc[ex], c, wgt)
            a[loose & ~strict] = True
    # 5 vehicles: slot order, opaque, front quarter darkened
    for x, y, th, st, aid in zip(*bodies(state)):
        if st not in (ST_ALIVE, ST_WRECK):
            continue
        c = np.array(WRECK if st == ST_WRECK else PALETTE[aid % 12], np.int64)
        win = _window((x - ext, x + ext, y - ext, y + ext), X, Y, m)
        if win is None:
            continue
        xx, yy = np.meshgrid(X[win[1]], Y[win[0]])
        (ex, strict, loose), u = obb_test(xx, yy, float(x), float(y), math.cos(th), math.sin(th), mp.hl, mp.hw)
        front = (u >= 0.5 * mp.hl, u >= 0.5 * mp.hl + EPS, u >= 0.5 * mp.hl - EPS)
        cc, a = col[win], amb[win]
        cc[ex & ~front[0]] = c
        cc[ex & front[0]] = marker(c)
        settled = strict & (front[1] | ~front[2])       # inside for sure, and on a definite side of the marker line
        a[settled] = False
        a[loose & ~settled] = True
    return col.astype(np.uint8), amb


def render_frames(mp, state, env, scenes, views, W, H, trail_snaps=(), K=0):
    out = [render_frame(mp, state, env, int(e), v, W, H, trail_snaps, K) for e, v in zip(scenes, views)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
