"""The linear-bound rule (copo_lin_obs_seats_f32) restated in float64, row by row.  It shares no code with the kernels
or with copo_amd/eval/certify.py.  A net is adversary_numpy's (W1 [H][O], b1, W2 [H][H], b2, W3 [4][H], b3) in float64; a level is (eps,
delta_steer, delta_throttle); the input box (c0, r0) is certify_numpy's.

    forward, layer i = 1, 2:  zc = W_i c + b_i, zr = |W_i| r;  l = zc - zr, u = zc + zr;  tl = tanh(l), tu = max(tanh(u), tl);
                              c = (tl + tu) / 2, r = (tu - tl) / 2
    a unit on [l, u]:         lam = max(min(1 - tl^2, 1 - tu^2), 0), betaL = tl - lam l, betaU = tu - lam u
    backward, head a:         v2 = W3[a], g2 = v2 lam2;  v1 = W2^T g2, g1 = v1 lam1;  v0 = W1^T g1
                              base = b3[a] + g2 . b2 + g1 . b1 + v0 . c0, rad = |v0| . r0
                              hiL = base + v2+ . betaU2 + v2- . betaL2 + v1+ . betaU1 + v1- . betaL1 + rad
                              loL = base + v2+ . betaL2 + v2- . betaU2 + v1+ . betaL1 + v1- . betaU1 - rad
    interval box:             loI = mc - mr, hiI = mc + mr with mc = W3[a] . c2 + b3[a], mr = |W3[a]| . r2
    per axis:                 lo = max(loL, loI), hi = min(hiL, hiI); lo > hi: (loI, hiI); then lo - pad, hi + pad
    bounds = lo_0, hi_0, lo_1, hi_1, mu_0(o), mu_1(o), 1, eps;  parts = loL_0, hiL_0, loL_1, hiL_1, loI_0, hiI_0, loI_1, hiI_1 (no pad)"""
import math

import numpy as np

import certify_numpy as cz


def relax(l, u):
    """(tl, tu, lam, betaL, betaU) of one tanh unit on [l, u]."""
    tl = math.tanh(l)
    tu = max(math.tanh(u), tl)
    lam = max(min(1.0 - tl * tl, 1.0 - tu * tu), 0.0)
    return tl, tu, lam, tl - lam * l, tu - lam * u


def forward_layer(W, b, c, r):
    """One layer on the box (c, r): (c', r', lam, betaL, betaU), arrays over the units."""
    zc, zr = W @ c + b, np.abs(W) @ r
    q = np.array([relax(float(l), float(u)) for l, u in zip(zc - zr, zc + zr)])
    tl, tu = q[:, 0], q[:, 1]
    return (tl + tu) / 2.0, (tu - tl) / 2.0, q[:, 2], q[:, 3], q[:, 4]


def intersect(loL, hiL, loI, hiI):
    """The result of one axis before the pad."""
    lo, hi = max(loL, loI), min(hiL, hiI)
    return (loI, hiI) if lo > hi else (lo, hi)


def linear(net, o, eps, col_lo, col_hi, pad=0.0):
    """One row: (bounds [6] = lo_0, hi_0, lo_1, hi_1, mu_0, mu_1 with the pad; parts [8] without it)."""
    W1, b1, W2, b2, W3, b3 = net
    c0, r0 = cz.box(o, float(eps), col_lo, col_hi)
    c1, r1, lam1, bl1, bu1 = forward_layer(W1, b1, c0, r0)
    c2, r2, lam2, bl2, bu2 = forward_layer(W2, b2, c1, r1)
    m = cz.mu(net, o)
    bounds, parts = np.zeros(6), np.zeros(8)
    for a in range(2):
        v2 = W3[a]
        g2 = v2 * lam2
        v1 = W2.T @ g2
        g1 = v1 * lam1
        v0 = W1.T @ g1
        base = b3[a] + g2 @ b2 + g1 @ b1 + v0 @ c0
        rad = np.abs(v0) @ r0
        p2, n2, p1, n1 = np.maximum(v2, 0.0), np.minimum(v2, 0.0), np.maximum(v1, 0.0), np.minimum(v1, 0.0)
        hiL = base + p2 @ bu2 + n2 @ bl2 + p1 @ bu1 + n1 @ bl1 + rad
        loL = base + p2 @ bl2 + n2 @ bu2 + p1 @ bl1 + n1 @ bu1 - rad
        mc, mr = W3[a] @ c2 + b3[a], np.abs(W3[a]) @ r2
        loI, hiI = mc - mr, mc + mr
        lo, hi = intersect(loL, hiL, loI, hiI)
        bounds[2 * a], bounds[2 * a + 1], bounds[4 + a] = lo - pad, hi + pad, m[a]
        parts[2 * a], parts[2 * a + 1], parts[4 + 2 * a], parts[5 + 2 * a] = loL, hiL, loI, hiI
    return bounds, parts


def certify(nets, obs, N, rows, counts, group, level_of, levels, col_lo, col_hi, pad=0.0):
    """obs float32 [n_out][O] -> (bounds float64 [n_out][8], parts float64 [n_out][8], NaN in rows of no list, zeros in invalid rows;
    level index per row, -2 in no list, -1 invalid)."""
    n_out = obs.shape[0]
    bounds, parts, index = np.full((n_out, 8), np.nan), np.full((n_out, 8), np.nan), np.full(n_out, -2)
    for k in range(len(counts)):
        for r in rows[k][:counts[k]]:
            r = int(r)
            if not 0 <= r < n_out:          # an index outside the rows is no row (the kernels' row look-up): nothing is written
                continue
            lv = cz.level_of_row(r, N, k, group, level_of, len(levels))
            index[r] = lv
            if lv < 0:
                bounds[r], parts[r] = 0.0, 0.0
                continue
            eps = float(np.float32(levels[lv][0]))
            b, p = linear(nets[k], obs[r].astype(np.float64), eps, col_lo, col_hi, pad)
            bounds[r], parts[r] = list(b) + [1.0, eps], p
    return bounds, parts, index
