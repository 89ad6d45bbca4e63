"""The certified-bounds rule (copo_cert_obs_seats_f32, copo_certify_tally) restated: interval propagation in
float64, row by row, and the fold as python loops on float32 differences.  It shares no code with the kernels or with
copo_amd/eval/certify.py.  A net is adversary_numpy's (W1 [H][O], b1, W2 [H][H], b2, W3 [4][H], b3) in float64; a level is (eps,
delta_steer, delta_throttle).

    lo[j] = max(o[j] - eps, 0), hi[j] = min(o[j] + eps, 1) on [col_lo, col_hi), lo = hi = o[j] elsewhere; c0 = (lo + hi) / 2, r0 = (hi - lo) / 2
    layer i = 1, 2:  zc = W_i c + b_i, zr = |W_i| r;  l = tanh(zc - zr), u = max(tanh(zc + zr), l);  c = (l + u) / 2, r = (u - l) / 2
    heads a = 0, 1:  mc = W3[a] . c2 + b3[a], mr = |W3[a]| . r2;  lo_a = mc - mr - pad, hi_a = mc + mr + pad
    bounds = lo_0, hi_0, lo_1, hi_1, mu_0(o), mu_1(o), 1, eps;  eight zeros for a listed row whose level or group is out of range"""
import math

import numpy as np

F = np.float32
ACTED, SPAWNED = 1, 64           # COPO_F_ACTED, COPO_F_SPAWNED of include/copo_hip.h (test_certify_cpu.py checks them against the package)


def box(o, eps, col_lo, col_hi):
    """(c0, r0) of one row."""
    c, r = np.array(o, np.float64), np.zeros(len(o))
    for j in range(col_lo, col_hi):
        lo, hi = max(float(o[j]) - eps, 0.0), min(float(o[j]) + eps, 1.0)
        c[j], r[j] = (lo + hi) / 2.0, (hi - lo) / 2.0
    return c, r


def layer(W, b, c, r):
    zc, zr = W @ c + b, np.abs(W) @ r
    l = np.array([math.tanh(v) for v in zc - zr])
    u = np.maximum(np.array([math.tanh(v) for v in zc + zr]), l)
    return (l + u) / 2.0, (u - l) / 2.0


def mu(net, x):
    """The two action means of one row."""
    W1, b1, W2, b2, W3, b3 = net
    c, _ = layer(W2, b2, *layer(W1, b1, np.asarray(x, np.float64), np.zeros(W1.shape[1])))
    return W3[:2] @ c + b3[:2]


def ibp(net, o, eps, col_lo, col_hi, pad=0.0):
    """(lo [2], hi [2], mu(o) [2]) of one row."""
    W1, b1, W2, b2, W3, b3 = net
    c, r = layer(W2, b2, *layer(W1, b1, *box(o, float(eps), col_lo, col_hi)))
    mc, mr = W3[:2] @ c + b3[:2], np.abs(W3[:2]) @ r
    return mc - mr - pad, mc + mr + pad, mu(net, o)


def trivial_width(net):
    """2 |W3[a]|_1: the width of the box when nothing is known of h2 but |h2| <= 1."""
    return 2.0 * np.abs(net[4][:2]).sum(axis=1)


def level_of_row(row, N, k, group, level_of, n_levels):
    """The level index of row e N + n driven by member k, or -1 (the group or the index is out of range)."""
    g = int(group[row // N])
    if not 0 <= g < len(level_of):
        return -1
    lv = int(level_of[g][k])
    return lv if 0 <= lv < n_levels else -1


def certify(nets, obs, N, rows, counts, group, level_of, levels, col_lo, col_hi, pad=0.0):
    """obs float32 [n_out][O] -> (bounds float64 [n_out][8], NaN in rows of no list; level index per row, -2 in no list, -1 invalid)."""
    n_out = obs.shape[0]
    bounds, index = np.full((n_out, 8), np.nan), np.full(n_out, -2)
    for k in range(len(counts)):
        for r in rows[k][:counts[k]]:
            r = int(r)
            if not 0 <= r < n_out:          # an index outside the rows is no row (the kernels' row look-up): nothing is written
                continue
            lv = level_of_row(r, N, k, group, level_of, len(levels))
            index[r] = lv
            if lv < 0:
                bounds[r] = 0.0
                continue
            eps = float(F(levels[lv][0]))
            lo, hi, m = ibp(nets[k], obs[r].astype(np.float64), eps, col_lo, col_hi, pad)
            bounds[r] = [lo[0], hi[0], lo[1], hi[1], m[0], m[1], 1.0, eps]
    return bounds, index


def q16(x):
    """rint(min(max(x, 0), 1024) * 65536) of a float32: the product is exact, the rounding is half to even."""
    return int(np.rint(np.float64(min(max(F(x), F(0.0)), F(1024.0))) * 65536.0))


def fold(flags, bounds, seat, group, level_of, levels, K, G, out):
    """One step added to out int64 [G][K][8], slot by slot.  `bounds` is float32 [E][N][8]; every difference is one float32 operation."""
    E, N = seat.shape
    bounds, levels = np.asarray(bounds, F), np.asarray(levels, F)
    for e in range(E):
        g = int(group[e])
        if not 0 <= g < G:
            continue
        for n in range(N):
            s = int(seat[e][n])
            if not 0 <= s < K:
                continue
            lv = int(level_of[g][s])
            if not 0 <= lv < len(levels) or not int(flags[e][n]) & ACTED or bounds[e][n][6] != F(1.0):
                continue
            w = out[g][s]
            w[0] += 1
            lo0, hi0, lo1, hi1, mu0, mu1 = (F(v) for v in bounds[e][n][:6])
            if not all(np.isfinite(v) for v in (lo0, hi0, lo1, hi1, mu0, mu1)):
                w[7] += 1
                continue
            dev0, dev1 = max(F(hi0 - mu0), F(mu0 - lo0)), max(F(hi1 - mu1), F(mu1 - lo1))
            ok0, ok1 = bool(dev0 <= levels[lv][1]), bool(dev1 <= levels[lv][2])
            w[1] += ok0 and ok1
            w[2] += ok0
            w[3] += ok1
            w[4] += q16(F(hi0 - lo0))
            w[5] += q16(F(hi1 - lo1))
            w[6] = max(int(w[6]), q16(max(dev0, dev1)))
    return out
