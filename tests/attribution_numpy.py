"""The input-attribution rule (copo_ig_obs_seats_f32, copo_attrib_tally) restated: integrated gradients in float64,
row by row, and the fold as python integers.  It shares no code with the kernels or with copo_amd/eval/attribution.py.  A net is (W1
[H][O], b1 [H], W2 [H][H], b2 [H], W3 [4][H], b3 [4]) in float64.

    b[j]  = base[j] if it is a number, o[j] where it is NaN;  d = o - b
    x_s   = b + ((s - 1/2) / m) d,  s = 1 .. m
    G_a   = sum_s d mu_a / d x at x_s,  d mu_a / d x = W1^T (d1 * W2^T (d2 * W3[a])),  d_i = 1 - h_i^2
    attr_a[j] = d[j] G_a[j] / m (0 where d[j] == 0);  gap_a = (mu_a(o) - mu_a(b)) - sum_j attr_a[j]
"""
import numpy as np

F_ACTED = 1
Q_CLAMP, Q_ONE = 2.0 ** 20, 2.0 ** 32


def forward(net, x):
    """(h1, h2, mu[:2]) of one row."""
    W1, b1, W2, b2, W3, b3 = net
    h1 = np.tanh(W1 @ x + b1)
    h2 = np.tanh(W2 @ h1 + b2)
    return h1, h2, W3[:2] @ h2 + b3[:2]


def mean_gradient(net, x, a):
    """d mu_a / d x of one row."""
    W1, _b1, W2, _b2, W3, _b3 = net
    h1, h2, _mu = forward(net, x)
    u2 = (1.0 - h2 * h2) * W3[a]
    u1 = (1.0 - h1 * h1) * (W2.T @ u2)
    return W1.T @ u1


def baseline_of(o, base):
    return np.where(np.isnan(base), o, base)


def points_of(o, base, m):
    """x_s for s = 1 .. m, [m][O]."""
    b = baseline_of(o, base)
    return np.stack([b + ((s - 0.5) / m) * (o - b) for s in range(1, m + 1)])


def ig_row(net, o, base, m):
    """(attr [2][O], heads [6] = mu_0(o), mu_1(o), mu_0(b), mu_1(b), gap_0, gap_1) of one row."""
    o, base = np.asarray(o, np.float64), np.asarray(base, np.float64)
    b = baseline_of(o, base)
    d = o - b
    mu_o, mu_b = forward(net, o)[2], forward(net, b)[2]
    attr = np.zeros((2, len(o)))
    for a in range(2):
        G = np.zeros(len(o))
        for x in points_of(o, base, m):
            G = G + mean_gradient(net, x, a)
        attr[a] = np.where(d == 0.0, 0.0, d * G / m)
    gap = (mu_o - mu_b) - attr.sum(axis=1)
    return attr, np.concatenate([mu_o, mu_b, gap])


def level_index(row, N, k, group, level_of, L):
    """The level of row e N + n driven by member k, or -1 (group or index out of range)."""
    g = int(group[row // N])
    if not 0 <= g < len(level_of):
        return -1
    lv = int(level_of[g][k])
    return lv if 0 <= lv < L else -1


def integrated_gradients(nets, obs, N, rows, counts, group, level_of, points, base, max_points):
    """obs float [n_out][O] -> (attr [n_out][2][O], heads [n_out][8], listed [n_out], index [n_out]) over the seat lists: `index` is the
    level of an attributed row and -1 elsewhere; a listed row that is not attributed holds zeros; heads[7] is min(m, max_points)."""
    n_out, O = obs.shape
    attr, heads = np.zeros((n_out, 2, O)), np.zeros((n_out, 8))
    listed, index = np.zeros(n_out, bool), np.full(n_out, -1)
    for k in range(len(counts)):
        for r in rows[k][:counts[k]]:
            r = int(r)
            if not 0 <= r < n_out:
                continue
            listed[r] = True
            lv = level_index(r, N, k, group, level_of, len(points))
            m = min(int(points[lv]), int(max_points)) if lv >= 0 else 0
            if m <= 0:
                continue
            index[r] = lv
            attr[r], heads[r][:6] = ig_row(nets[k], obs[r], base[lv], m)
            heads[r][6], heads[r][7] = 1.0, m
    return attr, heads, listed, index


def q32(v):
    """llrint(min(|v|, 2^20) * 2^32) from the fp32 value in float64; NaN counts as 0."""
    v = float(np.float32(v))
    if v != v:
        return 0
    return int(np.rint(min(abs(v), Q_CLAMP) * Q_ONE))


def fold(flags, attr, heads, seat, group, K, G):
    """(words [G][K][8], cols [G][K][2][O]) as python integers in object arrays, from fp32 `attr` [E N][2][O] and `heads` [E N][8]."""
    E, N = seat.shape
    O = attr.shape[-1]
    words, cols = np.zeros((G, K, 8), object), np.zeros((G, K, 2, O), object)
    f32 = np.float32
    for e in range(E):
        g = int(group[e])
        if not 0 <= g < G:
            continue
        for n in range(N):
            k, r = int(seat[e][n]), e * N + n
            if not 0 <= k < K or not int(flags[e][n]) & F_ACTED:
                continue
            h, w = heads[r].astype(f32), words[g][k]
            if h[6] != 1.0:
                w[6] += 1
                continue
            w[0] += 1
            w[1] += q32(f32(h[0]) - f32(h[2]))
            w[2] += q32(f32(h[1]) - f32(h[3]))
            w[3] += q32(h[4])
            w[4] += q32(h[5])
            w[5] = max(w[5], q32(h[4]), q32(h[5]))
            for a in range(2):
                for j in range(O):
                    cols[g][k][a][j] += q32(attr[r][a][j])
    return words, cols
