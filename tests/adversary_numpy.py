"""The adversarial-observation rule (copo_adv_obs_seats_f32) restated in float64, row by row and unit by unit.
It shares no code with the kernel or with copo_amd/eval/adversary.py.  A net is (W1 [H][O], b1 [H], W2 [H][H], b2 [H], W3 [4][H],
b3 [4]) in float64; a level is (eps, steer, throttle).

    mu(o)  = the first two outputs of the net on the TRUE row o
    J(o)   = steer mu_0(o) + throttle mu_1(o)
    g      = dJ/do = W1^T (d1 * W2^T (d2 * W3[:2]^T c)),  d_i = 1 - h_i^2,  c = (steer, throttle)
    seen_j = clamp(o_j + eps sign(g_j), 0, 1) for col_lo <= j < col_hi, sign(0) = 0; o_j elsewhere

A row passes through untouched when its level index is outside [0, L), when eps == 0 or when steer == throttle == 0."""
import math

import numpy as np


def forward(net, o):
    """(h1, h2, mu) of one row."""
    W1, b1, W2, b2, W3, b3 = net
    H = len(b1)
    h1 = np.empty(H)
    for i in range(H):
        h1[i] = math.tanh(float(np.dot(W1[i], o)) + b1[i])
    h2 = np.empty(H)
    for i in range(H):
        h2[i] = math.tanh(float(np.dot(W2[i], h1)) + b2[i])
    mu = np.array([float(np.dot(W3[j], h2)) + b3[j] for j in range(2)])
    return h1, h2, mu


def input_gradient(net, o, steer, throttle):
    """dJ/do of one row, J = steer mu_0 + throttle mu_1."""
    W1, b1, W2, b2, W3, b3 = net
    H, O = W1.shape
    h1, h2, _mu = forward(net, o)
    u2 = np.empty(H)
    for i in range(H):
        u2[i] = (1.0 - h2[i] * h2[i]) * (steer * W3[0][i] + throttle * W3[1][i])
    u1 = np.empty(H)
    for i in range(H):
        u1[i] = (1.0 - h1[i] * h1[i]) * float(np.dot(W2[:, i], u2))
    g = np.empty(O)
    for j in range(O):
        g[j] = float(np.dot(W1[:, j], u1))
    return g


def level_index(row, N, k, group, level_of, L):
    """The level of row e N + n driven by member k, or -1: it passes through."""
    g = int(group[row // N])
    lv = int(level_of[g][k])
    return lv if 0 <= lv < L else -1


def is_identity(level):
    eps, steer, throttle = level
    return eps == 0.0 or (steer == 0.0 and throttle == 0.0)


def sign(v):
    return 1.0 if v > 0.0 else (-1.0 if v < 0.0 else 0.0)


def perturb_row(o, g, eps, col_lo, col_hi):
    """One gradient-sign step on a row, in float64."""
    seen = np.array(o, np.float64)
    for j in range(col_lo, col_hi):
        seen[j] = min(max(o[j] + eps * sign(g[j]), 0.0), 1.0)
    return seen


def adversary(nets, obs, N, rows, counts, group, level_of, levels, col_lo, col_hi):
    """obs float [n_out][O] -> (seen, grad, written, perturbed) over the seat lists `rows` [K][cap] / `counts` [K]: `seen` holds NaN in
    rows of no list, `grad` the gradient of every listed row whose level has a direction (zeros for the others), `written` / `perturbed`
    mark the rows that were listed / moved."""
    n_out, O = obs.shape
    seen, grad = np.full((n_out, O), np.nan), np.zeros((n_out, O))
    written, perturbed = np.zeros(n_out, bool), np.zeros(n_out, bool)
    for k in range(len(counts)):
        for r in rows[k][:counts[k]]:
            r = int(r)
            if not 0 <= r < n_out:          # an index outside the rows is no row (the kernels' row look-up): nothing is written
                continue
            o = obs[r].astype(np.float64)
            written[r] = True
            lv = level_index(r, N, k, group, level_of, len(levels))
            seen[r] = o
            if lv < 0:
                continue
            eps, steer, throttle = (float(v) for v in levels[lv])
            if steer == 0.0 and throttle == 0.0:
                continue
            grad[r] = input_gradient(nets[k], o, steer, throttle)
            if eps != 0.0:
                seen[r] = perturb_row(o, grad[r], eps, col_lo, col_hi)
                perturbed[r] = True
    return seen, grad, written, perturbed
