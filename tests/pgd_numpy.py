"""The iterated adversarial-observation rule (copo_pgd_obs_seats_f32) restated in numpy.  The start, the step and
the projection are float32, operation by operation, so they give the kernel's bits; the gradient of both objectives is float64, on
adversary_numpy's functions.  It shares no code with the kernel or with copo_amd/eval/pgd.py.  A net is adversary_numpy's; a level is
(eps, steer, throttle, alpha, iters, flags), flags bit 0 = random start, bit 1 = untargeted.

    it       = min(iters, max_iters)
    x_0      = o; with a random start x_0[j] = clamp(o[j] + eps u, 0, 1) on [col_lo, col_hi), u = 2 uniform01(h) - 1,
               h = hash_rng(seed, row, tick, j - col_lo, 40)
    g_i      = dJ/dx at x_i; J = steer mu_0 + throttle mu_1, or untargeted J = |mu(x) - mu(o)|^2 / 2
    x_{i+1}  = clamp(min(max(x_i + alpha sign(g_i), o - eps), o + eps), 0, 1) on the columns, sign(0) = 0

A row passes through when its level or group is out of range, eps == 0, it <= 0, or the level is targeted with steer == throttle == 0."""
import numpy as np

import adversary_numpy as an
from fault_numpy import hash_rng

F = np.float32
RANDOM_START, UNTARGETED, STREAM = 1, 2, 40


def uniform_pm1(h):
    """2 uniform01(h) - 1 in float32; every operation is exact."""
    u01 = F(F(F(h >> 9) + F(0.5)) * F(2.0 ** -23))
    return F(F(F(2.0) * u01) - F(1.0))


def level_of_row(row, N, k, group, level_of, n_levels):
    """The level index of row e N + n driven by member k, or -1 (the group or the index is out of range)."""
    g = int(group[row // N])
    if not 0 <= g < len(level_of):
        return -1
    lv = int(level_of[g][k])
    return lv if 0 <= lv < n_levels else -1


def iterations(level, max_iters):
    """How often a row at `level` iterates; 0: it passes through."""
    eps, steer, throttle, _alpha, iters, flags = level
    it = min(int(iters), int(max_iters))
    if eps == 0.0 or it <= 0 or (not (int(flags) & UNTARGETED) and steer == 0.0 and throttle == 0.0):
        return 0
    return it


def start(o, level, seed, row, tick, col_lo, col_hi):
    x = np.array(o, F)
    if int(level[5]) & RANDOM_START:
        eps = F(level[0])
        for j in range(col_lo, col_hi):
            y = F(x[j] + F(eps * uniform_pm1(hash_rng(seed, row, tick, j - col_lo, STREAM))))
            x[j] = min(max(y, F(0.0)), F(1.0))
    return x


def step(x, o, g, level, col_lo, col_hi):
    """x_{i+1} of x_i (float32) under the gradient g (any float type: only its signs count)."""
    eps, alpha = F(level[0]), F(level[3])
    out = np.array(x, F)
    for j in range(col_lo, col_hi):
        y = F(x[j] + F(alpha * F(an.sign(g[j]))))
        y = min(max(y, F(o[j] + F(-eps))), F(o[j] + eps))
        out[j] = min(max(y, F(0.0)), F(1.0))
    return out


def mu(net, x):
    return an.forward(net, np.asarray(x, np.float64))[2]


def objective(net, x, o, level):
    """J(x) in float64."""
    m = mu(net, x)
    if int(level[5]) & UNTARGETED:
        d = m - mu(net, o)
        return 0.5 * float(d @ d)
    return float(level[1]) * m[0] + float(level[2]) * m[1]


def gradient(net, x, o, level):
    """dJ/dx at x in float64: the seed is (steer, throttle), or mu(x) - mu(o)."""
    if int(level[5]) & UNTARGETED:
        c = mu(net, x) - mu(net, o)
    else:
        c = (float(level[1]), float(level[2]))
    return an.input_gradient(net, np.asarray(x, np.float64), float(c[0]), float(c[1]))


def run_row(net, o, level, it, seed, row, tick, col_lo, col_hi, grads=None):
    """The iterates [x_0 .. x_it] of one row.  `grads` [it][O]: gradients to follow (a kernel's trace) instead of the model's own."""
    xs = [start(o, level, seed, row, tick, col_lo, col_hi)]
    for i in range(it):
        g = gradient(net, xs[-1], o, level) if grads is None else grads[i]
        xs.append(step(xs[-1], o, g, level, col_lo, col_hi))
    return xs


def pgd(nets, obs, N, rows, counts, group, level_of, levels, col_lo, col_hi, seed, tick, max_iters, trace=None):
    """obs float32 [n_out][O] -> dict over the seat lists: `seen` float32 (NaN in rows of no list), `its` (iterations per row, -1 in no
    list), `iterates` {row: [x_0 ..]}, `level` {row: level}, `member` {row: k}.  `tick`: int per row or None (0).  With `trace`
    [max_iters][n_out][O] the steps follow the trace's signs, else the float64 gradient."""
    n_out, O = obs.shape
    seen, its = np.full((n_out, O), np.nan, F), np.full(n_out, -1)
    iterates, level, member = {}, {}, {}
    for k in range(len(counts)):
        for r in rows[k][:counts[k]]:
            r = int(r)
            if not 0 <= r < n_out:          # an index outside the rows is no row (the kernels' row look-up): nothing is written
                continue
            seen[r], its[r], member[r] = obs[r], 0, k
            lv = level_of_row(r, N, k, group, level_of, len(levels))
            if lv < 0:
                continue
            it = iterations(levels[lv], max_iters)
            if it == 0:
                continue
            t = 0 if tick is None else int(tick[r])
            xs = run_row(nets[k], obs[r], levels[lv], it, seed, r, t, col_lo, col_hi, None if trace is None else trace[:it, r])
            seen[r], its[r], iterates[r], level[r] = xs[-1], it, xs, levels[lv]
    return dict(seen=seen, its=its, iterates=iterates, level=level, member=member)
