"""Shared by tests/test_attribution_cpu.py and tests/test_gpu_attribution.py: the inputs of the kernel tests -- adversary_cases' 48 rows,
lists, members and observations -- the attribution levels and tables, and the float64 / float32 references.  No GPU and no native
library is touched at import."""
import functools

import numpy as np

import adversary_cases as ac
import attribution_numpy as az

HIDDENS, IN_DIMS, TABLES = ac.HIDDENS, ac.IN_DIMS, ("A", "B", "C")
E, N, K, CAP, G = ac.E, ac.N, ac.K, ac.CAP, ac.G
COL_LO, COL_HI = ac.COL_LO, ac.COL_HI
MAX_POINTS = 32
# level 0: the identity.  1: one point from a row baseline with masked columns (the first ten, and every third beam).  2: four points
# from the clear road (LiDAR block 1.0, everything else masked).  3: thirty-two points from zeros.
POINTS = np.array([0, 1, 4, 32], np.int32)
# level_of [G][K] (member 0 has no seat, member 1 row 9 of group 0, member 2 seventeen rows: adversary_cases).  A: member 2's tile 0
# holds rows at 4 points, at 32 points and rows with index -1; its tile 1 (row 42, index -1) is a tile without an attributed row.
# B: tile 0 holds identity rows, one-point rows and four-point rows, tile 1 is a one-row tile that IS attributed; member 1's row runs 32
# points.  C: A's table with scene 2 (rows 16 .. 23) in a group outside [0, G).
LEVEL_OF = dict(A=np.array([[0, 1, 2], [0, 0, 3], [0, 0, -1]], np.int32), B=np.array([[0, 3, 0], [0, 0, 1], [0, 0, 2]], np.int32))
LEVEL_OF["C"] = LEVEL_OF["A"]
GROUPS = dict(A=ac.GROUP, B=ac.GROUP, C=np.array([0, 0, 7, 1, 2, 2], np.int32))
ATTRIBUTED = dict(A=11, B=13, C=6)         # rows attributed per table


def baselines(in_dim):
    """base float32 [4][in_dim]: NaN keeps the row's own value."""
    base = np.full((len(POINTS), in_dim), np.nan, np.float32)
    row = np.random.RandomState(4300 + in_dim).rand(in_dim).astype(np.float32)
    row[:10] = np.nan
    row[COL_LO:COL_HI:3] = np.nan
    base[1] = row
    base[2][COL_LO:COL_HI] = 1.0
    base[3] = 0.0
    return base


def level_words():
    w = np.zeros((len(POINTS), 4), np.int32)
    w[:, 0] = POINTS
    return w


def torch_ig_row(weights, o, base, m, dtype):
    """attribution_numpy.ig_row by torch on the CPU in `dtype`, all points of the row in one batch."""
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a).to(dtype) for a in ac.net_of(weights))
    o, base = torch.from_numpy(np.asarray(o, np.float64)).to(dtype), torch.from_numpy(np.asarray(base, np.float64)).to(dtype)
    b = torch.where(torch.isnan(base), o, base)
    d = o - b
    cs = (torch.arange(1, m + 1, dtype=dtype) - 0.5) / m
    X = torch.cat([torch.stack([o, b]), b[None] + cs[:, None] * d[None]])
    h1 = torch.tanh(X @ W1.T + b1)
    h2 = torch.tanh(h1 @ W2.T + b2)
    mu = h2[:2] @ W3[:2].T + b3[:2]
    attr = []
    for a in range(2):
        u2 = (1.0 - h2[2:] * h2[2:]) * W3[a]
        u1 = (u2 @ W2) * (1.0 - h1[2:] * h1[2:])
        G = (u1 @ W1).sum(0)
        attr.append(torch.where(d == 0, torch.zeros_like(d), d * G / m))
    attr = torch.stack(attr)
    gap = (mu[0] - mu[1]) - attr.sum(1)
    return attr.numpy(), torch.cat([mu[0], mu[1], gap]).numpy()


def rel(x, x64):
    return float((np.abs(np.asarray(x, np.float64) - x64) / np.maximum(1.0, np.abs(x64))).max())


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim):
    """What one case's tests share, computed once: per table the float64 model's `attr`, `heads`, `listed`, `index`; `dev` = the largest
    |x32 - x64| / max(1, |x64|) over attr and heads[:6] of every attributed row of every table, x32 by `torch_ig_row` in fp32; tau = 4 dev."""
    import torch
    ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
    rows, counts = ac.lists()
    nets, base = [ac.net_of(w) for w in ws], baselines(in_dim)
    seat = np.full(E * N, -1, np.int32)
    for k in range(K):
        seat[rows[k][:counts[k]]] = k
    tables, dev = {}, 0.0
    for t in TABLES:
        attr, heads, listed, index = az.integrated_gradients(nets, obs, N, rows, counts, GROUPS[t], LEVEL_OF[t], POINTS, base.astype(np.float64),
                                                             MAX_POINTS)
        tables[t] = dict(attr=attr, heads=heads, listed=listed, index=index)
        for r in np.flatnonzero(index >= 0):
            a32, h32 = torch_ig_row(ws[seat[r]], obs[r], base[index[r]], int(POINTS[index[r]]), torch.float32)
            dev = max(dev, rel(a32, attr[r]), rel(h32, heads[r][:6]))
    return dict(members=ws, obs=obs, rows=rows, counts=counts, seat=seat.reshape(E, N), base=base, tables=tables, dev=dev, tau=4.0 * dev)


def step_flags(seed=4400):
    """uint8 [E][N] of one step: about three quarters of the slots acted, a few of them done."""
    rng = np.random.RandomState(seed)
    return ((rng.rand(E, N) < 0.75) * 1 + (rng.rand(E, N) < 0.2) * 2).astype(np.uint8)
