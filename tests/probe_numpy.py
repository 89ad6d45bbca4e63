"""The rules of the linear probes (copo_amd/eval/probes.py, copo_probe_targets, copo_probe_accumulate) restated in
numpy: the step's targets with the kernel's own individually rounded fp32 operations (so that the two agree in BITS), the mask of the
positions counted in a fold, the float64 accumulators G / C / T from the rows, and the ridge fit computed from the rows DIRECTLY
(centred design matrix, residuals of every row) -- the reference of `probe_fit`, which only ever sees the accumulators.  No GPU and no
native library."""
import numpy as np

import similarity_numpy as sn

F_ACTED, F_DONE, F_CRASH = 0x01, 0x02, 0x08          # COPO_F_*
PANEL, N_TARGETS, TILE, FOLD_NONE = 16, 8, 64, 255
F32 = np.float32


def trig_table(n):
    a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)


def front_beams(n):
    """The beams of the front quadrant: attribution.column_blocks' rule, ((k + n // 8) % n) * 4 // n == 0."""
    k = np.arange(n)
    return k[((k + n // 8) % n) * 4 // n == 0]


def targets_of(obs, lidar_lo, n, flags, reward):
    """float32 [rows][16] of every row of obs [rows][O] (float32), each operation rounded to fp32 as the kernel rounds it."""
    obs = np.asarray(obs, F32)
    beams = obs[:, lidar_lo:lidar_lo + n]
    trig = trig_table(n)
    out = np.zeros((len(obs), PANEL), F32)
    hits = (beams < F32(1.0)).sum(axis=1)
    any_ = hits > 0
    at = np.argmin(beams, axis=1)                      # the first (lowest) beam at the minimum
    nearest = np.where(any_, beams.min(axis=1), F32(1.0)).astype(F32)
    reach = (F32(1.0) - nearest).astype(F32)
    out[:, 0] = nearest
    out[:, 1] = np.where(any_, (reach * trig[at, 0]).astype(F32), F32(0.0))
    out[:, 2] = np.where(any_, (reach * trig[at, 1]).astype(F32), F32(0.0))
    out[:, 3] = hits.astype(F32) / F32(n)
    out[:, 4] = np.minimum(beams[:, front_beams(n)].min(axis=1), F32(1.0))
    out[:, 5] = np.asarray(reward, F32)
    fl = np.asarray(flags).reshape(-1)
    out[:, 6] = (fl & F_CRASH) != 0
    out[:, 7] = (fl & F_DONE) != 0
    out[:, PANEL - 1] = 1.0
    return out


def padded(obs, width):
    out = np.zeros((len(obs), width), F32)
    out[:, :obs.shape[1]] = obs
    return out


def counted(rows, count, flags, seat, rows_of, fold, slots, f):
    """bool [len(rows)]: similarity's rule, and the fold of the row's scene rows[p] // slots is f."""
    ok = sn.counted(rows, count, flags, seat, -1 if rows_of is None else rows_of)
    r = np.where(ok, np.asarray(rows, np.int64), 0)
    return ok & (np.asarray(fold)[r // int(slots)] == f)


def accumulate(blocks, targets, masks, acc=None):
    """One step added to acc = dict(G [2][B][D][D], C [2][B][D][16], T [2][16][16]) in float64: `blocks` a list of [cap][D] arrays,
    `targets` [cap][16], `masks` the two folds' bool [cap].  Whatever the arrays hold outside a mask is never touched.  G is FULL."""
    B, D = len(blocks), blocks[0].shape[1]
    if acc is None:
        acc = dict(G=np.zeros((2, B, D, D)), C=np.zeros((2, B, D, PANEL)), T=np.zeros((2, PANEL, PANEL)))
    for f in range(2):
        m = np.asarray(masks[f], bool)
        t = np.asarray(targets)[m].astype(np.float64)
        acc["T"][f] += t.T @ t
        for b, x in enumerate(blocks):
            xm = np.asarray(x)[m].astype(np.float64)
            acc["G"][f, b] += xm.T @ xm
            acc["C"][f, b] += xm.T @ t
    return acc


def upper_tiles(G):
    """G with the 64 x 64 tiles below the diagonal set to zero: what the kernel's planes hold."""
    t = np.arange(G.shape[-1]) // TILE
    return np.where(t[:, None] <= t[None, :], G, 0.0)


def fit_direct(X, t, fold, ridge=1e-4):
    """The probes of one block from the rows: X [n][D], t [n][Q], fold [n] (0 train, 1 test, others ignored).  dict(n_train, n_test,
    r2_train [Q], r2_test [Q], weight_norm [Q]); NaN under probes.probe_fit's rules (a target is constant on a fold when its values
    there are all equal)."""
    X, t, fold = np.asarray(X, np.float64), np.asarray(t, np.float64), np.asarray(fold)
    Q, D = t.shape[1], X.shape[1]
    tr, te = fold == 0, fold == 1
    out = dict(n_train=int(tr.sum()), n_test=int(te.sum()), r2_train=np.full(Q, np.nan), r2_test=np.full(Q, np.nan), weight_norm=np.full(Q, np.nan))
    if out["n_train"] < 2:
        return out
    xbar, tbar = X[tr].mean(axis=0), t[tr].mean(axis=0)
    Xc = X[tr] - xbar
    Cxx = Xc.T @ Xc
    trace = float(np.trace(Cxx))
    if not trace > 0.0:
        return out
    w = np.linalg.solve(Cxx + ridge * trace / D * np.eye(D), Xc.T @ (t[tr] - tbar))
    out["weight_norm"] = np.sqrt((w * w).sum(axis=0))
    for m, key in ((tr, "r2_train"), (te, "r2_test")):
        if m.sum() < 2:
            continue
        res = (t[m] - tbar) - (X[m] - xbar) @ w
        sse, sst = (res * res).sum(axis=0), ((t[m] - tbar) ** 2).sum(axis=0)
        varies = np.ptp(t[m], axis=0) > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            out[key] = np.where(varies, 1.0 - sse / sst, np.nan)
    return out


def hash_noise(index, salt=0):
    """A counter hash of the row index -> float64 in [-1, 1): independent of any feature (splitmix64's finaliser)."""
    z = (np.asarray(index, np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 52) - 1.0
