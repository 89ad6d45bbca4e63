"""Shared by tests/test_probe_cpu.py and tests/test_gpu_probes.py: the inputs of the probe tests and their float64 references, computed
once per case.  No GPU and no native library is touched at import.

The planted cases (`planted`): 640 rows, D = 64, fixed seeds, the folds alternating in blocks of 16 rows.  The features are what hidden
activations are -- strongly correlated: six latent directions mixed into 64 columns plus 1e-3 of independent noise, so the ridge (1e-4
of the mean feature variance) leaves about six effective degrees of freedom.  With 64 independent columns an ordinary fit of pure noise
on 320 rows scores about -64 / 320 = -0.2 out of sample, which says nothing about the probe; at six it is -0.02.  Column 63 is zero (a
pad column) and column 62 repeats column 61.  Targets: 0 a fixed linear function of the features, 1 a counter hash of the row index, 2 a
constant.

The targets rows (`target_rows`): observations of 91 / 92 columns with the 72 beams of the bank cases at columns 19 .. 90, rows with
nothing in range, a tie at the minimum, a minimum in each quadrant, and crash / done flags.

The grid cases of the Gram kernel (`grid_case`): workspaces [2 members][cap][2 layers][D] and targets with values in {-1, -0.5, 0, 0.5,
1} (column 15 is 1), NaN at every position that no fold counts, three steps.  Every product is a multiple of 1/4 and every partial sum
stays far below 2^24 quarters, so fp32 holds them exactly in any order: the kernel must equal the float64 model bit for bit.

The forward cases (`rows_case`): n rows like adversary_cases.observations, its members, one scene per row."""
import functools

import numpy as np

import adversary_cases as ac
import probe_numpy as pn

COL_LO, N_BEAMS = ac.COL_LO, ac.COL_HI - ac.COL_LO
POISON = 0x7FC0BEEF
RIDGE = 1e-4
PLANTED_ROWS, PLANTED_D, PLANTED_LATENT, PLANTED_SEEDS = 640, 64, 6, (11, 12, 13)
GRID_VALUES = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32)
GRID_WIDTHS, GRID_COUNTS, GRID_PLANES, GRID_LAUNCHES, GRID_SLACK = (64, 256, 512), (1, 31, 33, 320), (1, 2), 3, 5
GRID_FOLDS, GRID_ROWS_OF = ("mixed", "train", "none"), (None, 1)
GRID_PANEL = (1, 0)              # the blocks in the order (member 1, h1), (member 1, h2), (member 0, h1), (member 0, h2)
GRID_SLOTS = 3                   # rows per scene
E2E_ROWS = 4096                  # the end-to-end case at hidden 64


def block_folds(n, block=16):
    """[n]: train, test, train, ... in blocks of `block` rows."""
    return ((np.arange(n) // block) % 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def planted(seed):
    rng = np.random.RandomState(seed)
    n, D = PLANTED_ROWS, PLANTED_D
    X = rng.randn(n, PLANTED_LATENT) @ rng.randn(PLANTED_LATENT, D) + 1e-3 * rng.randn(n, D) + rng.randn(D)
    X[:, 63] = 0.0
    X[:, 62] = X[:, 61]
    v = rng.randn(D) / np.sqrt(D)
    t = np.stack([X @ v + 0.7, pn.hash_noise(np.arange(n), seed), np.full(n, 0.25)], axis=1)
    return dict(X=X, t=t, fold=block_folds(n))


def stats_of(X, t, fold):
    """The accumulators `probe_fit` reads, from rows: one block, the targets padded to the panel."""
    panel = np.zeros((len(X), pn.PANEL))
    panel[:, :t.shape[1]], panel[:, -1] = t, 1.0
    return pn.accumulate([X], panel, [fold == 0, fold == 1])


def target_rows(in_dim, seed=0):
    """dict(obs [n_out][in_dim], flags, reward, rows, count, cap): the listed rows are 0 .. count - 1 of a shuffled order."""
    rng = np.random.RandomState(500 + in_dim + seed)
    n_out, n = 24, N_BEAMS
    obs = rng.rand(n_out, in_dim).astype(np.float32)
    beams = obs[:, COL_LO:COL_LO + n]
    beams[:] = 0.3 + 0.7 * beams
    beams[rng.rand(n_out, n) < 0.3] = 1.0
    beams[0] = 1.0                                           # nothing in range
    beams[1] = 1.0
    beams[1, [40, 7, 55]] = 0.25                             # a tie at the minimum: beam 7 is the nearest
    for r, k in ((2, 0), (3, 8), (4, 9), (5, 20), (6, 36), (7, 50), (8, 62), (9, 63), (10, 71)):      # a minimum in every quadrant and at their edges
        beams[r, k] = 0.125
    beams[11, 65] = 0.0                                      # a beam at zero, in front
    beams[12] = np.float32(0.5)                              # every beam ties
    flags = (rng.randint(0, 256, n_out) & ~(pn.F_CRASH | pn.F_DONE)).astype(np.uint8)
    flags[[2, 5, 13]] |= pn.F_CRASH | pn.F_DONE
    flags[[3, 14]] |= pn.F_DONE
    flags[15] |= pn.F_CRASH
    reward = rng.randn(n_out).astype(np.float32)
    count, cap = 20, 23
    rows = np.zeros(cap, np.int64)
    rows[:count] = np.concatenate([np.arange(16), rng.choice(np.arange(16, n_out), count - 16, replace=False)])[rng.permutation(count)]
    return dict(obs=obs, flags=flags, reward=reward, rows=rows, count=count, cap=cap, n_out=n_out)


@functools.lru_cache(maxsize=None)
def grid_case(D, count, rows_of, folds, seed=0):
    """One grid case: the list, seat and fold tables, GRID_LAUNCHES steps of (workspace [2][cap][2][D], targets [cap][16], flags, the two
    masks) and the float64 model's accumulators over all steps, the blocks in GRID_PANEL's order."""
    rng = np.random.RandomState(1000 * D + 10 * count + seed + (0 if rows_of is None else 7) + 3 * GRID_FOLDS.index(folds))
    cap = count + GRID_SLACK
    E = 2 * cap // GRID_SLOTS + 2
    n_out = E * GRID_SLOTS
    listed = np.sort(rng.choice(n_out, cap, replace=False)).astype(np.int64)
    seat = rng.randint(-1, 2, n_out).astype(np.int32)
    if count >= 31:
        seat[listed[:count:3]] = 1
    fold = dict(mixed=rng.choice(np.array([0, 1, pn.FOLD_NONE], np.uint8), E, p=[0.45, 0.45, 0.1]), train=np.zeros(E, np.uint8),
                none=np.full(E, pn.FOLD_NONE, np.uint8))[folds]
    steps, acc = [], None
    for _ in range(GRID_LAUNCHES):
        flags = (rng.randint(0, 128, n_out) & ~pn.F_ACTED).astype(np.uint8)
        flags[rng.rand(n_out) < 0.8] |= pn.F_ACTED
        masks = [pn.counted(listed, count, flags, seat, rows_of, fold, GRID_SLOTS, f) for f in range(2)]
        ws = GRID_VALUES[rng.randint(0, len(GRID_VALUES), (2, cap, 2, D))]
        tg = GRID_VALUES[rng.randint(0, len(GRID_VALUES), (cap, pn.PANEL))]
        tg[:, -1] = 1.0
        dead = ~(masks[0] | masks[1])
        ws[:, dead] = np.nan
        tg[dead] = np.nan
        acc = pn.accumulate([ws[m, :, layer] for m in GRID_PANEL for layer in range(2)], tg, masks, acc)
        steps.append((ws, tg, flags, masks))
    return dict(rows=listed, count=count, cap=cap, n_out=n_out, E=E, seat=seat, fold=fold, steps=steps, acc=acc,
                base=np.array([(m * cap * 2 + layer) * D for m in GRID_PANEL for layer in range(2)], np.int64))


@functools.lru_cache(maxsize=None)
def grid_obs_case(seed=0):
    """The observation block's call shape: ONE block of width 128 at base 0, stride 128, 75 listed rows."""
    rng = np.random.RandomState(77 + seed)
    D, count, cap, slots = 128, 75, 80, 4
    E = 50
    n_out = E * slots
    listed = np.sort(rng.choice(n_out, cap, replace=False)).astype(np.int64)
    seat = rng.randint(0, 2, n_out).astype(np.int32)
    fold = rng.choice(np.array([0, 1, pn.FOLD_NONE], np.uint8), E, p=[0.45, 0.45, 0.1])
    steps, acc = [], None
    for _ in range(GRID_LAUNCHES):
        flags = np.where(rng.rand(n_out) < 0.8, pn.F_ACTED, 0).astype(np.uint8)
        masks = [pn.counted(listed, count, flags, seat, None, fold, slots, f) for f in range(2)]
        x = GRID_VALUES[rng.randint(0, len(GRID_VALUES), (cap, D))]
        tg = GRID_VALUES[rng.randint(0, len(GRID_VALUES), (cap, pn.PANEL))]
        tg[:, -1] = 1.0
        dead = ~(masks[0] | masks[1])
        x[dead], tg[dead] = np.nan, np.nan
        acc = pn.accumulate([x], tg, masks, acc)
        steps.append((x, tg, flags, masks))
    return dict(rows=listed, count=count, cap=cap, n_out=n_out, E=E, D=D, seat=seat, fold=fold, steps=steps, acc=acc)


def observations(in_dim, n, seed=0):
    """[n][in_dim] float32 like adversary_cases.observations: in [0, 1], a tenth of the beams exactly 1 and a few exactly 0."""
    rng = np.random.RandomState(ac.OBS_SEED + in_dim + 17 * n + seed)
    obs = rng.rand(n, in_dim).astype(np.float32)
    beams = obs[:, ac.COL_LO:ac.COL_HI]
    u = rng.rand(*beams.shape)
    beams[u < 0.10] = 1.0
    beams[u > 0.98] = 0.0
    return obs


@functools.lru_cache(maxsize=None)
def rows_case(hidden, in_dim, n):
    """Members and n observation rows, per-row folds in blocks of 16, and the step's targets of the rows with made-up flags and rewards."""
    rng = np.random.RandomState(9000 + hidden + in_dim + n)
    obs = observations(in_dim, n)
    flags = rng.randint(0, 256, n).astype(np.uint8)
    reward = rng.randn(n).astype(np.float32)
    return dict(members=ac.members(in_dim, hidden), obs=obs, fold=block_folds(n), flags=flags, reward=reward,
                targets=pn.targets_of(obs, COL_LO, N_BEAMS, flags, reward))


def planted_targets(h1, n):
    """[n][2]: a fixed linear function of member 0's first layer `h1` [n][H], and the counter hash of the row index."""
    H = h1.shape[1]
    v = np.random.RandomState(31).randn(H) / np.sqrt(H)
    return np.stack([np.asarray(h1, np.float64) @ v + 0.1, pn.hash_noise(np.arange(n), 5)], axis=1).astype(np.float32)


def torch_stats32(blocks, panel, masks):
    """dict(G, C, T) formed by torch fp32 matmuls on the CPU: the yardstick of the kernel's fp32 deviation."""
    import torch
    B, D = len(blocks), blocks[0].shape[1]
    out = dict(G=np.zeros((2, B, D, D)), C=np.zeros((2, B, D, pn.PANEL)), T=np.zeros((2, pn.PANEL, pn.PANEL)))
    for f in range(2):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(panel, np.float32)[masks[f]]))
        out["T"][f] = (t.T @ t).numpy()
        for b, x in enumerate(blocks):
            xm = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)[masks[f]]))
            out["G"][f, b], out["C"][f, b] = (xm.T @ xm).numpy(), (xm.T @ t).numpy()
    return out
