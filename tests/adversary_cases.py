"""Shared by tests/test_adversary_cpu.py and tests/test_gpu_adversary.py: the inputs of the kernel tests (the premise test measures, on
the float64 model alone, what the GPU tests rely on for exactly these inputs) and the float64 / float32 references.  No GPU and no
native library is touched at import."""
import functools

import numpy as np

import adversary_numpy as an
import bank_cases as bc

HIDDENS, IN_DIMS, TABLES = (64, 128, 256, 512), (91, 92), ("A", "B")
E, N, K, CAP, G = 6, 8, 3, 32, 3                  # 48 rows, three members, lists of 32 rows at the most, three scene groups
COL_LO, COL_HI = 19, 91                           # the LiDAR block of both observation widths
WEIGHT_SEED, OBS_SEED = 4100, 4200                # + in_dim
GROUP = np.array([0, 0, 1, 1, 2, 2], np.int32)
# member 0: no seat.  Member 1: row 9 alone (a one-row tile).  Member 2: seventeen rows -- tile 0 = rows of groups 0 (five), 1 (five)
# and 2 (six), tile 1 = row 42 alone (masked)
ROWS_1 = [9]
ROWS_2 = [0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 32, 33, 34, 35, 40, 41, 42]
LEVELS = np.array([[0.0, 0.0, 0.0, 0.0], [0.05, 0.0, 1.0, 0.0], [0.1, 1.0, -0.5, 0.0], [0.0, 1.0, 0.0, 0.0]], np.float32)
# level_of [G][K].  A: tile 0 of member 2 holds rows of levels 1 and 2 and rows with index -1; its tile 1 (row 42, index -1) is an
# all-identity tile.  B: tile 0 holds identity rows (level 0), index -1 rows and level-2 rows; tile 1 is a one-row tile WITH a gradient;
# member 1's row is at level 3 (eps == 0 with a direction: it passes through, and has a gradient where `grad` is asked for)
LEVEL_OF = dict(A=np.array([[0, 1, 1], [0, 0, 2], [0, 0, -1]], np.int32), B=np.array([[0, 3, 0], [0, 0, -1], [0, 0, 2]], np.int32))


def lists():
    rows = np.zeros((K, CAP), np.int64)
    rows[1, :len(ROWS_1)] = ROWS_1
    rows[2, :len(ROWS_2)] = ROWS_2
    return rows, np.array([0, len(ROWS_1), len(ROWS_2)], np.int32)


def members(in_dim, hidden):
    """Three random populations in the torch key layout: tanh layers of unit gain, a small head (bank_cases.random_population)."""
    base = bc.random_population(in_dim, hidden, WEIGHT_SEED + in_dim)
    return [base] + [bc.perturbed(base, s) for s in range(1, K)]


def net_of(weights, dtype=np.float64):
    """(W1, b1, W2, b2, W3, b3), weights [out][in], of a population in the torch key layout."""
    out = []
    for name in bc.TORCH_LAYERS:
        out += [np.asarray(weights[name + ".weight"], dtype), np.asarray(weights[name + ".bias"], dtype)]
    return tuple(out)


def observations(in_dim):
    """[E N][in_dim] float32 in [0, 1]; a tenth of the beams read exactly 1 (nothing in range) and a few exactly 0, so both clamps act."""
    rng = np.random.RandomState(OBS_SEED + in_dim)
    obs = rng.rand(E * N, in_dim).astype(np.float32)
    beams = obs[:, COL_LO:COL_HI]
    u = rng.rand(*beams.shape)
    beams[u < 0.10] = 1.0
    beams[u > 0.98] = 0.0
    return obs


def torch_gradient(weights, o, steer, throttle, dtype):
    """dJ/do of one row by torch CPU autograd in `dtype`."""
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a).to(dtype) for a in net_of(weights))
    x = torch.from_numpy(np.asarray(o, np.float64)).to(dtype).requires_grad_(True)
    h2 = torch.tanh(W2 @ torch.tanh(W1 @ x + b1) + b2)
    mu = W3 @ h2 + b3
    (steer * mu[0] + throttle * mu[1]).backward()
    return x.grad.numpy()


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim, table):
    """What one case's tests share, computed once: the float64 model's outputs, the fp32 deviation and tau.
    `dev` = max over the rows with a gradient of max_j |g32 - g64| / max_j |g64|, g32 by torch fp32 CPU autograd; `tau` = 4 dev."""
    import torch
    ws, obs = members(in_dim, hidden), observations(in_dim)
    rows, counts = lists()
    nets = [net_of(w) for w in ws]
    seen, grad, written, perturbed = an.adversary(nets, obs, N, rows, counts, GROUP, LEVEL_OF[table], LEVELS[:, :3], COL_LO, COL_HI)
    dev = 0.0
    for k in range(K):
        for r in rows[k][:counts[k]]:
            lv = an.level_index(int(r), N, k, GROUP, LEVEL_OF[table], len(LEVELS))
            if lv < 0 or (LEVELS[lv][1] == 0.0 and LEVELS[lv][2] == 0.0):
                continue
            g32 = torch_gradient(ws[k], obs[r], float(LEVELS[lv][1]), float(LEVELS[lv][2]), torch.float32)
            dev = max(dev, float(np.abs(g32.astype(np.float64) - grad[r]).max() / np.abs(grad[r]).max()))
    return dict(members=ws, obs=obs, rows=rows, counts=counts, seen=seen, grad=grad, written=written, perturbed=perturbed, dev=dev, tau=4.0 * dev)


def small_share(ref):
    """(share of the LiDAR elements of the perturbed rows with |g| <= tau max|g| of their row, rows with an all-zero gradient)."""
    g = ref["grad"][ref["perturbed"]]
    top = np.abs(g).max(axis=1, keepdims=True)
    small = np.abs(g[:, COL_LO:COL_HI]) <= ref["tau"] * top
    return float(small.mean()), int((top == 0.0).sum())
