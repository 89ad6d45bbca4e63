"""Shared by tests/test_pgd_cpu.py and tests/test_gpu_pgd.py: the inputs of the PGD kernel tests, on adversary_cases' 48 rows (E = 6,
N = 8, K = 3, lists of 32, members with 0 / 1 / 17 rows, `COL_LO, COL_HI = 19, 91`, the same weights and observations), and what the
tests share of the references.  No GPU and no native library is touched at import.

One level table.  Member 2's first tile (sixteen rows of the scenes 0, 2, 4 and 5) holds rows of four kinds: targeted with `iters` 4
and alpha = eps / 2 (group 0), untargeted with a random start and `iters` 3 (group 1), noise only -- alpha = 0, a random start, `iters`
1 (group 2) -- and rows that pass through because their scene's group is outside [0, G) (scene 5).  A tile holds rows of four scenes
and a level is chosen per (group, member), so four kinds is what one tile can hold; rows at an identity level and at the index -1 are those of
adversary_cases' table A, which test_gpu_pgd.py also runs.  Member 2's second tile (row 42, scene
5) passes through as a whole.  Member 1's one-row tile (row 9) is targeted with `iters` 2 and a random start.  The launches take `max_iters` = 4;
test_gpu_pgd.py runs the case once more at `max_iters` = 1, which cuts every level short."""
import functools

import numpy as np

import adversary_cases as ac
import pgd_numpy as pn

HIDDENS, IN_DIMS = ac.HIDDENS, ac.IN_DIMS
E, N, K, CAP, G = ac.E, ac.N, ac.K, ac.CAP, ac.G
COL_LO, COL_HI = ac.COL_LO, ac.COL_HI
MAX_ITERS, SEED = 4, 0x5EED0123456789
GROUP = np.array([0, 0, 1, 1, 2, 7], np.int32)          # three groups; scene 5's is out of range
# (eps, steer, throttle, alpha, iters, flags)
LEVELS = [(0.0, 0.0, 0.0, 0.0, 0, 0),                   # 0: identity
          (0.05, 0.0, 1.0, 0.025, 4, 0),                # 1: targeted, four steps of eps / 2
          (0.1, 0.0, 0.0, 0.04, 3, 3),                  # 2: untargeted from a random start, three steps
          (0.1, 0.0, 0.0, 0.0, 1, 3),                   # 3: noise only (untargeted, so that the rows iterate; alpha = 0)
          (0.1, 1.0, -0.5, 0.06, 2, 1)]                 # 4: targeted from a random start, two steps
LEVEL_OF = np.array([[0, 4, 1], [-1, 0, 2], [0, 0, 3]], np.int32)


def words():
    """LEVELS as the kernel reads them: int32 [L][8]."""
    w = np.zeros((len(LEVELS), 8), np.int32)
    for i, lv in enumerate(LEVELS):
        w[i, :4] = np.array(lv[:4], np.float32).view(np.int32)
        w[i, 4], w[i, 5] = lv[4], lv[5]
    return w


def fgsm_levels():
    """adversary_cases' levels as PGD levels: iters = 1, alpha = eps, no flags."""
    return [(float(e), float(s), float(t), float(e), 1, 0) for e, s, t, _ in ac.LEVELS]


def fgsm_words():
    w = np.zeros((len(ac.LEVELS), 8), np.int32)
    w[:, :3] = ac.LEVELS[:, :3].view(np.int32)
    w[:, 3] = ac.LEVELS[:, 0].view(np.int32)
    w[:, 4] = 1
    return w


@functools.lru_cache(maxsize=None)
def inputs(hidden, in_dim):
    ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
    rows, counts = ac.lists()
    return dict(members=ws, nets=[ac.net_of(w) for w in ws], obs=obs, rows=rows, counts=counts)


def model(hidden, in_dim, max_iters=MAX_ITERS, trace=None, tick=None):
    """The model's run of the case at tick 0: on its own float64 gradients, or following a kernel's `trace`."""
    c = inputs(hidden, in_dim)
    return pn.pgd(c["nets"], c["obs"], N, c["rows"], c["counts"], GROUP, LEVEL_OF, LEVELS, COL_LO, COL_HI, SEED, tick, max_iters, trace)


def torch_gradient(weights, x, o, level, dtype):
    """dJ/dx at x of either objective by torch CPU autograd in `dtype`."""
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a).to(dtype) for a in ac.net_of(weights))

    def mu(v):
        return (W3 @ torch.tanh(W2 @ torch.tanh(W1 @ v + b1) + b2) + b3)[:2]
    xt = torch.from_numpy(np.asarray(x, np.float64)).to(dtype).requires_grad_(True)
    m = mu(xt)
    if int(level[5]) & pn.UNTARGETED:
        d = m - mu(torch.from_numpy(np.asarray(o, np.float64)).to(dtype)).detach()
        J = 0.5 * (d * d).sum()
    else:
        J = float(level[1]) * m[0] + float(level[2]) * m[1]
    J.backward()
    return xt.grad.numpy()
