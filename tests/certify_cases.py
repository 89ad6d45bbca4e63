"""Shared by tests/test_certify_cpu.py and tests/test_gpu_certify.py: the inputs of the certified-bounds kernel tests, on adversary_cases'
48 rows (E = 6, N = 8, K = 3, lists of 32, members with 0 / 1 / 17 rows, `COL_LO, COL_HI = 19, 91`, the same weights and observations),
and what the tests share of the references.  No GPU and no native library is touched at import.

The MAIN table.  Member 2's first tile (sixteen rows of the scenes 0, 2, 4 and 5) holds a row kind per scene: eps = 0 (group 0), the
small eps (group 1), the larger eps (group 2) and rows whose group is out of range (scene 5: eight zeros).  Its second tile (row 42,
scene 5) is an all-invalid tile.  Member 1's one-row tile (row 9, masked) is certified at the larger eps.  Three UNIFORM tables put
every listed row of a valid group at eps = 0, at the small and at the larger eps: what the eps = 0, monotonicity and soundness tests
compare across.

EPS_SMALL and EPS_LARGE were chosen on the CPU (test_certify_cpu.py::test_premise_of_the_gpu_tests measures it for every case): interval
propagation through a hidden layer of H units widens a radius by about 0.8 sqrt(H), so at hidden 512 a budget of 0.01 already gives the
trivial box; at these two budgets every width is strictly inside (0, 2 |W3[a]|_1) and every attack stays strictly inside its bound."""
import functools

import numpy as np

import adversary_cases as ac
import certify_numpy as cz
import pgd_cases as pc
import pgd_numpy as pn

HIDDENS, IN_DIMS = ac.HIDDENS, ac.IN_DIMS
E, N, K, CAP, G = ac.E, ac.N, ac.K, ac.CAP, ac.G
COL_LO, COL_HI = ac.COL_LO, ac.COL_HI
GROUP = pc.GROUP                                        # [0, 0, 1, 1, 2, 7]: three groups; scene 5's is out of range
EPS_SMALL, EPS_LARGE = 0.0005, 0.002
# (eps, delta_steer, delta_throttle, 0)
LEVELS = np.array([[0.0, 0.0, 0.0, 0.0], [EPS_SMALL, 0.01, 0.01, 0.0], [EPS_LARGE, 0.01, 0.02, 0.0]], np.float32)
LEVEL_OF = dict(main=np.array([[0, 2, 0], [0, 0, 1], [0, 0, 2]], np.int32), zero=np.zeros((G, K), np.int32),
                small=np.full((G, K), 1, np.int32), large=np.full((G, K), 2, np.int32))
TABLES = tuple(LEVEL_OF)
PAD = 2.0 ** -7
# the attacks of the soundness tests at budget eps: +steer (group 0), +throttle (group 1), untargeted from a random start (group 2)
ATTACK_LEVEL_OF = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.int32)
ATTACK_ITERS, ATTACK_SEED, BOX_DRAWS = 8, 0xCE47, 64


def attack_levels(eps):
    """pgd_numpy levels (eps, steer, throttle, alpha, iters, flags) at one budget."""
    return [(eps, 1.0, 0.0, eps / 4.0, ATTACK_ITERS, 0), (eps, 0.0, 1.0, eps / 4.0, ATTACK_ITERS, 0), (eps, 0.0, 0.0, eps / 4.0, ATTACK_ITERS, 3)]


def attack_words(eps):
    w = np.zeros((3, 8), np.int32)
    for i, lv in enumerate(attack_levels(eps)):
        w[i, :4] = np.array(lv[:4], np.float32).view(np.int32)
        w[i, 4], w[i, 5] = lv[4], lv[5]
    return w


inputs = pc.inputs          # members, nets, obs, rows, counts of a case


def box_draws(obs, eps, seed):
    """BOX_DRAWS observation arrays inside the budget: float32, uniform on [max(o - eps, 0), min(o + eps, 1)] on the LiDAR columns, computed
    so that no rounding leaves the box (a draw is clipped to the float32 interval ends)."""
    rng = np.random.RandomState(seed)
    e = np.float32(eps)
    lo, hi = np.maximum(obs - e, np.float32(0.0)), np.minimum(obs + e, np.float32(1.0))
    # the kernel's own ends are the same two float32 operations, so a draw inside [lo, hi] is inside the kernel's box
    out = []
    for _ in range(BOX_DRAWS):
        x = obs.copy()
        u = rng.rand(*obs.shape).astype(np.float32)
        d = np.clip(lo + u * (hi - lo), lo, hi).astype(np.float32)
        x[:, COL_LO:COL_HI] = d[:, COL_LO:COL_HI]
        out.append(x)
    return out


def torch_ibp(weights, o, eps, dtype):
    """(lo_0, hi_0, lo_1, hi_1, mu_0, mu_1) of one row by the same rule in torch on the CPU, every operation in `dtype`."""
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a).to(dtype) for a in ac.net_of(weights))
    x = torch.from_numpy(np.asarray(o, np.float32)).to(dtype)
    e = torch.tensor(float(np.float32(eps)), dtype=dtype)
    lo, hi = x.clone(), x.clone()
    lo[COL_LO:COL_HI] = torch.clamp(x[COL_LO:COL_HI] - e, min=0.0)
    hi[COL_LO:COL_HI] = torch.clamp(x[COL_LO:COL_HI] + e, max=1.0)
    c, r = (lo + hi) / 2, (hi - lo) / 2
    for W, b in ((W1, b1), (W2, b2)):
        zc, zr = W @ c + b, W.abs() @ r
        l = torch.tanh(zc - zr)
        u = torch.maximum(torch.tanh(zc + zr), l)
        c, r = (l + u) / 2, (u - l) / 2
    mc, mr = W3[:2] @ c + b3[:2], W3[:2].abs() @ r
    m = W3[:2] @ torch.tanh(W2 @ torch.tanh(W1 @ x + b1) + b2) + b3[:2]
    return np.array([mc[0] - mr[0], mc[0] + mr[0], mc[1] - mr[1], mc[1] + mr[1], m[0], m[1]], np.float64)


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim):
    """What one case's tests share, computed once: the float64 model's bounds of the four tables, and the tolerance.  `dev` = the
    deviation of the same rule evaluated in torch fp32 on the CPU from float64, max over the tables, the valid rows and the six numbers
    of |x32 - x64| / max(1, |x64|); `tau` = 4 dev."""
    import torch
    c = inputs(hidden, in_dim)
    out, dev = {}, 0.0
    for table in TABLES:
        bounds, index = cz.certify(c["nets"], c["obs"], N, c["rows"], c["counts"], GROUP, LEVEL_OF[table], LEVELS[:, :3], COL_LO, COL_HI)
        out[table] = dict(bounds=bounds, index=index)
        for k in range(K):
            for r in c["rows"][k][:c["counts"][k]]:
                if index[r] < 0:
                    continue
                x32 = torch_ibp(c["members"][k], c["obs"][r], LEVELS[index[r]][0], torch.float32)
                x64 = bounds[r][:6]
                dev = max(dev, float((np.abs(x32 - x64) / np.maximum(1.0, np.abs(x64))).max()))
    return dict(tables=out, dev=dev, tau=4.0 * dev, member={int(r): k for k in range(K) for r in c["rows"][k][:c["counts"][k]]})


def attacked(hidden, in_dim, eps):
    """pgd_numpy's run of the three attacks at budget eps on the case's lists (float64 gradients): its dict."""
    c = inputs(hidden, in_dim)
    return pn.pgd(c["nets"], c["obs"], N, c["rows"], c["counts"], GROUP, ATTACK_LEVEL_OF, attack_levels(eps), COL_LO, COL_HI, ATTACK_SEED, None, ATTACK_ITERS)
