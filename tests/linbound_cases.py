"""Shared by tests/test_linbound_cpu.py and tests/test_gpu_linbound.py: the inputs of the linear-bound kernel tests, on certify_cases' /
pgd_cases' 48 rows (E = 6, N = 8, K = 3, lists of 32, members with 0 / 1 / 17 rows, `COL_LO, COL_HI = 19, 91`, the same weights and
observations), and what the tests share of the references.  No GPU and no native library is touched at import.

Three budgets: certify_cases' EPS_SMALL and EPS_LARGE, and EPS_WIDE = 0.01, where interval propagation alone is close to trivial at
hidden 512 and the linear box is not.  The MAIN table has 8o's positions: member 2's first tile (sixteen rows of the scenes 0, 2, 4 and 5)
holds eps = 0 (group 0), the small budget (group 1), the wide budget (group 2) and rows whose group is out of range (scene 5: eight
zeros); its second tile (row 42, scene 5) is an all-invalid tile; member 1's one-row tile (row 9, masked) runs at the larger budget.  Four
UNIFORM tables put every listed row of a valid group at eps = 0 and at each of the three budgets."""
import functools

import numpy as np

import adversary_cases as ac
import certify_cases as cc
import linbound_numpy as lz

HIDDENS, IN_DIMS = cc.HIDDENS, cc.IN_DIMS
E, N, K, CAP, G = cc.E, cc.N, cc.K, cc.CAP, cc.G
COL_LO, COL_HI = cc.COL_LO, cc.COL_HI
GROUP = cc.GROUP
EPS_SMALL, EPS_LARGE, EPS_WIDE = cc.EPS_SMALL, cc.EPS_LARGE, 0.01
BUDGETS = (("small", EPS_SMALL), ("large", EPS_LARGE), ("wide", EPS_WIDE))
# (eps, delta_steer, delta_throttle, 0)
LEVELS = np.array([[0.0, 0.0, 0.0, 0.0], [EPS_SMALL, 0.01, 0.01, 0.0], [EPS_LARGE, 0.01, 0.02, 0.0], [EPS_WIDE, 0.05, 0.05, 0.0]], np.float32)
LEVEL_OF = dict(main=np.array([[0, 2, 0], [0, 0, 1], [0, 0, 3]], np.int32), zero=np.zeros((G, K), np.int32),
                small=np.full((G, K), 1, np.int32), large=np.full((G, K), 2, np.int32), wide=np.full((G, K), 3, np.int32))
TABLES = tuple(LEVEL_OF)
PAD = cc.PAD
NUMBERS = 14          # what a row is compared on: lo_0, hi_0, lo_1, hi_1, mu_0, mu_1 of `bounds` and the eight `parts`

inputs = cc.inputs          # members, nets, obs, rows, counts of a case


def torch_linear(weights, o, eps, dtype):
    """The NUMBERS of one row by the same rule in torch on the CPU, every operation in `dtype`."""
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a).to(dtype) for a in ac.net_of(weights))
    x = torch.from_numpy(np.asarray(o, np.float32)).to(dtype)
    e = torch.tensor(float(np.float32(eps)), dtype=dtype)
    lo, hi = x.clone(), x.clone()
    lo[COL_LO:COL_HI] = torch.clamp(x[COL_LO:COL_HI] - e, min=0.0)
    hi[COL_LO:COL_HI] = torch.clamp(x[COL_LO:COL_HI] + e, max=1.0)
    c0, r0 = (lo + hi) / 2, (hi - lo) / 2
    c, r, relax = c0, r0, []
    for W, b in ((W1, b1), (W2, b2)):
        zc, zr = W @ c + b, W.abs() @ r
        l, u = zc - zr, zc + zr
        tl = torch.tanh(l)
        tu = torch.maximum(torch.tanh(u), tl)
        lam = torch.clamp(torch.minimum(1 - tl * tl, 1 - tu * tu), min=0.0)
        relax.append((lam, tl - lam * l, tu - lam * u))
        c, r = (tl + tu) / 2, (tu - tl) / 2
    (lam1, bl1, bu1), (lam2, bl2, bu2) = relax
    m = W3[:2] @ torch.tanh(W2 @ torch.tanh(W1 @ x + b1) + b2) + b3[:2]
    bounds, parts = [0.0] * 6, [0.0] * 8
    for a in range(2):
        v2 = W3[a]
        g2 = v2 * lam2
        v1 = W2.T @ g2
        g1 = v1 * lam1
        v0 = W1.T @ g1
        base = b3[a] + g2 @ b2 + g1 @ b1 + v0 @ c0
        rad = v0.abs() @ r0
        p2, n2, p1, n1 = v2.clamp(min=0.0), v2.clamp(max=0.0), v1.clamp(min=0.0), v1.clamp(max=0.0)
        hiL = base + p2 @ bu2 + n2 @ bl2 + p1 @ bu1 + n1 @ bl1 + rad
        loL = base + p2 @ bl2 + n2 @ bu2 + p1 @ bl1 + n1 @ bu1 - rad
        mc, mr = W3[a] @ c + b3[a], W3[a].abs() @ r
        loI, hiI = mc - mr, mc + mr
        lo_a, hi_a = lz.intersect(float(loL), float(hiL), float(loI), float(hiI))
        bounds[2 * a], bounds[2 * a + 1], bounds[4 + a] = lo_a, hi_a, float(m[a])
        parts[2 * a], parts[2 * a + 1], parts[4 + 2 * a], parts[5 + 2 * a] = float(loL), float(hiL), float(loI), float(hiI)
    return np.array(bounds + parts, np.float64)


def numbers(bounds, parts):
    """[.., 14]: the six numbers of `bounds` and the eight of `parts`."""
    return np.concatenate([np.asarray(bounds, np.float64)[..., :6], np.asarray(parts, np.float64)], axis=-1)


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim):
    """What one case's tests share, computed once: the float64 model's bounds and parts of the five tables (pad = 0), and the tolerance.
    `dev` = the deviation of the same rule evaluated in torch fp32 on the CPU from float64, max over the tables, the valid rows and the
    fourteen numbers of |x32 - x64| / max(1, |x64|); `tau` = 4 dev (the project's standing margin for a re-associated fp32 sum against
    torch's)."""
    import torch
    c = inputs(hidden, in_dim)
    out, dev = {}, 0.0
    for table in TABLES:
        bounds, parts, index = lz.certify(c["nets"], c["obs"], N, c["rows"], c["counts"], GROUP, LEVEL_OF[table], LEVELS[:, :3], COL_LO, COL_HI)
        out[table] = dict(bounds=bounds, parts=parts, index=index)
        for k in range(K):
            for r in c["rows"][k][:c["counts"][k]]:
                if index[r] < 0:
                    continue
                x32 = torch_linear(c["members"][k], c["obs"][r], LEVELS[index[r]][0], torch.float32)
                x64 = numbers(bounds[r], parts[r])
                dev = max(dev, float((np.abs(x32 - x64) / np.maximum(1.0, np.abs(x64))).max()))
    return dict(tables=out, dev=dev, tau=4.0 * dev, member={int(r): k for k in range(K) for r in c["rows"][k][:c["counts"][k]]})


def intersect_f32(parts, pad):
    """The intersection-and-fallback rule and the pad on float32 `parts` [n][8], every operation one float32 operation -> float32 [n][4]."""
    p = np.ascontiguousarray(parts, np.float32)
    out = np.zeros((len(p), 4), np.float32)
    pad = np.float32(pad)
    for a in range(2):
        loL, hiL, loI, hiI = p[:, 2 * a], p[:, 2 * a + 1], p[:, 4 + 2 * a], p[:, 5 + 2 * a]
        lo, hi = np.where(loL > loI, loL, loI), np.where(hiL < hiI, hiL, hiI)
        bad = lo > hi
        lo, hi = np.where(bad, loI, lo), np.where(bad, hiI, hi)
        out[:, 2 * a], out[:, 2 * a + 1] = lo + (-pad), hi + pad
    return out
