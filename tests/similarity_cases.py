"""Shared by tests/test_similarity_cpu.py and tests/test_gpu_similarity.py: the inputs of the similarity tests and their float64
references, computed once per case.  No GPU and no native library is touched at import.

The forward cases are jury_cases': its seat and group tables (E = 6 scenes of N = 8 slots, K = 3 members, G = 3; scene 5 lies in group 7,
outside [0, G)), its members and observations at hidden 64 / 128 / 256 / 512 and observation widths 91 / 92, its flags.  The panel is all
three members, so every member's list is the common one: the 18 seated rows of groups 0 .. 2 -- one full 16-row tile and a partial tile
of two rows.  `rows_of` is None or 1.

The twin: member 0 with its hidden units permuted consistently in both layers (rows of W1 and b1, columns of W2; rows of W2 and b2,
columns of W3).  The same function, linear CKA exactly 1 in both layers, and far away in weight space.

The grid cases of the Gram kernel: hand-made workspaces whose values are drawn from {-1, -0.5, 0, 0.5, 1}, so that every product is a
multiple of 1/4 and every partial sum is exact in fp32 (`grid_premise` measures it): the kernel must equal the float64 model bit for
bit.  Row counts 1, 13, 16, 17 and 320: one chunk of 32 positions, partial chunks, and ten chunks -- 320 positions cross the promotion
interval of 128 rows twice with one plane, and with two planes each plane takes five chunks, so it crosses it once more."""
import functools

import numpy as np

import adversary_cases as ac
import jury_cases as jc
import similarity_numpy as sn

HIDDENS, IN_DIMS = jc.HIDDENS, jc.IN_DIMS
E, N, K, G = jc.E, jc.N, jc.K, jc.G
SEAT, GROUP = jc.SEAT, jc.GROUP
ROWS_OF = (None, 1)
COUNT = 18
POISON = jc.POISON
GRID_VALUES = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32)
GRID_COUNTS, GRID_PLANES, GRID_LAUNCHES, GRID_K = (1, 13, 16, 17, 320), (1, 2), 3, 3
GRID_SLACK = 5                    # positions behind the count, inside the capacity
CHUNK, PROMOTE_ROWS = 32, 128     # COPO_CKA_CHUNK, COPO_CKA_PROMOTE_ROWS


def rows():
    r = sn.common_rows(SEAT, GROUP, G)
    assert len(r) == COUNT
    return r


def twin_of(weights, seed=7):
    """The population with its hidden units permuted in both layers (two independent permutations)."""
    rng = np.random.RandomState(seed)
    l1, l2, l3 = ac.bc.TORCH_LAYERS
    H = weights[l1 + ".bias"].shape[0]
    p1, p2 = rng.permutation(H), rng.permutation(H)
    out = {k: np.array(v, np.float32) for k, v in weights.items()}
    out[l1 + ".weight"], out[l1 + ".bias"] = weights[l1 + ".weight"][p1], weights[l1 + ".bias"][p1]
    out[l2 + ".weight"], out[l2 + ".bias"] = weights[l2 + ".weight"][p2][:, p1], weights[l2 + ".bias"][p2]
    out[l3 + ".weight"] = weights[l3 + ".weight"][:, p2]
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


def weight_distance(a, b):
    """The relative L2 distance of two populations over all their arrays."""
    num = sum(float(((np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)) ** 2).sum()) for k in a)
    den = sum(float((np.asarray(a[k], np.float64) ** 2).sum()) for k in a)
    return float(np.sqrt(num / den))


def hidden_of(members, obs, dtype=np.float64):
    """[K][n][2][H]: both layers of every member on every row of obs, float64 model."""
    out = []
    for w in members:
        h1, h2 = sn.hidden64(ac.net_of(w), obs)
        out.append(np.stack([h1, h2], axis=1))
    return np.stack(out).astype(dtype)


def torch_hidden32(members, obs):
    """[K][n][2][H] float32 by torch on the CPU in fp32: the yardstick of the fp32 deviation."""
    import torch
    out = []
    for w in members:
        W1, b1, W2, b2 = (torch.from_numpy(np.asarray(a, np.float32)) for a in ac.net_of(w, np.float32)[:4])
        x = torch.from_numpy(np.asarray(obs, np.float32))
        h1 = torch.tanh(x @ W1.T + b1)
        h2 = torch.tanh(h1 @ W2.T + b2)
        out.append(torch.stack([h1, h2], dim=1).numpy())
    return np.stack(out)


def torch_heads32(members, obs):
    """[n][K][4] float32: the four head outputs by torch on the CPU in fp32."""
    import torch
    h = torch_hidden32(members, obs)
    out = []
    for k, w in enumerate(members):
        W3, b3 = (torch.from_numpy(np.asarray(a, np.float32)) for a in ac.net_of(w, np.float32)[4:])
        out.append((torch.from_numpy(h[k][:, 1]) @ W3.T + b3).numpy())
    return np.stack(out, axis=1)


def torch_gram32(hidden32, panel, mask):
    """S [P][2][H][H] by torch fp32 matmul on the CPU of the fp32 activations: the yardstick of the Gram kernel's fp32 deviation."""
    import torch
    h = [torch.from_numpy(np.ascontiguousarray(hidden32[int(m)][mask])) for m in panel]
    out = []
    for a in range(len(panel)):
        for b in range(a, len(panel)):
            out.append(np.stack([(h[a][:, layer].T @ h[b][:, layer]).numpy() for layer in range(2)]))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim):
    """What one forward case's tests share, computed once: members, observations, the float64 hidden layers and heads of every member
    on every row, torch fp32's own deviation from them (`dev_hidden`, `dev_heads`: max absolute) and tau = 4 dev."""
    ref = jc.reference(hidden, in_dim)
    members, obs = ref["members"], ref["obs"]
    h64 = hidden_of(members, obs)
    dev_hidden = float(np.abs(torch_hidden32(members, obs).astype(np.float64) - h64).max())
    dev_heads = float(np.abs(torch_heads32(members, obs).astype(np.float64) - ref["verdict64"]).max())
    return dict(members=members, obs=obs, hidden64=h64, verdict64=ref["verdict64"], dev_hidden=dev_hidden, tau_hidden=4.0 * dev_hidden,
                dev_heads=dev_heads, tau_heads=4.0 * dev_heads)


def model(hidden, rows_of, flags=None, panel=(0, 1, 2)):
    """The float64 model on a workspace [K][cap][2][H] over the common list: dict(acc, hsic, cka, mean, var, mask)."""
    flags = jc.flags() if flags is None else flags
    mask = sn.counted(rows(), COUNT, flags, SEAT, -1 if rows_of is None else rows_of)
    acc = sn.accumulate(hidden, panel, mask)
    M = len(panel)
    hs = sn.hsic(acc, M)
    mean, var = sn.unit_stats(acc, M)
    return dict(acc=acc, hsic=hs, cka=sn.cka(hs, acc["n"]), mean=mean, var=var, mask=mask)


def workspace_of(full, cap=COUNT):
    """[K][cap][2][H] from activations on all E N rows [K][E N][2][H]: position p holds row rows()[p]."""
    return np.ascontiguousarray(full[:, rows()[:cap]])


@functools.lru_cache(maxsize=None)
def grid_case(H, count, rows_of, seed=0):
    """One grid case: GRID_LAUNCHES steps of (workspace with NaN poison at every position that is not counted, flags), the list, the seat
    table and the float64 model's accumulators over all steps."""
    rng = np.random.RandomState(1000 * H + 10 * count + seed + (0 if rows_of is None else 7))
    cap = count + GRID_SLACK
    n_out = 2 * cap + 3
    listed = np.sort(rng.choice(n_out, cap, replace=False)).astype(np.int64)
    seat = rng.randint(-1, GRID_K, n_out).astype(np.int32)
    if count >= 13:
        seat[listed[:count:3]] = 1          # (rows_of = 1 keeps a third of the list at the least)
    steps, acc = [], None
    for _ in range(GRID_LAUNCHES):
        flags = (rng.randint(0, 128, n_out) & ~sn.F_ACTED).astype(np.uint8)
        flags[rng.rand(n_out) < 0.8] |= sn.F_ACTED
        mask = sn.counted(listed, count, flags, seat, -1 if rows_of is None else rows_of)
        ws = GRID_VALUES[rng.randint(0, len(GRID_VALUES), (GRID_K, cap, 2, H))]
        ws[:, ~mask] = np.nan
        acc = sn.accumulate(ws, range(GRID_K), mask, acc)
        steps.append((ws, flags, mask))
    return dict(rows=listed, count=count, cap=cap, n_out=n_out, seat=seat, steps=steps, acc=acc)


def grid_premise(case):
    """The largest |partial sum| of any accumulator element over any prefix of the counted positions of a step, in units of 1/4 (the
    grid of the products): below 2^24 every fp32 partial sum is exact whatever the order."""
    worst = 0.0
    for ws, _, mask in case["steps"]:
        n = int(mask.sum())
        worst = max(worst, float(n))          # |h| <= 1: no prefix sum of products or of values exceeds the count
    return 4.0 * worst
