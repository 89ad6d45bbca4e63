"""Shared by tests/test_lowp_cpu.py and tests/test_gpu_lowp.py: the inputs of the low-precision forward's tests.  No GPU and no native
library is touched at import.

The exact case.  Observations in {0, 0.5, 1}; W1 in {0, +-64} with eight entries per row (the last column among them), b1 in {0, +-32}:
every layer-1 pre-activation is a multiple of 32, so it is 0 or has magnitude >= 32 and tanh is exactly its sign.  W2 in {0, +-32} with
eight entries per row (a few rows all zero: the scale of a zero row), b2 in {0, +-32}: the same for layer 2.  W3 in {0, +-0.25, +-0.5}
with eight entries per row, b3 in {0, +-0.5}.  Every value is a power of two times at most 3, held exactly by e4m3 after the row scale
and by bfloat16; every partial sum is a small multiple of a power of two and exact in fp32, in any order; the four outputs are multiples
of 0.25 below 5 in magnitude, which bfloat16 holds.  So the low-precision kernels, the fp32 kernel and float64 must agree to the bit."""
import functools

import numpy as np

import bank_cases as bc

F = np.float32
EXACT_HIDDENS, EXACT_IN_DIMS = (64, 128, 256, 512), (92, 96)
EXACT_ROWS = 40                      # rows of the shared arrays
EXACT_LISTS = ([0, 1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 39], [38, 37, 36, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19])
POISON = 0x7FC0BEEF                  # a NaN with a payload: what an entry nobody wrote still holds
# the list shapes of the list test: counts per member with cap 40 (a count above cap is cut at cap), n_out 64; indices -1 and n_out inside a list
LIST_COUNTS = (0, 1, 15, 16, 17, 33, 50)
LIST_CAP, LIST_N_OUT = 40, 64


def _sparse(rng, rows, cols, values, per_row, last_col=False):
    W = np.zeros((rows, cols), F)
    for u in range(rows):
        idx = rng.choice(cols, per_row, replace=False)
        if last_col:
            idx[0] = cols - 1
        W[u, idx] = rng.choice(values, per_row)
    return W


def exact_net(hidden, in_dim, seed):
    """(W1, b1, W2, b2, W3, b3) float32 of the exact case."""
    rng = np.random.RandomState(7000 + 13 * hidden + in_dim + seed)
    W1 = _sparse(rng, hidden, in_dim, np.array([-64.0, 64.0], F), 8, last_col=True)
    W2 = _sparse(rng, hidden, hidden, np.array([-32.0, 32.0], F), 8)
    W2[rng.choice(hidden, 3, replace=False)] = 0.0
    W3 = _sparse(rng, 4, hidden, np.array([-0.5, -0.25, 0.25, 0.5], F), 8)
    b = lambda n, v: rng.choice(np.array([-v, 0.0, v], F), n)  # noqa: E731
    return W1, b(hidden, 32.0), W2, b(hidden, 32.0), W3, b(4, 0.5)


def as_weights(net):
    """A net as a population in the torch key layout (`PolicyBank` loads it)."""
    out = {}
    for name, W, b in zip(bc.TORCH_LAYERS, net[0::2], net[1::2]):
        out[name + ".weight"], out[name + ".bias"] = np.asarray(W, F), np.asarray(b, F)
    return out


@functools.lru_cache(maxsize=None)
def exact_case(hidden, in_dim):
    rng = np.random.RandomState(7100 + hidden + in_dim)
    obs = rng.choice(np.array([0.0, 0.5, 1.0], F), (EXACT_ROWS, in_dim), p=[0.5, 0.25, 0.25])
    obs[:, -1] = rng.choice(np.array([0.5, 1.0], F), EXACT_ROWS)
    eps = rng.randn(EXACT_ROWS, 2).astype(F)
    nets = [exact_net(hidden, in_dim, s) for s in range(2)]
    cap = max(len(l) for l in EXACT_LISTS) + 4
    rows = np.zeros((2, cap), np.int64)
    for k, l in enumerate(EXACT_LISTS):
        rows[k, :len(l)] = l
    return dict(obs=obs, eps=eps, nets=nets, rows=rows, counts=np.array([len(l) for l in EXACT_LISTS], np.int32))


def list_case(count):
    """(rows int64 [1][LIST_CAP], counts int32 [1], the rows a launch must write) of a one-member list of `count` entries: a permutation of
    the rows, with -1 and n_out in places 0 and 2 where the list is long enough."""
    rng = np.random.RandomState(7200 + count)
    rows = np.zeros((1, LIST_CAP), np.int64)
    rows[0] = rng.permutation(LIST_N_OUT)[:LIST_CAP]
    n = min(count, LIST_CAP)
    if n >= 3:
        rows[0, 0], rows[0, 2] = -1, LIST_N_OUT
    listed = [int(r) for r in rows[0, :n] if 0 <= r < LIST_N_OUT]
    return rows, np.array([count], np.int32), listed
