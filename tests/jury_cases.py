"""Shared by tests/test_jury_cpu.py and tests/test_gpu_jury.py: the inputs of the jury's kernel tests, on the 48 rows of adversary_cases
(E = 6 scenes of N = 8 slots, K = 3 members, its weights and observations), and the float64 model of the verdicts.  No GPU and no native
library is touched at import.

Scene 5 is in group 7, outside [0, G): none of its rows is listed or counted.  Slots with seat -1 are in nobody's list.

Two judge tables, because at K = 3 "a row judged by all three members" and "a judge with an empty list" cannot hold under one table;
every test runs both.
  A  group 0: all three judge its 13 seated rows (each of them is judged by all three); group 1: member 1 alone (rows 16 .. 18 are
     driven by member 1 and judged only by their own driver; row 24 is driven by 2, judged by 1); group 2: nobody (row 35 is seated and
     judged by none).  Lists: 13, 17 (a full tile and a one-row masked tile), 13 rows.
  B  groups 0 and 1: member 2 alone (17 rows across two tiles; the rows member 2 drives are judged only by their own driver); group 2:
     member 1 alone (row 35: a one-row list, a one-row masked tile); member 0 judges nothing: an empty list.
"""
import functools

import numpy as np

import adversary_cases as ac
import jury_numpy as jn

HIDDENS, IN_DIMS, TABLES = ac.HIDDENS, ac.IN_DIMS, ("A", "B")
E, N, K, G = ac.E, ac.N, ac.K, 3
GROUP = np.array([0, 0, 1, 1, 2, 7], np.int32)
SEAT = np.array([[0, 1, 2, 0, 1, 2, -1, -1],
                 [0, 0, 1, 1, 2, 2, -1, 0],
                 [1, 1, 1, -1, -1, -1, -1, -1],
                 [2, -1, -1, -1, -1, -1, -1, -1],
                 [-1, -1, -1, 0, -1, -1, -1, -1],
                 [0, 1, 2, 0, 1, 2, 0, 1]], np.int32)
JUDGES = dict(A=np.array([[1, 1, 1], [0, 1, 0], [0, 0, 0]], np.int32), B=np.array([[0, 0, 1], [0, 0, 1], [0, 1, 0]], np.int32))
COUNTS = dict(A=(13, 17, 13), B=(0, 1, 17))
# the disagreement thresholds on the two means: the float64 model puts no |mu_a(judge) - mu_a(driver)| of any case within MARGIN of
# them (test_jury_cpu.py checks it), so that the fp32 kernel and the model count the same pairs
DELTAS = (0.075, 0.089)
MARGIN = 1e-4
FLAG_SEED = 4300
POISON = 0x7FC0BEEF              # a NaN with a payload: what an entry nobody wrote still holds


def flags():
    """uint8 [E][N]: COPO_F_ACTED on about five slots in six (whatever their seat), other bits at random."""
    rng = np.random.RandomState(FLAG_SEED)
    f = (rng.randint(0, 128, (E, N)) & ~jn.F_ACTED).astype(np.uint8)
    f[rng.rand(E, N) < 0.85] |= jn.F_ACTED
    return f


def forward64(weights, obs):
    """[n][4] float64: mu_steer, mu_throttle, logstd_steer, logstd_throttle of a population on the rows of obs."""
    W1, b1, W2, b2, W3, b3 = ac.net_of(weights)
    h2 = np.tanh(np.tanh(np.asarray(obs, np.float64) @ W1.T + b1) @ W2.T + b2)
    return h2 @ W3.T + b3


@functools.lru_cache(maxsize=None)
def reference(hidden, in_dim):
    """What one case's tests share, computed once: the members, the observations and the float64 verdict of every member on every row."""
    ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
    return dict(members=ws, obs=obs, verdict64=np.stack([forward64(w, obs) for w in ws], axis=1))


def judged_pairs(table):
    """[(row, driver, judge)] of every pair a fold may count under `table` (before the flags)."""
    out = []
    for e in range(E):
        g = int(GROUP[e])
        for n in range(N):
            if SEAT[e, n] >= 0 and 0 <= g < G:
                out += [(e * N + n, int(SEAT[e, n]), j) for j in range(K) if JUDGES[table][g, j]]
    return out
