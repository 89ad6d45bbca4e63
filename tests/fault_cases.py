"""Seeded inputs of the fault kernels, used by the numpy model's tests and by the GPU comparison: observations, seat / group / level
tables with every way a row can pass through, ticks that differ per row, and hand-made previous flags for the sticky rule."""
import numpy as np

import fault_numpy as fn

SEED = 0x9E3779B97F4A7C15            # a fault seed with both halves set

# L = 3: the identity, a mild level (noise only) and a harsh one (everything, dropout to 1.0 = "nothing in range")
LEVELS = (dict(), dict(lidar_sigma=0.02, act_sigma=0.05),
          dict(lidar_sigma=0.3, lidar_dropout=0.25, dropout_value=1.0, act_sigma=0.5, sticky=0.5))

# (E, N, O, col_lo, col_hi): 15 rows, less than a wave and a multiple of nothing, two columns behind the beams; 200 rows of the
# Intersection's width (odd) with an odd first column and 72 beams to the row's end, a row of two rounds of 64 lanes
SHAPES = ((3, 5, 13, 3, 11), (5, 40, 91, 19, 91))


def level_words():
    return np.stack([fn.words(**lv) for lv in LEVELS])


def tables(E, N, seed):
    """(seat [E][N], group [E], level_of [G][K], K, G): K = 4 members, G = 3 groups, N >= 5; seats of -1 and of K (outside), one scene of
    group -1 and, above three scenes, one of group G; level_of holds every level, -1 and L (outside)."""
    K, G, L = 4, 3, len(LEVELS)
    rng = np.random.RandomState(seed)
    seat = rng.randint(0, K, (E, N)).astype(np.int32)
    pick = rng.permutation(E * N)
    seat.reshape(-1)[pick[:max(E * N // 10, 1)]] = -1
    seat.reshape(-1)[pick[-1]] = K
    seat[0, :5] = [0, 1, 2, 3, -1]                # scene 0 (group 0): levels 2, 1, 0, L and nobody
    group = (np.arange(E) % G).astype(np.int32)
    group[E - 1] = -1
    if E > 3:
        group[E - 2] = G
    level_of = rng.randint(0, L, (G, K)).astype(np.int32)
    level_of[0, 0], level_of[0, 1], level_of[0, 2], level_of[0, 3] = 2, 1, 0, L          # group 0 holds every case
    level_of[1, 0], level_of[1, 1] = -1, 2
    return seat, group, level_of, K, G


def observations(E, N, O, seed):
    """float32 [E][N][O] in [0, 1] with exact 0 and 1 among the beams (the clamp's ends) and values outside [0, 1] in the other columns
    (they must be copied, not clamped)."""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(0.0, 1.0, (E, N, O)).astype(np.float32)
    obs[rng.uniform(size=obs.shape) < 0.2] = 1.0
    obs[rng.uniform(size=obs.shape) < 0.05] = 0.0
    obs[:, :, 0] = rng.normal(0.0, 3.0, (E, N)).astype(np.float32)
    return obs


def ticks(E, N, seed):
    """int32 [E N], non-zero and different per row"""
    return (np.random.RandomState(seed).permutation(E * N) * 7 + 3).astype(np.int32)


def actions(E, N, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.0, 1.0, (E, N, 2)).astype(np.float32)
    a[rng.uniform(size=a.shape) < 0.1] = 1.0
    a[rng.uniform(size=a.shape) < 0.1] = -1.0
    return a


def previous_flags(E, N, seed):
    """uint8 [E][N]: the five cases of the sticky rule in turn over the rows, other bits mixed in -- ACTED alone or with outcome bits
    but no DONE (same occupant), ACTED | DONE, ACTED | SPAWNED, no ACTED, ACTED | ENV_RESET."""
    rng = np.random.RandomState(seed)
    cases = np.array([fn.ACTED, fn.ACTED | fn.DONE | 0x04, fn.ACTED | fn.SPAWNED, fn.SPAWNED, fn.ACTED | fn.ENV_RESET, 0, fn.ACTED | 0x20],
                     np.uint8)
    return cases[rng.randint(0, len(cases), (E, N))]
