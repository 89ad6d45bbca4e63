"""The fault kernels (copo_fault_obs, copo_fault_act) restated as plain python loops: `mix32` / `hash_rng` of
csrc/sim_math.h in uint32 arithmetic, the normal stand-in `z` and every product and sum in float32, one rounding each.  It shares no
code with the kernels or with copo_amd/eval/faults.py, apart from the numbers written down here: the streams, the word layout and the
flag bits.  The GPU tests compare raw bits with it."""
import numpy as np

M32 = 0xFFFFFFFF
DROP, LIDAR_A, LIDAR_B, STICKY, ACT_A, ACT_B = 32, 33, 34, 35, 36, 37       # csrc/fault_common.h
ACTED, DONE, SPAWNED, ENV_RESET = 0x01, 0x02, 0x40, 0x80                     # include/copo_hip.h
WORDS = 8
Z_OFFSET = np.float32(131070.0)
Z_SCALE = np.float32(np.sqrt(3.0) / 65536.0)
Z_MAX = 131070.0 * np.sqrt(3.0) / 65536.0                                    # 3.46405


def mix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def hash_rng(seed, a, b, c, stream):
    h = mix32((seed & M32) + 0x9E3779B9)
    h = mix32(h ^ ((seed >> 32) & M32))
    for v in (a, b, c, stream):
        h = mix32(h ^ (v & M32))
    return h


def z_of(h1, h2):
    """((float)S - 131070) * (float)(sqrt(3) / 65536): S < 2^18, so the conversion and the difference are exact; one rounded product."""
    S = (h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16)
    return np.float32(np.float32(np.float32(S) - Z_OFFSET) * Z_SCALE)


def clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v) -- the sign of a zero survives, as on the device."""
    lo, hi = np.float32(lo), np.float32(hi)
    return lo if v < lo else (hi if v > hi else v)


def words(lidar_sigma=0.0, lidar_dropout=0.0, dropout_value=0.0, act_sigma=0.0, sticky=0.0):
    """One level row: f32 sigma, u32 rint(p 2^24), f32 value, f32 sigma, u32 rint(p 2^24), three zeros."""
    w = np.zeros(WORDS, np.uint32)
    w[0] = np.array([lidar_sigma], np.float32).view(np.uint32)[0]
    w[1] = int(np.rint(lidar_dropout * 2.0 ** 24))
    w[2] = np.array([dropout_value], np.float32).view(np.uint32)[0]
    w[3] = np.array([act_sigma], np.float32).view(np.uint32)[0]
    w[4] = int(np.rint(sticky * 2.0 ** 24))
    return w


def level_of_row(row, N, seat, group, K, G, level_of, L):
    """The level of row e N + n, or -1: it passes through."""
    e, n = divmod(row, N)
    s, g = int(seat[e][n]), int(group[e])
    if not 0 <= s < K or not 0 <= g < G:
        return -1
    lv = int(level_of[g][s])
    return lv if 0 <= lv < L else -1


def _f32(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def fault_obs(obs, col_lo, col_hi, seat, group, level_of, levels, tick, seed):
    """obs float32 [E][N][O] -> obs_seen; `tick` int32 [E N] is read only."""
    E, N, O = obs.shape
    G, K = np.asarray(level_of).shape
    L = len(levels)
    out = obs.copy()
    for row in range(E * N):
        lv = level_of_row(row, N, seat, group, K, G, level_of, L)
        if lv < 0:
            continue
        e, n = divmod(row, N)
        sigma, thr, value = _f32(levels[lv][0]), int(levels[lv][1]), _f32(levels[lv][2])
        t = int(tick[row])
        for c in range(col_lo, col_hi):
            b = c - col_lo
            if (hash_rng(seed, row, t, b, DROP) >> 8) < thr:
                out[e, n, c] = value
            elif sigma != 0:
                z = z_of(hash_rng(seed, row, t, b, LIDAR_A), hash_rng(seed, row, t, b, LIDAR_B))
                out[e, n, c] = clamp(np.float32(obs[e, n, c] + np.float32(sigma * z)), 0.0, 1.0)
    return out


def fault_act(act, prev, flags_prev, seat, group, level_of, levels, tick, seed):
    """act float32 [E][N][2], prev the same, flags_prev uint8 [E][N] or None, tick int32 [E N] -> (act, prev, tick) after the call."""
    E, N, _ = act.shape
    G, K = np.asarray(level_of).shape
    L = len(levels)
    act, prev, tick = act.copy(), prev.copy(), np.asarray(tick).copy()
    for row in range(E * N):
        e, n = divmod(row, N)
        lv = level_of_row(row, N, seat, group, K, G, level_of, L)
        t = int(tick[row])
        if lv >= 0:
            sigma, thr = _f32(levels[lv][3]), int(levels[lv][4])
            if flags_prev is not None:
                f = int(flags_prev[e][n])
                same = bool(f & ACTED) and not f & (DONE | SPAWNED | ENV_RESET)
                if same and (hash_rng(seed, row, t, 0, STICKY) >> 8) < thr:
                    act[e, n] = prev[e, n]
            if sigma != 0:
                for j in range(2):
                    z = z_of(hash_rng(seed, row, t, j, ACT_A), hash_rng(seed, row, t, j, ACT_B))
                    act[e, n, j] = clamp(np.float32(act[e, n, j] + np.float32(sigma * z)), -1.0, 1.0)
        prev[e, n] = act[e, n]
        tick[row] = t + 1
    return act, prev, tick
