"""The rules of the influence graph (copo_amd/eval/influence.py, copo_influence_*) restated as python loops on a
table of fp32 distances d [ego][vehicle][beam] plus s [ego][beam] (the static boxes): owners, ties, min2, the candidates, truncation, the
variant rows, the members' variant lists and the fold.  Distances are >= +0, so fp32 values and their bit patterns order alike; every
comparison here is on fp32 values.  The fold's integer words are exact; its KL word is float64 (jury_numpy.kl)."""
import numpy as np

import jury_numpy as jn

WORDS = 8
F_ACTED = 0x01
f32 = np.float32


def beams(d, s, rng):
    """(min1 [A][B] fp32, owner [A][B] int (-1: nobody), min2 [A][B] fp32) of d [A][V][B] and s [A][B]; a value that is not below `rng`
    counts as `rng`; a vehicle that is not there has `rng` on every beam (the ego's own column included)."""
    d, s, rng = np.asarray(d, f32), np.asarray(s, f32), f32(rng)
    A, V, B = d.shape
    min1, owner, min2 = np.full((A, B), rng, f32), np.full((A, B), -1, np.int64), np.full((A, B), rng, f32)
    for a in range(A):
        for b in range(B):
            sb = s[a, b] if s[a, b] < rng else rng
            vals = [d[a, j, b] if d[a, j, b] < rng else rng for j in range(V)]
            m1 = min([sb] + vals)
            own = -1
            if m1 < rng and sb > m1:
                own = min(j for j in range(V) if vals[j] == m1)          # no lower slot attains the same value
            rest = [sb] + [vals[j] for j in range(V) if j != own]
            min1[a, b], owner[a, b], min2[a, b] = m1, own, min(rest)
    return min1, owner, min2


def candidates(min1, owner, M):
    """(who [A][M] int, -1 = none; kept [A]; truncated [A]; hit [A][M] fp32, the candidate's smallest owned distance, 0 where none): the
    owners of at least one beam by (smallest owned distance, slot), the first M kept."""
    A, B = owner.shape
    who, hit = np.full((A, M), -1, np.int64), np.zeros((A, M), f32)
    kept, trunc = np.zeros(A, np.int64), np.zeros(A, np.int64)
    for a in range(A):
        best = {}
        for b in range(B):
            j = int(owner[a, b])
            if j >= 0 and (j not in best or min1[a, b] < best[j]):
                best[j] = min1[a, b]
        order = sorted(best, key=lambda j: (best[j], j))
        kept[a], trunc[a] = min(len(order), M), max(len(order) - M, 0)
        for c, j in enumerate(order[:M]):
            who[a, c], hit[a, c] = j, best[j]
    return who, kept, trunc, hit


def variants(obs, col, min1, owner, min2, who, inv_range):
    """{(a, c): row}: obs[a] with (owner == who[a][c] ? min2 : min1) * inv_range on the LiDAR block, for every kept candidate."""
    out = {}
    B = min1.shape[1]
    for a in range(who.shape[0]):
        for c in range(who.shape[1]):
            if who[a, c] < 0:
                continue
            row = np.array(obs[a], f32)
            row[col:col + B] = np.where(owner[a] == who[a, c], min2[a], min1[a]).astype(f32) * f32(inv_range)
            out[a, c] = row
    return out


def variant_lists(rows, counts, kept, M):
    """(vrows int64 [K][cap M], vcounts int32 [K]): member k walks its seat list in order; row r adds r M + c for c < kept[r]."""
    rows, counts = np.asarray(rows), np.asarray(counts)
    K, cap = rows.shape
    vrows, vcounts = np.zeros((K, cap * M), np.int64), np.zeros(K, np.int32)
    for k in range(K):
        for r in rows[k, :counts[k]]:
            for c in range(int(kept[r])):
                vrows[k, vcounts[k]] = r * M + c
                vcounts[k] += 1
    return vrows, vcounts


def pair_words(p, q, deltas):
    """(moved, q16 d_steer, q16 d_throttle, q16 KL(p || q), q16 max) of one (ego, candidate) pair, and the fp32 (d0, d1)."""
    w = jn.pair_words(p, q, deltas)
    return w[1], w[2], w[3], w[5], w[7]


def fold(flags, dist, verdict_cf, who, trunc, seat, group, K, G, deltas, out=None):
    """out int64 [G][K][8] += one step: flags [E N] (COPO_F_ACTED on an ego), dist [E N][4], verdict_cf [E N M][K][4], who [E N][M],
    trunc [E N], seat [E][N], group [E]."""
    seat, group, who = np.asarray(seat), np.asarray(group), np.asarray(who)
    E, N = seat.shape
    M = who.shape[1]
    flags, dist = np.asarray(flags).reshape(E * N), np.asarray(dist, f32).reshape(E * N, 4)
    verdict_cf = np.asarray(verdict_cf, f32).reshape(E * N * M, K, 4)
    out = np.zeros((G, K, WORDS), np.int64) if out is None else out
    for e in range(E):
        g = int(group[e])
        if g < 0 or g >= G:
            continue
        for n in range(N):
            r, k = e * N + n, int(seat[e, n])
            if k < 0 or k >= K or not (int(flags[r]) & F_ACTED):
                continue
            out[g, k, 0] += 1
            out[g, k, 7] += int(trunc[r])
            for c in range(M):
                if who[r, c] < 0:
                    continue
                moved, q0, q1, qkl, qmx = pair_words(dist[r], verdict_cf[r * M + c, k], deltas)
                out[g, k, 1:6] += (1, moved, q0, q1, qkl)
                out[g, k, 6] = max(out[g, k, 6], qmx)
    return out
