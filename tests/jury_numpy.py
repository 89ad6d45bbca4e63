"""The rules of the policy jury (copo_amd/eval/jury.py, copo_jury_obs_seats_f32, copo_jury_tally) restated as
python loops: the judges' row lists and the fold.  Words 0-4 and 7 of the fold are restated EXACTLY, every fp32 rounding spelled out
(numpy float32 arithmetic rounds once per operation, as the kernel's __fsub_rn / __fadd_rn do); the two divergences are float64."""
import numpy as np

WORDS = 8
F_ACTED = 0x01                  # COPO_F_ACTED
f32 = np.float32


def jury_lists(seat, group, judges):
    """(rows int64 [K][cap], counts int32 [K], cap): judge j's ascending list of the rows e N + n with seat >= 0, 0 <= group[e] < G and
    judges[group[e]][j] != 0."""
    seat, group, judges = np.asarray(seat), np.asarray(group), np.asarray(judges)
    E, N = seat.shape
    G, K = judges.shape
    lists = [[] for _ in range(K)]
    for e in range(E):
        for n in range(N):
            g = int(group[e])
            if seat[e, n] < 0 or g < 0 or g >= G:
                continue
            for j in range(K):
                if judges[g, j] != 0:
                    lists[j].append(e * N + n)
    counts = np.array([len(li) for li in lists], np.int32)
    cap = max(int(counts.max()), 1)
    rows = np.zeros((K, cap), np.int64)
    for j, li in enumerate(lists):
        rows[j, :len(li)] = li
    return rows, counts, cap


def q16(x):
    """rint(min(max(x, 0), 1024) * 65536) as int; NaN counts as 0.  For an fp32 x the product is exact, so the one rounding is rint's."""
    x = float(x)
    if x != x:
        return 0
    return int(np.rint(min(max(x, 0.0), 1024.0) * 65536.0))


def kl(p, q):
    """KL(p || q) of two diagonal Gaussians (mu_0, mu_1, logstd_0, logstd_1), float64 from the fp32 inputs, in the header's form."""
    p, q = np.asarray(p, f32).astype(np.float64), np.asarray(q, f32).astype(np.float64)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for a in range(2):
            mp, sp, mq, sq = p[a], p[2 + a], q[a], q[2 + a]
            dm = mp - mq
            total = total + ((sq - sp) + (0.5 * (np.exp(2.0 * (sp - sq)) + dm * dm * np.exp(-2.0 * sq)) - 0.5))
    return float(total)


def pair_words(own, v, deltas):
    """The eight words one counted (slot, judge) pair adds (word 7: the candidate of the max): `own` the driver's four fp32 numbers, `v`
    the judge's."""
    own, v = np.asarray(own, f32), np.asarray(v, f32)
    with np.errstate(all="ignore"):
        d0, d1 = np.abs(f32(v[0] - own[0])), np.abs(f32(v[1] - own[1]))                 # one rounding each
        ds = f32(np.abs(f32(v[2] - own[2])) + np.abs(f32(v[3] - own[3])))               # either difference, then the sum, rounded once
        apart = bool(d0 > f32(deltas[0])) or bool(d1 > f32(deltas[1]))                  # (a NaN exceeds nothing)
        mx = np.fmax(d0, d1)                                                            # (a NaN yields to the other axis)
    return [1, int(apart), q16(d0), q16(d1), q16(ds), q16(kl(own, v)), q16(kl(v, own)), q16(mx)]


def jury_fold(flags, dist, verdict, seat, group, judges, deltas, out=None):
    """out int64 [G][K][K][8] += one step: flags [E][N], dist [E][N][4], verdict [E N][K][4], seat [E][N], group [E], judges [G][K]."""
    seat, group, judges = np.asarray(seat), np.asarray(group), np.asarray(judges)
    E, N = seat.shape
    G, K = judges.shape
    flags, dist, verdict = np.asarray(flags).reshape(E, N), np.asarray(dist, f32).reshape(E, N, 4), np.asarray(verdict, f32).reshape(E * N, K, 4)
    out = np.zeros((G, K, K, WORDS), np.int64) if out is None else out
    for e in range(E):
        g = int(group[e])
        if g < 0 or g >= G:
            continue
        for n in range(N):
            k = int(seat[e, n])
            if k < 0 or k >= K or not (int(flags[e, n]) & F_ACTED):
                continue
            for j in range(K):
                if judges[g, j] == 0:
                    continue
                w = pair_words(dist[e, n], verdict[e * N + n, j], deltas)
                out[g, k, j, :7] += w[:7]
                out[g, k, j, 7] = max(out[g, k, j, 7], w[7])
    return out
