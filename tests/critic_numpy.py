"""Two independent float64 models of the critic audit (copo_audit_record, csrc/audit_kernels.hip; include/copo_hip.h states the rules),
as python loops over a recorded stream of env steps:

  forward_fold   the recurrence the device runs: per (scene, slot, head) the carried sums q, c, z, u, e_b, one update per acting row in
                 the header's order, a commit on COPO_F_DONE;
  backward_fold  the definition: every agent's rows are kept, its returns come from G_t = r_t + gamma G_(t+1) backward from its last
                 step (no bootstrap), and the sums are taken directly.

Both return (sums float64 [G][K][heads][56], words int64 of the same shape): `sums` adds the agents' unquantised sums (the counts are
exact), `words` quantises every agent's sums once, as the device does.  tests/test_critics_cpu.py holds the two `sums` together to 1e-10
relative, which is the identity the forward form rests on.

A stream: flags uint8 [T][E][N], values float32 [T][E][N][heads], rew / nei_rew float32 [T][E][N], glob_rew float32 [T][E], seat int32
[E][N], group int32 [E]."""
import numpy as np

F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = (1 << i for i in range(8))
WORDS, MAX_BINS, BIN_COUNT, BIN_VALUE, BIN_RETURN = 56, 16, 8, 24, 40
AGENTS, STEPS, TRUNCATED, SUM_V, SUM_VV, SUM_G, SUM_VG, SUM_GG = range(8)
CLAMP, Q = 2.0 ** 32, 65536.0
COUNT_WORDS = (AGENTS, STEPS, TRUNCATED) + tuple(range(BIN_COUNT, BIN_COUNT + MAX_BINS))


def bin_of(v, lo, hi, bins):
    t = (float(v) - lo) / (hi - lo) * bins
    if not t >= 0.0:
        return 0
    return bins - 1 if t >= bins else int(t)


def quantise(x):
    if x != x:
        return 0
    return int(np.rint(min(max(x, -CLAMP), CLAMP) * Q))


def reward_of(stream, head, t, e, n):
    if head == 2:
        return float(stream["glob_rew"][t, e])
    return float((stream["rew"], stream["nei_rew"])[head][t, e, n])


def truncated_of(f):
    return bool(f & F_MAXSTEP) and not f & (F_ARRIVE | F_CRASH | F_OUT)


def _commit(sums, words, cell, agent, truncated, count_truncated):
    """`agent`: the 56 unquantised words of one finished agent (counts in the count words)."""
    if truncated:
        sums[cell][TRUNCATED] += 1
        words[cell][TRUNCATED] += 1
    if truncated and not count_truncated:
        return
    for w in range(WORDS):
        if w == TRUNCATED:
            continue
        sums[cell][w] += agent[w]
        words[cell][w] += int(agent[w]) if w in COUNT_WORDS else quantise(agent[w])


def _audited(stream, e, n, K, G):
    g, m = int(stream["group"][e]), int(stream["seat"][e, n])
    return (g, m) if 0 <= g < G and 0 <= m < K else None


def forward_fold(stream, gammas, ranges, bins, count_truncated, K, G):
    T, E, N = stream["flags"].shape
    H = len(gammas)
    sums, words = np.zeros((G, K, H, WORDS), np.float64), np.zeros((G, K, H, WORDS), np.int64)
    fresh = lambda: dict(q=0.0, c=0.0, z=0.0, u=0.0, e=[0.0] * bins, w=[0.0] * WORDS)  # noqa: E731
    state = {}
    for t in range(T):
        for e in range(E):
            for n in range(N):
                gm = _audited(stream, e, n, K, G)
                if gm is None:
                    continue
                f = int(stream["flags"][t, e, n])
                for h in range(H):
                    s = state.setdefault((e, n, h), fresh())
                    if f & F_ACTED:
                        gam, V, r = float(gammas[h]), float(stream["values"][t, e, n, h]), reward_of(stream, h, t, e, n)
                        b = bin_of(V, ranges[h][0], ranges[h][1], bins)
                        s["q"] = gam * gam * s["q"] + 1.0
                        s["c"] = gam * s["c"] + 1.0
                        s["z"] = gam * s["z"] + V
                        w = s["w"]
                        w[SUM_V] += V
                        w[SUM_VV] += V * V
                        w[STEPS] += 1
                        w[SUM_G] += r * s["c"]
                        w[SUM_VG] += r * s["z"]
                        w[SUM_GG] += r * (r * s["q"] + 2.0 * gam * s["u"])
                        s["u"] = gam * s["u"] + r * s["q"]
                        for bb in range(bins):
                            hit = 1.0 if bb == b else 0.0
                            s["e"][bb] = gam * s["e"][bb] + hit
                            w[BIN_COUNT + bb] += hit
                            w[BIN_VALUE + bb] += V * hit
                            w[BIN_RETURN + bb] += r * s["e"][bb]
                        if f & F_DONE:
                            w[AGENTS] = 1
                            _commit(sums, words, gm + (h,), w, truncated_of(f), count_truncated)
                    if f & (F_DONE | F_SPAWNED | F_ENV_RESET):
                        state[(e, n, h)] = fresh()
    return sums, words


def backward_fold(stream, gammas, ranges, bins, count_truncated, K, G):
    T, E, N = stream["flags"].shape
    H = len(gammas)
    sums, words = np.zeros((G, K, H, WORDS), np.float64), np.zeros((G, K, H, WORDS), np.int64)
    for e in range(E):
        for n in range(N):
            gm = _audited(stream, e, n, K, G)
            if gm is None:
                continue
            life = []          # the rows (t) of the agent in the slot now
            for t in range(T):
                f = int(stream["flags"][t, e, n])
                if f & F_ACTED:
                    life.append(t)
                    if f & F_DONE:
                        for h in range(H):
                            gam = float(gammas[h])
                            V = np.array([float(stream["values"][k, e, n, h]) for k in life])
                            r = np.array([reward_of(stream, h, k, e, n) for k in life])
                            Gt = np.zeros(len(life))
                            acc = 0.0
                            for i in range(len(life) - 1, -1, -1):
                                acc = r[i] + gam * acc
                                Gt[i] = acc
                            agent = [0.0] * WORDS
                            agent[AGENTS], agent[STEPS] = 1, len(life)
                            agent[SUM_V], agent[SUM_VV], agent[SUM_G] = V.sum(), (V * V).sum(), Gt.sum()
                            agent[SUM_VG], agent[SUM_GG] = (V * Gt).sum(), (Gt * Gt).sum()
                            for i, v in enumerate(V):
                                b = bin_of(v, ranges[h][0], ranges[h][1], bins)
                                agent[BIN_COUNT + b] += 1
                                agent[BIN_VALUE + b] += v
                                agent[BIN_RETURN + b] += Gt[i]
                            _commit(sums, words, gm + (h,), agent, truncated_of(f), count_truncated)
                if f & (F_DONE | F_SPAWNED | F_ENV_RESET):
                    life = []
    return sums, words
