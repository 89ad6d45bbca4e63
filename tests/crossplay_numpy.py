"""The rules of cross-play (copo_amd/eval/crossplay.py, copo_seat_tally) restated as python loops, for
tests/test_crossplay_cpu.py and tests/test_gpu_crossplay.py.  No GPU and no native library is touched."""
import numpy as np

ACTED, DONE, ARRIVE, CRASH, OUT, MAXSTEP, SPAWNED, ENV_RESET = (1 << i for i in range(8))
WORDS = 8


# ---- the end-to-end case: two CoPO Intersection populations (the reference's and a perturbed copy), every ordered pair on the same
# three scenes of 40 slots, half of the seats each, 60 env steps ----
E2E_PAIRS = (2, 3, 40, 0.5)          # SeatPlan.pairs(K, scenes_per_pair, N, share)
E2E_STEPS, E2E_T, E2E_SEED = 60, 20, 0


def e2e_members(golden_dir):
    import bank_cases as bc
    w = bc.golden_population(golden_dir, "copo_inter")
    return [w, bc.perturbed(w, 1, 0.05)]


def e2e_config():
    """The scenes `make_eval_trainer("copo", "inter", num_envs=12, num_agents=40, seed=0)` builds, for the CPU oracle."""
    from copo_amd.sim import SimConfig
    K, S, N, _ = E2E_PAIRS
    return SimConfig(map="intersection", num_envs=K * K * S, num_agents=N, start_seed=5000)


def e2e_seeds():
    K, S, _, _ = E2E_PAIRS
    return np.tile(np.arange(S, dtype=np.uint64) + np.uint64(e2e_config().start_seed), K * K)


def trip_join(d, seat, group, K, G):
    """[G][K][5] (acted, done, arrive, crash, out) from the decoded rows `d` of a trip log that recorded every step and was flushed at
    the end (`trips.decode`), joined on (scene, slot) -> seat.  The rule: only the rows of kind 1 (done) carry a DONE step, and their end
    byte its bits; their `steps` are the agent's ACTED steps.  An open trip (kind 3, flushed) counts the records that saw its agent, the
    first of which -- the reset's or the one with SPAWNED -- is no ACTED step: steps - 1.  Vanished trips (kind 2: a scene reset or a
    reset by hand took the agent away) have no place in the tally's words and must not occur in the run that is joined."""
    out = np.zeros((G, K, 5), np.int64)
    for i in range(len(d["scene"])):
        e, n = int(d["scene"][i]), int(d["slot"][i])
        k, g = int(seat[e][n]), int(group[e])
        if not (0 <= k < K and 0 <= g < G):
            continue
        kind = int(d["kind"][i])
        assert kind in (1, 3), "a vanished trip in scene %d slot %d" % (e, n)
        out[g, k, 0] += int(d["steps"][i]) - (kind == 3)
        if kind == 1:
            f = int(d["flags"][i])
            out[g, k, 1] += 1
            for j, bit in enumerate((ARRIVE, CRASH, OUT)):
                out[g, k, 2 + j] += 1 if f & bit else 0
    return out


def plan_lists(seat, K):
    """(rows [K][cap] int64, counts [K] int32, cap): row e * N + n goes to the list of member seat[e][n], in ascending order."""
    E, N = len(seat), len(seat[0])
    lists = [[] for _ in range(K)]
    for e in range(E):
        for n in range(N):
            k = int(seat[e][n])
            if k >= 0:
                lists[k].append(e * N + n)
    counts = [len(v) for v in lists]
    cap = max(max(counts), 1)
    rows = np.zeros((K, cap), np.int64)
    for k, v in enumerate(lists):
        rows[k, :len(v)] = v
    return rows, np.asarray(counts, np.int32), cap


def pair_seats(K, S, N, share):
    """(seat [K K S][N], group [K K S]) of SeatPlan.pairs: group i K + j, the first round(share N) seats to i, the rest to j."""
    nf = int(round(share * N))
    seat, group = [], []
    for i in range(K):
        for j in range(K):
            for _ in range(S):
                seat.append([i] * nf + [j] * (N - nf))
                group.append(i * K + j)
    return np.asarray(seat, np.int32), np.asarray(group, np.int32)


def reward_q16(r):
    """rint(min(max(r, -1024), 1024) * 65536) with the product in fp32 (exact: a power of two), half to even; NaN -> 0."""
    r = np.float32(r)
    if np.isnan(r):
        return 0
    c = np.float32(min(max(r, np.float32(-1024.0)), np.float32(1024.0)))
    return int(np.rint(np.float32(c * np.float32(65536.0))))


def tally(flags, rew, seat, group, K, G, out=None):
    """out [G][K][8] int64 += one step (python ints: no overflow question)."""
    out = np.zeros((G, K, WORDS), np.int64) if out is None else out
    E, N = flags.shape
    for e in range(E):
        g = int(group[e])
        if not 0 <= g < G:
            continue
        for n in range(N):
            k, f = int(seat[e][n]), int(flags[e][n])
            if not 0 <= k < K:
                continue
            w = out[g, k]
            if f & SPAWNED:
                w[7] += 1
            if not f & ACTED:
                continue
            w[0] += 1
            if rew is not None:
                w[6] += reward_q16(rew[e][n])
            if f & DONE:
                w[1] += 1
                for i, bit in enumerate((ARRIVE, CRASH, OUT, MAXSTEP)):
                    if f & bit:
                        w[2 + i] += 1
    return out
