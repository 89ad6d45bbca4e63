"""Crafted streams of the critic audit, shared by tests/test_critics_cpu.py (the two numpy models against each other) and
tests/test_gpu_critics.py (copo_audit_record against the numpy model).  6 scenes x 5 slots, K = 2 members plus seats at -1, 2 scene groups
(one scene outside them), 40 steps, three heads with the discounts 1.0, 0.99 and 0.9.  A slot's timeline is written as a script of
agents: (steps the agent acts, how it ends, empty steps before the next one spawns):

  end "arrive" / "crash" / "out"     COPO_F_DONE with that flag: terminated
  end "maxstep"                      COPO_F_DONE | COPO_F_MAXSTEP alone: truncated
  end "crash+maxstep"                both flags: terminated (the max-step flag ALONE makes a truncation)
  gap 0                              the next agent spawns in the same step: COPO_F_DONE | COPO_F_SPAWNED on one row
  gap g > 0                          g steps without any flag, then a step with COPO_F_SPAWNED alone
An agent whose script runs past the stream stays open.  Scene 4 is reset at step 25 (COPO_F_ENV_RESET | COPO_F_SPAWNED on every slot):
the agents open there are dropped and new ones start.  Values are normal with scale 3 against the range [-2, 2], so both end bins take
values from outside it; a few are exactly on bin edges."""
import numpy as np

import critic_numpy as cn

E, N, K, G, T = 6, 5, 2, 2, 40
GAMMAS = (1.0, 0.99, 0.9)
RANGES = ((-2.0, 2.0), (-2.0, 2.0), (-1.0, 3.0))
END = dict(arrive=cn.F_ARRIVE, crash=cn.F_CRASH, out=cn.F_OUT, maxstep=cn.F_MAXSTEP, **{"crash+maxstep": cn.F_CRASH | cn.F_MAXSTEP})
# (bins, count_truncated)
CONFIGS = ((1, False), (16, False), (16, True), (5, True))

SCRIPTS = {
    (0, 0): [(1, "arrive", 0), (2, "crash", 0), (17, "out", 0), (30, "arrive", 0)],      # a slot re-used by three agents, a fourth left open
    (0, 1): [(17, "maxstep", 0), (3, "arrive", 2), (17, "crash+maxstep", 0)],
    (0, 2): [(60, "arrive", 0)],                                                         # open for the whole stream
    (0, 3): [(1, "crash", 3), (1, "arrive", 0), (1, "out", 0), (2, "maxstep", 1), (40, "arrive", 0)],
    (0, 4): [(5, "out", 5)] * 4,
}
SEAT = np.array([[0, 1, 0, 1, -1], [1, 1, 0, 0, 1], [0, -1, 1, 0, 1], [1, 0, 1, 0, 0], [0, 1, 1, 0, 1], [0, 0, 1, 1, 0]], np.int32)
GROUP = np.array([0, 1, 0, 1, 1, 2], np.int32)      # scene 5: outside the two groups, skipped
RESET_SCENE, RESET_STEP = 4, 25


def _timeline(script, start):
    """uint8 [T]: the flags of one slot whose first agent spawned before step `start` acts."""
    f = np.zeros(T, np.uint8)
    t = start
    for steps, end, gap in script:
        for k in range(steps):
            if t >= T:
                return f
            f[t] |= cn.F_ACTED
            if k == steps - 1:
                f[t] |= cn.F_DONE | END[end]
                if gap == 0:
                    f[t] |= cn.F_SPAWNED
            t += 1
        if gap > 0:
            t += gap - 1
            if t >= T:
                return f
            f[t] |= cn.F_SPAWNED
            t += 1
    return f


def stream(seed=0):
    rng = np.random.RandomState(5000 + seed)
    flags = np.zeros((T, E, N), np.uint8)
    for e in range(E):
        for n in range(N):
            script = SCRIPTS[(0, (n + e) % N)]
            flags[:, e, n] = _timeline(script, start=(e + 2 * n) % 4)
    # the reset of one scene: whatever is open is dropped, every slot gets a new agent that acts from the next step on
    flags[RESET_STEP, RESET_SCENE] |= cn.F_ENV_RESET | cn.F_SPAWNED
    flags[RESET_STEP + 1:, RESET_SCENE] = _timeline([(6, "arrive", 0), (60, "crash", 0)], 0)[:T - RESET_STEP - 1, None]
    values = (rng.standard_normal((T, E, N, len(GAMMAS))) * 3.0).astype(np.float32)
    values[3, 0, 0] = (-2.0, 2.0, 0.0)          # on the ends of the range and on a bin edge
    values[4, 1, 1] = (0.5, -0.5, 1.0)
    rew = rng.standard_normal((T, E, N)).astype(np.float32)
    nei = (rng.standard_normal((T, E, N)) * 2.0).astype(np.float32)
    glob = rng.standard_normal((T, E)).astype(np.float32)
    return dict(flags=flags, values=values, rew=rew, nei_rew=nei, glob_rew=glob, seat=SEAT.copy(), group=GROUP.copy())


def permuted(s, seed=1):
    """The same stream with its scenes in another order (seat and group tables permuted alike): the accumulators must not move."""
    p = np.random.RandomState(seed).permutation(E)
    assert (p != np.arange(E)).any()
    return dict(flags=np.ascontiguousarray(s["flags"][:, p]), values=np.ascontiguousarray(s["values"][:, p]), rew=np.ascontiguousarray(s["rew"][:, p]),
                nei_rew=np.ascontiguousarray(s["nei_rew"][:, p]), glob_rew=np.ascontiguousarray(s["glob_rew"][:, p]), seat=np.ascontiguousarray(s["seat"][p]),
                group=np.ascontiguousarray(s["group"][p]))


def covered(s):
    """What the stream exercises, counted on its flags: {episode lengths that finish}, rows with DONE | SPAWNED, truncations, open agents."""
    lengths, both, trunc, open_ = set(), 0, 0, 0
    for e in range(E):
        for n in range(N):
            run = 0
            for t in range(T):
                f = int(s["flags"][t, e, n])
                if f & cn.F_ACTED:
                    run += 1
                    if f & cn.F_DONE:
                        lengths.add(run)
                        both += bool(f & cn.F_SPAWNED)
                        trunc += cn.truncated_of(f)
                if f & (cn.F_DONE | cn.F_SPAWNED | cn.F_ENV_RESET):
                    run = 0
            open_ += run > 0
    return lengths, both, trunc, open_
