"""Streams for the tests of the evaluation recorders (tests/test_recorder_cpu.py, tests/test_gpu_recorder.py): the scripted episodes of
tests/golden/recorder.npz in the simulator's tensor format, and a scripted stream of E scenes with every kind of row the recorder has a
rule for.  A stream is a dict of numpy arrays: flags u8 [T, E, N], infos f32 [T, E, N, 8], rewards / nei_rewards f32 [T, E, N], nbr_cnt
i32 [T, E, N]."""
import os

import numpy as np

from recorder_numpy import F_ACTED, F_ARRIVE, F_CRASH, F_DONE, F_ENV_RESET, F_MAXSTEP, F_OUT, F_SPAWNED

KEYS = ("flags", "infos", "rewards", "nei_rewards", "nbr_cnt")
SVO = ("svo_estimate_deg_mean", "svo_estimate_deg_min", "svo_estimate_deg_max", "svo_reward")


def golden_cases(golden_dir):
    """[(stream, the reference's episode result as a dict)] for the three scripted episodes: the stream built as
    test_vectorised_recorder_equals_the_reference_recorder builds it, plus `rewards` = the reward rounded to fp32 and `nei_rewards` =
    the fp32-rounded mean reward of the present slots strictly within `distance`, 0 where there is none."""
    g = np.load(os.path.join(golden_dir, "recorder.npz"))
    out = []
    for c in range(int(g["n_cases"])):
        s = {k[len("c%d_in_" % c):]: g[k] for k in g.files if k.startswith("c%d_in_" % c)}
        T, N = s["present"].shape
        present, first, done = s["present"], s["first"] & s["present"], s["done"] & s["present"]
        acted = present & ~first
        fl = np.zeros((T, 1, N), np.uint8)
        fl[:, 0][acted] |= F_ACTED
        fl[:, 0][first] |= F_SPAWNED
        fl[:, 0][done & acted] |= F_DONE
        for kind, bit in ((0, F_ARRIVE), (1, F_CRASH), (2, F_OUT)):
            fl[:, 0][done & acted & (s["kind"] == kind)] |= bit
        fl[T - 1, 0, :] |= F_ENV_RESET
        info = np.zeros((T, 1, N, 8), np.float32)
        for col, key in ((0, "velocity"), (4, "cost"), (5, "episode_length"), (6, "episode_reward")):
            info[:, 0, :, col] = np.where(acted, s[key], 0.0)
        dist = float(s["distance"])
        d = np.linalg.norm(s["pos"][:, :, None, :] - s["pos"][:, None, :, :], axis=-1)          # [T, N, N]
        near = (d < dist) & present[:, :, None] & present[:, None, :] & ~np.eye(N, dtype=bool)[None]
        nbr = near.sum(-1).astype(np.int32)
        rew = np.where(present, s["rew"], 0.0).astype(np.float64)
        nei = np.where(nbr > 0, (near * rew[:, None, :]).sum(-1) / np.maximum(nbr, 1), 0.0)
        stream = dict(flags=fl, infos=info, rewards=rew.astype(np.float32)[:, None, :], nei_rewards=nei.astype(np.float32)[:, None, :],
                      nbr_cnt=nbr[:, None, :])
        out.append((stream, dict(zip(list(g["c%d_keys" % c]), (float(v) for v in g["c%d_vals" % c])))))
    return out


def scripted(E, N, T, resets, seed=0, lonely=()):
    """A stream of T steps.  `resets[e]`: the steps at which scene e's episode ends (every driving agent carries F_DONE there, every slot
    F_ENV_RESET | F_SPAWNED: the next episode's agents).  A slot waits 0..3 steps, is spawned (a spawned-only row, reward 0), drives 3..12
    steps and terminates with a random outcome; a wait of 0 puts the next agent into the terminating row (F_DONE | F_SPAWNED).  The slots
    in `lonely` (pairs (e, n)) never have a neighbour and earn a positive reward in every step.  Rewards, velocities and neighbourhood
    rewards are random fp32; a row with no neighbour has neighbourhood reward 0, as the simulator writes it."""
    rng = np.random.RandomState(seed)
    fl = np.zeros((T, E, N), np.uint8)
    info = np.zeros((T, E, N, 8), np.float32)
    rew, nrew = np.zeros((T, E, N), np.float32), np.zeros((T, E, N), np.float32)
    nbr = np.zeros((T, E, N), np.int32)
    ends = (F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP)
    for e in range(E):
        for n in range(N):
            alone = (e, n) in lonely
            alive, left, wait, length, total = False, 0, 1 + int(rng.randint(0, 3)), 0, np.float32(0.0)
            for t in range(T):
                reset = t in resets.get(e, ())
                f = 0
                nbr[t, e, n] = 0 if alone else rng.randint(0, 6)
                if nbr[t, e, n] > 0:
                    nrew[t, e, n] = rng.normal(0.3, 1.0)
                if alive:
                    f |= F_ACTED
                    length, left = length + 1, left - 1
                    rew[t, e, n] = rng.uniform(0.1, 2.0) if alone else rng.normal(0.4, 1.0)
                    total = np.float32(total + rew[t, e, n])
                    info[t, e, n, 0], info[t, e, n, 4] = rng.uniform(0.0, 80.0), float(rng.rand() < 0.15)
                    info[t, e, n, 5], info[t, e, n, 6] = length, total
                    if left == 0 or reset:
                        f |= F_DONE | ends[rng.randint(0, 4)]
                        alive, wait = False, int(rng.randint(0, 4))
                if not alive:
                    if reset or wait == 0:
                        f |= F_SPAWNED
                        alive, left, length, total = True, 3 + int(rng.randint(0, 10)), 0, np.float32(0.0)
                    else:
                        wait -= 1
                if reset:
                    f |= F_ENV_RESET
                fl[t, e, n] = f
    return dict(flags=fl, infos=info, rewards=rew, nei_rewards=nrew, nbr_cnt=nbr)


def cut(stream, size):
    """The stream as fragments of `size` steps."""
    T = stream["flags"].shape[0]
    return [{k: np.ascontiguousarray(v[t:t + size]) for k, v in stream.items()} for t in range(0, T, size)]


def restate(fragments, E, N, **kwargs):
    """A `RecorderNumpy` that has consumed the fragments."""
    from recorder_numpy import RecorderNumpy
    ref = RecorderNumpy(E, N, **kwargs)
    for b in fragments:
        ref.add(*(b[k] for k in KEYS))
    return ref
