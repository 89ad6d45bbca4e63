"""Cases shared by the interaction meter's tests (test_interact_cpu.py, test_gpu_interact.py): hand-set scenes, random poses and the
rollout of the reference's CoPO Intersection population.  States are the simulator's blocks [16][E][N] of 32-bit words."""
import os

import numpy as np

import interact_numpy as im
from copo_amd.sim import SimConfig

HL, HW = 2.2575, 0.926
ALIVE, WRECK, EMPTY = im.ST_ALIVE, im.ST_WRECK, im.ST_EMPTY

# every hand case of test_interact_cpu.py: name -> (body i, body j) as (x, y, heading, speed, status); expected (gap, TTC) of body i
HAND_CASES = {
    "head on": (((100.0, 40.0, 0.0, 5.0, ALIVE), (120.0, 40.0, np.pi, 5.0, ALIVE)), (15.485, 1.5485)),
    "side by side": (((100.0, 40.0, 0.0, 7.0, ALIVE), (100.0, 43.5, 0.0, 7.0, ALIVE)), (1.648, np.inf)),
    "perpendicular crossing": (((100.0, 40.0, 0.0, 10.0, ALIVE), (120.0, 25.0, np.pi / 2, 10.0, ALIVE)), (np.hypot(16.8165, 11.8165), 1.68165)),
    "cross-shaped overlap": (((100.0, 40.0, 0.0, 3.0, ALIVE), (100.3, 40.2, np.pi / 2, 2.0, ALIVE)), (0.0, 0.0)),
    "wreck ahead": (((100.0, 40.0, 0.0, 8.0, ALIVE), (115.0, 40.0, 0.0, 5.0, WRECK)), (10.485, 10.485 / 8)),
}


def put(st, e, n, body, aid):
    x, y, th, v, status = body
    st[0, e, n], st[1, e, n], st[2, e, n], st[3, e, n] = x, y, th, v
    si = st.view(np.int32)
    si[13, e, n] = (si[13, e, n] & ~0xFF) | status
    si[14, e, n] = aid


def hand_state(st0, case):
    """E = 2, N = 5.  Scene 0: the pair in slots 1 and 3, the other slots EMPTY with poses on top of body i (they must not count);
    scene 1: the pair in slots 4 and 0 (the other order) and a third vehicle driving away 200 m off."""
    (bi, bj), _ = HAND_CASES[case]
    st = st0.copy()
    assert st.shape[1:] == (2, 5)
    for e in range(2):
        for n in range(5):
            put(st, e, n, bi[:4] + (EMPTY,), 50 + n)
    put(st, 0, 1, bi, 7)
    put(st, 0, 3, bj, 8)
    put(st, 1, 4, bi, 7)
    put(st, 1, 0, bj, 8)
    put(st, 1, 2, (bi[0] - 200.0, bi[1] + 90.0, np.pi, 9.0, ALIVE), 9)
    return st


def random_state(st0, seed, aligned=False):
    """Random bodies over the slots of every scene: 65 % ALIVE, 20 % WRECK, 15 % EMPTY, inside an 80 m (N > 16) or 30 m box -- dense
    enough for overlaps and near misses --, speeds 0..15 m/s (one in eight standing).  `aligned`: headings are multiples of 90
    degrees and speeds multiples of 5 m/s, so that pairs with no relative motion along an axis (q == 0) occur."""
    rng = np.random.RandomState(seed)
    st = st0.copy()
    _, E, N = st.shape
    box = 80.0 if N > 16 else 30.0
    for e in range(E):
        for n in range(N):
            status = rng.choice([ALIVE, WRECK, EMPTY], p=[0.65, 0.2, 0.15])
            x, y = 60.0 + box * rng.rand(), -40.0 + box * rng.rand()
            th = rng.uniform(-np.pi, np.pi)
            v = 0.0 if rng.rand() < 0.125 else rng.uniform(0.0, 15.0)
            if aligned:
                th, v = (np.pi / 2) * rng.randint(-1, 3), 5.0 * rng.randint(0, 4)
                x, y = np.round(x * 2) / 2, np.round(y * 2) / 2
            put(st, e, n, (x, y, th, v, status), int(rng.randint(0, 1000)))
    return st


# (seed, aligned) of the random-pose cases: one scene of 64 slots, three scenes of 7
RANDOM_SEEDS_64 = ((1, False), (2, True))
RANDOM_SEEDS_7 = ((1, False), (2, True), (3, False))


def ambiguous_samples(st, P):
    """(ALIVE samples, ambiguous ones) of one recorded state, by the restatement alone"""
    tr = im.Tracker(P, st.shape[1], st.shape[2])
    tr.record(st, np.zeros((st.shape[1], 4), np.int32))
    return tr.alive_samples, tr.ambiguous_samples


# ---- rollout: Intersection, 3 scenes x 10 slots, 120 steps of the reference's CoPO population.  An agent ends after 55 steps of driving
# at the latest (`horizon`), wrecks stay for 3 steps (`delay_done`); with these seeds agents crash early enough for three slots to be
# taken over by new agents inside an episode, and the scenes are reset at steps 54 / 83 / 109 (they stop respawning after 55 steps
# and drain) ----
ROLLOUT_STEPS = 120


def rollout_config():
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    mean, std = meta_svo_lookup_table["copo_inter"]
    return SimConfig(map="intersection", num_envs=3, num_agents=10, horizon=55, delay_done=3, start_seed=11, lcf_mean=float(mean), lcf_std=float(std))


def rollout_policy(golden_dir):
    """obs [E, N, O] -> actions [E, N, 2] (the Gaussian head's mean: no random draw)"""
    from copo_amd.eval.get_policy_function import _gaussian_head, layer_arrays, population_layout
    with np.load(os.path.join(golden_dir, "eval_policy_function.npz")) as f:
        pre = "copo_inter/w/"
        w = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    layout, sfx = population_layout("copo_inter")
    layers = layer_arrays(w, layout, "default", sfx)

    def act(obs):
        E, N, O = obs.shape
        return np.ascontiguousarray(_gaussian_head(layers, obs.reshape(E * N, O).astype(np.float32), True).reshape(E, N, 2), np.float32)
    return act
