"""Cases shared by the encroachment log's tests (test_pet_cpu.py, test_gpu_pet.py, test_gpu_env_pet.py): a hand-made sequence of twelve
records whose rows are written out by hand -- three scenes at 7 slots, five at 64 -- and two rollouts of the reference's populations.
States are the simulator's blocks [16][E][N] of 32-bit words, env [E][4] int32.

The hand grid: 32 x 32 cells of 1 m from (0, 0), window 4, critical_records 2.  A body (hl 2.2575, hw 0.926) with heading 0 and its centre at
(k + 0.5, j + 0.5) covers the cells (k - 2 .. k + 2, j); with heading fp32(pi / 2) the cells (k, j - 2 .. j + 2); every cell centre is at
least 0.07 m from an edge of a body."""
import numpy as np

import field_numpy as fn
import interact_cases as ic
import pet_numpy as pn

ALIVE, EMPTY = pn.ST_ALIVE, pn.ST_EMPTY
HL, HW = ic.HL, ic.HW
UP = float(np.float32(np.pi / 2))
HAND_W = HAND_H = 32
HAND_WINDOW, HAND_CRITICAL, HAND_RECORDS, HAND_FORGET_BEFORE = 4, 2, 12, 10
HAND_EPISODES = {2: (5,) * 8 + (6,) * 4}          # scene -> the episode word per record; every other scene: 0


def hand_grid():
    return fn.Grid(0.0, 0.0, HAND_W, HAND_H, 1.0)


def hand_scenes(N):
    assert N in (7, 64)
    return 3 if N == 7 else 5


# (scene, slot) -> [(first record, aid, x, y, heading)] in record order; a pose holds until the next entry, aid None = EMPTY.  A slot that
# is not listed is EMPTY at (0.5, 0.5), on top of nothing that matters: it must not count.
OUT = -10.5                                        # no cell
HAND_SLOTS = {
    # scene 0.  Slot 1 goes up column 10 and enters cell (10, 10), which slot 0 left after record 0, in record 3: a perpendicular crossing
    # with PET 3; in record 4 it touches (10, 11), which slot 0 left after record 1: the same partner, no second row
    (0, 0): [(0, 10, 8.5, 10.5, 0.0), (1, 10, 8.5, 11.5, 0.0), (2, 10, 20.5, 10.5, 0.0)],
    (0, 1): [(0, 11, 10.5, 2.5, UP), (1, 11, 10.5, 4.5, UP), (2, 11, 10.5, 6.5, UP), (3, 11, 10.5, 8.5, UP), (4, 11, 10.5, 9.5, UP)],
    # slot 2 has arrived (EMPTY from record 2) before slot 3 enters (8, 20) in record 2: the earlier agent is not driving, no row
    (0, 2): [(0, 12, 8.5, 20.5, 0.0), (1, 12, 14.5, 20.5, 0.0), (2, None, 14.5, 20.5, 0.0)],
    (0, 3): [(0, 13, 8.5, 14.5, UP), (1, 13, 8.5, 16.5, UP), (2, 13, 8.5, 18.5, UP)],
    # slot 4 enters (4, 26) of slot 5 and (6, 26) of slot 6 in record 2: two new partners in one record; slot 5 moves half out of the grid
    # (rows 29 .. 31 of 29 .. 33)
    (0, 4): [(0, 14, OUT, 26.5, 0.0), (1, 14, -4.5, 26.5, 0.0), (2, 14, 5.5, 26.5, 0.0)],
    (0, 5): [(0, 15, 4.5, 26.5, UP), (1, 15, 4.5, 31.5, UP)],
    (0, 6): [(0, 16, 6.5, 26.5, UP), (1, 16, 28.5, 26.5, UP)],
    # scene 1.  A follower (slot 1, half outside in record 1: columns 0 and 1 of -3 .. 1) enters (2, 5) and (3, 5) of its leader in record 2
    # and more of them in record 3
    (1, 0): [(0, 20, 4.5, 5.5, 0.0), (1, 20, 9.5, 5.5, 0.0), (2, 20, 14.5, 5.5, 0.0), (3, 20, 25.5, 5.5, 0.0)],
    (1, 1): [(0, 21, OUT, 5.5, 0.0), (1, 21, -0.5, 5.5, 0.0), (2, 21, 1.5, 5.5, 0.0), (3, 21, 6.5, 5.5, 0.0)],
    # the window: slot 2 leaves (2 .. 6, 15) after record 0; slot 4 enters (6, 15) in record 4 = window: a row; slot 3 enters (4, 15) in
    # record 5 = window + 1: none
    (1, 2): [(0, 22, 4.5, 15.5, 0.0), (1, 22, 25.5, 15.5, 0.0)],
    (1, 3): [(0, 23, 4.5, 25.5, UP), (5, 23, 4.5, 15.5, UP)],
    (1, 4): [(0, 24, 6.5, 25.5, UP), (4, 24, 6.5, 15.5, UP)],
    # two bodies over the centre of (14, 25) from record 6 on: the stamp kept is slot 6's (agent 26 > 25), which slot 5 reads in record 7;
    # `forget` before record 10 voids it and clears the masks: no row in record 10, the same row again in record 11
    (1, 5): [(0, None, 0.5, 0.5, 0.0), (6, 25, 14.5, 25.5, 0.0)],
    (1, 6): [(0, None, 0.5, 0.5, 0.0), (6, 26, 14.5, 25.5, UP)],
    # scene 2.  Slot 1 enters (10, 5) of slot 0 in record 2 (a row) and (13, 5) in record 3 (none); in record 4 it holds agent 32 instead of
    # 31, without DONE: the turnover clears its mask and (18, 5) counts anew.  Slot 2 enters (10, 15) of agent 31 in record 3; the turnover
    # clears bit 1 of its mask too, so (18, 5) of agent 32 counts in record 6, next to (16, 5), (17, 5), (19, 5) of slot 0 at exactly the
    # window ((15, 5) is one record older)
    (2, 0): [(0, 30, 8.5, 5.5, 0.0), (1, 30, 13.5, 5.5, 0.0), (2, 30, 18.5, 5.5, 0.0), (3, 30, 23.5, 5.5, 0.0), (4, 30, 28.5, 5.5, 0.0)],
    (2, 1): [(0, 31, 10.5, 15.5, UP), (2, 31, 10.5, 5.5, UP), (3, 31, 13.5, 5.5, UP), (4, 32, 18.5, 5.5, UP), (5, 32, 18.5, 25.5, UP)],
    (2, 2): [(0, 33, 25.5, 15.5, 0.0), (3, 33, 9.5, 15.5, 0.0), (6, 33, 17.5, 5.5, 0.0)],
    # the episode word changes in record 8: (8, 28), which slot 3 left after record 7, is void for slot 4 in record 8; (20, 28), left after
    # record 8, counts in record 9
    (2, 3): [(0, None, 0.5, 0.5, 0.0), (7, 34, 8.5, 28.5, 0.0), (8, 34, 20.5, 28.5, 0.0), (9, 34, 27.5, 28.5, 0.0)],
    (2, 4): [(0, None, 0.5, 0.5, 0.0), (8, 35, 8.5, 28.5, UP), (9, 35, 20.5, 28.5, UP)],
}
# N = 64 only: the last two lanes, a low lane with a partner in lane 63, and a scene with one lone agent
HAND_SLOTS_64 = {
    (3, 62): [(0, 962, 8.5, 10.5, 0.0), (1, 962, 20.5, 10.5, 0.0)],
    (3, 63): [(0, 963, 10.5, 2.5, UP), (1, 963, 10.5, 9.5, UP)],
    (3, 1): [(0, None, 0.5, 0.5, 0.0), (3, 901, 10.5, 3.5, 0.0)],
    (4, 7): [(0, 907, 5.5, 5.5, 0.0)],
}


def hand_slots(N):
    return {**HAND_SLOTS, **HAND_SLOTS_64} if N == 64 else HAND_SLOTS


def _speed(slot, r):
    return 1.0 + slot + 0.25 * r


def _at(spans, r):
    return [s for s in spans if s[0] <= r][-1]


def hand_record(st0, env0, r):
    """(state, env) of record r on the base arrays [16, E, N] / [E, 4] (E, N = 3, 7 or 5, 64)"""
    st, env = st0.copy(), env0.copy()
    _, E, N = st.shape
    assert E == hand_scenes(N)
    slots = hand_slots(N)
    for e in range(E):
        env[e, 1] = HAND_EPISODES.get(e, (0,) * HAND_RECORDS)[r]
        for n in range(N):
            spans = slots.get((e, n))
            if spans is None or _at(spans, r)[1] is None:
                ic.put(st, e, n, (0.5, 0.5, 0.0, 0.0, EMPTY), 60 + n)
                continue
            _, aid, x, y, th = _at(spans, r)
            ic.put(st, e, n, (x, y, th, _speed(n, r), ALIVE), aid)
    return st, env


def _row(N, scene, r, b, a, pet, cell_xy, n_cells):
    """b entered in record r what a had left; the row's words, the poses and ids from the script"""
    bt = lambda v: int(np.float32(v).view(np.uint32))      # noqa: E731
    slots = hand_slots(N)
    _, aid_b, x, y, th_b = _at(slots[(scene, b)], r)
    _, aid_a, _, _, _ = _at(slots[(scene, a)], r)
    hq = lambda th: 64 if th == UP else 0                  # noqa: E731
    th_a = _at(slots[(scene, a)], r - pet)[4]              # the heading in the stamp: of the record that wrote it
    ep = HAND_EPISODES.get(scene, (0,) * HAND_RECORDS)[r]
    return [scene, b | (a << 6), aid_b, aid_a, ep, r, pet, cell_xy[1] * HAND_W + cell_xy[0], n_cells, bt(_speed(a, r)), bt(x), bt(y), bt(th_b),
            bt(_speed(b, r)), hq(th_a), hq(th_b)]


# The rows, worked out by hand: (scene, record, slot_b, slot_a, pet, (ix, iy) of the cell, n_cells), in (record, scene, slot_b, slot_a) order
HAND_ROWS = [
    (0, 2, 4, 5, 2, (4, 26), 1), (0, 2, 4, 6, 2, (6, 26), 1), (1, 2, 1, 0, 2, (2, 5), 2), (2, 2, 1, 0, 2, (10, 5), 1),
    (0, 3, 1, 0, 3, (10, 10), 1), (2, 3, 2, 1, 2, (10, 15), 1), (3, 3, 1, 63, 3, (10, 3), 1),
    (1, 4, 4, 2, 4, (6, 15), 1), (2, 4, 1, 0, 2, (18, 5), 1),
    (2, 6, 2, 0, 4, (16, 5), 3), (2, 6, 2, 1, 2, (18, 5), 1),
    (1, 7, 5, 6, 1, (14, 25), 1),
    (2, 9, 4, 3, 1, (20, 28), 1),
    (1, 11, 5, 6, 1, (14, 25), 1),
]
HAND_ROWS_64_REC1 = (3, 1, 63, 62, 1, (10, 10), 1)     # ahead of every row above: record 1
# by hand from the rows (7 slots, one group): hist[type][pet - 1], and the critical map's cells (pet <= 2) as (ix, iy) -> count
HAND_HIST = [[0, 1, 0, 1], [3, 6, 1, 1], [0, 0, 0, 0]]
HAND_CRITICAL_MAP = {(4, 26): 1, (6, 26): 1, (2, 5): 1, (10, 5): 1, (10, 15): 1, (18, 5): 2, (14, 25): 2, (20, 28): 1}


def hand_expected(N, upto=HAND_RECORDS):
    """the rows of the records below `upto`, uint32 [n, 16]"""
    rows = [q for q in HAND_ROWS if q[0] < hand_scenes(N)]
    if N == 64:
        rows = [HAND_ROWS_64_REC1] + rows
    rows = sorted((q for q in rows if q[1] < upto), key=lambda q: (q[1], q[0], q[2], q[3]))
    return np.array([[w & 0xFFFFFFFF for w in _row(N, *q)] for q in rows], np.uint32).reshape(-1, 16)


def hand_log(N, **kwargs):
    """the restatement for the hand sequence"""
    kw = dict(window=HAND_WINDOW, critical_records=HAND_CRITICAL)
    kw.update(kwargs)
    return pn.EncroachmentLog(hand_scenes(N), N, hand_grid(), HL, HW, **kw)


def run_hand(N, record, forget, st0=None, env0=None, upto=HAND_RECORDS):
    """Drive the hand sequence: `record(r, st, env)` makes record r, `forget()` comes before record HAND_FORGET_BEFORE."""
    E = hand_scenes(N)
    st0 = np.zeros((16, E, N), np.float32) if st0 is None else st0
    env0 = np.zeros((E, 4), np.int32) if env0 is None else env0
    for r in range(upto):
        if r == HAND_FORGET_BEFORE:
            forget()
        record(r, *hand_record(st0, env0, r))


# ---- rollouts: 6 scenes x 40 slots of the reference's CoPO populations (the Intersection population, on the two maps where paths cross), a grid of 1 m cells over the
# map; seeds and lengths picked on the CPU oracle so that the premises of test_pet_cpu.py hold ----
ROLLOUTS = {
    "intersection": dict(key="copo_inter", start_seed=11, steps=100),
    "roundabout": dict(key="copo_inter", start_seed=11, steps=100),
}
ROLLOUT_WINDOW, ROLLOUT_CRITICAL = 50, 10
GPU_ROLLOUT_STEPS = 60                              # of the same rollouts, on the GPU: the restatement runs next to the device


def rollout_config(name, num_envs=6, num_agents=40):
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    from copo_amd.sim import SimConfig
    c = ROLLOUTS[name]
    mean, std = meta_svo_lookup_table[c["key"]]
    return SimConfig(map=name, num_envs=num_envs, num_agents=num_agents, start_seed=c["start_seed"], lcf_mean=float(mean), lcf_std=float(std))


def rollout_policy(golden_dir, name):
    """obs [E, N, O] -> actions [E, N, 2] of the population of map `name` (the Gaussian head's mean: no random draw)"""
    import os
    from copo_amd.eval.get_policy_function import _gaussian_head, layer_arrays, population_layout
    key = ROLLOUTS[name]["key"]
    with np.load(os.path.join(golden_dir, "eval_policy_function.npz")) as f:
        pre = key + "/w/"
        w = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    layout, sfx = population_layout(key)
    layers = layer_arrays(w, layout, "default", sfx)

    def act(obs):
        E, N, O = obs.shape
        return np.ascontiguousarray(_gaussian_head(layers, obs.reshape(E * N, O).astype(np.float32), True).reshape(E, N, 2), np.float32)
    return act


def rollout_grid(cfg, cell=1.0, margin=5.0):
    """the grid `EncroachmentLog.for_map` gives for the map of `cfg`"""
    from copo_amd import fields
    x0, y0, W, H = fields.grid_for_map(cfg.resolved()[0], cell, margin)
    return fn.Grid(x0, y0, W, H, cell)


def refused_configs(_capi):
    """the configurations `copo_pet_create` refuses whatever the body, with their codes"""
    nan, inf = float("nan"), float("inf")
    K = lambda **kw: _capi.PetCfg(**{**dict(x0=0.0, y0=0.0, cell=1.0, W=32, H=32, G=1, window=50, critical_records=10, max_rows=16), **kw})   # noqa: E731
    return ((K(max_rows=0), -2), (K(W=0), -2), (K(H=1025), -2), (K(G=0), -2), (K(G=65), -2), (K(window=0), -2), (K(window=4097), -2),
            (K(critical_records=-1), -2), (K(cell=0.0), -2), (K(cell=nan), -2), (K(cell=inf), -2), (K(x0=nan), -5), (K(y0=inf), -5),
            (K(cell=1e-40), -5), (K(cell=1.5), -5))


def check_invariants(ref):
    """what holds for every run on a restatement: the order rule, and what a row says about itself"""
    rows = ref.rows().astype(np.int64)
    b, a = rows[:, 1] & 63, (rows[:, 1] >> 6) & 63
    assert (a != b).all() and (a < ref.N).all() and (b < ref.N).all()
    assert (rows[:, 6] >= 1).all() and (rows[:, 6] <= ref.window).all() and (rows[:, 8] >= 1).all() and (rows[:, 7] < ref.grid.W * ref.grid.H).all()
    order = [(c, int(s), int(x), int(y)) for c, s, x, y in zip(ref.close_rec, rows[:, 0], b, a)]
    assert order == sorted(order) and len(set(order)) == len(order) and ref.close_rec == rows[:, 5].tolist()
    if ref.dropped == 0 and (ref.group >= 0).all() and (ref.group < ref.G).all():
        assert ref.hist.sum() == len(rows) and ref.critical.sum() == (rows[:, 6] <= ref.critical_records).sum()
