"""Cases shared by the traffic gates' tests (test_gates_cpu.py, test_gpu_gates.py): a hand-made sequence of six records whose crossings,
headways and travel times are worked out by hand, padded gate and section tables for the launch limits, and the rollout of the reference's
CoPO Intersection population.  States are the simulator's blocks [16][E][N] of 32-bit words, env [E][4] int32."""
import numpy as np

import gate_numpy as gn
import interact_cases as ic
from copo_amd.sim import SimConfig

ALIVE, WRECK, EMPTY = gn.ST_ALIVE, gn.ST_WRECK, gn.ST_EMPTY
NAN = float("nan")
Y_PAST_A = float(np.nextafter(np.float32(50.0), np.float32(60.0)))      # one fp32 step beyond endpoint A of the hand gates

# Gate 0: A = (100, 50) -> B = (100, 40): d = (0, -10), side(P) = 10 (P.x - 100): FORWARD is driving in +x across x = 100 between y = 40
# and 50; the right-hand side of A -> B is x < 100.  Gate 1: the same at x = 110.
HAND_GATES = np.array([(100.0, 50.0, 100.0, 40.0), (110.0, 50.0, 110.0, 40.0)], np.float32)
HAND_SECTIONS = [(0, 1), (1, 0), (0, 0)]
HAND_KW = dict(groups=3, bins=(2, 3), headway_bins=3, tt_bins=(2, 2))       # series: records 0..2 / 3..5; headway clips at 2, tt at 2 records
HAND_E, HAND_RECORDS = 5, 6


def _drive(xs, y, v, aid, status=ALIVE):
    status = status if isinstance(status, (list, tuple)) else [status] * len(xs)
    aid = aid if isinstance(aid, (list, tuple)) else [aid] * len(xs)
    return [(x, y, v, s, a) for x, s, a in zip(xs, status, aid)]


# slot -> its (x, y, speed, status, agent id) in records 0..5
_SCENE_A = {
    0: _drive([99, 101, 103, 99, 101, 111], 45.0, 10.0, 10),          # fwd g0 at 1, bwd g0 at 3, fwd g0 at 4, fwd g1 at 5
    1: _drive([99, 100, 105, 109, 111, 111], 45.0, 5.0, 11),          # cur exactly on the line: fwd g0 at 1; fwd g1 at 4
    2: _drive([100, 99, 99, 99, 99, 99], 45.0, 2.0, 12),              # prev exactly on the line, moving right of A -> B: bwd g0 at 1
    3: _drive([100, 101, 101, 101, 101, 101], 45.0, 2.0, 13),         # prev on the line, moving left: nothing
    4: _drive([99, 101, 101, 101, 101, 111], 50.0, 300.0, 14),        # through endpoint A: fwd g0 at 1, fwd g1 at 5; speed clamps to 255
    5: _drive([99, 101, 101, 101, 101, 111], Y_PAST_A, 9.0, 15),      # one fp32 step beyond A: nothing
    6: [(100.0, y, 4.0, ALIVE, 16) for y in (41, 49, 41, 49, 41, 49)],  # along the gate: nothing
}
_SCENE_B = {
    0: _drive([100] * 6, 45.0, 3.0, 20),                              # zero motion on the line
    1: _drive([99] * 6, 45.0, 3.0, 21),                               # zero motion
    2: _drive([99, 101, 101, 101, 101, 101], 45.0, 3.0, [22, 23, 23, 23, 23, 23]),        # the agent id changes with the move: nothing
    3: _drive([99, 101, 103, 99, 101, 101], 45.0, 1.0, 24, [ALIVE, WRECK, WRECK, ALIVE, ALIVE, ALIVE]),   # fwd g0 at 4 only
    4: _drive([99, 101, 99, 101, 99, 101], 45.0, 3.0, 25, EMPTY),     # an EMPTY slot: nothing
    5: _drive([NAN, 101, NAN, 99, 99, 99], 45.0, 3.0, 26),            # a NaN never crosses (99 <- NaN, NaN <- 101)
    6: _drive([99, 101, 99, 99, 99, 99], 45.0, 0.0, 27),              # fwd g0 at 1 (tt = 0 in section (0, 0)), bwd g0 at 2; standing: q = 0
}
_SCENE_C = {                                                          # the episode word changes between records 0 and 1
    0: _drive([99, 101, 99, 99, 99, 99], 45.0, 3.0, 30),              # nothing at 1; bwd g0 at 2
    1: _drive([99, 101, 101, 101, 101, 101], 45.0, 3.0, 31),          # nothing
}
HAND_SCENES = (_SCENE_A, _SCENE_B, _SCENE_C, _SCENE_A, _SCENE_A)      # scene 3 names a group that does not exist
HAND_EPISODES = ((0,) * 6, (0,) * 6, (0, 1, 1, 1, 1, 1), (4,) * 6, (0,) * 6)


def hand_groups(G, r):
    """groups of record r: G = 3: scenes 0, 4 -> 0, scene 1 -> 1, scene 2 -> 2, scene 3 -> 3 (no such group) and, from record 4 on, -> 2
    (its slot memory, last_fwd and entries were kept while it was off); G = 1: all 0 but scene 3 = 5 throughout"""
    return (0, 1, 2, 3 if r < 4 else 2, 0) if G == 3 else (0, 0, 0, 5, 0)


def hand_record(st0, env0, r, seed=7):
    """(state, env) of record r on the base arrays [16, 5, N] / [5, 4] (N >= 7): slots 0..6 as above, every other slot of the first
    seven EMPTY; slots 7.. (N = 64) drive at random around both gates, one in ten a wreck or empty in any record."""
    st, env = st0.copy(), env0.copy()
    _, E, N = st.shape
    assert E == HAND_E and N >= 7
    rng = np.random.RandomState(seed)
    walk = rng.uniform([95.0, 38.0], [115.0, 52.0], (E, N, 2))
    for k in range(r + 1):
        step = rng.uniform(-4.0, 4.0, (E, N, 2)) * (rng.rand(E, N, 1) < 0.8)
        status = rng.choice([ALIVE, WRECK, EMPTY], p=[0.9, 0.05, 0.05], size=(E, N))
        aid = 100 + np.arange(N)[None, :] + 64 * (rng.rand(E, N) < 0.03)
        walk = walk + step if k else walk
    for e in range(E):
        env[e, 1] = HAND_EPISODES[e][r]
        for n in range(N):
            if n < 7:
                x, y, v, s, a = HAND_SCENES[e].get(n, [(0.0, 0.0, 0.0, EMPTY, 90 + n)] * HAND_RECORDS)[r]
            else:
                x, y, v, s, a = walk[e, n, 0], walk[e, n, 1], float(3 * n % 17), int(status[e, n]), int(aid[e, n])
            ic.put(st, e, n, (x, y, 0.0, v, s), a)
    return st, env


# What the six hand records give with HAND_GATES / HAND_SECTIONS / HAND_KW and N = 7, worked out by hand (speed x 256: 10 -> 2560,
# 5 -> 1280, 2 -> 512, 300 -> 65280, 1 -> 256, 3 -> 768).  One copy of scene A:
#   g0 fwd: slots 0, 1, 4 at record 1, slot 0 at 4; g0 bwd: slot 2 at 1, slot 0 at 3; g1 fwd: slot 1 at 4, slots 0, 4 at 5.
#   headway g0: record 1 has three crossings, the first finds no earlier one: bin 0 += 2; record 4: h = 3 -> bin 2.  g1: record 4 is
#   the first; record 5: h = 1 -> bin 1, the second crossing bin 0.
#   section (0, 1): slot 1 enters at 1, leaves at 4: tt 3 -> bin 1; slot 0 enters at 1, again at 4, leaves at 5: tt 1 -> bin 0; slot 4
#   enters at 1, leaves at 5: tt 4 -> bin 2, clipped to 1.  Section (0, 0): every forward crossing of g0 with tt = 0.
_A = dict(count=[[4, 2], [3, 0]], speed_q=[[2560 + 1280 + 65280 + 2560, 512 + 2560], [1280 + 2560 + 65280, 0]],
          series=[[[3, 1], [1, 1]], [[0, 3], [0, 0]]], headway=[[2, 0, 1], [1, 1, 0]], sec_count=[3, 0, 4], sec_sum=[8, 0, 0],
          sec_hist=[[1, 2], [0, 0], [4, 0]], scene_records=6, alive=42)
# scene B: fwd g0 by slot 6 at 1 (q 0) and slot 3 at 4 (q 256, h = 3 -> bin 2), bwd g0 by slot 6 at 2 (q 0); ALIVE: five slots always, slot 3
# in four records.
_B = dict(count=[[2, 1], [0, 0]], speed_q=[[256, 0], [0, 0]], series=[[[1, 1], [1, 0]], [[0, 0], [0, 0]]], headway=[[0, 0, 1], [0, 0, 0]],
          sec_count=[0, 0, 2], sec_sum=[0, 0, 0], sec_hist=[[0, 0], [0, 0], [2, 0]], scene_records=6, alive=34)
# group 2 = scene C (bwd g0 by slot 0 at 2) + records 4 and 5 of scene 3, a copy of scene A that was remembered while switched off: slot 0
# fwd g0 at 4 with h = 3 and tt = 0; slot 1 fwd g1 at 4 (the first there) with tt 3; slots 0, 4 fwd g1 at 5 with tt 1 and 4.
_C = dict(count=[[1, 1], [3, 0]], speed_q=[[2560, 768], [1280 + 2560 + 65280, 0]], series=[[[0, 1], [1, 0]], [[0, 3], [0, 0]]],
          headway=[[0, 0, 1], [1, 1, 0]], sec_count=[3, 0, 1], sec_sum=[8, 0, 0], sec_hist=[[1, 2], [0, 0], [1, 0]], scene_records=6 + 2,
          alive=12 + 14)
HAND_EXPECTED = {k: np.array([np.array(_A[k]) * 2, np.array(_B[k]), np.array(_C[k])], np.int64) for k in gn.RAW}


def padded_gates(L):
    """L gates: the two hand gates, then gates across the random walkers' box every 0.37 m, every other one reversed"""
    g = [tuple(q) for q in HAND_GATES][:L]
    for k in range(len(g), L):
        x = 100.0 + 0.37 * k
        g.append((x, 50.0, x, 40.0) if k % 2 == 0 else (x, 38.5, x, 51.5))
    return np.array(g, np.float32)


def padded_sections(S, L):
    return [(s % min(L, 8), (3 * s + 1) % L) for s in range(S)]


# ---- rollout: Intersection, 6 scenes x 40 slots, 200 steps of the reference's CoPO population with the default horizon, gates 30 m from
# the ends of every route (the spawn slots 4 .. 29 m along the entry roads lie before the entry gates, and a trip between the gates takes
# 90 .. 220 steps in this traffic).  tests/test_gates_cpu.py asserts what the case is chosen for ----
ROLLOUT_STEPS, ROLLOUT_MID, ROLLOUT_INSET = 200, 100, 30.0
ROLLOUT_KW = dict(groups=2, bins=(8, 32), headway_bins=32, tt_bins=(32, 10))
ROLLOUT_GROUPS = (0, 1, 0, 1, -1, 0)


def rollout_config():
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    mean, std = meta_svo_lookup_table["copo_inter"]
    return SimConfig(map="intersection", num_envs=6, num_agents=40, delay_done=3, start_seed=11, lcf_mean=float(mean), lcf_std=float(std))


def rollout_gates(cfg):
    from copo_amd.gates import gates_for_map
    return gates_for_map(cfg.tables(), ROLLOUT_INSET)


def check_invariants(ref):
    """what holds for every run, on the accumulators of a restatement (or anything with the same attributes)"""
    fwd = ref.count[:, :, 0]
    for s, (gi, go) in enumerate(ref.sections):
        assert (ref.sec_count[:, s] <= np.minimum(fwd[:, gi], fwd[:, go])).all(), s
    assert ref.headway.sum() == fwd.sum() - ref.first_crossings
    assert np.array_equal(ref.series.sum(-1), ref.count) and np.array_equal(ref.sec_hist.sum(-1), ref.sec_count)


def check_premises(ref):
    """what the rollout case is chosen for: without these the comparison with the device would be vacuous"""
    fwd = ref.count[:, :, 0].sum(0)
    assert (fwd >= 1).all(), fwd.tolist()
    assert ref.sec_count.sum() >= 1 and ref.headway[:, :, 1:].sum() >= 1
    assert ref.max_crossings_of_a_gate_in_a_scene_record >= 2
