"""Cases shared by the field maps' tests (test_fields_cpu.py, test_gpu_fields.py): hand-set bodies with the cells worked out by hand,
grids for the random poses of interact_cases.py, and the rollout of the reference's CoPO Intersection population."""
import numpy as np

import field_numpy as fn
import interact_cases as ic
from copo_amd.sim import SimConfig

HL, HW = 2.2575, 0.926
ALIVE, WRECK, EMPTY = fn.ST_ALIVE, fn.ST_WRECK, fn.ST_EMPTY
PI = float(np.pi)

# 24 x 20 cells of 1 m from (90, 30): cell (ix, iy) has the centre (90.5 + ix, 30.5 + iy)
HAND_GRID = dict(x0=90.0, y0=30.0, W=24, H=20, cell=1.0)


def _row(ix0, ix1, iy, v=1):
    return {(ix, iy): v for ix in range(ix0, ix1 + 1)}


# name -> (bodies (x, y, heading, speed, status), {layer: {(ix, iy): value}}); layers not named are all zero.
# A body at (100.5, 40.5) sits on the centre of cell (10, 10).  Heading 0: |dx| <= 2.2575 keeps dx = 0, +-1, +-2 and |dy| <= 0.926 keeps
# dy = 0: five cells in a row.  Heading 45 degrees: u = (dx + dy) / sqrt 2, n = (dy - dx) / sqrt 2, so |dx + dy| <= 3 (3.19) and
# |dy - dx| <= 1 (1.31): dy = dx gives dx = -1, 0, 1; dy = dx + 1 gives dx = -2 .. 1; dy = dx - 1 gives dx = -1 .. 2: eleven cells.
_DIAG = {(10 + d, 10 + d): 1 for d in (-1, 0, 1)}
_DIAG.update({(10 + d, 11 + d): 1 for d in (-2, -1, 0, 1)})
_DIAG.update({(10 + d, 9 + d): 1 for d in (-1, 0, 1, 2)})
HAND_CASES = {
    # 10 + 1/512 m/s: x 256 = 2560.5, half to even = 2560
    "axis aligned": ([(100.5, 40.5, 0.0, 10.001953125, ALIVE)],
                     dict(occupancy=_row(8, 12, 10), visits={(10, 10): 1}, speed_q={(10, 10): 2560}, vx_q={(10, 10): 2560})),
    # 5 cos 45 x 256 = 905.097
    "45 degrees": ([(100.5, 40.5, PI / 4, 5.0, ALIVE)],
                   dict(occupancy=_DIAG, visits={(10, 10): 1}, speed_q={(10, 10): 1280}, vx_q={(10, 10): 905}, vy_q={(10, 10): 905})),
    # centre in cell (0, 10): the cells at 88.5 and 89.5 are not in the grid; standing: v = 0 quantises to 0
    "half outside": ([(90.5, 40.5, 0.0, 0.0, ALIVE)], dict(occupancy=_row(0, 2, 10), visits={(0, 10): 1})),
    # centre in cell (-1, 10): no centre-cell layer, the two footprint cells inside the grid count
    "centre outside": ([(89.5, 40.5, 0.0, 7.0, ALIVE)], dict(occupancy=_row(0, 1, 10))),
    # heading 90 degrees: five cells in a column; a wreck owns no visit and no speed
    "wreck": ([(105.5, 35.5, PI / 2, 5.0, WRECK)], dict(wreck={(15, iy): 1 for iy in range(3, 8)})),
    # an EMPTY slot lying on top counts nowhere; a negative speed: speed_q clamps to 0, the velocity keeps its sign (-3 x 256)
    "empty on top": ([(100.5, 40.5, 0.0, -3.0, ALIVE), (100.5, 40.5, 0.0, 9.0, EMPTY)],
                     dict(occupancy=_row(8, 12, 10), visits={(10, 10): 1}, vx_q={(10, 10): -768})),
    # 300 m/s clamps to 255 x 256 = 65 280; heading pi: cos = -1, sin(fp32 pi) x 65 280 = -0.006 -> 0
    "above 255": ([(100.5, 40.5, PI, 300.0, ALIVE)],
                  dict(occupancy=_row(8, 12, 10), visits={(10, 10): 1}, speed_q={(10, 10): 65280}, vx_q={(10, 10): -65280})),
}


def expected_maps(case, grid, scale=1):
    """int64 [10][H][W] of a hand case"""
    m = np.zeros((len(fn.LAYERS), grid.H, grid.W), np.int64)
    for layer, cells in HAND_CASES[case][1].items():
        for (ix, iy), v in cells.items():
            m[fn.L[layer], iy, ix] = v * scale
    return m


def hand_state(st0, case):
    """E = 2, N = 5.  Scene 0: the case's bodies in slots 1 and 3; every other slot of both scenes EMPTY with the first body's pose."""
    bodies = HAND_CASES[case][0]
    st = st0.copy()
    assert st.shape[1:] == (2, 5) and len(bodies) <= 2
    for e in range(2):
        for n in range(5):
            ic.put(st, e, n, bodies[0][:4] + (EMPTY,), 50 + n)
    for slot, b in zip((1, 3), bodies):
        ic.put(st, 0, slot, b, 7 + slot)
    return st


# grids of the random poses (interact_cases.random_state: bodies in [60, 140] x [-40, 40] at 64 slots, [60, 90] x [-40, -10] at 7);
# origins off the half-metre lattice of the aligned cases.  40 x 24: neither side a multiple of the 32-cell tile; 33 x 65: tile
# borders crossed in both directions
RANDOM_GRIDS = {
    64: (dict(x0=88.37, y0=-8.63, W=40, H=24, cell=1.0), dict(x0=93.37, y0=-28.13, W=33, H=65, cell=1.0)),
    7: (dict(x0=43.37, y0=-27.63, W=40, H=24, cell=1.0), dict(x0=60.87, y0=-41.13, W=33, H=65, cell=0.5)),
}
RANDOM_GROUPS = (0, 2, -1, 1, 3)        # E = 5, G = 3: scene 2 is switched off, scene 4 names a group that does not exist

# ---- rollout: Intersection, 6 scenes x 30 slots, 120 steps of the reference's CoPO population; an agent ends after 55 steps of driving at
# the latest, wrecks stay 3 steps, so slots are reused and every scene is reset inside the run ----
ROLLOUT_STEPS = 120
ROLLOUT_GROUPS = (0, 1, 2, 0, -1, 1)
TTC_BELOW = 1.5


def rollout_config():
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    mean, std = meta_svo_lookup_table["copo_inter"]
    return SimConfig(map="intersection", num_envs=6, num_agents=30, horizon=55, delay_done=3, start_seed=11, lcf_mean=float(mean), lcf_std=float(std))


def rollout_grids(cfg):
    """The two recorders of the rollout: (grid kwargs, groups, stride): 1 m cells / one group / every record, and 0.5 m cells / three
    groups / every third record; origins 0.37 m off the map's bounding box so that no spawn pose sits on a cell edge."""
    from copo_amd.fields import grid_for_map
    out = []
    for cell, groups, stride in ((1.0, 1, 1), (0.5, 3, 3)):
        x0, y0, W, H = grid_for_map(cfg.tables(), cell=cell, margin=5.0)
        out.append((dict(x0=x0 - 0.37, y0=y0 - 0.37, W=W + 1, H=H + 1, cell=cell), groups, stride))
    return out
