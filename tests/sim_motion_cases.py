"""Crafted scenes for the float64 motion model (sim_motion_numpy.py), shared by test_sim_motion_cpu.py and test_gpu_sim_motion.py.

Every case is set with `set_state` on a freshly reset simulator and then stepped with crafted actions; the model is stepped next to it from
the same crafted words, carrying its own float64 state, and the two are compared after every step (`check_motion`), or -- the lifecycle
case, where everything stands still -- the model predicts the integer side of every step from the simulator's state before it
(`check_lifecycle`).  The crafted words do not depend on what the reset drew, so a case's model is evaluated once and shared.

A simulator enters through a small adapter: reset(), get_state() -> (st, env) numpy, set_state(st, env), step(actions numpy) -> dict of numpy
copies (obs, flags, info, rew), set_capacity(c), close().
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from copo_amd import sim as _sim
from copo_amd.sim import SimConfig

import sim_motion_numpy as motion
import sim_truth_cases as tc
import sim_truth_numpy as truth

W, HL, HW = tc.W, tc.HL, tc.HW
HORIZON = 500
BRAKE = (0.0, -1.0)


@dataclass
class MV(tc.V):
    """A crafted vehicle that moves: speed, the action of the step BEFORE the first (state words 4, 5), age, booth wait counter, wreck
    timer, LCF, its actions (one pair for every step, or a list per step; full brake after the list ends) and the number of steps it is
    compared for (None: every step of the case)."""
    v: float = 0.0
    prev: tuple = (0.0, 0.0)
    age: int = 0
    wait: int = 0
    timer: int = 10
    lcf: float = 0.0
    actions: object = BRAKE
    steps: int = None

    def action(self, t):
        if isinstance(self.actions, tuple):
            return self.actions
        return self.actions[t] if t < len(self.actions) else BRAKE


@dataclass
class MotionCase(tc.Case):
    steps: int = 1
    clocks: list = None                 # env clock per scene (None: `horizon`, no respawn)
    # (`scenes`: per scene a list of MV or None -- an empty slot --, in slot order)

    def state(self, st, env):
        """The crafted state on the arrays of a freshly reset simulator: everything is overwritten but the id and spawn-count words."""
        st, env = tc.Case(self.name, self.cfg, [[] for _ in self.scenes]).state(st, env)          # every slot empty, the clock at `horizon`
        iw = st.view(np.int32)
        t = self.cfg.tables()
        st[3:12] = 0.0
        for e, scene in enumerate(self.scenes):
            assert len(scene) <= st.shape[2]
            for n, v in enumerate(scene):
                if v is None:
                    continue
                st[0, e, n], st[1, e, n], st[2, e, n], st[3, e, n] = v.x, v.y, v.th, v.v
                st[4, e, n], st[5, e, n] = v.prev
                rec = t.route_segs[v.route, v.road]
                st[9, e, n] = float(rec[6]) + truth.project(rec, float(np.float32(v.x)), float(np.float32(v.y)), float(np.float32(v.th)))[0]
                st[10, e, n] = v.lcf
                iw[12, e, n] = v.route | (v.road << 16)
                iw[13, e, n] = (truth.WRECK | (v.timer << 8)) if v.wreck else (truth.ALIVE | (v.age << 16))
                iw[15, e, n] = (iw[15, e, n] & 0xFFFF) | (v.wait << 16)
        if self.clocks is not None:
            env[:, 0] = self.clocks
        return st, env

    def actions(self, t):
        a = np.zeros((self.cfg.num_envs, self.cfg.num_agents, 2), np.float32)
        a[..., 1] = -1.0
        for e, scene in enumerate(self.scenes):
            for n, v in enumerate(scene):
                if v is not None:
                    a[e, n] = v.action(t)
        return a

    def compared(self, t):
        """[E][N]: the slots whose vehicle is compared in step t."""
        m = np.zeros((self.cfg.num_envs, self.cfg.num_agents), bool)
        for e, scene in enumerate(self.scenes):
            for n, v in enumerate(scene):
                m[e, n] = v is not None and not v.wreck and (v.steps is None or t < v.steps)
        return m


def mv(t, route, road, s, lane=0, lat=0.0, psi=0.0, **kw):
    """MV `s` metres along road `road` of `route` in lane `lane`, `lat` metres left of that lane's centre, turned `psi` from the lane."""
    b = tc.on_road(t, route, road, s, -lane * W + lat, psi)
    return MV(b.x, b.y, b.th, route, road, **kw)


def _cfg(map_name, E, N, **kw):
    return SimConfig(map=map_name, num_envs=E, num_agents=N, num_lasers=12, horizon=HORIZON, nbr_k=4, **kw)


def entry_lanes(t):
    """[(route, 0, lane)] of the eight entry lanes of the Intersection, arm by arm (arm 0 heads east, 1 north, 2 west, 3 south)."""
    return [(int(r[0]), 0, int(r[2])) for r in np.asarray(t.spawn_tab) if r[3] == 1]


def arc_route(t, arm, left):
    """(route, 1) of the left / right turn that leaves arm `arm`."""
    first, count = t.entries[arm]
    for r in range(first, first + count):
        g = t.route_segs[r, 1]
        if (g[5] > 0) == left and g[5] != 0 and g[12] > 6.0:
            return r, 1
    raise AssertionError("no such turn")


def final_road(t, arm_from, pick):
    """(route, index of its last road, length of that road) of the `pick`-th route of arm `arm_from`."""
    r = t.entries[arm_from][0] + pick
    k = int(t.route_meta[r, 1]) - 1
    return r, k, float(t.route_segs[r, k, 4])


def _pad(scene, N, keeper):
    assert len(scene) <= N - 1, len(scene)
    return list(scene) + [None] * (N - 1 - len(scene)) + [keeper]


# ---------------------------------------------------------------------------------------------------------------------------------
def case_motion_straight():
    cfg = _cfg("intersection", 1, 12)
    t = cfg.tables()
    L = entry_lanes(t)
    s0 = lambda k: 30.0 if k in (4, 5) else 15.0          # (arm 2 starts at x = 154 m: its vehicles begin where x < 128 m)
    at = lambda k, **kw: mv(t, L[k][0], 0, s0(k), L[k][2], **kw)
    changing = [(0.2 * math.sin(1.3 * k + 0.4), 0.5 * math.cos(0.9 * k)) for k in range(10)]
    r_out, k_out, _ = final_road(t, 1, 0)
    sc = [at(0, v=0.0, actions=(0.0, 1.0), tag=("full throttle",)),
          at(1, v=22.0, actions=(0.0, 0.3), tag=("engine cut",)),
          at(2, v=20.0, actions=(0.0, -1.0), prev=(0.3, -0.4), tag=("full brake",)),
          at(3, v=15.0, actions=(0.0, -0.2), tag=("brake linear",)),
          at(4, v=15.0, actions=(0.0, -0.5), tag=("brake friction",)),
          at(5, v=10.0, actions=(float("nan"), float("nan")), prev=(-0.7, 0.6), tag=("nan",)),
          at(7, v=5.0, actions=(3.0, -7.0), tag=("clip",)),
          at(6, v=8.0, actions=changing, prev=(0.25, -0.5), lcf=-0.35, tag=("changing",)),
          mv(t, r_out, k_out, 20.0, 0, v=5.0, actions=[(-3.0, 7.0), (-3.0, 7.0)], lcf=0.8, tag=("clip throttle",)),
          # (8.8 m/s^2 take 20 m/s to 11.2 m/s in ten steps: the clamp at 0, and two steps beyond it, are reached from 7 m/s)
          mv(t, r_out, k_out, 8.0, 1, v=7.0, actions=(0.0, -1.0), tag=("brake to a stop",))]
    keeper = mv(t, r_out, k_out, 35.0, 1)
    return MotionCase("motion-straight", cfg, [_pad(sc, 12, keeper)], lidar=False, keeper=11, steps=10)


def case_motion_turn():
    cfg = _cfg("intersection", 1, 8)
    t = cfg.tables()
    L = entry_lanes(t)
    at = lambda k, s, **kw: mv(t, L[k][0], 0, s, L[k][2], **kw)
    west = next((r, k) for r in range(t.n_routes) for k in [int(t.route_meta[r, 1]) - 1] if t.route_segs[r, k, 2] < -0.99)      # the exit that heads west
    a, b = mv(t, west[0], west[1], 12.0, 1, v=8.0, actions=(0.1, 0.0)), mv(t, west[0], west[1], 34.0, 0, v=8.0, actions=(-0.1, 0.0))
    a.th, b.th = math.pi - 0.02, -math.pi + 0.02
    a.tag, b.tag = ("wrap left",), ("wrap right",)
    sc = [at(3, 15.0, v=2.0, actions=(1.0, 0.0)), at(2, 38.0, v=2.0, actions=(-1.0, 0.0)),
          at(7, 15.0, v=8.0, actions=(0.3, 0.0)), at(6, 35.0, v=15.0, actions=(-0.2, 0.0), tag=("leaves",)), a, b]
    return MotionCase("motion-turn", cfg, [_pad(sc, 8, at(4, 40.0))], lidar=False, keeper=7, steps=10)


TURN_STEERS, TURN_SPEEDS = (1.0, -1.0, 0.5, -0.5, 0.05, -0.05), (2.0, 8.0, 15.0)


def case_motion_turn_breadth():
    cfg = _cfg("intersection", 2, 11)
    t = cfg.tables()
    L = entry_lanes(t)
    r_out, k_out, _ = final_road(t, 1, 0)
    combos = [(a, v) for v in TURN_SPEEDS for a in TURN_STEERS]
    scenes = []
    for e in range(2):
        sc = []
        for q, (a0, v) in enumerate(combos[9 * e:9 * e + 9]):
            if q < 8:
                sc.append(mv(t, L[q][0], 0, 30.0 if q in (4, 5) else 20.0, L[q][2], v=v, actions=(a0, 0.0), tag=(a0, v)))
            else:
                sc.append(mv(t, r_out, k_out, 20.0, 0, v=v, actions=(a0, 0.0), tag=(a0, v)))
        scenes.append(_pad(sc, 11, mv(t, r_out, k_out, 36.0, 1)))
    return MotionCase("motion-turn-breadth", cfg, scenes, lidar=False, keeper=10, steps=1)


REWARD_SPEEDS = (5.0, 10.0, 20.0)


def case_reward_roads():
    cfg = _cfg("intersection", 4, 16)
    t = cfg.tables()
    L = entry_lanes(t)
    keeper = mv(t, L[5][0], 0, 40.0, 1)
    scenes = []
    for v in REWARD_SPEEDS:
        sc = [mv(t, L[0][0], 0, 20.0, 0, v=v, actions=(0.0, 0.0), tag=("straight", 0)), mv(t, L[0][0], 0, 32.0, 1, v=v, actions=(0.0, 0.0), tag=("straight", 1))]
        for arm, left, lane in ((1, True, 0), (3, True, 1), (0, False, 0), (2, False, 1)):
            r, k = arc_route(t, arm, left)
            kap0 = float(t.route_segs[r, k, 5])
            kap = kap0 / (1.0 + kap0 * lane * W)                          # curvature of the lane's own line, `lane` lanes to the right
            a0, beta = motion.steer_for_curvature(cfg, kap)
            sc.append(mv(t, r, k, 3.0, lane, psi=-beta, v=v, actions=(a0, 0.0), tag=("left" if left else "right", lane)))
        scenes.append(_pad(sc, 16, keeper))
    # scene 3: road advance, the arrival window, the priorities, max_step
    r_left, _ = arc_route(t, 0, True)
    len0 = float(t.route_segs[r_left, 0, 4])
    sc = [mv(t, r_left, 0, len0 - 0.5, 0, v=10.0, actions=(0.0, 0.0), tag=("advance",))]
    go = dict(v=5.0, actions=(0.0, 0.0))                                  # 0.5 m per step
    rx, kx, lx = final_road(t, 1, 0)      # three different final roads: the exits that head west, south and north (all of them within 128 m)
    ry, ky, ly = final_road(t, 0, 1)
    rz, kz, lz = final_road(t, 0, 3)
    sc += [mv(t, rx, kx, lx - 5.0 + 0.05 - 0.5, 0, tag=("window", "near inside"), **go), mv(t, rx, kx, lx + 5.0 - 0.05 - 0.5, 1, tag=("window", "far inside"), **go),
           mv(t, ry, ky, ly - 5.0 - 0.05 - 0.5, 0, tag=("window", "near outside"), **go), mv(t, ry, ky, ly + 5.0 + 0.05 - 0.5, 1, tag=("window", "far outside"), **go),
           mv(t, rz, kz, lz - 2.0 - 0.5, 0, tag=("arrive pair", "arrives"), **go), mv(t, rz, kz, lz - 6.0 - 0.5, 0, tag=("arrive pair", "crashes"), **go),
           mv(t, L[2][0], 0, 25.0, 0, lat=1.5, tag=("out pair", "out"), **go), mv(t, L[2][0], 0, 25.0, 0, tag=("out pair", "on road"), **go),
           mv(t, L[6][0], 0, 25.0, 0, age=HORIZON - 1, tag=("max step",), **go)]
    scenes.append(_pad(sc, 16, keeper))
    return MotionCase("reward-roads", cfg, scenes, lidar=False, keeper=15, steps=1)


TOLL_WAITS = (0, 29, 30, 31)


def case_tollgate_booth():
    cfg = _cfg("tollgate", 1, 8, **{k: v for k, v in _sim.TOLLGATE_METADRIVE_RULES.items()})
    t = cfg.tables()
    b0, b1 = int(t.route_meta[0, 2]), int(t.route_meta[1, 2])
    end1 = float(t.route_segs[1, b1, 4])
    sc = [mv(t, 0, b0, 3.0, 2 * q, v=(0.5, 2.0)[q % 2], wait=wait, actions=(0.0, 0.0), tag=("booth", wait)) for q, wait in enumerate(TOLL_WAITS)]
    sc += [mv(t, 1, b1, end1 - 0.5, 0, v=8.0, wait=5, actions=(0.0, 0.0), tag=("exit", "early")),
           mv(t, 1, b1, end1 - 0.5, 2, v=8.0, wait=31, actions=(0.0, 0.0), tag=("exit", "legal"))]
    k = tc.spawn_vehicle(t, 0)
    return MotionCase("tollgate-booth", cfg, [_pad(sc, 8, MV(k.x, k.y, k.th, k.route, k.road))], lidar=False, keeper=7, steps=3)


def _beside_region(t, place, gap, psi):
    """A vehicle ahead of respawn place `place` (row of the spawn table), turned by `psi`, whose box is `gap` metres from the place's 8 x 3 m
    region (negative: inside it) -- found by bisection on the model's own box distance."""
    first, _, lane, _ = (int(v) for v in t.spawn_tab[place])
    p = [q for q in motion.respawn_places(t) if q[0] == place][0]
    region = ((p[1], p[2]), p[3], 4.0, 1.5)
    lo, hi = float(t.spawn_s[place]), float(t.spawn_s[place]) + 12.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        v = mv(t, first, 0, mid, lane, psi=psi)
        lo, hi = (mid, hi) if truth.box_gap(region, ((v.x, v.y), v.th, HL, HW)) < gap else (lo, mid)
    return mv(t, first, 0, 0.5 * (lo + hi), lane, psi=psi)


LIFE_BLOCKED, LIFE_NEAR = (0, 3), (4, 7)          # respawn places (in table order) with a vehicle 0.5 m inside / outside the region


def case_lifecycle():
    cfg = _cfg("intersection", 4, 8)
    t = cfg.tables()
    L = entry_lanes(t)
    places = [q[0] for q in motion.respawn_places(t)]
    crowd = [None] * 4 + [_beside_region(t, places[LIFE_BLOCKED[0]], -0.5, 0.0), _beside_region(t, places[LIFE_BLOCKED[1]], -0.5, 0.3),
                          _beside_region(t, places[LIFE_NEAR[0]], 0.5, 0.0), _beside_region(t, places[LIFE_NEAR[1]], 0.5, -0.3)]
    wrecks = [mv(t, L[0][0], 0, 30.0, 0, tag=("living",)), mv(t, L[0][0], 0, 30.0, 1, wreck=True, timer=1), mv(t, L[0][0], 0, 36.0, 0, wreck=True, timer=2),
              mv(t, L[0][0], 0, 24.0, 0, wreck=True, timer=25), mv(t, L[2][0], 0, 30.0, 0, tag=("crashes",)), mv(t, L[2][0], 0, 33.0, 0, wreck=True, timer=2), None, None]
    r, k, ln = final_road(t, 1, 0)
    single = [mv(t, r, k, ln - 2.0, 0, tag=("arrives",))] + [None] * 7
    return MotionCase("lifecycle", cfg, [crowd, list(crowd), wrecks, single], lidar=False, keeper=None, steps=30, clocks=[0, HORIZON, HORIZON, HORIZON])


CASES = {
    "motion-straight": case_motion_straight,
    "motion-turn": case_motion_turn,
    "motion-turn-breadth": case_motion_turn_breadth,
    "reward-roads": case_reward_roads,
    "tollgate-booth": case_tollgate_booth,
}
LIFECYCLE = "lifecycle"


@lru_cache(maxsize=None)
def get_case(name):
    return case_lifecycle() if name == LIFECYCLE else CASES[name]()


def crafted_state(name):
    """The crafted words of case `name` on an all-zero template: what the model needs, without any simulator."""
    cfg = get_case(name).cfg
    return get_case(name).state(np.zeros((16, cfg.num_envs, cfg.num_agents), np.float32), np.zeros((cfg.num_envs, 4), np.int32))


@lru_cache(maxsize=None)
def motion_truth(name):
    """The model's answers for every step of case `name`, evaluated once: (crafted words, [T of step 0, T of step 1, ...])."""
    case = get_case(name)
    st, _ = crafted_state(name)
    t = case.cfg.tables()
    out, state = [], st
    for k in range(case.steps):
        T = motion.step_truth_moving(case.cfg, t, state, case.actions(k))
        out.append(T)
        state = T["next"]
    return st, out


# ---------------------------------------------------------------------------------------------------------------------------------
# running a simulator through a case
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL_WORDS = list(range(0, 14))          # (14 = id, 15 low half = spawn count: the reset's)


def drive(case, sim, capacity=None):
    """One reset, one set_state, `case.steps` steps.  Returns (crafted words, env words, [dict(obs, flags, info, rew, st, env) per step])."""
    sim.reset()
    if capacity is not None:
        sim.set_capacity(capacity)
    st, env = case.state(*sim.get_state())
    sim.set_state(st, env)
    records = []
    for k in range(case.steps):
        out = sim.step(case.actions(k))
        st1, env1 = sim.get_state()
        records.append(dict(obs=out["obs"], flags=out["flags"], info=out["info"], rew=out["rew"], st=np.array(st1), env=np.array(env1)))
    return st, env, records


def _angle_err(a, b):
    return np.abs((np.asarray(a, np.float64) - b + math.pi) % (2.0 * math.pi) - math.pi)


def check_motion(case, st, records):
    """Hold every step of a simulator's run of `case` to the model.  Returns the measured maxima and the counts of compared / skipped rows."""
    cfg, name = case.cfg, case.name
    st0, truths = motion_truth(name)
    assert np.array_equal(st0[MODEL_WORDS].view(np.uint32), np.asarray(st, np.float32)[MODEL_WORDS].view(np.uint32)), "the crafted words differ"
    assert np.array_equal(st0.view(np.uint32)[15] >> 16, np.asarray(st, np.float32).view(np.uint32)[15] >> 16)
    oc = truth.obs_columns(cfg)
    c_state, c_lane = oc["heading"], oc["lane"]
    c_navi = c_lane + (int(cfg.lane_line_lasers) or 1)
    c_toll = c_navi + int(cfg.navi_dim) + int(cfg.num_lasers)
    stats = dict(rows=0, skipped=0)

    def worst(key, err, bound, tag):
        m = float(np.max(err)) if np.size(err) else 0.0
        stats[key] = max(stats.get(key, 0.0), m)
        assert m <= bound, "%s step %d: %s is %.3g from the model (bound %g)" % (name, tag, key, m, bound)

    E, N = cfg.num_envs, cfg.num_agents
    valid = np.ones((E, N), bool)                      # the slot's decisions were all beyond the band so far
    for k, (T, R) in enumerate(zip(truths, records)):
        flags, info, obs = R["flags"].astype(int), R["info"].astype(np.float64), R["obs"]
        assert not (flags & motion.F_ENV_RESET).any() and not (flags & motion.F_SPAWNED).any(), "%s: the scene must outlast the run" % name
        rows = T["acted"] & case.compared(k)
        stats["skipped"] += int((rows & ~(valid & T["sure"])).sum())
        valid &= T["sure"] | ~T["acted"]
        rows &= valid
        stats["rows"] += int(rows.sum())
        if case.keeper is not None:
            assert T["acted"][:, case.keeper].all() and not (flags[:, case.keeper] & motion.F_DONE).any(), "%s: the keeper must come through" % name
        assert ((flags & motion.F_ACTED) != 0)[rows].all()
        S = motion.unpack(R["st"])
        # decisions: every flag, the status words, the road, the wait counter
        assert np.array_equal(flags[rows], T["flags"][rows]), "%s step %d: flags %s, model %s" % (name, k, flags[rows], T["flags"][rows])
        for key in ("status", "timer", "age", "wait", "road"):
            assert np.array_equal(S[key][rows], T[key][rows]), "%s step %d: %s %s, model %s" % (name, k, key, S[key][rows], T[key][rows])
        # the pose and the speed
        assert (np.abs(T["x"][rows]) < motion.COORD_MAX).all() and (np.abs(T["y"][rows]) < motion.COORD_MAX).all(), "%s: a coordinate beyond 128 m" % name
        worst("position_m", np.hypot(S["x"] - T["x"], S["y"] - T["y"])[rows], motion.POS_TOL, k)
        worst("heading_rad", _angle_err(S["th"], T["th"])[rows], motion.HEADING_TOL, k)
        worst("speed_mps", np.abs(S["v"] - T["v"])[rows], motion.SPEED_TOL, k)
        worst("progress_m", np.abs(S["prog"] - T["prog"])[rows], motion.POS_TOL, k)
        # reward and info row
        worst("reward", np.abs(R["rew"].astype(np.float64) - T["reward"])[rows], motion.REWARD_TOL, k)
        with np.errstate(invalid="ignore"):
            terminal = rows & (((T["flags"] & (motion.F_ARRIVE | motion.F_CRASH)) != 0) | (T["out_margin"] < 0))
        assert np.array_equal(R["rew"][terminal].astype(np.float64), T["reward"][terminal]), "%s: a terminal reward" % name
        assert np.array_equal(R["rew"][rows], R["info"][..., 3][rows])
        worst("info_kmh", np.abs(info[..., 0] - T["info"][..., 0])[rows], 3.6 * motion.SPEED_TOL, k)
        worst("info_steering", np.abs(info[..., 1] - T["info"][..., 1])[rows], 1e-7, k)
        worst("info_acceleration", np.abs(info[..., 2] - T["info"][..., 2])[rows], motion.ACC_TOL, k)
        assert np.array_equal(info[..., 4][rows], T["info"][..., 4][rows]), "%s step %d: cost" % (name, k)
        assert np.array_equal(info[..., 5][rows], T["info"][..., 5][rows]), "%s step %d: episode length" % (name, k)
        worst("info_episode_reward", np.abs(info[..., 6] - T["info"][..., 6])[rows], (k + 1) * motion.REWARD_TOL, k)
        worst("info_completion_m", (np.abs(info[..., 7] - T["info"][..., 7]) * T["total"])[rows], motion.POS_TOL, k)
        # observation columns
        C = T["cols"]
        q = obs[..., c_state:c_state + 6].astype(np.float64)
        worst("col_speed", np.abs(q[..., 1] - C["speed"])[rows], motion.COL_TOL, k)
        worst("col_steering", np.abs(q[..., 2] - C["steering"])[rows], motion.COL_TOL, k)
        worst("col_last_action", np.abs(q[..., 3:5] - C["last_action"])[rows], motion.COL_TOL, k)
        worst("col_yaw", np.abs(q[..., 5] - C["yaw"])[rows], motion.YAW_COL_TOL, k)
        worst("col_heading", np.abs(q[..., 0] - C["heading"])[rows], motion.COL_TOL, k)
        if not cfg.side_lasers:
            worst("col_side", np.abs(obs[..., 0:2].astype(np.float64) - C["side"])[rows], motion.COL_TOL, k)
        if not cfg.lane_line_lasers:
            worst("col_lane", np.abs(obs[..., c_lane].astype(np.float64) - C["lane"])[rows], motion.COL_TOL, k)
        if cfg.navi_dim:
            nv = obs[..., c_navi:c_navi + 10]
            worst("col_navi", np.abs(nv.astype(np.float64) - C["navi"])[rows], motion.COL_TOL, k)
            assert np.array_equal(nv[..., [2, 4, 7, 9]][rows].view(np.uint32), C["navi_const"][rows].view(np.uint32)), "%s: radius / angle columns are the records' fields" % name
            assert np.array_equal(nv[..., [3, 8]][rows].astype(np.float64), C["navi"][..., [3, 8]][rows]), "%s: direction columns" % name
        if cfg.toll_dim:
            assert np.array_equal(obs[..., c_toll:c_toll + 2][rows].astype(np.float64), C["toll"][rows]), "%s step %d: toll columns %s, model %s" % (
                name, k, obs[..., c_toll:c_toll + 2][rows], C["toll"][rows])
        worst("col_lcf", np.abs(obs[..., cfg.lcf_col].astype(np.float64) - C["lcf"])[rows], motion.COL_TOL, k)
        assert np.array_equal(obs[..., cfg.lcf_col][rows].view(np.uint32), C["lcf"][rows].astype(np.float32).view(np.uint32)), "%s: LCF column" % name
    return stats


_LIFE = {}


def _lifecycle_model(case, st, env, capacity):
    key = (case.name, capacity, st.tobytes(), env.tobytes())
    if key not in _LIFE:
        _LIFE[key] = motion.lifecycle_truth(case.cfg, case.cfg.tables(), st, env, capacity)
    return _LIFE[key]


def check_lifecycle(case, st, env, records, capacity=None):
    """Hold the integer side of every step of the lifecycle case to the model: status, timer, age and clock words exactly, the number of
    spawns, every spawned pose the pose of an eligible place, no place twice.  Returns counts."""
    cfg, t = case.cfg, case.cfg.tables()
    E, N = cfg.num_envs, cfg.num_agents
    stats = dict(spawns=np.zeros(E, int), resets=np.zeros(E, int), skipped=0, decisions=0, max_slot=np.full(E, -1), place_err_m=0.0)
    places = {q[0]: q[1:] for q in motion.respawn_places(t)}
    everywhere = motion.spawn_slot_poses(t)
    trace = []
    for k, R in enumerate(records):
        M = _lifecycle_model(case, np.asarray(st, np.float32), np.asarray(env, np.int32), capacity)
        S0, S1 = motion.unpack(st), motion.unpack(R["st"])
        flags = R["flags"].astype(int)
        for e in range(E):
            m = M[e]
            acted = S0["status"][e] == motion.ALIVE
            stats["decisions"] += int(acted.sum())
            if not (m["done_margin"][acted] > motion.DECISION_BAND).all():
                stats["skipped"] += 1
                continue
            tag = "%s step %d scene %d" % (case.name, k, e)
            assert bool((flags[e] & motion.F_ENV_RESET).any()) == m["reset"] and R["env"][e, 0] == m["clock"], tag
            if m["reset"]:
                cap = m["capacity"]
                assert (S1["status"][e, :cap] == motion.ALIVE).all() and (S1["status"][e, cap:] == motion.EMPTY).all() and (S1["age"][e] == 0).all(), tag
                d = np.hypot(S1["x"][e, :cap, None] - everywhere[None, :, 0], S1["y"][e, :cap, None] - everywhere[None, :, 1])
                assert (d.min(1) < 1e-3).all() and len(set(d.argmin(1).tolist())) == cap, tag + ": a reset populates distinct spawn slots"
                stats["resets"][e] += 1
                stats["max_slot"][e] = max(stats["max_slot"][e], cap - 1)
                continue
            spawned = np.zeros(N, bool)
            spawned[m["spawn_slots"]] = True
            assert np.array_equal((flags[e] & motion.F_SPAWNED) != 0, spawned), "%s: spawned %s, model %s" % (tag, np.nonzero(flags[e] & motion.F_SPAWNED)[0], m["spawn_slots"])
            for key in ("status", "timer", "age"):
                assert np.array_equal(S1[key][e][~spawned], m[key][~spawned]), "%s: %s %s, model %s" % (tag, key, S1[key][e], m[key])
            used = []
            for n in m["spawn_slots"]:
                assert S1["status"][e, n] == motion.ALIVE and S1["age"][e, n] == 0 and S1["v"][e, n] == 0.0, tag
                d = {p: math.hypot(S1["x"][e, n] - places[p][0], S1["y"][e, n] - places[p][1]) for p in m["eligible"]}
                p = min(d, key=d.get)
                assert d[p] < 1e-3 and _angle_err(S1["th"][e, n], places[p][2]) < 1e-5, tag + ": a spawn away from every eligible place"
                stats["place_err_m"] = max(stats["place_err_m"], d[p])
                used.append(p)
                stats["max_slot"][e] = max(stats["max_slot"][e], n)
            assert len(set(used)) == len(used), tag + ": a place used twice"
            stats["spawns"][e] += len(used)
        trace.append(S1["status"].copy())
        st, env = R["st"], R["env"]
    stats["status_trace"] = np.array(trace)          # [steps][E][N] status after every step
    return stats
