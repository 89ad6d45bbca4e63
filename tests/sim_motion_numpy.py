"""Float64 model of what MOVES and what PASSES in one simulator step: the kinematic bicycle, progress and reward, the terminal rules and
their priority, the info row, the motion-dependent observation columns, the Tollgate's booth rules and the slot lifecycle.  Written from
SPEC.md sections 3.1, 3.2b, 3.4 and from copo_amd/maps.py.  Test infrastructure only.

sim_truth_numpy.py is the model of a scene that stands still; this file adds time.  It shares no expression with the simulator: the
heading is an ANGLE that is advanced sub-step by sub-step and whose sine and cosine are taken afresh (math.sin / math.cos) every time, the
slip angle is math.atan(math.tan(delta) / 2), nothing is fused, nothing is a polynomial.  The geometry of the pose after the move is
sim_truth_numpy's (`project`, `road_decisions`, `box_gap`).

Tolerances (fp32 error budget of the simulator against this model; coordinates below 128 m, asserted by the tests: one ulp of a coordinate
is then <= 7.6e-6 m and a rounding to nearest <= 3.8e-6 m):

  position, per 10 steps = 50 sub-steps
    * each position update is one fused multiply-add rounded to the coordinate's grid: <= 3.8e-6 m, 50 of them <= 1.9e-4 m;
    * heading: one angle update rounds by <= 1.2e-7 rad (half an ulp below pi) -- 50 of them 6e-6 rad --, the yaw constant `tan(delta)
      cos(beta) / L` carries <= 2e-7 relative, which over at most 7 rad of turn is 1.4e-6 rad: together <= 8e-6 rad; a heading error
      of 8e-6 rad over at most 22 m of path (22.2 m/s x 1 s) displaces by <= 1.8e-4 m;
    * speed: one update rounds by <= 1e-6 m/s (half an ulp below 32 m/s); an error that grows to 5e-5 m/s over the second displaces by
      <= 5e-5 m;
    * the 3-term sine of the sub-step's angle |dth| <= 0.14 rad (22.2 m/s x 0.02 s x 0.32 / m) truncates at dth^7 / 5040 < 2e-10.
    Sum <= 4.2e-4 m, budget 5e-4 m.
  bounds asserted (twice the budget where the budget is the argument):
    position 1e-3 m (sim_truth_cases.DISTANCE_TOL), heading 2e-5 rad, speed 1e-4 m/s, yaw-rate column 2e-4 (two headings / 0.1 s... the
    column is |d theta| / 0.1 s clipped to 1: 2 x 8e-6 / 0.1 = 1.6e-4), state and navigation columns 1e-4 (lane offset: 4.2e-4 m / 4.5
    m = 9.3e-5; side pair: / 10.5 m; a check point: 0.01 x (1e-3 m + 50 m x 2e-5 rad) = 2e-5; speed: 3.6 x 1e-4 / 81), plus BIT equality
    for the columns that are constants (the navigation features against the road record's fields, direction and LCF against the model).
    step reward 2.5e-3: the progress difference of two poses, each within 1e-3 m, times the largest lane factor 1 + 3.5 / 13.5 = 1.26.
    acceleration of the info row = (v - v0) / 0.1 s: 2 x 1e-4 / 0.1 = 2e-3; km/h: 3.6 x 1e-4; episode reward: steps x 2.5e-3; route
    completion: 1e-3 m / route length.

Every decision comes with a signed margin in metres (m/s for the speed limit); the tests compare a decision where its margin is further
than 1 mm from zero, and the crafted cases keep every margin beyond 9 mm.
"""
import math

import numpy as np

import sim_truth_numpy as truth

EMPTY, ALIVE, WRECK = 0, truth.ALIVE, truth.WRECK
F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = 1, 2, 4, 8, 16, 32, 64, 128
NAVI_RADIUS_NORM, NAVI_ANGLE_NORM, NAVI_CLIP = 60.0, 135.0, 50.0

POS_TOL, HEADING_TOL, SPEED_TOL, YAW_COL_TOL, COL_TOL, REWARD_TOL, ACC_TOL = 1e-3, 2e-5, 1e-4, 2e-4, 1e-4, 2.5e-3, 2e-3
COORD_MAX = 128.0
DECISION_BAND, CRAFTED_MARGIN = 1e-3, 0.009


def _wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi


def clean_action(a):
    """NaN -> 0, then clipped to +-1 (SPEC 3.4 (1))."""
    a = float(a)
    if a != a:
        a = 0.0
    return min(max(a, -1.0), 1.0)


def yaw_constant(cfg, a0):
    """(tan(delta) cos(beta) / L, beta): the heading turns by v x dt x this; beta = slip angle of the body centre."""
    delta = clean_action(a0) * float(cfg.max_steer)
    beta = math.atan(math.tan(delta) / 2.0)
    return math.tan(delta) * math.cos(beta) / float(cfg.wheelbase), beta


def steer_for_curvature(cfg, kappa):
    """(steering action, slip angle) with which the body centre follows a circle of curvature `kappa`: tan(delta) cos(beta) / L = 2 sin(beta) / L."""
    beta = math.asin(0.5 * kappa * float(cfg.wheelbase))
    return math.atan(2.0 * math.tan(beta)) / float(cfg.max_steer), beta


def bicycle_step(cfg, x, y, th, v, a0, a1):
    """One step of the kinematic bicycle referenced to the body centre (SPEC 3.1): `substeps` sub-steps of dt / substeps, each in the order
    speed, position along th + beta, heading.  Returns x, y, th (wrapped to [-pi, pi)), v, yaw rate (turned angle / dt, not wrapped),
    acceleration ((v - v0) / dt)."""
    a0, a1 = clean_action(a0), clean_action(a1)
    yawk, beta = yaw_constant(cfg, a0)
    n = int(cfg.substeps)
    h = float(cfg.dt) / n
    v0, turned = v, 0.0
    for _ in range(n):
        if a1 >= 0.0:
            acc = float(cfg.acc_max) * a1 if v < float(cfg.max_speed) else 0.0
        else:
            acc = -min(float(cfg.brake_gain) * abs(a1), float(cfg.brake_max))
        v = max(v + acc * h, 0.0)                                    # no reverse gear
        x += v * math.cos(th + beta) * h
        y += v * math.sin(th + beta) * h
        dth = v * yawk * h
        th += dth
        turned += dth
    return x, y, _wrap(th), v, turned / float(cfg.dt), (v - v0) / float(cfg.dt)


def lane_factor(cfg, kappa, lane):
    """Lane `lane` of an arc is this much longer than lane 0, whose line the progress is measured on (lane i lies i w to the RIGHT)."""
    return 1.0 + kappa * lane * float(cfg.lane_width)


def driving_reward(cfg, dprog, kappa, lane, v):
    return float(cfg.driving_reward) * dprog * lane_factor(cfg, kappa, lane) + float(cfg.speed_reward) * abs(v) / float(cfg.max_speed)


def navi_point(x, y, th, px, py):
    """The two navigation columns of check point (px, py) seen from pose (x, y, th): the vector to it, clipped at 50 m, forward and to the
    right, mapped by 0.5 + 0.01 x."""
    vx, vy = px - x, py - y
    n = math.hypot(vx, vy)
    if n > NAVI_CLIP:
        vx, vy = vx * NAVI_CLIP / n, vy * NAVI_CLIP / n
    fwd, right = vx * math.cos(th) + vy * math.sin(th), vx * math.sin(th) - vy * math.cos(th)
    return min(max(0.5 + 0.01 * fwd, 0.0), 1.0), min(max(0.5 + 0.01 * right, 0.0), 1.0)


def road_features(cfg, rec):
    """(radius, direction, angle) columns of a road from its LENGTH and CURVATURE (copo_amd/maps.py: radius over 60 + lanes x w, left = 0 /
    straight = 0.5 / right = 1, (angle / 135 deg + 1) / 2; a straight reports radius 0 and angle 0.5)."""
    length, kappa, lanes = float(rec[4]), float(rec[5]), math.floor(float(rec[10]))
    if kappa == 0.0:
        return 0.0, 0.5, 0.5
    radius = 1.0 / abs(kappa)
    return (min(1.0, radius / (NAVI_RADIUS_NORM + lanes * float(cfg.lane_width))), 0.0 if kappa > 0.0 else 1.0,
            min(1.0, (math.degrees(abs(kappa) * length) / NAVI_ANGLE_NORM + 1.0) / 2.0))


def road_end(rec):
    """End pose of the lane-0 line of a road record, from its start pose, length and curvature."""
    x, y, th, length, kappa = float(rec[0]), float(rec[1]), truth.road_direction(rec), float(rec[4]), float(rec[5])
    if kappa == 0.0:
        return x + length * math.cos(th), y + length * math.sin(th), th
    r = 1.0 / kappa                                                   # signed: the centre lies r to the left
    cx, cy = x - r * math.sin(th), y + r * math.cos(th)
    th1 = th + kappa * length
    return cx + r * math.sin(th1), cy - r * math.cos(th1), th1


def navigation(cfg, tables, route, road, x, y, th):
    """The ten navigation columns and the five that are constants of the road records ([2, 3, 4, 7, 8, 9] -> fields of the records)."""
    w = float(cfg.lane_width)
    nroads = int(tables.route_meta[route, 1])
    lanes_here = math.floor(float(tables.route_segs[route, road, 10]))
    cols, recs = [], []
    for j in range(2):
        k = min(road + j, nroads - 1)
        rec = tables.route_segs[route, k]
        ex, ey, eth = road_end(rec)
        off = (lanes_here / 2.0 - 0.5) * w                            # to the RIGHT of the lane-0 line: the middle of the CURRENT road's lanes
        cols += list(navi_point(x, y, th, ex + off * math.sin(eth), ey - off * math.cos(eth))) + list(road_features(cfg, rec))
        recs.append(rec)
    return np.array(cols), recs


# ---------------------------------------------------------------------------------------------------------------------------------
# the state words
# ---------------------------------------------------------------------------------------------------------------------------------
FLOAT_WORDS = ("x", "y", "th", "v", "steer", "throttle", "psteer", "pthrottle", "yaw", "prog", "lcf", "eprew")


def unpack(st):
    """Raw words [16][E][N] float32 -> dict of float64 / int arrays [E][N]."""
    st = np.ascontiguousarray(st, np.float32)
    iw = st.view(np.int32)
    S = {k: st[i].astype(np.float64) for i, k in enumerate(FLOAT_WORDS)}
    S.update(route=iw[12] & 0xFFFF, road=iw[12] >> 16, status=iw[13] & 0xFF, timer=(iw[13] >> 8) & 0xFF,
             age=(iw[13].view(np.uint32) >> 16).astype(np.int64), wait=(iw[15].view(np.uint32) >> 16).astype(np.int64))
    return {k: np.array(v) for k, v in S.items()}


def _boxes(cfg, tables):
    if not cfg.toll_buildings or tables.boxes is None:
        return []
    return [((float(b[0]), float(b[1])), math.atan2(float(b[3]), float(b[2])), float(b[4]), float(b[5])) for b in np.asarray(tables.boxes, np.float64)]


def _tick(cfg, S):
    """(0) wreck timers tick: a wreck whose timer runs out is an empty slot.  Returns (status, timer) after the tick."""
    status, timer = S["status"].copy(), S["timer"].copy()
    wreck = status == WRECK
    timer[wreck] -= 1
    gone = wreck & (timer <= 0)
    status[gone], timer[gone] = EMPTY, int(cfg.respawn_cooldown)
    cooling = (S["status"] == EMPTY) & (S["timer"] > 0)
    timer[cooling] -= 1
    return status, timer


def _decide(cfg, tables, S, status, e, i, others, buildings):
    """Decisions of the acting slot (e, i) at the pose S holds: dict with margins.  `others`: indices of the solid slots of the scene."""
    hl, hw = float(cfg.veh_half_len), float(cfg.veh_half_wid)
    x, y, th = S["x"][e, i], S["y"][e, i], S["th"][e, i]
    me = ((x, y), th, hl, hw)
    gaps = [truth.box_gap(me, ((S["x"][e, j], S["y"][e, j]), S["th"][e, j], hl, hw)) for j in others if j != i]
    gaps += [truth.box_gap(me, b) for b in buildings]
    route, road0 = int(S["route"][e, i]), int(S["road"][e, i])
    r = truth.road_decisions(cfg, tables, route, road0, x, y, th)
    nroads = int(tables.route_meta[route, 1])
    final = r["road"] == nroads - 1
    window = min(r["long"] - (r["length"] - float(cfg.arrive_margin)), r["length"] + float(cfg.arrive_margin) - r["long"]) if final else -np.inf
    r.update(crash_gap=min(gaps, default=np.inf), road_before=road0, final=final, window=window, route=route)
    return r


def step_truth_moving(cfg, tables, state, actions):
    """One full step for the acting slots.  state: raw words [16][E][N] or the dict `unpack` gives (float64: the model carries its own
    state from step to step); actions [E][N][2].  Returns T: arrays [E][N] --
      acted; x, y, th, v, yaw, acc; road, lane, prog; the margins crash_gap, out_margin, long_margin, lane_margin, window (signed distance
      into the arrival window; -inf off the final road), speed_margin (|v| - limit on the booth road, else nan); sure (every margin that
      enters the outcome is beyond 1 mm) and min_margin; flags, reward, info [E][N][8]; status, timer, age, wait after the step;
      cols: dict of observation columns (speed, steering, last_action [2], yaw, side [2], lane, navi [10], navi_const [5] float32 fields
      of the road records, lcf, toll [2], heading);
    and T["next"], the state dict after the step."""
    S = unpack(state) if not isinstance(state, dict) else {k: v.copy() for k, v in state.items()}
    E, N = S["x"].shape
    actions = np.asarray(actions, np.float64)
    status, timer = _tick(cfg, S)
    acted = S["status"] == ALIVE
    w, vmax, dt = float(cfg.lane_width), float(cfg.max_speed), float(cfg.dt)
    buildings = _boxes(cfg, tables)
    v0 = S["v"].copy()
    acc, yaw = np.zeros((E, N)), np.zeros((E, N))
    for e, i in zip(*np.nonzero(acted)):                              # (1) dynamics
        a0, a1 = clean_action(actions[e, i, 0]), clean_action(actions[e, i, 1])
        S["x"][e, i], S["y"][e, i], S["th"][e, i], S["v"][e, i], yaw[e, i], acc[e, i] = bicycle_step(
            cfg, S["x"][e, i], S["y"][e, i], S["th"][e, i], S["v"][e, i], a0, a1)
        S["psteer"][e, i], S["pthrottle"][e, i] = S["steer"][e, i], S["throttle"][e, i]
        S["steer"][e, i], S["throttle"][e, i], S["yaw"][e, i] = a0, a1, yaw[e, i]
    age = np.where(acted, S["age"] + 1, 0)
    Z = lambda fill=0.0, dtype=np.float64: np.full((E, N), fill, dtype)
    T = dict(acted=acted, crash_gap=Z(np.inf), out_margin=Z(np.nan), long_margin=Z(np.inf), lane_margin=Z(np.inf), window=Z(-np.inf),
             speed_margin=Z(np.nan), exit_early=Z(False, bool), on_booth=Z(False, bool), advanced=Z(0, int), sure=Z(True, bool),
             min_margin=Z(np.inf), road=Z(0, int), lane=Z(0, int), prog=Z(), total=Z(1.0), flags=Z(0, int), reward=Z(), info=np.zeros((E, N, 8)),
             lanes=Z(), lat=Z())
    cols = dict(speed=Z(), steering=Z(), last_action=np.zeros((E, N, 2)), yaw=Z(), side=np.zeros((E, N, 2)), lane=Z(), heading=Z(),
                navi=np.zeros((E, N, 10)), navi_const=np.zeros((E, N, 4), np.float32), lcf=Z(), toll=np.zeros((E, N, 2)))
    new_status, new_timer, new_age = status.copy(), timer.copy(), age.copy()
    for e in range(E):
        solid = np.nonzero(acted[e] | ((status[e] == WRECK) & (timer[e] > 0)))[0]
        for i in np.nonzero(acted[e])[0]:
            r = _decide(cfg, tables, S, status, e, i, solid, buildings)          # (2), (3)
            v = S["v"][e, i]
            booth = int(tables.route_meta[r["route"], 2]) if cfg.toll_dim else -1
            on_booth = booth >= 0 and r["road"] == booth
            wait = int(S["wait"][e, i])
            if on_booth:
                wait = min(wait + 1, 0xFFFF)
            early = bool(cfg.toll_dim) and booth >= 0 and r["road"] > booth >= r["road_before"] and wait < int(cfg.toll_min_steps)
            lane_kappa = float(tables.route_segs[r["route"], r["road"], 5])
            dprog = r["prog"] - S["prog"][e, i]
            speed_share = abs(v) / vmax
            margins = [r["crash_gap"], r["long_margin"]]
            if math.isnan(r["out_margin"]):                           # the straight of a Merge / Split block: wider than the model's road
                margins.append(r["out_margin_narrow"] if r["out_margin_narrow"] > 0.0 else 0.0)
                out = False
            else:
                margins.append(r["out_margin"])
                out = r["out_margin"] < 0.0
            if float(cfg.toll_speed_limit) > 0.0 and on_booth:
                T["speed_margin"][e, i] = abs(v) - float(cfg.toll_speed_limit)
                margins.append(T["speed_margin"][e, i])
                # on the booth road: the driving reward alone up to the limit, the penalty above it
                reward = -float(cfg.overspeed_penalty) * speed_share if T["speed_margin"][e, i] > 0.0 else driving_reward(cfg, dprog, lane_kappa, r["lane"], 0.0)
            else:
                reward = driving_reward(cfg, dprog, lane_kappa, r["lane"], v)
            if lane_kappa != 0.0 or not cfg.lane_line_lasers:
                margins.append(r["lane_margin"])
            crash = r["crash_gap"] < 0.0 or (early and not cfg.toll_early_exit)
            if r["final"]:
                margins.append(r["window"])
            arrive = r["final"] and r["window"] > 0.0 and not out
            flags = F_ACTED
            if arrive:                                                # (4) arrive > out of road > crash
                reward, flags = float(cfg.success_reward), flags | F_ARRIVE
            elif out:
                reward = -float(cfg.out_penalty)
            elif crash:
                reward = -float(cfg.crash_penalty)
            if out or (early and cfg.toll_early_exit):
                flags |= F_OUT
            if crash:
                flags |= F_CRASH
            done = arrive or out or crash or early
            if not done and age[e, i] >= int(cfg.horizon):
                flags, done = flags | F_MAXSTEP, True
            if done:
                flags |= F_DONE
                if arrive or int(cfg.delay_done) <= 0:                # (5) an arrived vehicle leaves at once, the others linger
                    new_status[e, i], new_timer[e, i], new_age[e, i] = EMPTY, int(cfg.respawn_cooldown), 0
                else:
                    new_status[e, i], new_timer[e, i], new_age[e, i] = WRECK, int(cfg.delay_done), 0
            S["prog"][e, i], S["eprew"][e, i], S["road"][e, i], S["wait"][e, i] = r["prog"], S["eprew"][e, i] + reward, r["road"], wait
            total = float(tables.route_meta[r["route"], 0])
            for k in ("crash_gap", "out_margin", "long_margin", "lane_margin", "window", "road", "lane", "prog", "lanes", "lat"):
                T[k][e, i] = r[k]
            T["total"][e, i], T["flags"][e, i], T["reward"][e, i] = total, flags, reward
            T["exit_early"][e, i], T["on_booth"][e, i], T["advanced"][e, i] = early, on_booth, r["road"] - r["road_before"]
            T["min_margin"][e, i] = min(abs(m) for m in margins)
            T["sure"][e, i] = T["min_margin"][e, i] > DECISION_BAND
            T["info"][e, i] = [abs(v) * 3.6, S["steer"][e, i], acc[e, i], reward, 1.0 if crash else 0.0, age[e, i], S["eprew"][e, i],
                               min(max(r["prog"] / total, 0.0), 1.0)]
            # (9) observation of the slot's occupant
            cols["heading"][e, i] = 0.5 - 0.5 * math.sin(r["psi"])
            cols["speed"][e, i] = min(max((abs(v) * 3.6 + 1.0) / (vmax * 3.6 + 1.0), 0.0), 1.0)
            cols["steering"][e, i] = (S["steer"][e, i] / 60.0 + 1.0) / 2.0
            cols["last_action"][e, i] = [(S["psteer"][e, i] + 1.0) / 2.0, (S["pthrottle"][e, i] + 1.0) / 2.0]
            cols["yaw"][e, i] = min(abs(yaw[e, i] * dt) / 0.1, 1.0)
            width = (r["lanes"] + 1.0) * w
            cols["side"][e, i] = np.clip([(0.5 * w - r["lat"]) / width, ((r["lanes"] - 0.5) * w + r["lat"]) / width], 0.0, 1.0)
            cols["lane"][e, i] = min(max(-(r["lat"] + r["lane"] * w) / 4.5 + 0.5, 0.0), 1.0)
            cols["lcf"][e, i] = (S["lcf"][e, i] + 1.0) / 2.0
            if cfg.navi_dim:
                cols["navi"][e, i], recs = navigation(cfg, tables, r["route"], r["road"], S["x"][e, i], S["y"][e, i], S["th"][e, i])
                cols["navi_const"][e, i] = [recs[0][11], recs[0][13], recs[1][11], recs[1][13]]
            if cfg.toll_dim:
                cols["toll"][e, i] = [1.0 if on_booth else 0.0, 1.0 if (on_booth and wait > int(cfg.toll_min_steps)) else 0.0]
    S["status"], S["timer"], S["age"] = new_status, new_timer, new_age
    for k in ("x", "y", "th", "v"):
        T[k] = S[k].copy()
    T.update(yaw=yaw, acc=acc, v0=v0, status=new_status, timer=new_timer, age=new_age, wait=S["wait"].copy(), cols=cols, next=S)
    return T


# ---------------------------------------------------------------------------------------------------------------------------------
# the slot lifecycle
# ---------------------------------------------------------------------------------------------------------------------------------
def respawn_places(tables):
    """[(spawn slot, x, y, heading)] of the respawn places: the slots of the spawn table marked safe, on their lane of the spawn road."""
    out = []
    for p in np.nonzero(np.asarray(tables.spawn_tab)[:, 3] == 1)[0]:
        first, _, lane, _ = (int(v) for v in tables.spawn_tab[p])
        rec = tables.route_segs[first, 0]
        th = truth.road_direction(rec)
        s, off = float(tables.spawn_s[p]), lane * float(tables.lane_width)
        out.append((int(p), float(rec[0]) + s * math.cos(th) + off * math.sin(th), float(rec[1]) + s * math.sin(th) - off * math.cos(th), th))
    return out


def spawn_slot_poses(tables):
    """[P][3] pose of EVERY spawn slot (a reset draws from all of them)."""
    out = []
    for p in range(len(tables.spawn_tab)):
        first, _, lane, _ = (int(v) for v in tables.spawn_tab[p])
        rec = tables.route_segs[first, 0]
        th = truth.road_direction(rec)
        s, off = float(tables.spawn_s[p]), lane * float(tables.lane_width)
        out.append((float(rec[0]) + s * math.cos(th) + off * math.sin(th), float(rec[1]) + s * math.sin(th) - off * math.cos(th), th))
    return np.array(out)


def lifecycle_truth(cfg, tables, state, env, capacity=None):
    """The integer side of one step of scenes in which every vehicle STANDS (speed 0, full brake): per scene a dict --
      status, timer, age [N] after the step for the slots that are not respawned (and not reset);
      done_margin [N]: the smallest margin of the decisions of an acting slot;
      spawn_slots: the slots the step fills, in order (the first `spawns` waiting slots below the capacity);
      eligible: {spawn slot of a respawn place: clearance of its region from the nearest vehicle, > 0}; blocked: the same for the others (< 0);
      reset: nobody is left driving -- the scene is reset: every slot below the capacity populated, the clock 0; clock: the clock after.
    Which place or route a spawn draws is the RNG's business and is not said."""
    S = unpack(state)
    env = np.asarray(env)
    E, N = S["x"].shape
    cap = N if capacity is None else min(max(int(capacity), 1), N)
    hl, hw = float(cfg.veh_half_len), float(cfg.veh_half_wid)
    acted = S["status"] == ALIVE
    assert (S["v"][acted] == 0.0).all(), "lifecycle_truth is for standing scenes"
    status, timer = _tick(cfg, S)
    buildings = _boxes(cfg, tables)
    places = respawn_places(tables)
    out = []
    for e in range(E):
        st, tm, age = status[e].copy(), timer[e].copy(), np.where(acted[e], S["age"][e] + 1, 0)
        solid = np.nonzero(acted[e] | ((status[e] == WRECK) & (timer[e] > 0)))[0]
        margin = np.full(N, np.inf)
        for i in np.nonzero(acted[e])[0]:
            r = _decide(cfg, tables, S, status, e, i, solid, buildings)
            ms = [r["crash_gap"], r["long_margin"], r["out_margin"]] + ([r["window"]] if r["final"] else [])
            margin[i] = min(abs(m) for m in ms)
            out_of_road = r["out_margin"] < 0.0
            arrive = r["final"] and r["window"] > 0.0 and not out_of_road
            done = arrive or out_of_road or r["crash_gap"] < 0.0 or age[i] >= int(cfg.horizon)
            if done:
                st[i], tm[i], age[i] = (EMPTY, int(cfg.respawn_cooldown), 0) if (arrive or int(cfg.delay_done) <= 0) else (WRECK, int(cfg.delay_done), 0)
        clock = int(env[e, 0])
        eligible, blocked, spawn_slots = {}, {}, []
        if clock + 1 < int(cfg.horizon):                               # (6) fewer than `horizon` env steps have run
            present = np.nonzero(st != EMPTY)[0]
            for p, px, py, pth in places:
                region = ((px, py), pth, 0.5 * float(cfg.spawn_region_len), 0.5 * float(cfg.spawn_region_wid))
                gap = min([truth.box_gap(region, ((S["x"][e, j], S["y"][e, j]), S["th"][e, j], hl, hw)) for j in present], default=np.inf)
                (eligible if gap > 0.0 else blocked)[p] = gap
            waiting = [n for n in range(cap) if not acted[e, n] and st[n] == EMPTY and tm[n] == 0]
            spawn_slots = waiting[:len(eligible)]
        reset = not (st == ALIVE).any() and not spawn_slots
        out.append(dict(status=st, timer=tm, age=age, done_margin=margin, spawn_slots=spawn_slots, eligible=eligible, blocked=blocked, reset=reset,
                        clock=0 if reset else clock + 1, capacity=cap))
    return out
