"""Crafted scenes for the float64 geometry model (sim_truth_numpy.py), shared by test_sim_truth_cpu.py and test_gpu_sim_truth.py.

Every case is set with `set_state` on a freshly reset simulator: vehicles at rest, every other slot empty, the env clock at `horizon`
(no respawn), then ONE step with zero steering and full brake -- the poses of the step are the crafted ones.  The crafted words do not
depend on what the reset drew (only the LCF / id words are kept), so a case's model is evaluated once and shared.
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from copo_amd import maps
from copo_amd.sim import SimConfig

import sim_truth_numpy as truth

HL, HW = 2.2575, 0.926
W = 3.5
BODY = 0.75


@dataclass
class V:
    """One crafted vehicle: pose, the route / road its state word names, and whether it is a lingering wreck."""
    x: float
    y: float
    th: float
    route: int = 0
    road: int = 0
    wreck: bool = False
    tag: tuple = ()


@dataclass
class Case:
    name: str
    cfg: SimConfig
    scenes: list                       # per scene a list of V, slot order
    lidar: bool = True                 # evaluate / compare the LiDAR block
    caps: dict = field(default_factory=dict)        # scene -> largest share of unstable rays among the model's LiDAR hits (default 0.10)
    detector_cap: float = None         # the same for the detector beams of a detector case
    keeper: int = None                 # slot (of every scene) that must come through the step alive: the episode does not end

    def state(self, st, env):
        """The crafted state: st [16][E][N] float32 words, env [E][4] int32 of a freshly reset simulator -> new arrays."""
        st, env = np.array(st, np.float32), np.array(env, np.int32)
        iw = st.view(np.int32)
        iw[13] = 0                                               # every slot empty, its pose and route words cleared ...
        st[0:4] = 0.0
        iw[12] = 0
        iw[15] &= 0xFFFF
        for e, scene in enumerate(self.scenes):
            assert len(scene) <= st.shape[2]
            for n, v in enumerate(scene):
                st[0, e, n], st[1, e, n], st[2, e, n] = v.x, v.y, v.th
                st[3:10, e, n] = 0.0
                st[11, e, n] = 0.0
                iw[12, e, n] = v.route | (v.road << 16)
                iw[13, e, n] = (truth.WRECK | (10 << 8)) if v.wreck else truth.ALIVE
        env[:, 0] = self.cfg.horizon
        return st, env


def on_road(tables, route, road, s, lat=0.0, psi=0.0, **kw):
    """Vehicle `s` metres along road `road` of `route`, `lat` metres left of its lane-0 line, turned `psi` from the lane's direction."""
    rec = tables.route_segs[route, road].astype(np.float64)
    p = maps.shift(maps.advance((rec[0], rec[1], math.atan2(rec[3], rec[2])), s, rec[5]), lat)
    return V(p[0], p[1], float(truth._wrap(p[2] + psi)), route, road, **kw)


def spawn_vehicle(tables, p, psi=0.0, **kw):
    first, _, lane, _ = (int(v) for v in tables.spawn_tab[p])
    return on_road(tables, first, 0, float(tables.spawn_s[p]), -lane * tables.lane_width, psi, **kw)


def _cfg(map_name, E, N, lasers=72, **kw):
    return SimConfig(map=map_name, num_envs=E, num_agents=N, num_lasers=lasers, horizon=500, nbr_k=8, **kw)


def _finish(name, cfg, scenes, keeper_vehicle, **kw):
    """Pad every scene to N - 1 slots with nothing and put the keeper into the last slot."""
    N = cfg.num_agents
    out = []
    for sc in scenes:
        assert len(sc) <= N - 1, (name, len(sc))
        out.append(list(sc))
    case = Case(name, cfg, out, keeper=N - 1, **kw)
    state0 = case.state

    def state(st, env):
        st, env = state0(st, env)
        k, iw = keeper_vehicle, st.view(np.int32)
        st[0, :, N - 1], st[1, :, N - 1], st[2, :, N - 1] = k.x, k.y, k.th
        st[3:10, :, N - 1] = 0.0
        iw[12, :, N - 1] = k.route | (k.road << 16)
        iw[13, :, N - 1] = truth.ALIVE
        return st, env
    case.state = state
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
SPECIAL_HEADINGS = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi]


def heading_list(count):
    f = np.float32
    hs = []
    for a in SPECIAL_HEADINGS:
        a = f(a)
        hs += [a, np.nextafter(a, f(0.0) if a != 0 else f(1.0)), np.nextafter(a, f(4.0) if abs(a) < 3 else f(0.0))]
    hs += [np.nextafter(f(0.0), f(-1.0)), f(-0.0)]
    hs += [f(v) for v in (9e-5, -9e-5, 1e-5, -3e-6, 3e-7, -1e-8, 1e-10, 1e-20, 1e-38)]
    rest = count - len(hs)
    hs += [f(v) for v in np.linspace(-math.pi, math.pi, rest + 2)[1:-1]]
    return [float(h) for h in hs[:count]]


def case_headings():
    cfg = _cfg("intersection", 2, 40)
    t = cfg.tables()
    hs = heading_list(2 * 39)
    scenes = []
    for e in range(2):
        sc = []
        for n in range(39):
            v = spawn_vehicle(t, n)
            v.th = hs[e * 39 + n]
            sc.append(v)
        scenes.append(sc)
    return _finish("headings", cfg, scenes, spawn_vehicle(t, 47), lidar=False)


# ---------------------------------------------------------------------------------------------------------------------------------
def ring(ego_xy, ego_h, scene, rng, count, ranges=None):
    """An ego and `count` targets at every bearing around it, at ranges from 3 m to just inside and just outside `rng`, each turned
    another 7.5 degrees against the ego (all 48 relative rotations over four scenes of 23 targets)."""
    ranges = ranges or [3.2, 5.0, 0.22 * rng, 0.35 * rng, 0.55 * rng, 0.78 * rng, rng - 1.5, rng + 0.6, rng + 2.5]
    sc = [V(ego_xy[0], ego_xy[1], ego_h, tag=("ego",))]
    for k in range(count):
        g = scene * count + k
        bearing = ego_h - math.radians((k + 0.37) * 360.0 / count)
        r = ranges[(2 * k + scene) % len(ranges)]
        rot = math.radians((g % 48) * 7.5)
        sc.append(V(ego_xy[0] + r * math.cos(bearing), ego_xy[1] + r * math.sin(bearing), float(truth._wrap(ego_h + rot)), tag=("target", g % 48)))
    return sc


RIGHT_OF_HEADING_DEG = 30.0


def case_lidar_intersection():
    cfg = _cfg("intersection", 6, 26)
    t = cfg.tables()
    c = (75.6, 2.1)
    scenes = [ring(c, h, s, cfg.lidar_range, 23) for s, h in enumerate((0.3, -1.2, 2.5, -2.9))]
    # the pile: coincident vehicles, vehicles one and two circumradii away, a lingering wreck, a few around
    pile = [V(c[0], c[1], 0.7), V(c[0], c[1], 0.7), V(c[0], c[1], 1.6), V(c[0] + 2.432, c[1], -0.4), V(c[0], c[1] + 4.864, 2.2),
            V(c[0] + 6.0, c[1] - 3.0, 2.0, wreck=True)]
    pile += [V(c[0] + r * math.cos(b), c[1] + r * math.sin(b), b * 1.7 - 1.0) for r, b in ((8.0, 0.5), (11.0, 2.1), (14.0, -2.4), (9.5, -1.0), (19.0, 3.0), (27.0, 1.2))]
    scenes.append(pile)
    # handedness: ONE target 30 degrees to the right of the heading
    h = 0.4
    b = h - math.radians(RIGHT_OF_HEADING_DEG)
    scenes.append([V(c[0], c[1], h), V(c[0] + 12.0 * math.cos(b), c[1] + 12.0 * math.sin(b), 1.0)])
    return _finish("lidar-intersection", cfg, scenes, spawn_vehicle(t, 0), caps={4: 0.25})


PILE_SCENE, HANDED_SCENE = 4, 5


def case_lidar_parkinglot():
    cfg = _cfg("parkinglot", 6, 10, lasers=240)
    t = cfg.tables()
    x0, x1, y0, y1 = maps.bounding_box(t)
    c = (0.5 * (x0 + x1) + 3.3, 0.5 * (y0 + y1) + 14.2)
    scenes = [ring(c, h, s, cfg.lidar_range, 8) for s, h in enumerate((0.3, -1.2, 2.5, -2.9, 1.3, -0.2))]
    return _finish("lidar-parkinglot", cfg, scenes, spawn_vehicle(t, 0))


def case_lidar_tollgate(visible):
    cfg = _cfg("tollgate", 4, 24, lasers=30, toll_buildings=1 if visible else 2)
    t = cfg.tables()
    egos = [((78.0, -7.0), 0.2), ((87.0, -7.0), -1.4), ((96.0, 10.5), 2.8), ((87.2, 0.1), 3.0)]
    scenes = [ring(c, h, s, cfg.lidar_range, 22) for s, (c, h) in enumerate(egos)]
    return _finish("lidar-tollgate-" + ("visible" if visible else "hidden"), cfg, scenes, spawn_vehicle(t, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
GAPS = (0.01, -0.01, 0.10, -0.10)


def _radius(phi, hl=HL, hw=HW):
    """Half extent of a box turned by `phi` along a fixed axis."""
    return hl * abs(math.cos(phi)) + hw * abs(math.sin(phi))


def pair(centre, alpha, kind, gap, swap=False):
    """Two boxes whose signed gap is `gap` by construction.  A stands at `centre` with heading `alpha`; B is displaced along one axis of A:
    parallel (side by side), inline (nose to tail), tbone (B's nose against A's side), corner30/45/60 (B turned by that angle, its corner
    against A's side), axis_len / axis_wid (B turned by 20 degrees, separated along A's long / cross axis ONLY), inside (a deep overlap)."""
    u = np.array([math.cos(alpha), math.sin(alpha)])
    v = np.array([-u[1], u[0]])
    c = np.asarray(centre, np.float64)
    if kind == "parallel":
        phi, off = 0.0, v * (2 * HW + gap)
    elif kind == "inline":
        phi, off = 0.0, u * (2 * HL + gap)
    elif kind == "tbone":
        phi, off = math.pi / 2, v * (HW + HL + gap)
    elif kind.startswith("corner"):
        phi = math.radians(float(kind[6:]))
        off = v * (HW + _radius(math.pi / 2 - phi) + gap)
    elif kind == "axis_len":
        phi = math.radians(20.0)
        off = u * (HL + _radius(phi) + gap)
    elif kind == "axis_wid":
        phi = math.radians(20.0)
        off = v * (HW + _radius(math.pi / 2 - phi) + gap)
    elif kind == "inside":      # (equal boxes: deep overlap; a vehicle wholly inside a building is in case_collisions_tollgate)
        phi, off = math.radians(10.0), u * 0.2 + v * 0.2
    a, b = V(c[0], c[1], alpha, tag=(kind, gap, swap)), V(c[0] + off[0], c[1] + off[1], float(truth._wrap(alpha + phi)), tag=(kind, gap, swap))
    return [b, a] if swap else [a, b]


def collision_pairs():
    """(kind, gap, swap) of every crafted pair.  `swap` puts the turned box first: the pair is then separated along an axis of the
    SECOND box of the slot order."""
    ps = [(k, g, False) for k in ("parallel", "inline", "tbone", "corner30", "corner45", "corner60") for g in GAPS]
    ps += [("inside", None, False)]
    ps += [("axis_len", 0.05, False), ("axis_wid", 0.05, False), ("axis_len", 0.05, True), ("axis_wid", 0.05, True)]
    return ps


def case_collisions():
    ps = collision_pairs()
    per = 7
    E = (len(ps) + per - 1) // per
    cfg = _cfg("intersection", E, 2 * per + 1)
    t = cfg.tables()
    scenes = [[] for _ in range(E)]
    for k, (kind, gap, swap) in enumerate(ps):
        e, q = divmod(k, per)
        centre = (40.0 + 16.0 * (q % 4), 20.0 + 16.0 * (q // 4))          # off the roads, 16 m apart: pairs do not meet
        scenes[e] += pair(centre, 0.3 + 0.41 * k, kind, gap if gap is not None else 0.0, swap)
    return _finish("collisions", cfg, scenes, spawn_vehicle(t, 0), lidar=False)


def case_collisions_tollgate():
    cfg = _cfg("tollgate", 1, 10, toll_buildings=1)
    t = cfg.tables()
    sc = []
    for k, b in enumerate(np.asarray(t.boxes, np.float64)):
        ang = math.atan2(b[3], b[2])
        v = np.array([-b[3], b[2]])
        gap = GAPS[k % 4]
        side = 1.0 if k % 2 == 0 else -1.0
        if k < 4:       # beside the building, parallel to it
            th, off = ang, side * v * (b[5] + HW + gap)
        else:           # nose against the building's side
            th, off = ang + math.pi / 2, side * v * (b[5] + HL + gap)
        sc.append(V(b[0] + off[0], b[1] + off[1], float(truth._wrap(th)), tag=("building", k, gap)))
    b = np.asarray(t.boxes, np.float64)[0]          # one box inside another: a vehicle fits into a building's outline
    sc.append(V(b[0], b[1], math.atan2(b[3], b[2]), tag=("inside",)))
    return _finish("collisions-tollgate", cfg, [sc], spawn_vehicle(t, 0), lidar=False)


# ---------------------------------------------------------------------------------------------------------------------------------
PSIS = (math.radians(30.0), -math.radians(30.0), math.radians(45.0), math.radians(90.0), -math.radians(90.0))
NEAR = (0.01, -0.01, 0.10, -0.10)


def road_sweep(t, route, road):
    """Vehicles on one road: across every lane and both edges, +-1 cm and +-10 cm around every out-of-road threshold and every lane
    boundary, at both ends and the middle of the road; the thresholds again at heading offsets up to +-90 degrees."""
    rec = t.route_segs[route, road].astype(np.float64)
    L, lanes = rec[4], int(math.floor(rec[10]))
    code = int(round((rec[10] - lanes) * 8))

    def thresholds(psi):
        across = BODY * (HW * abs(math.cos(psi)) + HL * abs(math.sin(psi)))
        return 0.5 * W - (across if code & 2 else 0.0), -(lanes - 0.5) * W + (across if code & 4 else 0.0)

    out = []
    for s in (0.03 * L, 0.5 * L, 0.97 * L):
        lats = [th + d for th in thresholds(0.0) for d in NEAR]
        lats += [-(i + 0.5) * W + d for i in range(lanes - 1) for d in NEAR]
        lats += [-i * W for i in range(lanes)]
        out += [on_road(t, route, road, s, lat, 0.0, tag=("sweep",)) for lat in lats]
    for psi in PSIS:
        out += [on_road(t, route, road, 0.5 * L, th + d, psi, tag=("turned",)) for th in thresholds(psi) for d in NEAR]
    return out


def _find_road(t, pred):
    for r in range(t.n_routes):
        for k in range(int(t.route_meta[r, 1])):
            if pred(t.route_segs[r, k]):
                return r, k
    raise AssertionError("no such road")


def _split(vs, per):
    return [vs[i:i + per] for i in range(0, len(vs), per)]


def projection_roads(map_name, t):
    if map_name == "intersection":
        return [_find_road(t, lambda g: g[5] == 0 and g[4] > 40),                       # an entry straight: both edges continuous
                _find_road(t, lambda g: g[5] < 0 and g[12] > 5),                        # a right turn: right edge continuous
                _find_road(t, lambda g: g[5] > 0 and g[12] > 5)]                        # a left turn: no continuous line
    return [_find_road(t, lambda g: g[5] > 0 and g[12] > 30)]                           # a ring arc


def case_projection(map_name):
    t = SimConfig(map=map_name).tables()
    vs = []
    for route, road in projection_roads(map_name, t):
        vs += road_sweep(t, route, road)
    if map_name == "intersection":
        # the U-turn, an arc of half a turn: its two ends, and just past its end, where an angle measured from the arc's START would wrap
        r, k = _find_road(t, lambda g: g[5] > 0 and 0 < g[12] < 5)
        vs += [on_road(t, r, k, f * float(t.route_segs[r, k, 4]), lat, 0.0, tag=("u-turn",))
               for f, lat in ((0.05, 0.0), (0.5, 0.0), (0.95, 0.0), (1.02, 0.0), (1.02, -0.8), (1.05, 0.0), (1.05, -0.8))]
    scenes = _split(vs, 39)
    cfg = _cfg(map_name, len(scenes), 40)
    return _finish("projection-" + map_name, cfg, scenes, spawn_vehicle(t, 47 if map_name == "intersection" else 0), lidar=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# (four beams a quarter turn apart: headings between 15 and 75 degrees off the lines keep every beam off a grazing incidence)
DET_PSIS = (0.35, -0.45, 0.6, -0.8, 1.1, -1.2, 2.6, -2.0)


def case_detectors_bottleneck():
    cfg = _cfg("bottleneck", 2, 20)
    t = cfg.tables()
    scenes = []
    for e in range(2):          # the Merge road of either direction: 20 m, one lane and three wave lanes to its right
        sc, k = [], 0
        for s in (2.0, 6.5, 11.0, 15.5, 19.0):
            for lat in (0.6, -2.0, -4.4, -7.3):
                if lat < -2.5 and s > 12.0 or lat < -5.0 and s > 7.0:
                    continue
                sc.append(on_road(t, e, 1, s, lat, DET_PSIS[k % len(DET_PSIS)]))
                k += 1
        scenes.append(sc)
    return _finish("detectors-bottleneck", cfg, scenes, spawn_vehicle(t, 0), detector_cap=0.10)


def case_detectors_tollgate(lasers):
    """The booth road of either direction and the socket road next to it.

    lasers = 72 is the ordinary configuration: the detector kernels fold (beam, primitive) tests into rows of beam minima.  lasers = 8
    with 9 slots is the one that takes the fallback which walks the marked primitives beam by beam: the kernels' scratch is the LiDAR
    minima, (slots held at a time) x (LiDAR beams) words with at most min(N, 10) slots held by one wave, all N by several waves and
    min(N, 10) by the packed shape -- 9 x 8 = 72 words in every launch shape, fewer than the 72 + 4 = 76 words that one row of the
    Tollgate's detector beams needs.  (With 10 or more slots one wave holds 10: 80 words, and the fallback is not taken.)"""
    per, N = (8, 9) if lasers == 8 else (16, 24)
    t = SimConfig(map="tollgate").tables()
    vs = []
    for e in range(2):
        booth = int(t.route_meta[e, 2])
        k = 0
        for s in (2.0, 5.0, 8.0):
            for lane in (0, 2, 4, 6):
                vs.append(on_road(t, e, booth, s, -lane * W + (0.35, -0.3, 0.15)[k % 3], DET_PSIS[k % 8]))
                k += 1
        for j, lat in enumerate((0.4, -5.0, -12.5, -20.0)):        # the socket road
            vs.append(on_road(t, e, booth + (-1 if e == 0 else 1), 1.0, lat, DET_PSIS[4 + j]))
    scenes = _split(vs, per)
    cfg = _cfg("tollgate", len(scenes), N, lasers=lasers)
    assert lasers != 8 or N * lasers < cfg.side_lasers + cfg.lane_line_lasers
    return _finish("detectors-tollgate-%d" % lasers, cfg, scenes, spawn_vehicle(t, 0), detector_cap=0.10)


CASES = {
    "headings": case_headings,
    "lidar-intersection": case_lidar_intersection,
    "lidar-parkinglot": case_lidar_parkinglot,
    "lidar-tollgate-visible": lambda: case_lidar_tollgate(True),
    "lidar-tollgate-hidden": lambda: case_lidar_tollgate(False),
    "collisions": case_collisions,
    "collisions-tollgate": case_collisions_tollgate,
    "projection-intersection": lambda: case_projection("intersection"),
    "projection-roundabout": lambda: case_projection("roundabout"),
    "detectors-bottleneck": case_detectors_bottleneck,
    "detectors-tollgate-8": lambda: case_detectors_tollgate(8),
    "detectors-tollgate-72": lambda: case_detectors_tollgate(72),
}


@lru_cache(maxsize=None)
def get_case(name):
    return CASES[name]()


_TRUTH = {}


def crafted_state(name):
    """The crafted words of case `name` on an all-zero template: what the model needs, without any simulator."""
    cfg = get_case(name).cfg
    return get_case(name).state(np.zeros((16, cfg.num_envs, cfg.num_agents), np.float32), np.zeros((cfg.num_envs, 4), np.int32))[0]


def case_truth(name, st):
    """The model's answer for the crafted state of case `name`, evaluated once; `st` must be that state."""
    case = get_case(name)
    if name not in _TRUTH:
        _TRUTH[name] = (np.array(st, np.float32), truth.step_truth(case.cfg, case.cfg.tables(), st, lidar=case.lidar))
    st0, T = _TRUTH[name]
    assert np.array_equal(st0[[0, 1, 2, 3, 12, 13]].view(np.uint32), np.asarray(st, np.float32)[[0, 1, 2, 3, 12, 13]].view(np.uint32)), "the crafted words differ"
    return T


# ---------------------------------------------------------------------------------------------------------------------------------
# one step of a simulator, and its comparison with the model
# ---------------------------------------------------------------------------------------------------------------------------------
F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_ENV_RESET = 1, 2, 4, 8, 16, 128
DECISION_BAND = 1e-3       # decisions are compared where the model's signed margin is further than this from its threshold (metres)
DISTANCE_TOL = 1e-3        # stable beams and the side / lane columns: metres
HEADING_TOL = 3e-7


def brake_actions(cfg):
    a = np.zeros((cfg.num_envs, cfg.num_agents, 2), np.float32)
    a[..., 1] = -1.0
    return a


def _beam_block(tag, got, T, key, rng, rows, stats):
    """One block of beams of the rows `rows` ([E][N] mask) against the model."""
    want, stable, hit = T[key][rows], T[key + "_stable"][rows], T[key + "_hit"][rows]
    got = got[rows].astype(np.float64)
    assert (got <= 1.0).all() and (got >= 0.0).all(), tag
    err = np.abs(got - want) * rng
    worst = float(err[stable].max()) if stable.any() else 0.0
    stats[key + "_err_m"] = max(stats.get(key + "_err_m", 0.0), worst)
    stats[key + "_stable_hits"] = stats.get(key + "_stable_hits", 0) + int((stable & hit).sum())
    assert worst <= DISTANCE_TOL, "%s: a stable beam is %.3g m from the model (bound %g)" % (tag, worst, DISTANCE_TOL)
    miss, sure = T[key + "_clear_miss"][rows] & ~stable, T[key + "_clear_hit"][rows] & ~stable
    assert (got[miss] == 1.0).all(), "%s: a return where the model misses by more than 1 cm" % tag
    assert (got[sure] < 1.0).all(), "%s: no return where the model hits by more than 1 cm" % tag


def check_against_model(case, T, obs, flags, info):
    """Hold one step's outputs (obs [E][N][O], flags [E][N], info [E][N][8], numpy) to the model `T` of the case.  Returns the measured
    maxima."""
    cfg, cols, stats = case.cfg, truth.obs_columns(case.cfg), {}
    tag = case.name
    acted = T["acted"]
    assert not (flags & F_ENV_RESET).any() and not (flags & F_ARRIVE).any(), "%s: the scene must outlast the step" % tag
    assert np.array_equal((flags & F_ACTED) != 0, acted), tag
    k = case.keeper
    assert (T["crash_gap"][:, k] > truth.CLEAR).all() and (T["out_margin"][:, k] > truth.CLEAR).all() and not (flags[:, k] & F_DONE).any(), \
        "%s: the keeper must come through the step" % tag
    # decisions
    sure = acted & (np.abs(T["crash_gap"]) > DECISION_BAND)
    assert np.array_equal(((flags & F_CRASH) != 0)[sure], (T["crash_gap"] < 0.0)[sure]), "%s: crash flags" % tag
    located = acted & (T["long_margin"] > DECISION_BAND)
    with np.errstate(invalid="ignore"):
        known = located & (np.abs(T["out_margin"]) > DECISION_BAND)
    assert np.array_equal(((flags & F_OUT) != 0)[known], (T["out_margin"] < 0.0)[known]), "%s: out-of-road flags" % tag
    stats.update(crash_decisions=int(sure.sum()), out_decisions=int(known.sum()), crash_sure=sure, out_known=known, located=located)
    # longitudinal coordinate: the route-completion column of the info row is (start of the road on the route + long) / route length
    inside = located & (T["prog"] > DECISION_BAND) & (T["prog"] < T["total"] - DECISION_BAND)
    err = (np.abs(info[..., 7].astype(np.float64) * T["total"] - T["prog"]))[inside]
    stats.update(long_err_m=float(err.max()), long_rows=int(inside.sum()))
    assert stats["long_err_m"] <= DISTANCE_TOL, "%s: longitudinal coordinate %.3g m from the model (bound %g)" % (tag, stats["long_err_m"], DISTANCE_TOL)
    # heading column
    err = np.abs(obs[..., cols["heading"]].astype(np.float64) - T["heading"])[located]
    stats["heading_err"] = float(err.max())
    assert stats["heading_err"] <= HEADING_TOL, "%s: heading column %.3g from the model (bound %g)" % (tag, stats["heading_err"], HEADING_TOL)
    w = float(cfg.lane_width)
    if not cfg.side_lasers:
        width = (T["lanes"] + 1.0) * w
        err = (np.abs(obs[..., 0:2].astype(np.float64) - T["side"]) * width[..., None])[located]
        stats["side_err_m"] = float(err.max())
        assert stats["side_err_m"] <= DISTANCE_TOL, "%s: side columns %.3g m from the model" % (tag, stats["side_err_m"])
    else:
        _beam_block(tag + " side detector", obs[..., 0:cfg.side_lasers], T, "side", float(cfg.side_range), acted, stats)
    if not cfg.lane_line_lasers:
        col = obs[..., cols["lane"]].astype(np.float64)
        laned = located & (T["lane_margin"] > DECISION_BAND)
        err = (np.abs(col - T["lane_col"][..., 0]) * 4.5)[laned]
        stats["lane_err_m"] = float(err.max())
        assert stats["lane_err_m"] <= DISTANCE_TOL, "%s: lane column %.3g m from the model" % (tag, stats["lane_err_m"])
        # the lane index the simulator used, from its own column and the model's lateral coordinate (where the column is not clipped)
        seen = laned & (T["lane_col"][..., 0] > 1e-3) & (T["lane_col"][..., 0] < 1.0 - 1e-3)
        lane = (-T["lat"] - (col - 0.5) * 4.5) / w
        assert (np.abs(lane - np.rint(lane))[seen] * w <= DISTANCE_TOL).all() and np.array_equal(np.rint(lane)[seen].astype(int), T["lane"][seen]), "%s: lane index" % tag
        stats.update(lane_decisions=int(seen.sum()), lane_seen=seen)
    else:
        c0 = cols["lane"]
        _beam_block(tag + " lane-line detector", obs[..., c0:c0 + cfg.lane_line_lasers], T, "lane_col", float(cfg.lane_line_range), acted, stats)
    if case.lidar:
        c0 = cols["lidar"]
        _beam_block(tag + " lidar", obs[..., c0:c0 + cfg.num_lasers], T, "lidar", float(cfg.lidar_range), acted, stats)
    return stats


def unstable_shares(T, key):
    """Per scene: the share of unstable beams among the beams that hit in the model (rows of slots that act)."""
    hit = T[key + "_hit"] & T["acted"][..., None]
    bad = hit & ~T[key + "_stable"]
    return bad.sum((1, 2)) / np.maximum(hit.sum((1, 2)), 1), hit.sum((1, 2))
