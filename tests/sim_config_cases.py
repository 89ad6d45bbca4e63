"""Cases shared by test_gpu_sim_config_parity.py (HIP against the oracle, bit for bit) and test_sim_config_premises_cpu.py (the
oracle alone: the configurations really take the branches the GPU cases are there for).  Both files draw seeds, actions and setter
calls from here, so a premise that holds on the CPU holds for the inputs of the GPU case.  Test infrastructure only."""
import numpy as np

STEPS_A, STEPS_B = 100, 120


def seeds(E):
    return np.arange(E, dtype=np.uint64) * np.uint64(7919) + np.uint64(5000)


def actions(rng, E, N, t, sigma=0.12):
    """test_gpu_sim_parity._actions with the steering noise as a parameter (same draws, same NaN / clipping slot)."""
    steer = rng.normal(0, sigma, (E, N))
    thr = rng.uniform(-0.2, 1.0, (E, N))
    a = np.stack([steer, thr], -1).astype(np.float32)
    if t % 7 == 0:
        a[0, 0] = [np.nan, 5.0]     # NaN guard + clipping
    return a


def sim_config(map_name, E, N, lasers=72, horizon=90, **kw):
    from copo_amd.sim import SimConfig
    return SimConfig(map=map_name, num_envs=E, num_agents=N, num_lasers=lasers, horizon=horizon, delay_done=5, nbr_k=8, **kw)


# ---- A1: the Tollgate with buildings the LiDAR sees.  (id, block, E, N, beams, LiDAR fans per LDS pass or 0)
VISIBLE_SHAPES = [
    ("wave64", 64, 3, 40, 72, 0),              # one wave per scene: lane = box, ballot, readlane
    ("block512", 512, 3, 40, 72, 0),           # many waves per scene: one thread per (fan, ray)
    ("block1024", 1024, 3, 40, 72, 0),
    ("packed4-E5", -4, 5, 40, 72, 0),          # packed, one scene in the last workgroup
    ("packed2-E3", -2, 3, 40, 72, 0),
    ("wave64-8beams", 64, 3, 40, 8, 0),        # no room for the detector row: the box minima share the storage of the walking fallback
    ("block256-8beams", 256, 3, 40, 8, 0),
    ("wave64-30beams-chunk3", 64, 3, 24, 30, 3),   # several LDS passes (the fan index is pass-local), NL & 3 != 0 (scalar write-out)
]
# LiDAR cells that must differ between visible and hidden buildings over the rollout, by beam count
VISIBLE_MIN_CELLS = {72: 1000, 8: 500, 30: 500}


def visible_config(E, N, lasers, buildings=1):
    return sim_config("tollgate", E, N, lasers, toll_buildings=buildings)


# ---- B: configuration knobs.  (id, map, N, SimConfig keywords, steering sigma)
def knob_cases():
    from copo_amd.sim import TOLLGATE_ROUND5_SCENE
    return [
        ("lat_acc_max3", "roundabout", 40, dict(lat_acc_max=3.0), 0.5),
        ("respawn_cooldown8", "roundabout", 40, dict(respawn_cooldown=8), 0.12),
        ("substeps2", "intersection", 30, dict(substeps=2), 0.12),
        ("substeps7", "intersection", 30, dict(substeps=7), 0.12),
        ("lidar_counterclockwise", "intersection", 30, dict(lidar_clockwise=False), 0.12),
        ("body_margin0", "roundabout", 40, dict(body_margin=0.0), 0.12),
        ("body_margin1", "roundabout", 40, dict(body_margin=1.0), 0.12),
        ("mf6_nbr25", "intersection", 30, dict(mf_distance=6.0, neighbours_distance=25.0), 0.12),
        ("tollgate_round5", "tollgate", 40, dict(TOLLGATE_ROUND5_SCENE), 0.12),
        ("forced_lcf", "intersection", 30, dict(), 0.12),
    ]


KNOB_E = 3
KNOB_BLOCKS = (64, 512, -4)
# setter calls of a case: step -> [(method, arguments)]; -1 = before the reset
FORCED_LCF_CALLS = {-1: [("set_force_lcf", (0.5,))], 30: [("set_force_lcf", (-0.8,))], 60: [("set_force_lcf", (-100.0,))],
                    80: [("set_lcf_dist", (0.4, 0.3))]}
KNOB_CALLS = {"forced_lcf": FORCED_LCF_CALLS}

# ---- C: the captured step
# (a scene past its horizon stops respawning, so nobody spawns between replay 80 and the scenes' resets at replays 121..135: the 120
#  replays are followed by 20 more, in which every scene is reset -- under the capacity and the lifted forced LCF of replay 80)
GRAPH_E, GRAPH_N, GRAPH_HORIZON, GRAPH_STEPS, GRAPH_EXTRA = 4, 30, 70, 120, 20
GRAPH_CALLS = {40: [("set_lcf_dist", (0.4, 0.3))], 60: [("set_force_lcf", (0.5,))],
               80: [("set_force_lcf", (-100.0,)), ("set_capacity", (20,))]}


def apply_calls(calls, t, *sims):
    for name, args in (calls or {}).get(t, ()):
        for s in sims:
            getattr(s, name)(*args)


def oracle_rollout(cfg, steps, sigma=0.12, calls=None, keys=("obs", "flags", "lcf")):
    """The oracle alone on a case's inputs: a list with the reset's and every step's outputs (copies of `keys`)."""
    import oracle_lib as ol
    o = ol.OracleSim(cfg)
    E, N = o.E, o.N
    apply_calls(calls, -1, o)
    rec = [{k: o.reset(seeds(E))[k].copy() for k in keys}]
    rng = np.random.RandomState(3)
    for t in range(steps):
        apply_calls(calls, t, o)
        out = o.step(actions(rng, E, N, t, sigma))
        rec.append({k: out[k].copy() for k in keys})
    o.close()
    return rec


def lidar_cols(cfg):
    c0 = cfg.ego_dim + cfg.navi_dim
    return slice(c0, c0 + cfg.num_lasers)


# ---- A2: crafted scenes around the Tollgate's buildings
CRAFT_E, CRAFT_N, CRAFT_STEPS, CRAFT_KEEP = 6, 40, 3, 4


def _f32(x):
    return np.float32(x)


def cull_edge(centre, reach):
    """The three fp32 coordinates p > centre around the cull radius of the kernels' box test, `fl((centre - p)^2) <= fl(reach^2)`:
    (last one inside the cull, the one on it, first one outside) = one ulp below, exactly at, one ulp above the largest p that passes."""
    centre, reach = _f32(centre), _f32(reach)
    lim = _f32(reach * reach)

    def inside(p):
        d = _f32(centre - p)
        return _f32(d * d) <= lim

    p = _f32(centre + reach)
    for _ in range(64):                       # fl(centre + reach) is within a few ulps of the edge
        if not inside(p):
            p = np.nextafter(p, _f32(-np.inf))
        elif inside(np.nextafter(p, _f32(np.inf))):
            p = np.nextafter(p, _f32(np.inf))
        else:
            break
    assert inside(p) and not inside(np.nextafter(p, _f32(np.inf)))
    return np.nextafter(p, _f32(-np.inf)), p, np.nextafter(p, _f32(np.inf))


def crafted_building_scenes(cfg, st):
    """Poses around two of the Tollgate's buildings (long axis = world x, short axis = world y; the outermost building on either
    side of the road, so that what a pose sees is that building).  Writes x, y, heading, speed 0 of every slot into the state `st`
    [16][E][N] and returns {name: (scene, slot)} of the poses the premises name.  Slots that are not named stand far from everything
    (case e), but for the last CRAFT_KEEP, which stay where the reset put them.  The cull of the kernels is `distance^2 <= (range + half_len + half_wid)^2` from the building's centre: at that radius
    the nearest face is still range + min(half_len, half_wid) away, so NO pose on the cull radius can have a beam shortened -- the
    cull can only show if it is too tight by metres.  The poses `reach_in` / `reach_out` are therefore added: a vehicle that looks
    at a face along the axis with the face one step inside / outside the LiDAR's range, where the return itself appears."""
    E, N = st.shape[1:]
    assert (E, N) == (CRAFT_E, CRAFT_N)
    boxes = np.asarray(cfg.tables().boxes, np.float32)
    ys = boxes[:, 1]
    lo, hi = boxes[int(np.argmin(ys))], boxes[int(np.argmax(ys))]
    for B in (lo, hi):
        assert abs(abs(B[2]) - 1.0) < 1e-6 and abs(B[3]) < 1e-6, "the crafted poses assume buildings along the world's x axis"
    rng_ = _f32(cfg.lidar_range)
    hw = _f32(cfg.veh_half_wid)
    pi = np.pi
    x = np.zeros((E, N), np.float32)
    y = np.zeros((E, N), np.float32)
    th = np.zeros((E, N), np.float32)
    x[:] = 5000.0 + 137.0 * np.arange(N)[None, :]          # (e): far from every building and from each other
    y[:] = 3000.0 + 211.0 * np.arange(E)[:, None]
    th[:] = np.linspace(-3.0, 3.0, N, dtype=np.float32)[None, :]
    named = {}

    def put(name, e, n, px, py, heading):
        x[e, n], y[e, n], th[e, n] = px, py, heading
        if name:
            named[name] = (e, n)

    # (a) on the cull radius along the long axis of `lo` (+x) and the short axis of `hi` (+y): scenes 0, 1, 2 = inside, on, outside
    reach_lo, reach_hi = _f32(rng_ + _f32(lo[4] + lo[5])), _f32(rng_ + _f32(hi[4] + hi[5]))
    for e, (px, py) in enumerate(zip(cull_edge(lo[0], reach_lo), cull_edge(hi[1], reach_hi))):
        tag = ("inside", "on", "outside")[e]
        put("cull_long_" + tag, e, 0, px, lo[1], pi)              # looks back at the building
        put("cull_short_" + tag, e, 1, hi[0], py, -pi / 2)
    # the face one fp32 step inside (scene 0) / outside (scene 1) the range, seen along the axis by beam 0: from the -x end of `lo`,
    # and from the outer side of `lo`
    near_x, near_y = _f32(_f32(lo[0] - lo[4]) - rng_), _f32(_f32(lo[1] - lo[5]) - rng_)
    put("reach_in_long", 0, 2, np.nextafter(near_x, _f32(np.inf)), lo[1], 0.0)
    put("reach_out_long", 1, 2, np.nextafter(near_x, _f32(-np.inf)), lo[1], 0.0)
    put("reach_in_short", 0, 3, lo[0], np.nextafter(near_y, _f32(np.inf)), pi / 2)
    put("reach_out_short", 1, 3, lo[0], np.nextafter(near_y, _f32(-np.inf)), pi / 2)
    # (b) scene 3: 3 m off a long face, heading exactly along / exactly across the long axis -- rays parallel to the faces
    off_lo, off_hi = lo[1] - lo[5] - 3.0, hi[1] + hi[5] + 3.0
    put("parallel_along", 3, 0, lo[0] - 2.0, off_lo, 0.0)
    put("parallel_across", 3, 1, hi[0] + 1.0, off_hi, -pi / 2)
    put("parallel_along_back", 3, 2, hi[0] + 30.0, hi[1], pi)     # along the long axis itself, 25 m off the end face: out of range
    put("parallel_end_face", 3, 3, lo[0] + lo[4] + 4.0, lo[1], pi / 2)   # 4 m off the END face, heading across the long axis
    # (c) scene 4: the minimum of a vehicle's and a building's return, in both orders
    put("behind_vehicle", 4, 0, lo[0], lo[1] - lo[5] - 12.0, pi / 2)      # looks at the building ...
    put("blocker", 4, 1, lo[0], lo[1] - lo[5] - 6.0, pi / 2)              # ... past a vehicle standing in the line of sight
    put("before_building", 4, 2, hi[0], hi[1] + hi[5] + 8.0, -pi / 2)     # looks at the building ...
    put("hidden_by_building", 4, 3, hi[0], hi[1] - 3.5, 0.0)              # ... with a vehicle in the lane behind it, inside the range
    # (d) scene 5: a body that overlaps a building by a centimetre, and one that misses it by a centimetre
    put("touching", 5, 0, lo[0] + 1.0, lo[1] - lo[5] - hw + 0.01, 0.0)
    put("clear", 5, 1, hi[0] - 1.0, hi[1] + hi[5] + hw + 0.01, 0.0)
    keep = slice(N - CRAFT_KEEP, N)      # these stay on their spawn points: a scene whose agents all end in one step would be reset
    x[:, keep], y[:, keep], th[:, keep] = st[0][:, keep], st[1][:, keep], st[2][:, keep]
    st[0], st[1], st[2] = x, y, th
    st[3] = 0.0
    return named


def crafted_actions():
    a = np.zeros((CRAFT_E, CRAFT_N, 2), np.float32)
    a[..., 1] = -1.0                                   # brake: vehicles at rest stay where they were put
    return a
