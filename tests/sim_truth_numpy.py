"""Float64 model of the GEOMETRY of one simulator step, written from SPEC.md section 3 and textbook geometry.  Test infrastructure only.

Every simulator test compares the HIP kernel with the scalar oracle bit for bit; both restate the same fp32 expressions, so a geometric
error moves them together.  This model shares no expression with them: rays meet boxes by the slab method with divisions, boxes are
separated by projecting their corners, arcs are measured from a mid radial derived from the start pose and the length (not read from the
road record), detector beams solve a 2 x 2 system per segment and test an arc's extent from its start.

Inputs are the raw state words [16][E][N] (fields 0..3 = x, y, heading, speed; word 12 = route | road << 16; word 13 = status | timer << 8
| age << 16), a `SimConfig` and the map tables of `copo_amd/maps.py`.  The scenes this model is for stand still (speed 0, full brake, no
steering), so the poses of the step are the poses of the state.

`step_truth` returns per slot what the step decides and what the observation row reports, with signed margins next to every decision and a
stability mask next to every beam (see `_beams_vs_boxes`).
"""
import itertools
import math

import numpy as np

ALIVE, WRECK = 1, 2
POS_EPS, ANG_EPS = 1e-4, 1e-5              # pose perturbations of the stability filter: metres, radians
MIN_INCIDENCE = math.sin(math.radians(15.0))
CLEAR = 0.01                               # a hit / a miss "by more than 1 cm"
RIGHT_ANGLE = math.pi / 2


def _wrap(a):
    return (np.asarray(a, np.float64) + math.pi) % (2.0 * math.pi) - math.pi


# ---------------------------------------------------------------------------------------------------------------------------------
# ray against box
# ---------------------------------------------------------------------------------------------------------------------------------
def ray_box(origin, angle, centre, box_angle, half_len, half_wid):
    """Slab method in the box frame (all arguments broadcast; origin / centre have a last axis of 2).
    Returns (distance, face, sin_incidence): distance = inf on a miss, 0 when the origin is inside; face 0 = a face across the long
    axis (front / rear), 1 = a side face, -1 = origin inside or miss; sin_incidence = sine of the angle between ray and entering face."""
    origin, centre = np.asarray(origin, np.float64), np.asarray(centre, np.float64)
    rel = origin - centre
    ca, sa = np.cos(box_angle), np.sin(box_angle)
    o = np.stack([rel[..., 0] * ca + rel[..., 1] * sa, -rel[..., 0] * sa + rel[..., 1] * ca], -1)
    rel_angle = np.asarray(angle, np.float64) - box_angle
    d = np.stack([np.cos(rel_angle), np.sin(rel_angle)], -1) + 0.0 * o
    o = o + 0.0 * d
    half = np.stack(np.broadcast_arrays(np.asarray(half_len, np.float64), np.asarray(half_wid, np.float64)), -1) + 0.0 * o
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-half - o) / d, (half - o) / d
    near, far = np.minimum(t1, t2), np.maximum(t1, t2)
    par = d == 0.0                                     # parallel to a slab: inside it for every t, or for none
    inside_slab = np.abs(o) <= half
    near = np.where(par, np.where(inside_slab, -np.inf, np.inf), near)
    far = np.where(par, np.where(inside_slab, np.inf, -np.inf), far)
    t_in, t_out = near.max(-1), far.min(-1)
    hit = (t_in <= t_out) & (t_out >= 0.0)
    face = np.where(near[..., 0] >= near[..., 1], 0, 1)
    sin_inc = np.where(face == 0, np.abs(d[..., 0]), np.abs(d[..., 1]))
    inside = hit & (t_in <= 0.0)
    dist = np.where(hit, np.maximum(t_in, 0.0), np.inf)
    face = np.where(hit & ~inside, face, -1)
    return dist, face, np.where(face >= 0, sin_inc, 1.0)


def _combos(k):
    return [np.array(c, np.float64) for c in itertools.product((-1.0, 1.0), repeat=k)]


def _beams_vs_boxes(pos, head, rel_angles, tgt_pos, tgt_ang, tgt_hl, tgt_hw, tgt_mask, tgt_moves, rng):
    """LiDAR of the N egos of one scene against M boxes.  rel_angles [L]: beam directions relative to the heading (counter-clockwise
    positive); tgt_mask [N][M]: which boxes ego i sees; tgt_moves [M]: boxes that are vehicles (perturbed), as opposed to buildings.
    Returns value [N][L] = min(hits, range) / range, hit [N][L], stable [N][L], clear_miss, clear_hit [N][L].

    stable: the float64 model alone keeps the ray's outcome -- the same box through the same face is still (one of) the nearest, or
    nothing is hit -- when ego and boxes are moved by +-POS_EPS and turned by +-ANG_EPS in all 64 sign combinations, and the entering
    face is met at more than 15 degrees.  clear_miss / clear_hit: the outcome holds with every box grown / shrunk by 1 cm and the range
    likewise."""
    N, M, L = len(pos), len(tgt_pos), len(rel_angles)
    if M == 0:
        z = np.zeros((N, L), bool)
        return np.ones((N, L)), z, ~z, ~z, z

    def run(p, h, tp, ta, grow=0.0):
        d, f, s = ray_box(p[:, None, None, :], (h[:, None] + rel_angles[None, :])[:, :, None], tp[None, None], ta[None, None],
                          tgt_hl[None, None] + grow, tgt_hw[None, None] + grow)
        d = np.where(tgt_mask[:, None, :] & (d < rng + grow), d, np.inf)
        return d, f, s

    d0, f0, s0 = run(pos, head, tgt_pos, tgt_ang)
    best = d0.min(-1)
    which = d0.argmin(-1)[..., None]
    hit = np.isfinite(best)
    face = np.take_along_axis(f0, which, -1)[..., 0]
    sin_inc = np.take_along_axis(s0, which, -1)[..., 0]
    stable = np.where(hit, (face < 0) | (sin_inc > MIN_INCIDENCE), True)
    mv = tgt_moves.astype(np.float64)
    for c in _combos(6):
        d, f, _ = run(pos + c[:2] * POS_EPS, head + c[2] * ANG_EPS, tgt_pos + mv[:, None] * c[3:5] * POS_EPS, tgt_ang + mv * c[5] * ANG_EPS)
        b = d.min(-1)
        dn = np.take_along_axis(d, which, -1)[..., 0]
        fn = np.take_along_axis(f, which, -1)[..., 0]
        stable &= np.where(hit, np.isfinite(dn) & (fn == face) & (dn <= b + 1e-9), ~np.isfinite(b))
    clear_miss = ~np.isfinite(run(pos, head, tgt_pos, tgt_ang, CLEAR)[0].min(-1))
    clear_hit = np.isfinite(run(pos, head, tgt_pos, tgt_ang, -CLEAR)[0].min(-1))
    return np.minimum(best, rng) / rng, hit, stable, clear_miss, clear_hit


# ---------------------------------------------------------------------------------------------------------------------------------
# box against box
# ---------------------------------------------------------------------------------------------------------------------------------
def _corners(centre, angle, half_len, half_wid):
    u = np.array([math.cos(angle), math.sin(angle)])
    v = np.array([-u[1], u[0]])
    c = np.asarray(centre, np.float64)
    return np.array([c + a * half_len * u + b * half_wid * v for a in (-1, 1) for b in (-1, 1)]), (u, v)


def box_axis_gaps(box_a, box_b):
    """box = (centre, angle, half length, half width).  The separation of the two boxes along the four candidate axes -- long and cross
    axis of a, long and cross axis of b --: the gap between the intervals their corners project to (negative: the intervals overlap)."""
    ca, axes_a = _corners(*box_a)
    cb, axes_b = _corners(*box_b)
    gaps = []
    for ax in axes_a + axes_b:
        pa, pb = ca @ ax, cb @ ax
        gaps.append(max(pb.min() - pa.max(), pa.min() - pb.max()))
    return np.array(gaps)


def box_gap(box_a, box_b):
    """Signed gap of two convex boxes: the largest separation over the four axes; negative when they overlap."""
    return float(box_axis_gaps(box_a, box_b).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# road projection
# ---------------------------------------------------------------------------------------------------------------------------------
def road_direction(rec):
    return math.atan2(float(rec[3]), float(rec[2]))


def project(rec, x, y, heading):
    """(longitudinal, lateral (left +), psi = heading - lane direction at the vehicle) on the lane-0 line of road record `rec`."""
    x0, y0, length, kappa = (float(rec[k]) for k in (0, 1, 4, 5))
    th0 = road_direction(rec)
    if kappa == 0.0:
        dx, dy = x - x0, y - y0
        return dx * math.cos(th0) + dy * math.sin(th0), -dx * math.sin(th0) + dy * math.cos(th0), float(_wrap(heading - th0))
    sg, radius = (1.0 if kappa > 0 else -1.0), float(rec[12])
    cx, cy = x0 - sg * radius * math.sin(th0), y0 + sg * radius * math.cos(th0)
    start = math.atan2(y0 - cy, x0 - cx)                          # radial angle of the arc's start
    mid = start + sg * 0.5 * length / radius                      # ... of its mid point: the angle is measured from here
    ex, ey = x - cx, y - cy
    turned = float(_wrap(math.atan2(ey, ex) - mid))               # in [-pi, pi): no wrap inside an arc of up to a full turn
    tangent = math.atan2(ey, ex) + sg * RIGHT_ANGLE
    return 0.5 * length + sg * turned * radius, sg * (radius - math.hypot(ex, ey)), float(_wrap(heading - tangent))


def road_decisions(cfg, tables, route, road, x, y, heading):
    """The step's localisation and out-of-road decision of one vehicle (SPEC 3.4 (3), (4)).  dict: road (after at most two advances and
    one step back), long, lat, psi, lanes, lane, lane_margin, out_margin (signed distance of the centre to the nearest out-of-road
    threshold: < 0 = out of road; nan on the straight of a Merge / Split block, whose extra width this model leaves out) and
    long_margin (distance of the longitudinal coordinate to the nearest road-advance threshold that was looked at)."""
    w, hl, hw = float(cfg.lane_width), float(cfg.veh_half_len), float(cfg.veh_half_wid)
    nroads = int(tables.route_meta[route, 1])
    rec = tables.route_segs[route, road]
    lon, lat, psi = project(rec, x, y, heading)
    long_margin = np.inf
    for _ in range(2):
        if road < nroads - 1:
            long_margin = min(long_margin, abs(lon - float(rec[4])))
            if lon > float(rec[4]):
                road += 1
                rec = tables.route_segs[route, road]
                lon, lat, psi = project(rec, x, y, heading)
    if road > 0:
        long_margin = min(long_margin, abs(lon))
        if lon < 0.0:
            road -= 1
            rec = tables.route_segs[route, road]
            lon, lat, psi = project(rec, x, y, heading)
    lanes = int(math.floor(float(rec[10])))
    code = int(round((float(rec[10]) - lanes) * 8.0))              # eighths: 2 = left edge continuous, 4 = right, 1 = left edge open
    across = hw * abs(math.cos(psi)) + hl * abs(math.sin(psi))     # the body's half extent across the road
    to_left, to_right = 0.5 * w - lat, (lanes - 0.5) * w + lat     # distance of the centre to the two edges of the road
    need_left = cfg.body_margin * across if code & 2 else (-w if code & 1 else 0.0)
    need_right = cfg.body_margin * across if code & 4 else 0.0
    out_margin = out_margin_narrow = min(to_left - need_left, to_right - need_right)      # (narrow: without a funnel's extra width)
    if float(rec[5]) == 0.0 and float(rec[12]) != 0.0:
        out_margin = float("nan")
    lane = min(max(int(math.floor(-lat / w + 0.5)), 0), lanes - 1)
    lane_margin = min([abs(-lat - (i + 0.5) * w) for i in range(lanes - 1)], default=np.inf)
    return dict(road=road, long=lon, lat=lat, psi=psi, lanes=lanes, lane=lane, lane_margin=lane_margin, out_margin=out_margin,
                out_margin_narrow=out_margin_narrow, long_margin=long_margin, length=float(rec[4]), prog=float(rec[6]) + lon, total=float(tables.route_meta[route, 0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# detector beams against lane lines
# ---------------------------------------------------------------------------------------------------------------------------------
def _beams_vs_lines(pos, angles, lines, rng):
    """pos [N][2], angles [N][L] absolute beam directions, lines [P][8] = x0, y0, theta0, length, kappa, kind, ., .
    Returns (distance [N][L][P] with inf = no hit within `rng`, sin_incidence [N][L][P])."""
    N, L = angles.shape
    dist = np.full((N, L, len(lines)), np.inf)
    sinc = np.ones((N, L, len(lines)))
    dx, dy = np.cos(angles), np.sin(angles)
    for p, (x0, y0, th, ln, kap) in enumerate(np.asarray(lines, np.float64)[:, :5]):
        if kap == 0.0:
            # origin + t d = q0 + u e, a 2 x 2 system solved by Cramer's rule
            ex, ey = math.cos(th), math.sin(th)
            qx, qy = (x0 - pos[:, 0])[:, None], (y0 - pos[:, 1])[:, None]
            det = dx * ey - dy * ex
            with np.errstate(divide="ignore", invalid="ignore"):
                t, u = (qx * ey - qy * ex) / det, (qx * dy - qy * dx) / det
            ok = (det != 0.0) & (t >= 0.0) & (u >= 0.0) & (u <= ln)
            dist[:, :, p] = np.where(ok, t, np.inf)
            sinc[:, :, p] = np.abs(det)
        else:
            sg, radius = (1.0 if kap > 0 else -1.0), 1.0 / abs(kap)
            cx, cy = x0 - sg * radius * math.sin(th), y0 + sg * radius * math.cos(th)
            start, sweep = math.atan2(y0 - cy, x0 - cx), ln / radius
            mx, my = (pos[:, 0] - cx)[:, None], (pos[:, 1] - cy)[:, None]
            b, c = mx * dx + my * dy, mx * mx + my * my - radius * radius
            disc = b * b - c
            root = np.sqrt(np.where(disc >= 0.0, disc, np.nan))
            def on_arc(t):
                turned = (sg * (np.arctan2(my + t * dy, mx + t * dx) - start)) % (2.0 * math.pi)
                return (disc >= 0.0) & (t >= 0.0) & (turned <= sweep)

            t_lo, t_hi = -b - root, -b + root
            best = np.where(on_arc(t_lo), t_lo, np.where(on_arc(t_hi), t_hi, np.inf))
            tt = np.where(np.isfinite(best), best, 0.0)
            bs = np.abs((mx + tt * dx) * dx + (my + tt * dy) * dy) / radius
            dist[:, :, p], sinc[:, :, p] = best, bs
    dist = np.where(dist < rng, dist, np.inf)
    return dist, sinc


def detector(pos, head, n_beams, lines, min_kind, rng):
    """Side / lane-line detector of N vehicles: beam k is turned 90 + k * 360 / n_beams degrees CLOCKWISE of the heading and sees the
    lane-line primitives of kind >= min_kind.  Returns value [N][n] = min(hits, range) / range, hit, stable (as for the LiDAR: the
    nominal primitive stays the nearest when the vehicle is moved and turned in all 8 sign combinations, incidence above 15 degrees),
    clear_miss, clear_hit (outcome unchanged with the range 1 cm shorter / longer and the beam moved 1 cm either way)."""
    lines = np.asarray(lines, np.float64)
    lines = lines[lines[:, 5] >= min_kind]
    rel = -np.radians(90.0 + 360.0 * np.arange(n_beams) / n_beams)
    pos, head = np.asarray(pos, np.float64), np.asarray(head, np.float64)
    d0, s0 = _beams_vs_lines(pos, head[:, None] + rel[None], lines, rng)
    best, which = d0.min(-1), d0.argmin(-1)[..., None]
    hit = np.isfinite(best)
    stable = np.where(hit, np.take_along_axis(s0, which, -1)[..., 0] > MIN_INCIDENCE, True)
    clear_miss, clear_hit = ~hit, hit & (best < rng - CLEAR)
    for c in _combos(3):
        d, _ = _beams_vs_lines(pos + c[:2] * POS_EPS, head[:, None] + c[2] * ANG_EPS + rel[None], lines, rng)
        dn = np.take_along_axis(d, which, -1)[..., 0]
        stable &= np.where(hit, np.isfinite(dn) & (dn <= d.min(-1) + 1e-9), ~np.isfinite(d.min(-1)))
    for sh in ((CLEAR, 0.0), (-CLEAR, 0.0), (0.0, CLEAR), (0.0, -CLEAR)):      # 1 cm either way, with a range 1 cm longer
        dd = _beams_vs_lines(pos + np.array(sh), head[:, None] + rel[None], lines, rng + CLEAR)[0].min(-1)
        clear_miss &= ~np.isfinite(dd)
        clear_hit &= np.isfinite(dd)
    return np.minimum(best, rng) / rng, hit, stable, clear_miss, clear_hit


# ---------------------------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------------------------
def lidar_rel_angles(cfg):
    """Beam k is turned k * 360 / L degrees CLOCKWISE of the heading (SPEC 3.4)."""
    return -2.0 * math.pi * np.arange(cfg.num_lasers) / cfg.num_lasers


def step_truth(cfg, tables, st, lidar=True, detectors=True):
    """What one step at rest decides and reports.  st: raw state words [16][E][N] float32.  Arrays are [E][N] (+ beams):
    acted, solid, crash_gap (smallest signed gap to another solid slot or a building; < 0 = crash), out_margin, long_margin, lane,
    lane_margin, road, prog, total, heading, side [E][N][2 or side beams], lane_col [E][N][1 or lane-line beams] with their *_hit / *_stable /
    *_clear_miss / *_clear_hit masks where they are beams, lidar [E][N][L] with lidar_hit / _stable / _clear_miss / _clear_hit."""
    st = np.asarray(st, np.float32)
    E, N = st.shape[1:]
    X, Y, TH = (st[k].astype(np.float64) for k in (0, 1, 2))
    words = st[13].view(np.int32)
    status, timer = words & 0xFF, (words >> 8) & 0xFF
    routes = st[12].view(np.int32)
    acted = status == ALIVE
    # (0) wreck timers tick first: a wreck lingers through the step when its timer outlasts the tick
    solid = acted | ((status == WRECK) & (timer > 1))
    assert cfg.delay_done > 0, "a vehicle that ends in this step stays as an obstacle"
    hl, hw, w = float(cfg.veh_half_len), float(cfg.veh_half_wid), float(cfg.lane_width)
    boxes = np.zeros((0, 6)) if (not cfg.toll_buildings or tables.boxes is None) else np.asarray(tables.boxes, np.float64)
    box_ang = np.arctan2(boxes[:, 3], boxes[:, 2])
    seen = boxes if int(cfg.toll_buildings) == 1 else boxes[:0]
    nside, nlane = int(cfg.side_lasers), int(cfg.lane_line_lasers)
    T = dict(acted=acted, solid=solid, crash_gap=np.full((E, N), np.inf), out_margin=np.full((E, N), np.nan),
             long_margin=np.full((E, N), np.inf), lane=np.zeros((E, N), int), lane_margin=np.full((E, N), np.inf),
             road=np.zeros((E, N), int), heading=np.zeros((E, N)), lat=np.zeros((E, N)), lanes=np.zeros((E, N)), prog=np.zeros((E, N)), total=np.ones((E, N)),
             side=np.zeros((E, N, nside or 2)), lane_col=np.zeros((E, N, nlane or 1)))
    for e in range(E):
        for i in np.nonzero(acted[e])[0]:
            me = ((X[e, i], Y[e, i]), TH[e, i], hl, hw)
            gaps = [box_gap(me, ((X[e, j], Y[e, j]), TH[e, j], hl, hw)) for j in np.nonzero(solid[e])[0] if j != i]
            gaps += [box_gap(me, ((b[0], b[1]), a, b[4], b[5])) for b, a in zip(boxes, box_ang)]
            T["crash_gap"][e, i] = min(gaps, default=np.inf)
            r = road_decisions(cfg, tables, int(routes[e, i]) & 0xFFFF, int(routes[e, i]) >> 16, X[e, i], Y[e, i], TH[e, i])
            for k in ("out_margin", "long_margin", "lane", "lane_margin", "road", "lat", "lanes", "prog", "total"):
                T[k][e, i] = r[k]
            T["heading"][e, i] = 0.5 - 0.5 * math.sin(r["psi"])
            if not nside:
                width = (r["lanes"] + 1) * w
                T["side"][e, i] = np.clip([(0.5 * w - r["lat"]) / width, ((r["lanes"] - 0.5) * w + r["lat"]) / width], 0.0, 1.0)
            if not nlane:
                T["lane_col"][e, i, 0] = np.clip(-(r["lat"] + r["lane"] * w) / 4.5 + 0.5, 0.0, 1.0)
    lines = np.asarray(tables.lines, np.float64)
    for name, n, kind, rng in (("side", nside, 2.0, cfg.side_range), ("lane_col", nlane, 1.0, cfg.lane_line_range)):
        if n and detectors:
            parts = [detector(np.stack([X[e], Y[e]], -1), TH[e], n, lines, kind, float(rng)) for e in range(E)]
            for k, tag in enumerate(("", "_hit", "_stable", "_clear_miss", "_clear_hit")):
                T[name + tag] = np.stack([p[k] for p in parts])
    if lidar:
        rel = lidar_rel_angles(cfg)
        parts = []
        for e in range(E):
            M = N + len(seen)
            tp = np.concatenate([np.stack([X[e], Y[e]], -1), seen[:, :2]])
            ta = np.concatenate([TH[e], box_ang[:len(seen)]])
            mask = np.concatenate([solid[e][None, :] & ~np.eye(N, dtype=bool), np.ones((N, M - N), bool)], 1)
            parts.append(_beams_vs_boxes(np.stack([X[e], Y[e]], -1), TH[e], rel, tp, ta,
                                         np.concatenate([np.full(N, hl), seen[:, 4]]), np.concatenate([np.full(N, hw), seen[:, 5]]),
                                         mask, np.arange(M) < N, float(cfg.lidar_range)))
        for k, tag in enumerate(("", "_hit", "_stable", "_clear_miss", "_clear_hit")):
            T["lidar" + tag] = np.stack([p[k] for p in parts])
    return T


def obs_columns(cfg):
    """Columns of the observation row: dict(side, heading, lane, lidar) -> first column (SPEC 3.4: [side | 6 state | lane | navigation |
    LiDAR | ...])."""
    side = int(cfg.side_lasers) or 2
    lane = side + 6
    return dict(side=0, heading=side, lane=lane, lidar=lane + (int(cfg.lane_line_lasers) or 1) + int(cfg.navi_dim))
