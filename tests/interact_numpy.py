"""numpy (float64) restatement of the interaction meter's rules (copo_amd/csrc/interact_kernels.hip).

It shares no code with the kernel: bodies are rectangles given by their four corners, the extents r(a) of a body along an axis are
taken from its own axes, every quantity is float64 computed from the simulator's float32 state words.

Next to every measurement it says whether a float32 evaluation may legitimately decide the sample the other way (`ambiguous`):
  * pair: the pair that decides the sample's TTC is grazing -- |t_in - t_out| < 1e-3 s or |TTC - horizon| < 1e-3 s; where the TTC is
    +inf, a grazing pair that has not separated yet (t_out >= 0) decides that; or the two smallest partner TTCs differ by less than
    1e-4 s while only one of those pairs is grazing;
  * threshold: the sample's TTC is within 1e-3 s of `ttc_crit`, its gap within 1e-3 m of `gap_near`, or its deceleration within
    1e-3 x `brake` of `brake`.
`Tracker` follows the per-agent accumulators over a rollout and gives the totals with the ambiguous samples counted out and in.
"""
import numpy as np

ST_EMPTY, ST_ALIVE, ST_WRECK = 0, 1, 2
GRAZE_S, TIE_S, THRESH = 1e-3, 1e-4, 1e-3
COUNT_KEYS = ("agents", "steps", "tet_steps", "near_events", "brake_events", "agents_with_finite_ttc")
SUM_KEYS = ("min_gap", "min_ttc", "tit")
INF = float("inf")


class Params:
    def __init__(self, hl, hw, dt, horizon=6.0, ttc_crit=1.5, gap_near=0.5, brake=4.0):
        # the kernel receives every one of these as a float32
        self.hl, self.hw, self.dt = (float(np.float32(v)) for v in (hl, hw, dt))
        self.horizon, self.ttc_crit, self.gap_near, self.brake = (float(np.float32(v)) for v in (horizon, ttc_crit, gap_near, brake))

    @classmethod
    def of(cls, sim_config, **kw):
        return cls(sim_config.veh_half_len, sim_config.veh_half_wid, sim_config.dt, **kw)


def _corners(x, y, th, hl, hw):
    """[4, 2] corners of a body"""
    u = np.array([np.cos(th), np.sin(th)])
    n = np.array([-u[1], u[0]])
    c = np.array([x, y])
    return np.array([c + a * hl * u + b * hw * n for a in (1.0, -1.0) for b in (1.0, -1.0)])


def _point_to_body(pt, x, y, th, hl, hw):
    u = np.array([np.cos(th), np.sin(th)])
    n = np.array([-u[1], u[0]])
    rel = pt - np.array([x, y])
    return float(np.hypot(max(abs(rel @ u) - hl, 0.0), max(abs(rel @ n) - hw, 0.0)))


def pair(bi, bj, P):
    """(gap, TTC, grazing, t_out) of bodies (x, y, heading, speed -- 0 for a wreck) i and j, float64."""
    xi, yi, thi, vi = (float(v) for v in bi)
    xj, yj, thj, vj = (float(v) for v in bj)
    ui, uj = np.array([np.cos(thi), np.sin(thi)]), np.array([np.cos(thj), np.sin(thj)])
    ni, nj = np.array([-ui[1], ui[0]]), np.array([-uj[1], uj[0]])
    d = np.array([xj - xi, yj - yi])
    w = vj * uj - vi * ui
    overlap, never, t_in, t_out = True, False, -INF, INF
    for a in (ui, ni, uj, nj):
        r = (P.hl * abs(a @ ui) + P.hw * abs(a @ ni)) + (P.hl * abs(a @ uj) + P.hw * abs(a @ nj))
        p, q = float(a @ d), float(a @ w)
        overlap = overlap and abs(p) <= r
        if q == 0.0:
            never = never or abs(p) > r
        else:
            t1, t2 = (-r - p) / q, (r - p) / q
            t_in, t_out = max(t_in, min(t1, t2)), min(t_out, max(t1, t2))
    if overlap:
        gap = 0.0
    else:
        gap = min(min(_point_to_body(c, xj, yj, thj, P.hl, P.hw) for c in _corners(xi, yi, thi, P.hl, P.hw)),
                  min(_point_to_body(c, xi, yi, thi, P.hl, P.hw) for c in _corners(xj, yj, thj, P.hl, P.hw)))
    raw = max(t_in, 0.0) if (not never and t_in <= t_out and t_out >= 0.0) else INF
    ttc = INF if raw > P.horizon else raw
    graze = (not never and np.isfinite(t_in) and np.isfinite(t_out) and abs(t_in - t_out) < GRAZE_S) or \
            (np.isfinite(raw) and abs(raw - P.horizon) < GRAZE_S)
    return gap, ttc, bool(graze), (-INF if never else t_out)


def scene(x, y, th, v, status, P):
    """Per slot of one scene: gap [N], ttc [N] (+inf where the slot is not ALIVE or has no partner), pair-ambiguous [N]."""
    N = len(x)
    gap, ttc, amb = np.full(N, INF), np.full(N, INF), np.zeros(N, bool)
    body = [(float(x[k]), float(y[k]), float(th[k]), float(v[k]) if status[k] == ST_ALIVE else 0.0) for k in range(N)]
    present = [k for k in range(N) if status[k] in (ST_ALIVE, ST_WRECK)]
    cache = {}
    for i in present:
        if status[i] != ST_ALIVE:
            continue
        res = []
        for j in present:
            if j == i:
                continue
            key = (min(i, j), max(i, j))
            if key not in cache:
                cache[key] = pair(body[key[0]], body[key[1]], P)
            res.append(cache[key])
        if not res:
            continue
        gap[i] = min(r[0] for r in res)
        order = sorted(range(len(res)), key=lambda k: res[k][1])
        first = res[order[0]]
        ttc[i] = first[1]
        if np.isfinite(first[1]):
            amb[i] = first[2]
            if len(order) > 1:
                second = res[order[1]]
                if np.isfinite(second[1]) and second[1] - first[1] < TIE_S and first[2] != second[2]:
                    amb[i] = True
        else:
            amb[i] = any(r[2] and r[3] >= 0.0 for r in res)
    return gap, ttc, amb


def measure(st, P):
    """State block [16][E][N] float32 -> gap, ttc (float64 [E][N]), pair-ambiguous and ALIVE masks."""
    si = st.view(np.int32)
    status = si[13] & 0xFF
    E, N = status.shape
    gap, ttc, amb = np.full((E, N), INF), np.full((E, N), INF), np.zeros((E, N), bool)
    for e in range(E):
        gap[e], ttc[e], amb[e] = scene(st[0, e], st[1, e], st[2, e], st[3, e], status[e], P)
    return gap, ttc, amb, status == ST_ALIVE


class _Agent:
    def __init__(self, aid, ep):
        self.aid, self.ep = aid, ep
        self.steps = self.near_events = 0
        self.tet_sure = self.tet_amb_true = self.n_amb = self.n_pair_amb = 0      # critical steps; samples ambiguous for TTC / gap decisions
        self.brake_sure = self.brake_amb_true = self.brake_amb = 0
        self.min_gap = self.min_ttc = self.min_ttc_sure = INF                   # _sure: over the samples that are not pair-ambiguous
        self.tit = 0.0
        self.in_near, self.last_speed = False, None


class Tracker:
    """The per-agent accumulators and scene totals over a sequence of states."""

    def __init__(self, P, E, N):
        self.P, self.E, self.N = P, E, N
        self.open = [[None] * N for _ in range(E)]
        self.closed = [[] for _ in range(E)]
        self.alive_samples = self.ambiguous_samples = 0

    def record(self, st, env):
        """-> gap, ttc, pair-ambiguous, ALIVE masks of this state; the accumulators move on"""
        P = self.P
        gap, ttc, amb_pair, alive = measure(st, P)
        aid = st.view(np.int32)[14]
        speed = st[3].astype(np.float64)
        for e in range(self.E):
            ep = int(env[e, 1])
            for n in range(self.N):
                a = self.open[e][n]
                if a is not None and (not alive[e, n] or a.aid != int(aid[e, n]) or a.ep != ep):
                    self.closed[e].append(a)
                    a = self.open[e][n] = None
                if not alive[e, n]:
                    continue
                amb_brake = False
                if a is None:
                    a = self.open[e][n] = _Agent(int(aid[e, n]), ep)
                else:
                    dec = (a.last_speed - speed[e, n]) / P.dt
                    amb_brake = abs(dec / P.brake - 1.0) < THRESH
                    a.brake_amb += int(amb_brake)
                    a.brake_amb_true += int(amb_brake and dec > P.brake)
                    a.brake_sure += int(not amb_brake and dec > P.brake)
                g, t, pa = gap[e, n], ttc[e, n], bool(amb_pair[e, n])
                amb = pa or abs(t - P.ttc_crit) < THRESH or abs(g - P.gap_near) < THRESH
                self.alive_samples += 1
                self.ambiguous_samples += int(amb or amb_brake)
                a.steps += 1
                a.min_gap, a.min_ttc = min(a.min_gap, g), min(a.min_ttc, t)
                if not pa:
                    a.min_ttc_sure = min(a.min_ttc_sure, t)
                critical = t < P.ttc_crit
                a.n_amb += int(amb)
                a.n_pair_amb += int(pa)
                a.tet_amb_true += int(amb and critical)
                a.tet_sure += int(not amb and critical)
                if critical:
                    a.tit += (P.ttc_crit - t) * P.dt
                near = critical or g < P.gap_near
                a.near_events += int(near and not a.in_near)
                a.in_near = near
                a.last_speed = speed[e, n]
        return gap, ttc, amb_pair, alive

    def totals(self, flush_open=False):
        """dict: counts [E][6] (every sample decided as float64 decides it), lo / hi [E][6] (ambiguous samples counted out / in; a near
        event more or less per ambiguous sample), sums [E][3] added up in slot order, slack [E][3]: the most the ambiguous samples can
        move each sum (a pair-ambiguous sample an agent's minimum TTC by the horizon, an ambiguous sample the TIT by ttc_crit dt)."""
        P = self.P
        counts, lo, hi = (np.zeros((self.E, 6), np.int64) for _ in range(3))
        sums, slack = np.zeros((self.E, 3)), np.zeros((self.E, 3))
        for e in range(self.E):
            for a in list(self.closed[e]) + ([a for a in self.open[e] if a is not None] if flush_open else []):
                finite = bool(np.isfinite(a.min_ttc))
                counts[e] += [1, a.steps, a.tet_sure + a.tet_amb_true, a.near_events, a.brake_sure + a.brake_amb_true, int(finite)]
                lo[e] += [1, a.steps, a.tet_sure, max(a.near_events - a.n_amb, 0), a.brake_sure, int(np.isfinite(a.min_ttc_sure))]
                hi[e] += [1, a.steps, a.tet_sure + a.n_amb, a.near_events + a.n_amb, a.brake_sure + a.brake_amb, int(finite or a.n_pair_amb > 0)]
                sums[e, 0] += a.min_gap
                if finite:
                    sums[e, 1] += a.min_ttc
                sums[e, 2] += a.tit
                slack[e, 1] += P.horizon * (a.n_pair_amb > 0)
                slack[e, 2] += P.ttc_crit * P.dt * a.n_amb
        return dict(counts=counts, lo=lo, hi=hi, sums=sums, slack=slack)
