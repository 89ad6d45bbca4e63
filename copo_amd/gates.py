"""Traffic gates: how much traffic gets through, and how fast (host side of `copo_gate_*`).

A gate is a directed line segment A -> B in world coordinates.  `TrafficGates` owns one `copo_gate` handle over a `VecSim`; `record()`
decides on the GPU, for every slot of every scene, whether the same agent moved across each gate since the previous record, and adds the
crossings into int64 accumulators per gate and scene group: counts and quantised speeds forward / backward, the counts again in time
bins, headways between successive forward crossings of one scene, and travel times of sections (an entry gate followed by an exit gate
by the same agent).  Every accumulator is an integer, so the result does not depend on the order the device adds in and is compared
exactly.  `read()` turns them into numpy arrays with flow per hour, mean speed, mean travel time and density; `save` / `load` keep them in
one `.npz`; `gate_overlay` draws the gates into a frame of the top-down renderer.  The definitions are DESIGN.md section 8f;
`tests/gate_numpy.py` restates them.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from ._abi import (GATE_MAX_BINS as MAX_BINS, GATE_MAX_GATES as MAX_GATES, GATE_MAX_GROUPS as MAX_GROUPS, GATE_MAX_HIST as MAX_HIST,
                   GATE_MAX_SECTIONS as MAX_SECTIONS)
from . import _npz
from ._handle import Grouped, Handle

QUANT = 256
RAW = ("count", "speed_q", "series", "headway", "sec_count", "sec_sum", "sec_hist", "scene_records", "alive")
DERIVED = ("flow_per_hour", "mean_speed", "headway_s", "mean_travel_s", "density")
GATE_COLOUR, TICK_COLOUR = (255, 0, 255), (255, 255, 0)


def shapes(G, L, S, T, HB, TB):
    """name -> shape of the accumulators, in the order they lie in the handle's block (`copo_gate_read`)"""
    return dict(count=(G, L, 2), speed_q=(G, L, 2), series=(G, L, 2, T), headway=(G, L, HB), sec_count=(G, S), sec_sum=(G, S),
                sec_hist=(G, S, TB), scene_records=(G,), alive=(G,))


def split(block, G, L, S, T, HB, TB):
    """The accumulator block (1-D, numpy or torch) as a dict of views by name."""
    out, at = {}, 0
    for k, shp in shapes(G, L, S, T, HB, TB).items():
        n = int(np.prod(shp))
        out[k] = block[at:at + n].reshape(shp)
        at += n
    assert at == block.shape[0], (at, block.shape)
    return out


def derive(raw, dt):
    """The dict of `TrafficGates.read()` from the int64 accumulators and the seconds per record `dt`: the raw arrays and float64
    `flow_per_hour` [G, L, 2] = count / (scene_records x dt) x 3600 (vehicles per hour and scene; NaN for a group that received no
    record), `mean_speed` [G, L, 2] = speed_q / 256 / count (m/s, NaN where nothing crossed), `headway_s` [HB] = the headway of each bin
    in seconds (the last bin also holds everything longer), `mean_travel_s` [G, S] = sec_sum / sec_count x dt (NaN where no section
    completed) and `density` [G] = alive / scene_records (vehicles per scene)."""
    out = {k: np.asarray(raw[k], np.int64) for k in RAW}
    rec = out["scene_records"].astype(np.float64)
    cnt = out["count"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["flow_per_hour"] = np.where(rec[:, None, None] > 0, cnt / (rec[:, None, None] * float(dt)) * 3600.0, np.nan)
        out["mean_speed"] = np.where(cnt > 0, out["speed_q"] / float(QUANT) / cnt, np.nan)
        out["headway_s"] = np.arange(out["headway"].shape[2], dtype=np.float64) * float(dt)
        out["mean_travel_s"] = np.where(out["sec_count"] > 0, out["sec_sum"] / out["sec_count"].astype(np.float64) * float(dt), np.nan)
        out["density"] = np.where(rec > 0, out["alive"] / rec, np.nan)
    return out


def save(path, data):
    """One `.npz` without pickled objects (`np.load(path, allow_pickle=False)` reads it) of a `read()` dict: the integer accumulators
    and `meta` as JSON (gates, sections, bins and the `SimConfig` fields that rebuild the map)."""
    return _npz.save(path, data["meta"], **{k: np.asarray(data[k], np.int64) for k in RAW})


def load(path):
    """The `read()` dict of a file written by `save`."""
    *raw, meta = _npz.load(path, *RAW)
    return dict(derive(dict(zip(RAW, raw)), meta["dt"]), meta=meta)


def route_pose(tables, route, s):
    """((x, y, heading) of the route's lane-0 line at arc length `s`, lanes of the road there), float64, from the road records with the
    primitives `maps.route_points` walks them with."""
    from . import maps as M
    nseg = int(tables.route_meta[route, 1])
    for k in range(nseg):
        rec = tables.route_segs[route, k].astype(np.float64)
        if s < rec[M.SEG_S0] + rec[M.SEG_LEN] or k == nseg - 1:
            pose = M.advance((rec[M.SEG_X0], rec[M.SEG_Y0], rec[M.SEG_TH0]), s - rec[M.SEG_S0], rec[M.SEG_KAPPA])
            return pose, int(math.floor(rec[M.SEG_LANES]))
    raise ValueError("route %d has no road" % route)


def side(gate, p):
    """float64 side of the point(s) `p` [..., 2] of a gate {ax, ay, bx, by}: negative before a forward crossing"""
    ax, ay, bx, by = (float(v) for v in gate)
    p = np.asarray(p, np.float64)
    return (bx - ax) * (p[..., 1] - ay) - (by - ay) * (p[..., 0] - ax)


def gates_for_map(tables, inset=10.0, margin=0.5, merge=0.01):
    """(gates float32 [L, 4], sections [(gate_in, gate_out)], route_section [R]) of a map's road tables.  Per route one entry gate at arc
    length `inset` and one exit gate at total length - `inset`, perpendicular to the route there, from `margin` metres left of lane 0's
    left edge to `margin` metres right of the last lane's right edge (lanes x lane width of the road record), oriented so that driving
    along the route is FORWARD (the points of `maps.route_points` before the gate have side < 0); gates whose endpoints agree to `merge`
    metres are one gate; one section per (entry gate, exit gate) pair that some route connects; route_section[r] is the route's."""
    from . import maps as M
    gates, sections, route_section = [], [], []
    w = float(tables.lane_width)

    def gate_at(route, s):
        pose, lanes = route_pose(tables, route, s)
        a, b = M.shift(pose, 0.5 * w + margin), M.shift(pose, -((lanes - 0.5) * w + margin))
        g = np.array([a[0], a[1], b[0], b[1]], np.float32)
        pts = M.route_points(tables, route, step=1.0)
        # (the polyline restarts its 1 m steps at every road: take the points by distance to the gate, not by index)
        near = pts[np.hypot(pts[:, 0] - pose[0], pts[:, 1] - pose[1]) < 5.0]
        ahead = (near[:, 0] - pose[0]) * math.cos(pose[2]) + (near[:, 1] - pose[1]) * math.sin(pose[2])
        sd = side(g, near)
        if (sd[ahead < -0.5] >= 0).any() or (sd[ahead > 0.5] < 0).any():
            g = g[[2, 3, 0, 1]]
        for i, q in enumerate(gates):
            if np.abs(q.astype(np.float64) - g.astype(np.float64)).max() <= merge:
                return i
        gates.append(g)
        return len(gates) - 1

    for r in range(tables.n_routes):
        total = float(tables.route_meta[r, 0])
        if not total > 2.0 * inset:
            raise ValueError("route %d is %.1f m long: no room for gates %.1f m from its ends" % (r, total, inset))
        pair = (gate_at(r, inset), gate_at(r, total - inset))
        if pair not in sections:
            sections.append(pair)
        route_section.append(sections.index(pair))
    if len(gates) > MAX_GATES or len(sections) > MAX_SECTIONS:
        raise ValueError("%d gates and %d sections on this map (at most %d and %d): pass gates and sections by hand"
                         % (len(gates), len(sections), MAX_GATES, MAX_SECTIONS))
    return np.stack(gates), sections, route_section


def gate_overlay(frame_rgb, view, gates, colour=GATE_COLOUR, tick=TICK_COLOUR, tick_m=2.0):
    """Draw `gates` [L, 4] into a renderer frame uint8 [h, w, 3|4] drawn with `view` = (cx, cy, metres per pixel): the world point (x, y)
    lies in pixel column floor((x - cx) / m + w / 2) and row floor((cy - y) / m + h / 2) (section 8's mapping: pixel (i, j) has the
    centre (cx + (j + 0.5 - w / 2) m, cy - (i + 0.5 - h / 2) m)).  Each gate is a line in `colour`, sampled every half pixel, with a tick
    of `tick_m` metres in `tick` from its middle towards the FORWARD side.  Returns a new uint8 array [h, w, 3]."""
    frame = np.asarray(frame_rgb)
    assert frame.ndim == 3 and frame.shape[2] in (3, 4) and frame.dtype == np.uint8, (frame.shape, frame.dtype)
    out = np.ascontiguousarray(frame[..., :3]).copy()
    h, w = out.shape[:2]
    cx, cy, m = (float(v) for v in view)

    def line(x0, y0, x1, y1, col):
        n = int(math.ceil(math.hypot(x1 - x0, y1 - y0) / (0.5 * m))) + 1
        t = np.linspace(0.0, 1.0, n)
        j = np.floor((x0 + (x1 - x0) * t - cx) / m + 0.5 * w).astype(np.int64)
        i = np.floor((cy - (y0 + (y1 - y0) * t)) / m + 0.5 * h).astype(np.int64)
        ok = (i >= 0) & (i < h) & (j >= 0) & (j < w)
        out[i[ok], j[ok]] = col
    for ax, ay, bx, by in np.asarray(gates, np.float64).reshape(-1, 4):
        line(ax, ay, bx, by, colour)
        d = math.hypot(bx - ax, by - ay)
        # forward = towards side >= 0 = to the left of A -> B
        nx, ny = -(by - ay) / d, (bx - ax) / d
        mx, my = 0.5 * (ax + bx), 0.5 * (ay + by)
        line(mx, my, mx + nx * tick_m, my + ny * tick_m, tick)
    return out


class TrafficGates(Grouped, Handle):
    """Gates of a `VecSim`: `gates` [L, 4] = {ax, ay, bx, by} (1..32), `sections` = pairs (gate_in, gate_out) (0..64), `groups` scene
    groups (`set_groups`: scene e adds to group[e], a value outside 0..groups-1 to nothing; all 0 at first), `bins` = (T, records per
    bin) of the time series, `headway_bins` bins of one record each, `tt_bins` = (TB, records per bin) of the travel times; the last bin
    of each holds everything beyond.  Records count from 0 since creation / `reset()`.  `close()` it when done (before or after its
    simulator; no other call once the simulator is closed); every call is asynchronous on torch's current stream except `read()` /
    `save()`."""

    _prefix = "copo_gate_"

    def __init__(self, sim, gates, sections=(), groups=1, bins=(1, 1), headway_bins=32, tt_bins=(32, 10)):
        self._attach(sim)
        self.gates = np.ascontiguousarray(np.asarray(gates, np.float32).reshape(-1, 4))
        self.sections = [(int(a), int(b)) for a, b in sections]
        self.groups = int(groups)
        (self.T, self.bin_records), self.HB, (self.TB, self.tt_bin) = (int(v) for v in bins), int(headway_bins), (int(v) for v in tt_bins)
        self.L, self.S = int(self.gates.shape[0]), len(self.sections)
        cfg = self._capi.GateCfg(self.L, self.S, self.groups, self.T, self.bin_records, self.HB, self.TB, self.tt_bin)
        sec = np.ascontiguousarray(np.asarray(self.sections, np.int32).reshape(-1, 2))
        self._create(self._capi.lib.copo_gate_create, sim._h, C.byref(cfg), self.gates.ctypes.data, sec.ctypes.data if self.S else None)
        self._words = int(self._capi.lib.copo_gate_words(C.byref(cfg)))
        self.n_records = 0
        self.route_section = None

    @classmethod
    def for_map(cls, sim, inset=10.0, **kwargs):
        """An entry and an exit gate per route of the simulator's map, `inset` metres from its ends, and the sections between them
        (`gates_for_map`); `route_section[r]` names the section of route r."""
        gates, sections, route_section = gates_for_map(sim.tables, inset)
        self = cls(sim, gates, sections, **kwargs)
        self.route_section = route_section
        return self

    @classmethod
    def from_env(cls, sim, value):
        """The env's gates (config key `traffic_gates`: None, or the arguments of `TrafficGates` -- with `gates` explicit gates, else
        `for_map`)."""
        kwargs = dict(value)
        return cls(sim, **kwargs) if "gates" in kwargs else cls.for_map(sim, **kwargs)

    def env_record(self, feed):
        """One record after every step; after a reset by hand the memory is forgotten first, so that the reset fires nothing.  The
        accumulators are kept over resets."""
        if feed.after_reset:
            self.forget()
        self.record()

    dims =property(lambda self: (self.groups, self.L, self.S, self.T, self.HB, self.TB))

    def record(self):
        """One record of the current state (it reads simulator state only)."""
        self._capi.check(self._capi.lib.copo_gate_record(self._h, self._stream()))
        self.n_records += 1

    def forget(self):
        """Forget every slot, last forward crossing and section entry (after a manual `reset()` / `set_state`): the next record fires
        nothing."""
        self._call("forget")

    def reset(self):
        """`forget()`, zero the accumulators; records count from 0 again.  The groups stay."""
        self._call("reset")
        self.n_records = 0

    def counters(self):
        """dict of device int64 tensors by name (`RAW`), views of one copy of the accumulators"""
        torch = self.sim._torch
        block = torch.empty(self._words, dtype=torch.int64, device=self.sim.device)
        self._call("read", block.data_ptr(), None)
        return split(block, *self.dims)

    def meta(self):
        cfg = self.sim.cfg
        return dict(gates=[[float(v) for v in g] for g in self.gates], sections=[list(s) for s in self.sections], groups=self.groups,
                    bins=[self.T, self.bin_records], headway_bins=self.HB, tt_bins=[self.TB, self.tt_bin], route_section=self.route_section,
                    n_records=self.n_records, dt=float(cfg.dt), num_agents=int(self.sim.N), sim_config=dataclasses.asdict(cfg))

    def read(self):
        """numpy dict: the accumulators by name (int64), the derived float64 arrays of `derive`, and `meta`."""
        out = derive({k: v.cpu().numpy() for k, v in self.counters().items()}, self.sim.cfg.dt)
        out["meta"] = self.meta()
        return out

    def save(self, path):
        return save(path, self.read())

    load = staticmethod(load)

    def gate_overlay(self, frame_rgb, view):
        return gate_overlay(frame_rgb, view, self.gates)

    def table(self, data=None, group=0):
        """The per-gate and per-section table of `vis --gates` as text."""
        d = self.read() if data is None else data
        rows = ["gate  A -> B                                forward  backward  veh/h fwd  mean speed fwd (m/s)"]
        for l, q in enumerate(self.gates):
            rows.append("%4d  (%7.1f, %7.1f) -> (%7.1f, %7.1f)  %7d  %8d  %9.1f  %8.2f" % (
                l, q[0], q[1], q[2], q[3], d["count"][group, l, 0], d["count"][group, l, 1], d["flow_per_hour"][group, l, 0],
                d["mean_speed"][group, l, 0]))
        rows.append("section  in -> out  completed  mean travel time (s)")
        for s, (a, b) in enumerate(self.sections):
            rows.append("%7d  %2d -> %2d  %9d  %8.2f" % (s, a, b, d["sec_count"][group, s], d["mean_travel_s"][group, s]))
        rows.append("density %.2f vehicles per scene over %d scene-records" % (d["density"][group], d["scene_records"][group]))
        return "\n".join(rows)
