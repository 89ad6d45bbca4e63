"""Traffic field maps: where the scenes of a simulator drive, queue, crash and come close (host side of `copo_field_*`).

`FieldMaps` owns one `copo_field` handle over a `VecSim`.  `record()` adds, on the GPU, the current state of every scene to integer grids
of its scene group: footprint counts of driving bodies and wrecks, visits, quantised speed and velocity of the body centres, crash / out /
arrive events at the cell each slot was last seen in, and steps below a time-to-collision threshold.  Every accumulator is an integer, so
the maps do not depend on the order the device adds in and can be compared exactly.  `read()` turns them into numpy arrays with the
derived mean speed, flow and occupancy time; `save` / `load` keep them in one `.npz`; `heat_overlay` blends a layer over a frame of the
top-down renderer.  The definitions are DESIGN.md section 8e; `tests/field_numpy.py` restates them.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _npz
from ._abi import FIELD_MAX_GROUPS as MAX_GROUPS, FIELD_MAX_SIDE as MAX_SIDE
from ._grid import SceneGrid
from ._handle import Grouped, Handle

LAYERS = ("occupancy", "wreck", "visits", "speed_q", "vx_q", "vy_q", "crash", "out", "arrive", "critical")
DERIVED = ("mean_speed", "flow", "occupancy_s", "occupancy_frac")
QUANT = 256
# colour ramp of `heat_overlay`: stops at t = 0, 1/3, 2/3, 1, linear in between
RAMP = np.array([(40, 60, 200), (40, 200, 200), (240, 220, 40), (220, 40, 40)], np.float64)


def grid_for_map(tables, cell=1.0, margin=5.0):
    """(x0, y0, W, H) of the grid of `cell`-metre cells that covers the bounding box of the map's road tables plus `margin` metres."""
    from . import maps as _maps
    xa, xb, ya, yb = _maps.bounding_box(tables)
    x0, y0 = xa - margin, ya - margin
    W, H = int(math.ceil((xb + margin - x0) / cell)), int(math.ceil((yb + margin - y0) / cell))
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError("%d x %d cells of %g m for a map of %.0f x %.0f m: at most %d per side" % (W, H, cell, xb - xa, yb - ya, MAX_SIDE))
    return float(x0), float(y0), W, H


def derive(maps, scene_records, dt):
    """The dict of `FieldMaps.read()` from int64 maps [G, 10, H, W] and scene_records [G]: the layers by name, `scene_records`, and
    float64 `mean_speed` = speed_q / 256 / visits (m/s), `flow` [G, 2, H, W] = (vx_q, vy_q) / 256 / visits (m/s), NaN where nothing
    visited; `occupancy_s` = occupancy x dt (seconds, over all scenes of the group) and `occupancy_frac` = occupancy / scene_records
    (bodies over the cell per scene-record; NaN for a group that received none)."""
    maps = np.asarray(maps, np.int64)
    rec = np.asarray(scene_records, np.int64).reshape(-1)
    assert maps.ndim == 4 and maps.shape[1] == len(LAYERS) and rec.shape == (maps.shape[0],), (maps.shape, rec.shape)
    out = {k: maps[:, i] for i, k in enumerate(LAYERS)}
    out["scene_records"] = rec
    visits = maps[:, 2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        seen = visits > 0
        out["mean_speed"] = np.where(seen, maps[:, 3] / float(QUANT) / visits, np.nan)
        out["flow"] = np.where(seen[:, None], maps[:, 4:6] / float(QUANT) / visits[:, None], np.nan)
        out["occupancy_s"] = maps[:, 0].astype(np.float64) * float(dt)
        out["occupancy_frac"] = np.where(rec[:, None, None] > 0, maps[:, 0] / rec[:, None, None].astype(np.float64), np.nan)
    return out


def save(path, data):
    """One `.npz` without pickled objects (`np.load(path, allow_pickle=False)` reads it) of a `read()` dict: the integer maps,
    `scene_records` and `meta` as JSON (the grid and the `SimConfig` fields that rebuild the map)."""
    maps = np.stack([np.asarray(data[k], np.int64) for k in LAYERS], 1)
    return _npz.save(path, data["meta"], maps=maps, scene_records=np.asarray(data["scene_records"], np.int64))


def load(path):
    """The `read()` dict of a file written by `save`."""
    maps, scene_records, meta = _npz.load(path, "maps", "scene_records")
    return dict(derive(maps, scene_records, meta["dt"]), meta=meta)


def heat_overlay(frame_rgb, layer2d, view, lo=None, hi=None, alpha=160, grid=None):
    """Blend `layer2d` [H, W] of a grid `grid` = (x0, y0, cell) over a renderer frame uint8 [h, w, 3|4] drawn with `view` = (cx, cy,
    metres per pixel): pixel (i, j) is the world point (cx + (j + 0.5 - w / 2) m, cy - (i + 0.5 - h / 2) m) and takes the cell that
    holds it.  A value v gets the colour of `RAMP` at t = (v - lo) / (hi - lo) clipped to [0, 1] (`lo` / `hi` default to the smallest /
    largest non-zero finite value), blended as (below (256 - alpha) + colour alpha) >> 8; pixels outside the grid and cells whose
    value is 0 or NaN are left untouched.  Returns a new uint8 array [h, w, 3]."""
    if grid is None:
        raise ValueError("grid=(x0, y0, cell) of the layer is required")
    x0, y0, cell = (float(v) for v in grid)
    lay = np.asarray(layer2d, np.float64)
    frame = np.asarray(frame_rgb)
    assert lay.ndim == 2 and frame.ndim == 3 and frame.shape[2] in (3, 4) and frame.dtype == np.uint8, (lay.shape, frame.shape, frame.dtype)
    out = np.ascontiguousarray(frame[..., :3]).copy()
    h, w = out.shape[:2]
    cx, cy, m = (float(v) for v in view)
    px = cx + (np.arange(w) + 0.5 - 0.5 * w) * m
    py = cy - (np.arange(h) + 0.5 - 0.5 * h) * m
    ix, iy = np.floor((px - x0) / cell).astype(np.int64), np.floor((py - y0) / cell).astype(np.int64)
    inside = ((iy >= 0) & (iy < lay.shape[0]))[:, None] & ((ix >= 0) & (ix < lay.shape[1]))[None, :]
    val = lay[np.clip(iy, 0, lay.shape[0] - 1)[:, None], np.clip(ix, 0, lay.shape[1] - 1)[None, :]]
    paint = inside & np.isfinite(val) & (val != 0)
    live = lay[np.isfinite(lay) & (lay != 0)]
    if not paint.any() or live.size == 0:
        return out
    lo = float(live.min()) if lo is None else float(lo)
    hi = float(live.max()) if hi is None else float(hi)
    t = np.clip((val[paint] - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.ones(int(paint.sum()))
    s = t * (len(RAMP) - 1)
    k = np.minimum(s.astype(np.int64), len(RAMP) - 2)
    col = np.rint(RAMP[k] + (RAMP[k + 1] - RAMP[k]) * (s - k)[:, None]).astype(np.int64)
    a = int(alpha)
    out[paint] = ((out[paint].astype(np.int64) * (256 - a) + col * a) >> 8).astype(np.uint8)
    return out


class FieldMaps(SceneGrid, Grouped, Handle):
    """Field maps of a `VecSim` on a grid of `W` x `H` cells of `cell` metres with the origin (`x0`, `y0`), for `groups` scene groups
    (`set_groups`: scene e adds to group[e], a value outside 0..groups-1 to nothing; all 0 at first).  `ttc_below` > 0 switches the
    `critical` layer on (it reads the `ttc` handed to `record`).  Record r adds to the state layers iff `r % stride == 0` (records
    count from 0 since creation / `reset()`); events count in every record.  `close()` it when done (before or after its simulator;
    no other call once the simulator is closed); every call is asynchronous on torch's current stream except `read()` / `save()`."""

    _prefix = "copo_field_"

    def __init__(self, sim, x0, y0, W, H, cell=1.0, groups=1, ttc_below=0.0, stride=1):
        self._attach(sim)
        self._set_grid(x0, y0, W, H, cell)
        self.groups = int(groups)
        self.ttc_below, self.stride = float(ttc_below), int(stride)
        if self.stride < 1:
            raise ValueError("stride=%d (>= 1)" % self.stride)
        cfg = self._capi.FieldCfg(self.x0, self.y0, self.cell, self.W, self.H, self.groups, self.ttc_below)
        self._create(self._capi.lib.copo_field_create, sim._h, C.byref(cfg))
        self.n_records = 0

    def env_record(self, feed):
        """One record of the state after reset (no flags: no event) and after every step, fed with the step's flags and, for the
        critical layer, the meter's ttc of that state.  The maps are kept over resets."""
        self.record(flags=feed.flags, ttc=feed.ttc if self.ttc_below > 0.0 else None)

    def record(self, flags=None, ttc=None):
        """One record of the current state.  `flags`: uint8 [E, N], the output of the step that led to this state (None after a reset:
        no event); `ttc`: float32 [E, N], `InteractionMeter.record()`'s, for the `critical` layer."""
        torch = self.sim._torch
        if self.ttc_below > 0.0 and ttc is None and self.n_records % self.stride == 0:
            raise ValueError("ttc_below=%g needs the meter's ttc in every record that accumulates" % self.ttc_below)
        self._capi.check(self._capi.lib.copo_field_record(self._h, self._en_arg(flags, torch.uint8, "flags"), self._en_arg(ttc, torch.float32, "ttc"),
                                                          1 if self.n_records % self.stride == 0 else 0, self._stream()))
        self.n_records += 1

    def forget(self):
        """Forget where every slot was last seen (after a manual `reset()` / `set_state`): the next record fires no event."""
        self._call("forget")

    def reset(self):
        """Zero the maps, forget the last-seen cells; records count from 0 again.  The groups stay."""
        self._call("reset")
        self.n_records = 0

    def maps(self):
        """(maps int64 [G, 10, H, W], scene_records int64 [G]) device tensors, copies of the accumulators; layers in `LAYERS` order."""
        torch = self.sim._torch
        m = torch.empty(self.groups, len(LAYERS), self.H, self.W, dtype=torch.int64, device=self.sim.device)
        r = torch.empty(self.groups, dtype=torch.int64, device=self.sim.device)
        self._call("read", m.data_ptr(), r.data_ptr())
        return m, r

    def meta(self):
        cfg = self.sim.cfg
        return dict(x0=self.x0, y0=self.y0, cell=self.cell, W=self.W, H=self.H, groups=self.groups, ttc_below=self.ttc_below,
                    stride=self.stride, n_records=self.n_records, dt=float(cfg.dt), num_agents=int(self.sim.N),
                    sim_config=dataclasses.asdict(cfg))

    def read(self):
        """numpy dict: the ten layers by name (int64 [G, H, W]), `scene_records`, the derived float64 arrays of `derive`, and `meta`."""
        m, r = self.maps()
        out = derive(m.cpu().numpy(), r.cpu().numpy(), self.sim.cfg.dt)
        out["meta"] = self.meta()
        return out

    def save(self, path):
        return save(path, self.read())

    load = staticmethod(load)
