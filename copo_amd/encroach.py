"""Encroachment log: post-encroachment times from a device grid (host side of `copo_pet_*`); no counterpart in the reference.

`EncroachmentLog` owns one `copo_pet` handle over a `VecSim`.  Every scene owns a grid of `W` x `H` cells of `cell` metres; each cell
holds one 64-bit stamp: which driving agent's footprint covered it last, and in which record.  `record()` finds, on the GPU, the foreign
stamps under every ALIVE agent's footprint; the first record in which agent b touches stamps of agent a commits ONE row of 16 words -- the
encounter's PET, the time between a's body leaving a piece of road and b's body entering it -- into a pool of `max_rows`, in (scene,
slot_b, slot_a) order, and adds to an integer histogram (type x PET) and a map of critical encounters per scene group, without allocation
or host synchronisation.  `table()` reads the pool out as an `EncroachmentTable` (numpy only; `save` / `load` one `.npz`), `read()` the
aggregates.  The rules are DESIGN.md section 8i; `tests/pet_numpy.py` restates them.

Memory: 8 B per cell and scene dominate -- a 150 x 150 m map at 1 m is 180 KB per scene, 46 MB at 256 scenes, 2.9 GB at 16 384 scenes --
plus 20 B per slot, 16 B per scene, 8 B per histogram bin and map cell of a group and 64 B per pool row (`EncroachmentLog.state_bytes`).
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _npz, fields      # noqa: F401 (a public name: `encroach.fields`)
from ._abi import FIELD_MAX_GROUPS as MAX_GROUPS, PET_MAX_WINDOW as MAX_WINDOW, PET_WORDS as WORDS      # noqa: F401
from ._grid import SceneGrid
from ._handle import Grouped
from ._rowlog import RowLog, RowTable

ROW_KEYS = ("scene", "pair", "aid_b", "aid_a", "episode", "rec", "pet", "cell", "n_cells", "speed_a", "x_b", "y_b", "heading_b", "speed_b", "hq_a", "hq_b")
RAW = ("scene", "slot_b", "slot_a", "aid_b", "aid_a", "episode", "rec", "pet", "cell", "n_cells", "hq_a", "hq_b")
DERIVED = ("pet_s", "speed_a", "speed_b")
TYPES = ("following", "crossing", "opposing")
FOLLOW_Q, OPPOSE_Q = 21, 107                    # of 256 heading steps per turn: `ConflictTable`'s 30 / 150 degrees, quantised
BANDS = ((0.0, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, float("inf")))      # seconds, [lo, hi)


def max_cell(hw):
    """The widest cell a body of half width `hw` cannot pass between the centres of: 2 hw / sqrt(2)."""
    return 2.0 * float(hw) / math.sqrt(2.0)


def type_index(hq_a, hq_b):
    """0 following / 1 crossing / 2 opposing from the quantised headings: d = min(rel, 256 - rel), rel = (hq_b - hq_a) & 255."""
    rel = (np.asarray(hq_b, np.int64) - np.asarray(hq_a, np.int64)) & 255
    d = np.minimum(rel, 256 - rel)
    return np.where(d <= FOLLOW_Q, 0, np.where(d >= OPPOSE_Q, 2, 1))


def decode(raw, dt, grid):
    """dict of columns of the rows `raw` (anything numpy reads as [n, 16] 32-bit words), the seconds per record `dt` and `grid` = (x0, y0,
    cell, W).  Integer columns `RAW` (int64): b is the agent that entered (`second`), a the one that had left (`first`); `rec` the record
    of the encounter, `pet` in records, `cell` = iy * W + ix of the lowest cell that attains it.  float64: `pet_s` = pet x dt, `speed_a`,
    `speed_b`, `pose_b` [n, 4] {x, y, heading, speed} at `rec`, `cell_xy` [n, 2] the centre of `cell`; `type` by `type_index`;
    `second` / `first` int64 [n, 3]: (scene, aid, episode) of b and of a -- the key of a `TripTable` row."""
    w = np.ascontiguousarray(np.asarray(raw).reshape(-1, WORDS)).view(np.uint32)
    i64 = lambda k: w[:, k].astype(np.int64)                                # noqa: E731
    s32 = lambda k: w[:, k].copy().view(np.int32).astype(np.int64)          # noqa: E731
    f64 = lambda k: w[:, k].copy().view(np.float32).astype(np.float64)      # noqa: E731
    x0, y0, cell, W = float(grid[0]), float(grid[1]), float(grid[2]), int(grid[3])
    pk = i64(1)
    out = dict(scene=i64(0), slot_b=pk & 63, slot_a=(pk >> 6) & 63, aid_b=s32(2), aid_a=s32(3), episode=s32(4), rec=i64(5), pet=i64(6), cell=i64(7),
               n_cells=i64(8), hq_a=i64(14), hq_b=i64(15))
    out["pet_s"] = out["pet"].astype(np.float64) * float(dt)
    out["speed_a"], out["speed_b"] = f64(9), f64(13)
    out["pose_b"] = np.ascontiguousarray(w[:, 10:14]).view(np.float32).astype(np.float64)
    out["cell_xy"] = np.stack([x0 + (out["cell"] % W + 0.5) * cell, y0 + (out["cell"] // W + 0.5) * cell], -1)
    out["type"] = np.array(TYPES, dtype="<U9")[type_index(out["hq_a"], out["hq_b"])] if len(w) else np.zeros(0, "<U9")
    out["second"] = np.stack([out["scene"], out["aid_b"], out["episode"]], -1)
    out["first"] = np.stack([out["scene"], out["aid_a"], out["episode"]], -1)
    return out


class EncroachmentTable(RowTable):
    """Encounters as numpy: `raw` uint32 [n, 16] (the rows as the device wrote them, columns `ROW_KEYS`), `meta` (dict: `dt`, `x0`, `y0`,
    `cell`, `W`, `H`, `window`, `critical_records`, `num_agents`, `max_rows`, `dropped`, `n_records`, `sim_config`), and the columns of
    `decode` as attributes / items."""

    @staticmethod
    def _decode(raw, meta):
        return decode(raw, meta["dt"], (meta["x0"], meta["y0"], meta["cell"], meta["W"]))

    def frame(self):
        """pandas DataFrame of every scalar column."""
        import pandas as pd
        return pd.DataFrame({k: self.columns[k] for k in RAW + ("type",) + DERIVED})

    def of(self, scene, aid, episode):
        """Indices of the rows where agent `aid` of `scene` in `episode` is a party (a `TripTable` row's scene / aid / episode)."""
        c = self.columns
        return np.nonzero((c["scene"] == int(scene)) & (c["episode"] == int(episode)) & ((c["aid_a"] == int(aid)) | (c["aid_b"] == int(aid))))[0]

    def summary(self):
        """Buckets of the rows by type and PET band (`BANDS`, seconds, [lo, hi)): list of dicts with `type`, `band`, `count`, `share` and
        the mean `pet_s`, `speed_a`, `speed_b` of the bucket (empty buckets are left out)."""
        c, out = self.columns, []
        for key in TYPES:
            for lo, hi in BANDS:
                m = (c["type"] == key) & (c["pet_s"] >= lo) & (c["pet_s"] < hi)
                n = int(m.sum())
                if n:
                    out.append(dict(type=key, band=(lo, hi), count=n, share=n / len(self), **{k: float(c[k][m].mean()) for k in DERIVED}))
        return out

    def text(self):
        """`summary()` as a table of text."""
        rows = ["%-10s %-12s %6s %7s %8s %9s %9s" % ("type", "PET s", "count", "share", "PET s", "first m/s", "second m/s")]
        for r in self.summary():
            rows.append("%-10s %-12s %6d %7.3f %8.2f %9.2f %9.2f" % (r["type"], "%g .. %g" % r["band"], r["count"], r["share"], r["pet_s"], r["speed_a"],
                                                                      r["speed_b"]))
        return "\n".join(rows)

    def join(self, trips):
        """Joins both parties with the `TripTable` `trips` on (scene, aid, episode): dict with `second` and `first`, int64 [n]: the index
        of b's and of a's row in `trips`, -1 where the trip is not in the table, and `missing`, how many are not."""
        t = trips.columns
        at = {k: i for i, k in enumerate(zip(t["scene"].tolist(), t["aid"].tolist(), t["episode"].tolist()))}
        out = {k: np.array([at.get(tuple(key), -1) for key in self.columns[k].tolist()], np.int64).reshape(-1) for k in ("second", "first")}
        out["missing"] = int((out["second"] < 0).sum() + (out["first"] < 0).sum())
        return out


def derive(hist, critical, dt):
    """The dict of `EncroachmentLog.aggregates()` from int64 hist [G, 3, window] and critical [G, H, W]: both arrays, `pet_s` [window] =
    (bin + 1) x dt, `count` [G, 3] and `critical_frac` [G, 3]: the share of a type's encounters with pet <= critical_records -- that needs
    `critical_records`, so it is filled in by the caller's `meta` (see `aggregates_dict`)."""
    hist, critical = np.asarray(hist, np.int64), np.asarray(critical, np.int64)
    assert hist.ndim == 3 and hist.shape[1] == len(TYPES) and critical.ndim == 3 and critical.shape[0] == hist.shape[0], (hist.shape, critical.shape)
    return dict(hist=hist, critical=critical, pet_s=(np.arange(hist.shape[2]) + 1) * float(dt), count=hist.sum(-1))


def aggregates_dict(hist, critical, meta):
    out = derive(hist, critical, meta["dt"])
    k = min(int(meta["critical_records"]), out["hist"].shape[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["critical_frac"] = np.where(out["count"] > 0, out["hist"][:, :, :k].sum(-1) / out["count"].astype(np.float64), np.nan)
    out["meta"] = dict(meta)
    return out


def save(path, data):
    """One `.npz` without pickled objects of an `aggregates()` dict: `hist`, `critical` and `meta` as JSON."""
    return _npz.save(path, data["meta"], hist=np.asarray(data["hist"], np.int64), critical=np.asarray(data["critical"], np.int64))


def load(path):
    """The `aggregates()` dict of a file written by `save`."""
    return aggregates_dict(*_npz.load(path, "hist", "critical"))


def pet_meta(cfg, N, grid, window, critical_records, groups, max_rows, dropped=0, n_records=0):
    """`EncroachmentTable.meta` of a log over a simulator of `SimConfig` `cfg` with `N` slots; `grid` = (x0, y0, cell, W, H)."""
    x0, y0, cell, W, H = grid
    return dict(dt=float(cfg.dt), x0=float(x0), y0=float(y0), cell=float(cell), W=int(W), H=int(H), window=int(window),
                critical_records=int(critical_records), groups=int(groups), num_agents=int(N), max_rows=int(max_rows), dropped=int(dropped),
                n_records=int(n_records), sim_config=dataclasses.asdict(cfg))


def state_bytes(E, N, W, H, window, groups, max_rows):
    """Device memory of a log: 8 B per cell and scene, 20 B per slot, 16 B per scene, 8 B per histogram bin and map cell of a group, 64 B
    per pool row and the two counters."""
    return 8 * E * W * H + 20 * E * N + 16 * E + 8 * int(groups) * (3 * int(window) + W * H) + 64 * int(max_rows) + 16


class EncroachmentLog(SceneGrid, Grouped, RowLog):
    """PET rows and aggregates of a `VecSim` on a grid of `W` x `H` cells of `cell` metres with the origin (`x0`, `y0`) per scene: a stamp
    stays valid for `window` records; encounters with a PET of at most `critical_s` seconds (rounded to records) count in the critical map;
    `groups` scene groups (`set_groups`: scene e adds to the aggregates of group[e], a value outside 0..groups-1 to none; all 0 at first);
    a pool of `max_rows` rows (later ones are counted as dropped, and still count in the aggregates).  `cell` must not exceed 2 hw /
    sqrt(2) (`max_cell`).  Records count from 0 since creation / `reset()`.  `close()` it when done (before or after its simulator; no
    other call once the simulator is closed); every call is asynchronous on torch's current stream except `count()` and what reads to the
    host (`table()`, `drain()`, `aggregates()`, `memory()`)."""

    _prefix, _table_cls = "copo_pet_", EncroachmentTable

    def __init__(self, sim, x0, y0, W, H, cell=1.0, window=50, critical_s=1.0, groups=1, max_rows=65536):
        self._attach(sim)
        self._set_grid(x0, y0, W, H, cell)
        self.groups, self.window, self.max_rows = int(groups), int(window), int(max_rows)
        self.critical_s = float(critical_s)
        self.critical_records = int(math.floor(self.critical_s / float(sim.cfg.dt) + 0.5))
        cfg = self._capi.PetCfg(self.x0, self.y0, self.cell, self.W, self.H, self.groups, self.window, self.critical_records, self.max_rows)
        self._create(self._capi.lib.copo_pet_create, sim._h, C.byref(cfg))
        self.n_records = 0
        self.state_bytes = state_bytes(sim.E, sim.N, self.W, self.H, self.window, self.groups, self.max_rows)

    def env_record(self, feed):
        """One record of the state after reset and after every step.  After a reset by hand nothing written before may count: `forget()`
        first (a scene's own reset changes its episode word, which the record sees by itself)."""
        if feed.after_reset:
            self.forget()
        self.record()

    def record(self):
        """One record of the current state."""
        self._capi.check(self._capi.lib.copo_pet_record(self._h, self._stream()))
        self.n_records += 1

    def forget(self):
        """Void every stamp written so far and clear the `met` masks (after a manual `reset()` / `set_state`)."""
        self._call("forget")

    def flush(self):
        """Nothing: an encounter is one record, so nothing is ever open."""

    def _meta(self, dropped=0):
        return pet_meta(self.sim.cfg, self.sim.N, (self.x0, self.y0, self.cell, self.W, self.H), self.window, self.critical_records, self.groups,
                        self.max_rows, dropped, self.n_records)

    def aggregates(self):
        """numpy dict: `hist` int64 [G, 3, window] (type x PET bin, bin = pet - 1), `critical` int64 [G, H, W], `pet_s` [window] = (bin + 1)
        x dt, `count` [G, 3], `critical_frac` [G, 3] (NaN for a type without encounters) and `meta`."""
        torch = self._torch
        h = torch.empty(self.groups, len(TYPES), self.window, dtype=torch.int64, device=self.device)
        c = torch.empty(self.groups, self.H, self.W, dtype=torch.int64, device=self.device)
        self._call("aggregates", h.data_ptr(), c.data_ptr())
        return aggregates_dict(h.cpu().numpy(), c.cpu().numpy(), self._meta(self.count()[1]))

    read = aggregates

    def memory(self):
        """(stamps uint64 [E, H, W], met masks uint64 [E, N]) as numpy: what the tests compare."""
        torch = self._torch
        g = torch.empty(self.sim.E, self.H, self.W, dtype=torch.int64, device=self.device)
        m = torch.empty(self.sim.E, self.sim.N, dtype=torch.int64, device=self.device)
        self._call("memory", g.data_ptr(), m.data_ptr())
        return g.cpu().numpy().view(np.uint64), m.cpu().numpy().view(np.uint64)

    def save(self, path):
        """The aggregates into one `.npz` (`load` reads it; the rows have their own: `table().save`)."""
        return save(path, self.aggregates())

    load = staticmethod(load)
