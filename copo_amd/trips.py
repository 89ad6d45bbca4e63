"""Trip log: one device-written row per finished agent (host side of `copo_trip_*`).

`TripLog` owns one `copo_trip` handle over a `VecSim`.  `record()` follows, on the GPU, every agent from the first record that sees it
ALIVE in its slot to the step that ends it -- steps, quantised speed sum and maximum, stops, the step rewards, the smallest gap and time
to collision it was fed -- and then commits ONE row of 16 words into a pool of `max_rows`, in (scene, slot) order, without allocation or
host synchronisation.  `table()` reads the pool out as a `TripTable` (numpy only; `save` / `load` one `.npz`): the per-agent table that
analyses of a population start from -- success against the agent's LCF, travel time and route completion by route, the distribution of
the minimum TTC, and `of(scene, aid, episode)` for "which agent was that" of a clip header.  The rules are DESIGN.md section 8g;
`tests/trip_numpy.py` restates them.
"""
import ctypes as C
import dataclasses

import numpy as np

from ._abi import TRIP_DONE as KIND_DONE, TRIP_FLUSHED as KIND_FLUSHED, TRIP_VANISHED as KIND_VANISHED, TRIP_WORDS as WORDS
from ._rowlog import RowLog, RowTable

ROW_KEYS = ("scene", "slot_route", "aid", "episode", "first_rec", "steps", "end", "lcf", "prog0", "prog1", "speed_sum", "speed_max", "stops",
            "reward", "min_gap", "min_ttc")
RAW = ("scene", "slot", "route", "aid", "episode", "first_rec", "steps", "flags", "kind")
DERIVED = ("lcf", "distance", "duration_s", "mean_speed", "max_speed", "stop_frac", "reward", "min_gap", "min_ttc")
OUTCOMES = ("arrive", "crash", "out", "maxstep", "vanished", "open")
F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_ENV_RESET = 0x02, 0x04, 0x08, 0x10, 0x20, 0x80
QUANT = 256


def decode(raw, dt):
    """dict of columns of the rows `raw` (anything numpy reads as [n, 16] 32-bit words; the device's and the restatement's alike) and the
    seconds per record `dt`.  Integer columns `RAW` (int64; `flags` is the end byte, `kind` 1 done / 2 vanished / 3 flushed); `outcome`,
    an array of strings: a done trip by the simulator's precedence arrive > out > crash (> maxstep) over the bits of its end byte, a
    vanished trip (and a DONE byte without a cause, which the simulator never writes) "vanished", a flushed one "open"; float64 `lcf`,
    `distance` = float64(prog1) - float64(prog0) metres, `duration_s` = steps x dt, `mean_speed` = speed_sum / 256 / steps,
    `max_speed` = speed_max / 256, `stop_frac` = stops / steps, `reward`, `min_gap`, `min_ttc` (+inf: never fed / no partner)."""
    w = np.ascontiguousarray(np.asarray(raw).reshape(-1, WORDS)).view(np.uint32)
    f32 = lambda k: w[:, k].copy().view(np.float32).astype(np.float64)      # noqa: E731
    i64 = lambda k: w[:, k].astype(np.int64)                                # noqa: E731
    out = dict(scene=i64(0), slot=i64(1) & 0xFFFF, route=i64(1) >> 16, aid=w[:, 2].copy().view(np.int32).astype(np.int64),
               episode=w[:, 3].copy().view(np.int32).astype(np.int64), first_rec=i64(4), steps=i64(5), flags=i64(6) & 0xFF, kind=i64(6) >> 8)
    fl, kind = out["flags"], out["kind"]
    outcome = np.full(len(w), "vanished", dtype="<U8")
    done = kind == KIND_DONE
    for name, bit in (("maxstep", F_MAXSTEP), ("crash", F_CRASH), ("out", F_OUT), ("arrive", F_ARRIVE)):      # (the last one wins)
        outcome[done & ((fl & bit) != 0)] = name
    outcome[kind == KIND_FLUSHED] = "open"
    out["outcome"] = outcome
    steps = out["steps"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out.update(lcf=f32(7), distance=f32(9) - f32(8), duration_s=steps * float(dt), mean_speed=i64(10) / float(QUANT) / steps,
                   max_speed=i64(11) / float(QUANT), stop_frac=i64(12) / steps, reward=f32(13), min_gap=f32(14), min_ttc=f32(15))
    return out


class TripTable(RowTable):
    """Finished trips as numpy: `raw` uint32 [n, 16] (the rows as the device wrote them, columns `ROW_KEYS`), `meta` (dict: `dt`,
    `num_agents`, `max_rows`, `stop_speed`, `dropped`, `n_records`, `sim_config`), and the columns of `decode` as attributes / items."""

    @staticmethod
    def _decode(raw, meta):
        return decode(raw, meta["dt"])

    def frame(self):
        """pandas DataFrame of every column."""
        import pandas as pd
        return pd.DataFrame({k: self.columns[k] for k in RAW + ("outcome",) + DERIVED})

    def of(self, scene, aid, episode):
        """Indices of the rows of agent `aid` of `scene` in `episode` (a clip header's scene / trig_aid and its env word 1): at most one
        unless the agent was lost and found again (a `flush`, skipped records)."""
        c = self.columns
        return np.nonzero((c["scene"] == int(scene)) & (c["aid"] == int(aid)) & (c["episode"] == int(episode)))[0]

    def summary(self, by="outcome"):
        """Buckets of the rows by `by` = "route", "outcome", "scene" or a sequence of LCF bin edges (bucket k holds edges[k] <= lcf <
        edges[k + 1], the last bin closed): list of dicts with `bucket`, `count`, `success_rate` (arrive / count), and the mean of every
        derived column over the bucket's rows (`min_gap` / `min_ttc`: over the finite ones, NaN when none is)."""
        c = self.columns
        if isinstance(by, str):
            if by not in ("route", "outcome", "scene"):
                raise ValueError("by = %r: 'route', 'outcome', 'scene' or LCF bin edges" % (by,))
            keys = c[by]
            buckets = [(k.item() if hasattr(k, "item") else k, keys == k) for k in (OUTCOMES if by == "outcome" else np.unique(keys))]
            buckets = [(k, m) for k, m in buckets if m.any()]
        else:
            edges = np.asarray(by, np.float64).reshape(-1)
            if len(edges) < 2 or not (np.diff(edges) > 0).all():
                raise ValueError("LCF bin edges must increase")
            lcf = c["lcf"]
            buckets = []
            for k in range(len(edges) - 1):
                hi = (lcf <= edges[k + 1]) if k == len(edges) - 2 else (lcf < edges[k + 1])
                buckets.append(((float(edges[k]), float(edges[k + 1])), (lcf >= edges[k]) & hi))
        out = []
        for key, m in buckets:
            n = int(m.sum())
            row = dict(bucket=key, count=n, success_rate=float((c["outcome"][m] == "arrive").mean()) if n else float("nan"))
            for k in DERIVED:
                v = c[k][m]
                if k in ("min_gap", "min_ttc"):
                    v = v[np.isfinite(v)]
                row[k] = float(v.mean()) if len(v) else float("nan")
            out.append(row)
        return out

    def text(self, by="outcome"):
        """`summary(by)` as a table of text."""
        rows = ["%-22s %6s %8s %9s %9s %9s %9s %9s %9s" % ("bucket", "count", "success", "dist m", "time s", "speed", "stop", "reward", "min ttc")]
        for r in self.summary(by):
            r = dict(r, bucket="[%.3f, %.3f]" % r["bucket"] if isinstance(r["bucket"], tuple) else r["bucket"])
            rows.append("%-22s %6d %8.3f %9.2f %9.2f %9.2f %9.3f %9.3f %9.3f" % (r["bucket"], r["count"], r["success_rate"], r["distance"], r["duration_s"],
                                                                              r["mean_speed"], r["stop_frac"], r["reward"], r["min_ttc"]))
        return "\n".join(rows)


def trip_meta(cfg, N, max_rows, stop_speed, dropped=0, n_records=0):
    """`TripTable.meta` of a log over a simulator of `SimConfig` `cfg` with `N` slots."""
    return dict(dt=float(cfg.dt), num_agents=int(N), max_rows=int(max_rows), stop_speed=float(stop_speed), dropped=int(dropped),
                n_records=int(n_records), sim_config=dataclasses.asdict(cfg))


class TripLog(RowLog):
    """Per-agent trip rows of a `VecSim`: a pool of `max_rows` rows (later ones are counted as dropped), a record with speed below
    `stop_speed` m/s counts as a stop.  Records count from 0 since creation / `reset()`.  `close()` it when done (before or after its
    simulator; no other call once the simulator is closed); every call is asynchronous on torch's current stream except `count()` and
    what reads rows to the host (`table()`, `drain()`)."""

    _prefix, _table_cls = "copo_trip_", TripTable

    def __init__(self, sim, max_rows=65536, stop_speed=0.5):
        self._attach(sim)
        self.max_rows, self.stop_speed = int(max_rows), float(stop_speed)
        cfg = self._capi.TripCfg(self.max_rows, self.stop_speed)
        self._create(self._capi.lib.copo_trip_create, sim._h, C.byref(cfg))
        self.n_records = 0

    @classmethod
    def from_env(cls, sim, value):
        """The env's log (config key `trip_log`: None, or the arguments of `TripLog`)."""
        return cls(sim, **dict(value))

    def env_record(self, feed):
        """One record of the state after reset (no arrays: a trip that was open ends only because its agent is gone) and after every
        step, fed with the step's flags and rew and, with `interaction_metrics`, the meter's gap / ttc of that state.  The rows are
        kept over resets; a reset that restores a slot's agent id and episode word continues its trip (`flush()` before the reset
        cuts every trip there)."""
        self.record(flags=feed.flags, rew=feed.rew, gap=feed.gap, ttc=feed.ttc)

    def record(self, flags=None, rew=None, gap=None, ttc=None):
        """One record of the current state; `flags` (uint8 [E, N]) and `rew` (float32 [E, N]) are the step's outputs, `gap` / `ttc`
        (float32 [E, N]) `InteractionMeter.record()`'s of this state.  None: absent (no flags: the record after a reset, which ends a
        trip only when its agent is gone)."""
        torch = self._torch
        self._capi.check(self._capi.lib.copo_trip_record(self._h, self._en_arg(flags, torch.uint8, "flags"), self._en_arg(rew, torch.float32, "rew"),
                                                         self._en_arg(gap, torch.float32, "gap"), self._en_arg(ttc, torch.float32, "ttc"),
                                                         self._stream()))
        self.n_records += 1

    def _meta(self, dropped):
        return trip_meta(self.sim.cfg, self.sim.N, self.max_rows, self.stop_speed, dropped, self.n_records)
