"""Conflict log: one device-written row per pairwise encounter (host side of `copo_conflict_*`); no counterpart in the reference.

`ConflictLog` owns one `copo_conflict` handle over a `VecSim`.  `record()` follows, on the GPU, every pair of ALIVE agents of a scene
from the record that sees them closer than `radius` to the record in which a party ends (kind 1), vanishes (2) or the two part beyond
`leave_radius` (3) -- steps, the smallest squared distance and both poses at it -- and then commits ONE row of 16 words into a pool of
`max_rows`, in (scene, slot_a, slot_b) order, without allocation or host synchronisation.  `table()` reads the pool out as a
`ConflictTable` (numpy only; `save` / `load` one `.npz`): who met whom -- following, crossing or opposing, who led, how close, and how it
ended for both -- with `of(scene, aid, episode)` as the join with a clip header and a `TripTable`, and `route_matrix(trips)` for which
routes conflict.  The rules are DESIGN.md section 8h; `tests/conflict_numpy.py` restates them.

Memory: the pair memory is dense, 48 B x N (N - 1) / 2 per scene -- 37 KB at 40 slots, 9.6 MB at 256 scenes, 0.6 GB at 16 384 scenes --
plus 20 B per slot, 12 B per scene and 64 B per pool row (`ConflictLog.state_bytes`).  ALIVE-WRECK pairs are out of scope.
"""
import ctypes as C
import dataclasses

import numpy as np

from ._abi import (CONFLICT_DONE as KIND_DONE, CONFLICT_FLUSHED as KIND_FLUSHED, CONFLICT_PARTED as KIND_PARTED,
                   CONFLICT_VANISHED as KIND_VANISHED, CONFLICT_WORDS as WORDS)
from ._rowlog import RowLog, RowTable

ROW_KEYS = ("scene", "pair", "aid_a", "aid_b", "episode", "first_rec", "steps_off", "d2min", "x_a", "y_a", "heading_a", "speed_a", "x_b", "y_b",
            "heading_b", "speed_b")
RAW = ("scene", "slot_a", "slot_b", "aid_a", "aid_b", "episode", "first_rec", "steps", "min_off", "kind", "end_a", "end_b")
DERIVED = ("duration_s", "min_dist", "gap", "rel_heading", "rel_speed")
TYPES = ("following", "crossing", "opposing")
OUTCOMES = ("both_crashed", "one_crashed", "one_left", "parted", "vanished", "open")
F_DONE, F_CRASH = 0x02, 0x08
FOLLOW_RAD, OPPOSE_RAD = np.pi / 6.0, 5.0 * np.pi / 6.0      # |rel_heading| < 30 degrees: following, > 150 degrees: opposing


def _gap(pa, pb, hl, hw):
    """rectangle-to-rectangle gap of section 8b in float64: 0 when |a . d| <= r_a(a) + r_b(a) on the four axes u_a, n_a, u_b, n_b, else
    the smallest of the eight vertex-to-rectangle distances hypot(max(|x'| - hl, 0), max(|y'| - hw, 0)).  pa, pb: [n, 4] poses."""
    ca, cb = pa[:, :2], pb[:, :2]
    ua, ub = np.stack([np.cos(pa[:, 2]), np.sin(pa[:, 2])], -1), np.stack([np.cos(pb[:, 2]), np.sin(pb[:, 2])], -1)
    na, nb = np.stack([-ua[:, 1], ua[:, 0]], -1), np.stack([-ub[:, 1], ub[:, 0]], -1)
    dot = lambda p, q: (p * q).sum(-1)      # noqa: E731
    d = cb - ca
    overlap = np.ones(len(pa), bool)
    for ax in (ua, na, ub, nb):
        r = (hl * np.abs(dot(ax, ua)) + hw * np.abs(dot(ax, na))) + (hl * np.abs(dot(ax, ub)) + hw * np.abs(dot(ax, nb)))
        overlap &= np.abs(dot(ax, d)) <= r
    best = np.full(len(pa), np.inf)
    for c0, u0, n0, c1, u1, n1 in ((ca, ua, na, cb, ub, nb), (cb, ub, nb, ca, ua, na)):       # corners of body 0 against body 1
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                rel = c0 + sa * hl * u0 + sb * hw * n0 - c1
                best = np.minimum(best, np.hypot(np.maximum(np.abs(dot(rel, u1)) - hl, 0.0), np.maximum(np.abs(dot(rel, n1)) - hw, 0.0)))
    return np.where(overlap, 0.0, best)


def decode(raw, dt, hl, hw):
    """dict of columns of the rows `raw` (anything numpy reads as [n, 16] 32-bit words; the device's and the restatement's alike), the
    seconds per record `dt` and the vehicles' half length and width.  Integer columns `RAW` (int64; `kind` 1 done / 2 vanished / 3 parted
    / 4 flushed, `end_a` / `end_b` the step's flags byte of a party that ended, else 0); the poses `pose_a` / `pose_b` float64 [n, 4] {x,
    y, heading, speed} at the smallest centre distance; float64 `duration_s` = steps x dt, `min_dist` = sqrt(d2min), `gap` (the rectangle
    gap of section 8b at those poses), `rel_heading` = heading_b - heading_a wrapped into (-pi, pi], `rel_speed` = |v_b u_b - v_a u_a|;
    `type`: |rel_heading| < 30 degrees "following", > 150 degrees "opposing", else "crossing"; `leader` (following rows only, else ""):
    "a" or "b", the party ahead along a's heading; `outcome`: a kind-1 row by the number of its ends that carry CRASH -- 2 "both_crashed",
    1 "one_crashed", 0 "one_left" --, kind 3 "parted", kind 2 "vanished", kind 4 "open"."""
    w = np.ascontiguousarray(np.asarray(raw).reshape(-1, WORDS)).view(np.uint32)
    i64 = lambda k: w[:, k].astype(np.int64)                                # noqa: E731
    s32 = lambda k: w[:, k].copy().view(np.int32).astype(np.int64)          # noqa: E731
    pk, so = i64(1), i64(6)
    out = dict(scene=i64(0), slot_a=pk & 63, slot_b=(pk >> 6) & 63, aid_a=s32(2), aid_b=s32(3), episode=s32(4), first_rec=i64(5), steps=so & 0xFFFF,
               min_off=so >> 16, kind=(pk >> 12) & 15, end_a=(pk >> 16) & 0xFF, end_b=pk >> 24)
    pa = np.ascontiguousarray(w[:, 8:12]).view(np.float32).astype(np.float64)
    pb = np.ascontiguousarray(w[:, 12:16]).view(np.float32).astype(np.float64)
    out["pose_a"], out["pose_b"] = pa, pb
    with np.errstate(invalid="ignore"):
        out["duration_s"] = out["steps"].astype(np.float64) * float(dt)
        out["min_dist"] = np.sqrt(w[:, 7].copy().view(np.float32).astype(np.float64))
        out["gap"] = _gap(pa, pb, float(hl), float(hw))
        rel = np.remainder(pb[:, 2] - pa[:, 2], 2.0 * np.pi)                # [0, 2 pi)
        rel = np.where(rel > np.pi, rel - 2.0 * np.pi, rel)                 # (-pi, pi]
        out["rel_heading"] = rel
        ua, ub = np.stack([np.cos(pa[:, 2]), np.sin(pa[:, 2])], -1), np.stack([np.cos(pb[:, 2]), np.sin(pb[:, 2])], -1)
        out["rel_speed"] = np.hypot(*(pb[:, 3:4] * ub - pa[:, 3:4] * ua).T) if len(w) else np.zeros(0)
        kind_of = np.full(len(w), "crossing", dtype="<U9")
        kind_of[np.abs(rel) < FOLLOW_RAD] = "following"
        kind_of[np.abs(rel) > OPPOSE_RAD] = "opposing"
        out["type"] = kind_of
        ahead = ((pb[:, :2] - pa[:, :2]) * ua).sum(-1) > 0.0                # b ahead of a along a's heading
        out["leader"] = np.where(kind_of == "following", np.where(ahead, "b", "a"), "").astype("<U1")
    kind = out["kind"]
    crashes = ((out["end_a"] & F_CRASH) != 0).astype(np.int64) + ((out["end_b"] & F_CRASH) != 0)
    outcome = np.full(len(w), "vanished", dtype="<U12")
    for n, name in ((0, "one_left"), (1, "one_crashed"), (2, "both_crashed")):
        outcome[(kind == KIND_DONE) & (crashes == n)] = name
    outcome[kind == KIND_PARTED] = "parted"
    outcome[kind == KIND_FLUSHED] = "open"
    out["outcome"] = outcome
    return out


class ConflictTable(RowTable):
    """Encounters as numpy: `raw` uint32 [n, 16] (the rows as the device wrote them, columns `ROW_KEYS`), `meta` (dict: `dt`, `hl`, `hw`,
    `num_agents`, `max_rows`, `radius`, `leave_radius`, `dropped`, `n_records`, `sim_config`), and the columns of `decode` as attributes
    / items."""

    @staticmethod
    def _decode(raw, meta):
        return decode(raw, meta["dt"], meta["hl"], meta["hw"])

    def frame(self):
        """pandas DataFrame of every scalar column."""
        import pandas as pd
        return pd.DataFrame({k: self.columns[k] for k in RAW + ("type", "leader", "outcome") + DERIVED})

    def of(self, scene, aid, episode):
        """Indices of the rows where agent `aid` of `scene` in `episode` is a party (a clip header's scene / trig_aid and its env word 1;
        a `TripTable` row's scene / aid / episode)."""
        c = self.columns
        return np.nonzero((c["scene"] == int(scene)) & (c["episode"] == int(episode)) & ((c["aid_a"] == int(aid)) | (c["aid_b"] == int(aid))))[0]

    def summary(self, by="type"):
        """Buckets of the rows by `by` = "type" or "outcome": list of dicts with `bucket`, `count`, `share`, and the mean of every derived
        column over the bucket's rows (empty buckets are left out)."""
        if by not in ("type", "outcome"):
            raise ValueError("by = %r: 'type' or 'outcome'" % (by,))
        c, out = self.columns, []
        for key in (TYPES if by == "type" else OUTCOMES):
            m = c[by] == key
            n = int(m.sum())
            if n:
                out.append(dict(bucket=key, count=n, share=n / len(self), **{k: float(c[k][m].mean()) for k in DERIVED}))
        return out

    def text(self, by="type"):
        """`summary(by)` as a table of text."""
        rows = ["%-14s %6s %7s %9s %9s %9s %9s" % ("bucket", "count", "share", "time s", "dist m", "gap m", "rel m/s")]
        for r in self.summary(by):
            rows.append("%-14s %6d %7.3f %9.2f %9.2f %9.2f %9.2f" % (r["bucket"], r["count"], r["share"], r["duration_s"], r["min_dist"], r["gap"],
                                                                    r["rel_speed"]))
        return "\n".join(rows)

    def route_matrix(self, trips):
        """Joins both parties with the `TripTable` `trips` on (scene, aid, episode): dict with `routes` (the sorted route numbers that
        occur), `all` and `both_crashed` (int64 [R, R], symmetric: an encounter of routes p and q counts in [p, q] and [q, p], once on
        the diagonal) and `missing`, the parties whose trip is not in the table (their encounters are in neither matrix)."""
        t = trips.columns
        route_of = {k: int(r) for k, r in zip(zip(t["scene"].tolist(), t["aid"].tolist(), t["episode"].tolist()), t["route"].tolist())}
        c = self.columns
        pairs, missing = [], 0
        for s, a, b, ep, oc in zip(c["scene"].tolist(), c["aid_a"].tolist(), c["aid_b"].tolist(), c["episode"].tolist(), c["outcome"].tolist()):
            ra, rb = route_of.get((s, a, ep)), route_of.get((s, b, ep))
            missing += (ra is None) + (rb is None)
            if ra is not None and rb is not None:
                pairs.append((ra, rb, oc == "both_crashed"))
        routes = sorted({r for p in pairs for r in p[:2]})
        at = {r: k for k, r in enumerate(routes)}
        every, crashed = np.zeros((len(routes),) * 2, np.int64), np.zeros((len(routes),) * 2, np.int64)
        for ra, rb, cr in pairs:
            for m in (every,) + ((crashed,) if cr else ()):
                m[at[ra], at[rb]] += 1
                if ra != rb:
                    m[at[rb], at[ra]] += 1
        return {"routes": routes, "all": every, "both_crashed": crashed, "missing": int(missing)}


def conflict_meta(cfg, N, max_rows, radius, leave_radius, dropped=0, n_records=0):
    """`ConflictTable.meta` of a log over a simulator of `SimConfig` `cfg` with `N` slots."""
    return dict(dt=float(cfg.dt), hl=float(cfg.veh_half_len), hw=float(cfg.veh_half_wid), num_agents=int(N), max_rows=int(max_rows),
                radius=float(radius), leave_radius=float(leave_radius), dropped=int(dropped), n_records=int(n_records),
                sim_config=dataclasses.asdict(cfg))


def state_bytes(E, N, max_rows):
    """Device memory of a log: 48 B per pair, 20 B per slot, 12 B per scene, 64 B per pool row and the two counters."""
    return 48 * E * (N * (N - 1) // 2) + 20 * E * N + 12 * E + 64 * int(max_rows) + 16


class ConflictLog(RowLog):
    """Per-pair encounter rows of a `VecSim`: a pool of `max_rows` rows (later ones are counted as dropped); an encounter opens when two
    ALIVE agents of a scene are closer than `radius` metres (centre to centre) and parts at `leave_radius` or beyond.  Records count from
    0 since creation / `reset()`.  The pair memory is dense: 48 B x N (N - 1) / 2 per scene (37 KB at 40 slots, 9.6 MB at 256 scenes, 0.6
    GB at 16 384 scenes; `state_bytes` is the whole handle).  `close()` it when done (before or after its simulator; no other call once
    the simulator is closed); every call is asynchronous on torch's current stream except `count()` and what reads rows to the host
    (`table()`, `drain()`)."""

    _prefix, _table_cls = "copo_conflict_", ConflictTable

    def __init__(self, sim, max_rows=65536, radius=8.0, leave_radius=10.0):
        self._attach(sim)
        self.max_rows, self.radius, self.leave_radius = int(max_rows), float(radius), float(leave_radius)
        cfg = self._capi.ConflictCfg(self.max_rows, self.radius, self.leave_radius)
        self._create(self._capi.lib.copo_conflict_create, sim._h, C.byref(cfg))
        self.n_records = 0
        self.state_bytes = state_bytes(sim.E, sim.N, self.max_rows)

    @classmethod
    def from_env(cls, sim, value):
        """The env's log (`env.conflict_log(**value)`: the arguments of `ConflictLog`)."""
        return cls(sim, **dict(value or {}))

    def env_record(self, feed):
        """One record of the state after reset (no flags) and after every step with the step's flags.  Nothing special happens at a
        reset: identity decides, so an encounter whose parties are gone closes by kind 2."""
        self.record(flags=feed.flags)

    def record(self, flags=None):
        """One record of the current state; `flags` (uint8 [E, N]) is the step's output, None after a reset."""
        self._capi.check(self._capi.lib.copo_conflict_record(self._h, self._en_arg(flags, self._torch.uint8, "flags"), self._stream()))
        self.n_records += 1

    def _meta(self, dropped):
        return conflict_meta(self.sim.cfg, self.sim.N, self.max_rows, self.radius, self.leave_radius, dropped, self.n_records)
