"""Linear probes: what the hidden layers of bank members encode, as ridge regressions from a layer's activations to scene quantities.

`similarity.py` says whether two checkpoints compute the same thing inside; it cannot say WHAT a layer represents.  A linear probe can: a
ridge regression from the activations of a layer to a quantity of the scene (how near is the nearest vehicle and where, how clear is the
road ahead, does the step about to be taken end in a crash), fitted on the scenes of a TRAIN fold and scored by R^2 on the scenes of a TEST
fold.  The raw observation is probed as a control: `gain` is what a layer's R^2 adds to the input's own.

A `ProbePlan` is a panel of members that all read the same rows (a `PanelPlan` of `panel.py`, as `SimilarityPlan` is) and a fold table over the
scenes.  Per env step `copo_hidden_obs_seats_f32` keeps h1 and h2 of every panel member, `copo_probe_targets` (csrc/probe_kernels.hip)
writes the step's eight targets (`TARGETS`) and the zero-padded observation row of every listed position, and `copo_probe_accumulate`
adds the sufficient statistics of both folds to float64 accumulators -- once over the hidden blocks, once over the observation:
    G[f][b] += X_b^T X_b (upper 64 x 64 tiles)      C[f][b] += X_b^T t      T[f] += t^T t
over the rows that ACTED in the step (the seat tally's rule), optionally only over the rows one member drives (`rows_of`).  `probe_fit`
solves the regressions from them on the host in float64.  Nothing here changes anybody's driving: the drive and the seat tally are a
plain `SeatSampler`'s, bit for bit.

`r2_train` / `r2_test` are NaN where a fold has fewer than two rows, the features do not vary, or the target is constant on the fold;
never an exception.

Pieces: `ProbePlan` (numpy only), `probe_targets` / `probe_accumulate` (thin checked wrappers), `ProbeAccumulators`, `probe_fit` (numpy
only), `ProbeSeatSampler` (hidden launch, forward, step, seat tally, targets and both accumulates of a fragment stay one captured
graph), `probe_frame` / `probe_matrix`, `probe_rows` (`evaluate --probe`) and `probe_of` (caller-supplied targets on plain arrays).
"""
import numpy as np

from .crossplay import SeatPlan, run_pairs
from .panel import LAYERS, MAX_PANEL, MAX_PLANES, TILE, PanelPlan, PanelSeatSampler, every_row, hidden_activations, want

TARGETS = ("nearest", "nearest_cos", "nearest_sin", "beams_hit", "front_clear", "reward", "crash", "done")
PANEL, MAX_TARGETS, MAX_WIDTH, FOLD_NONE = 16, 15, 512, 255      # include/copo_hip.h, COPO_PROBE_*
TRAIN, TEST = 0, 1
OBS_LAYER = "obs"
CONSTANT = 1e-12          # a target whose sum of squares about its mean is below this share of its sum of squares is constant on the fold


def padded_width(obs_dim):
    """The observation width rounded up to a multiple of 64: the width of the control block."""
    return -(-int(obs_dim) // TILE) * TILE


def trig_table(num_lasers):
    """float32 [num_lasers][2]: (cos, sin)(2 pi k / n) computed in float64 and rounded once -- the table `probe_targets` reads."""
    a = 2.0 * np.pi * np.arange(int(num_lasers), dtype=np.float64) / float(num_lasers)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32))


def default_folds(seats):
    """uint8 [E]: inside every scene group in [0, G) the scenes alternate train, test, train, ... in ascending scene order; 255 elsewhere."""
    folds = np.full(seats.E, FOLD_NONE, np.uint8)
    for g in range(seats.n_groups):
        scenes = np.nonzero(np.asarray(seats.group) == g)[0]
        folds[scenes] = np.arange(len(scenes)) % 2
    return folds


class ProbePlan(PanelPlan):
    """A `PanelPlan` of bank members probed on the seated rows of the seat plan `seats` (one member is a panel).  `folds`: [E] of 0
    (train) / 1 (test) / 255 (never counted); default `default_folds(seats)`.  A plan in which a fold has no seated scene is refused, and
    the message names the scene groups.  Its own: `blocks` = 2 M hidden blocks in (member, layer) order, `planes(D, blocks)` (the row
    split R of an accumulator set: `PanelPlan.row_split` of its launch's 2 folds x blocks x (upper tiles + 1) workgroups),
    `accumulator_shapes(D, blocks)`, `accumulator_bytes(hidden, obs_dim)`.  `check_bytes(hidden, obs_dim)` refuses accumulators beyond
    `max_bytes` (default 1 GiB) with the figure; it runs at construction where `hidden` is given.  Nothing here touches a device."""

    def __init__(self, seats, members=None, rows_of=None, folds=None, hidden=None, max_bytes=1 << 30):
        super().__init__(seats, members, rows_of, max_bytes)
        self.blocks = 2 * self.M
        folds = default_folds(seats) if folds is None else np.asarray(folds)
        if folds.shape != (self.E,):
            raise ValueError("ProbePlan: a fold table of shape %s, one entry per scene [%d] wanted" % (folds.shape, self.E))
        if not np.isin(folds, (TRAIN, TEST, FOLD_NONE)).all():
            raise ValueError("ProbePlan: fold table entries %s, 0 (train) / 1 (test) / %d (never counted) wanted" % (np.unique(folds).tolist(), FOLD_NONE))
        self.folds = np.ascontiguousarray(folds, np.uint8)
        group = np.asarray(seats.group)
        seated = (np.asarray(seats.seat) >= 0).any(axis=1) & (group >= 0) & (group < self.G)
        for f, name in ((TRAIN, "train"), (TEST, "test")):
            have = set(group[seated & (self.folds == f)].tolist())
            if not have:
                raise ValueError("ProbePlan: no seated scene in the %s fold (scene groups %s have none)" % (name, sorted(set(range(self.G)) - have)))
        if hidden is not None:
            self.check_bytes(hidden)

    def planes(self, D, blocks=None):
        nt = int(D) // TILE
        return self.row_split(2 * (self.blocks if blocks is None else int(blocks)) * (nt * (nt + 1) // 2 + 1))

    def accumulator_shapes(self, D, blocks=None):
        D, B = int(D), self.blocks if blocks is None else int(blocks)
        R = self.planes(D, B)
        return dict(G=(R, 2, B, D, D), C=(R, 2, B, D, PANEL), T=(R, 2, PANEL, PANEL))

    def accumulator_bytes(self, hidden, obs_dim=None):
        return self.bytes_of(self.accumulator_shapes(hidden), *([] if obs_dim is None else [self.accumulator_shapes(padded_width(obs_dim), 1)]))

    def check_bytes(self, hidden, obs_dim=None):
        H = self.check_width(hidden, MAX_WIDTH)
        if obs_dim is not None and not 1 <= int(obs_dim) <= MAX_WIDTH:
            raise ValueError("ProbePlan: an observation of %d columns, 1..%d wanted" % (int(obs_dim), MAX_WIDTH))
        need = self.accumulator_bytes(H, obs_dim)
        if need > self.max_bytes:
            raise ValueError("ProbePlan: 2 folds x %d blocks x %d x %d float64 in %d planes and their panels are %d bytes of accumulators, max_bytes = %d" % (
                self.blocks, H, H, self.planes(H), need, self.max_bytes))
        return need


def probe_targets(obs, lidar_lo, num_lasers, trig, flags, reward, rows, count, targets, xobs):
    """The step's `targets` float32 [cap][16] (`TARGETS` in columns 0 .. 7, zeros, 1.0 in column 15) and `xobs` float32 [cap][Op] (the
    observation row, zero beyond O) of every position p < count of the common list `rows` int64 [cap] / `count` int32 [1], from `obs`
    float32 [n_out][O] (the LiDAR block at columns lidar_lo .. lidar_lo + num_lasers), `trig` float32 [num_lasers][2] (`trig_table`),
    the step's `flags` uint8 [n_out] and `reward` float32 [n_out].  Other positions keep what they held.  One launch on the current
    stream."""
    import torch
    from .. import _capi
    who = "probe_targets"
    if obs is None or obs.dim() != 2:
        raise ValueError("%s: obs of shape %s, [n_out][O] wanted" % (who, None if obs is None else tuple(obs.shape)))
    n_out, O = (int(v) for v in obs.shape)
    lo, n = int(lidar_lo), int(num_lasers)
    if n < 1 or lo < 0 or lo + n > O:
        raise ValueError("%s: a LiDAR block of %d beams at column %d of %d" % (who, n, lo, O))
    if rows is None or rows.dim() != 1 or xobs is None or xobs.dim() != 2:
        raise ValueError("%s: rows [cap] and xobs [cap][Op] wanted" % who)
    cap, Op = int(rows.shape[0]), int(xobs.shape[1])
    if Op != padded_width(O) or Op > MAX_WIDTH:
        raise ValueError("%s: xobs of %d columns for an observation of %d: %d wanted (%d at the most)" % (who, Op, O, padded_width(O), MAX_WIDTH))
    want(who, "obs", obs, (n_out, O), torch.float32)
    want(who, "trig", trig, (n, 2), torch.float32)
    want(who, "flags", flags, (n_out,), torch.uint8)
    want(who, "reward", reward, (n_out,), torch.float32)
    want(who, "rows", rows, (cap,), torch.int64)
    want(who, "count", count, (1,), torch.int32)
    want(who, "targets", targets, (cap, PANEL), torch.float32)
    want(who, "xobs", xobs, (cap, Op), torch.float32)
    _capi.check(_capi.lib.copo_probe_targets(obs.data_ptr(), n_out, O, lo, n, trig.data_ptr(), flags.data_ptr(), reward.data_ptr(), rows.data_ptr(),
                                             count.data_ptr(), cap, targets.data_ptr(), xobs.data_ptr(), Op, _capi.current_stream()))


def probe_accumulate(x, block_base, pos_stride, width, targets, rows, count, flags, seat, fold, rows_of, G, C, T):
    """One step's feature blocks added to the accumulators `G` float64 [R][2][B][D][D] (upper 64 x 64 tiles), `C` float64 [R][2][B][D][16]
    and `T` float64 [R][2][16][16] over the counted positions of the common list `rows` int64 [cap] / `count` int32 [1].  Block b holds
    the D = `width` features `x.view(-1)[block_base[b] + p * pos_stride:][:D]` of position p (`x` float32, contiguous; `block_base` int64
    [B], offsets in floats).  `targets` float32 [cap][16].  Position p counts in fold f when p < count, `flags` uint8 [n_out] carry
    ACTED at rows[p], (`rows_of` < 0 or `seat` int32 [n_out] is `rows_of` there) and `fold` uint8 [E] is f at the row's scene rows[p] //
    (n_out // E).  R is read off `G`.  The outputs accumulate; the caller clears them.  One launch on the current stream."""
    import torch
    from .. import _capi
    who = "probe_accumulate"
    D, stride = int(width), int(pos_stride)
    if D < TILE or D > MAX_WIDTH or D % TILE:
        raise ValueError("%s: width = %d, a multiple of %d up to %d wanted" % (who, D, TILE, MAX_WIDTH))
    if block_base is None or block_base.dim() != 1 or not 1 <= int(block_base.shape[0]) <= 2 * MAX_PANEL:
        raise ValueError("%s: block_base of shape %s, [B] with B in 1..%d wanted" % (who, None if block_base is None else tuple(block_base.shape), 2 * MAX_PANEL))
    B = int(block_base.shape[0])
    if G is None or G.dim() != 5 or not 1 <= int(G.shape[0]) <= MAX_PLANES:
        raise ValueError("%s: G of shape %s, [R][2][B][D][D] with R in 1..%d wanted" % (who, None if G is None else tuple(G.shape), MAX_PLANES))
    R = int(G.shape[0])
    if rows is None or rows.dim() != 1:
        raise ValueError("%s: rows of shape %s, [cap] wanted" % (who, None if rows is None else tuple(rows.shape)))
    cap = int(rows.shape[0])
    if x is None or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("%s: x must be a contiguous float32 tensor" % who)
    if stride < D or stride % 4 or cap * stride > int(x.numel()):
        raise ValueError("%s: pos_stride = %d for width %d and %d positions in %d floats: a multiple of 4 from the width up, every position inside x" % (
            who, stride, D, cap, int(x.numel())))
    if flags is None or seat is None or fold is None or flags.numel() != seat.numel() or flags.numel() < 1 or fold.dim() != 1 or fold.numel() < 1 \
            or flags.numel() % fold.numel():
        raise ValueError("%s: flags and seat must cover the same rows, a whole number of them per entry of fold (%s rows, a fold table of %s)" % (
            who, None if flags is None else flags.numel(), None if fold is None else tuple(fold.shape)))
    n_out, E = int(flags.numel()), int(fold.numel())
    want(who, "block_base", block_base, (B,), torch.int64)
    want(who, "targets", targets, (cap, PANEL), torch.float32)
    want(who, "rows", rows, (cap,), torch.int64)
    want(who, "count", count, (1,), torch.int32)
    want(who, "flags", flags, flags.shape, torch.uint8)
    want(who, "seat", seat, seat.shape, torch.int32)
    want(who, "fold", fold, (E,), torch.uint8)
    want(who, "G", G, (R, 2, B, D, D), torch.float64)
    want(who, "C", C, (R, 2, B, D, PANEL), torch.float64)
    want(who, "T", T, (R, 2, PANEL, PANEL), torch.float64)
    _capi.check(_capi.lib.copo_probe_accumulate(x.data_ptr(), int(x.numel()), block_base.data_ptr(), B, stride, D, targets.data_ptr(), rows.data_ptr(),
                                                count.data_ptr(), cap, flags.data_ptr(), seat.data_ptr(), fold.data_ptr(), n_out, n_out // E, int(rows_of), R,
                                                G.data_ptr(), C.data_ptr(), T.data_ptr(), _capi.current_stream()))


def mirror_tiles(G):
    """[..][D][D] whose 64 x 64 tiles below the diagonal are unset -> the full symmetric matrix."""
    D = G.shape[-1]
    t = np.arange(D) // TILE
    upper, strict = t[:, None] <= t[None, :], t[:, None] < t[None, :]
    return np.where(upper, G, 0.0) + np.swapaxes(np.where(strict, G, 0.0), -1, -2)


class ProbeStats:
    """One accumulator set: `G` / `C` / `T` of B blocks of width D in R planes."""

    def __init__(self, B, D, R, device):
        import torch
        self.B, self.D, self.R = int(B), int(D), int(R)
        self.G = torch.zeros(R, 2, B, D, D, dtype=torch.float64, device=device)
        self.C = torch.zeros(R, 2, B, D, PANEL, dtype=torch.float64, device=device)
        self.T = torch.zeros(R, 2, PANEL, PANEL, dtype=torch.float64, device=device)

    def tensors(self):
        return (self.G, self.C, self.T)

    @staticmethod
    def host(G, C, T):
        """The planes [R][..] as numpy summed in plane order, `G` mirrored to full symmetric: dict(G [2][B][D][D], C [2][B][D][16], T [2][16][16])."""
        out = []
        for a in (G, C, T):
            s = np.zeros(a.shape[1:], np.float64)
            for r in range(a.shape[0]):
                s = s + a[r]
            out.append(s)
        return dict(G=mirror_tiles(out[0]), C=out[1], T=out[2])


class ProbeAccumulators:
    """The float64 accumulators of a panel: `hidden` (`ProbeStats` of the 2 M hidden blocks at width H in R planes) and `obs` (one block at
    width Op in `obs_planes` planes)."""

    def __init__(self, M, H, R, obs_width, obs_planes, device):
        self.hidden, self.obs = ProbeStats(2 * int(M), H, R, device), ProbeStats(1, obs_width, obs_planes, device)

    def clear(self):
        for t in self.hidden.tensors() + self.obs.tensors():
            t.zero_()

    def read(self):
        """One host read of all six accumulators: dict(hidden=dict(G, C, T), obs=dict(G, C, T)) as `ProbeStats.host` forms them."""
        import torch
        ts = self.hidden.tensors() + self.obs.tensors()
        flat = torch.cat([t.reshape(-1) for t in ts]).cpu().numpy()
        parts, at = [], 0
        for t in ts:
            parts.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
            at += t.numel()
        return dict(hidden=ProbeStats.host(*parts[:3]), obs=ProbeStats.host(*parts[3:]))


def probe_fit(acc, ridge=1e-4, n_targets=len(TARGETS)):
    """The ridge probes of every block and target from the sufficient statistics `acc` = dict(G [2][B][D][D] full symmetric, C
    [2][B][D][16], T [2][16][16]) (`ProbeStats.host`; fold 0 = train, 1 = test; column 15 of a target row is 1), in float64 on the host.
    Per block and target: centre with the TRAIN fold's means, solve (Cxx + ridge trace(Cxx) / D I) w = Cxt, then from each fold's
    statistics ALONE
        sse = sum (t - tbar_train - w . (x - xbar_train))^2      sst = sum (t - tbar_train)^2      r2 = 1 - sse / sst.
    Returns dict(n_train, n_test, r2_train [B][Q], r2_test [B][Q], weight_norm [B][Q], weights [B][D][Q]).  An r2 is NaN where its fold
    has fewer than two rows, the train fold has fewer than two, trace(Cxx) is zero or the target is constant on the fold; everything is
    NaN where any accumulator entry is not finite."""
    G, C, T = (np.asarray(acc[k], np.float64) for k in ("G", "C", "T"))
    Q, ridge = int(n_targets), float(ridge)
    if not 1 <= Q <= MAX_TARGETS or not np.isfinite(ridge) or ridge < 0.0:
        raise ValueError("probe_fit: %d targets (1..%d) and ridge = %r (finite, >= 0) wanted" % (Q, MAX_TARGETS, ridge))
    B, D = G.shape[1], G.shape[2]
    one = PANEL - 1
    nan = lambda *shape: np.full(shape, np.nan)  # noqa: E731
    out = dict(n_train=0, n_test=0, r2_train=nan(B, Q), r2_test=nan(B, Q), weight_norm=nan(B, Q), weights=nan(B, D, Q))
    if not (np.isfinite(G).all() and np.isfinite(C).all() and np.isfinite(T).all()):
        return out
    n = [int(round(T[f, one, one])) for f in (TRAIN, TEST)]
    out["n_train"], out["n_test"] = n
    if n[TRAIN] < 2:
        return out
    tbar = T[TRAIN, :Q, one] / n[TRAIN]
    for b in range(B):
        xbar = C[TRAIN, b, :, one] / n[TRAIN]

        def centred(f):
            """(Sxx [D][D], Sxt [D][Q], Stt [Q]) of fold f about the TRAIN means."""
            sx, st = C[f, b, :, one], T[f, :Q, one]
            Sxx = G[f, b] - np.outer(xbar, sx) - np.outer(sx, xbar) + n[f] * np.outer(xbar, xbar)
            Sxt = C[f, b, :, :Q] - np.outer(xbar, st) - np.outer(sx, tbar) + n[f] * np.outer(xbar, tbar)
            Stt = np.diag(T[f])[:Q] - 2.0 * tbar * st + n[f] * tbar * tbar
            return Sxx, Sxt, Stt

        Cxx, Cxt, _ = centred(TRAIN)
        trace = float(np.trace(Cxx))
        if not trace > 0.0:
            continue
        try:
            w = np.linalg.solve(Cxx + ridge * trace / D * np.eye(D), Cxt)
        except np.linalg.LinAlgError:
            continue
        out["weights"][b], out["weight_norm"][b] = w, np.sqrt((w * w).sum(axis=0))
        for f, key in ((TRAIN, "r2_train"), (TEST, "r2_test")):
            if n[f] < 2:
                continue
            Sxx, Sxt, Stt = centred(f)
            sse = Stt - 2.0 * (w * Sxt).sum(axis=0) + np.einsum("iq,ij,jq->q", w, Sxx, w)
            raw, st = np.diag(T[f])[:Q], T[f, :Q, one]
            varies = raw - st * st / n[f] > CONSTANT * raw          # the target's sum of squares about the fold's OWN mean
            with np.errstate(invalid="ignore", divide="ignore"):
                r2 = 1.0 - sse / Stt
            out[key][b] = np.where(varies & np.isfinite(r2), r2, np.nan)
    return out


class ProbeSeatSampler(PanelSeatSampler):
    """`PanelSeatSampler` with a probe panel: per env step `hidden_seats` on the observation the policy reads, the seated forward on the
    same observation, the simulator step and the seat tally, then `probe_targets` of the step's observation, flags and reward and
    `probe_accumulate` once on the hidden workspace and once on the observation block -- the whole fragment is still one captured graph.
    `acc` (`ProbeAccumulators`) accumulates until `clear_tally()`; `read()` returns the two fits, `frame()` the table."""

    def __init__(self, vec_env, policy, bank, plan, probes, T, use_graph=True, ridge=1e-4):
        import torch
        from .levels import lidar_columns
        super().__init__(vec_env, policy, bank, plan, probes, T, use_graph=use_graph)
        H = int(bank.cfg.hidden)
        probes.check_bytes(H, self.O)
        self.probes, self.ridge = probes, float(ridge)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        cap, Op = probes.cap, padded_width(self.O)
        self.lidar_lo, hi = lidar_columns(self.sim.cfg)
        self.num_lasers = hi - self.lidar_lo
        self.trig, self.fold = up(trig_table(self.num_lasers)), up(probes.folds)
        self.block_base = up(np.array([(int(m) * cap * 2 + layer) * H for m in probes.members for layer in range(2)], np.int64))
        self.obs_base = up(np.zeros(1, np.int64))
        self.targets = torch.zeros(cap, PANEL, dtype=torch.float32, device=self.device)
        self.xobs = torch.zeros(cap, Op, dtype=torch.float32, device=self.device)
        self.acc = ProbeAccumulators(probes.M, H, probes.planes(H), Op, probes.planes(Op, 1), self.device)

    def _step(self, t):
        super()._step(t)          # (it wrote obs[t + 1]; obs[t] is still what the policy read)
        flags, seat, a, H = self.flags[t].view(-1), self.seated.buffers.seat.view(-1), self.acc, self.acc.hidden.D
        probe_targets(self.obs[t].view(-1, self.O), self.lidar_lo, self.num_lasers, self.trig, flags, self.rew3[0, t].view(-1), self._rows, self._count,
                      self.targets, self.xobs)
        probe_accumulate(self.hidden, self.block_base, 2 * H, H, self.targets, self._rows, self._count, flags, seat, self.fold, self.probes.rows_of,
                         *a.hidden.tensors())
        probe_accumulate(self.xobs, self.obs_base, a.obs.D, a.obs.D, self.targets, self._rows, self._count, flags, seat, self.fold, self.probes.rows_of,
                         *a.obs.tensors())

    def read(self):
        """One host read, then `probe_fit` of both accumulator sets: dict(hidden=fit, obs=fit)."""
        import torch
        torch.cuda.current_stream().synchronize()
        r = self.acc.read()
        return dict(hidden=probe_fit(r["hidden"], self.ridge), obs=probe_fit(r["obs"], self.ridge))

    def frame(self, labels=None):
        r = self.read()
        return probe_frame(r["hidden"], r["obs"], self.probes.members, self.probes.rows_of, labels, n_members=self.probes.K)


def probe_frame(hidden_fit, obs_fit, members, rows_of=-1, labels=None, names=TARGETS, n_members=None):
    """The fits of the hidden blocks ((member, layer) order) and of the observation control as a frame: one row per (member, layer,
    target) -- first the control's rows (member -1, layer "obs"), then h1 and h2 of every panel member.  Columns: `member`, `label`,
    `layer`, `target`, `rows_of` (-1: every acted row), `n_train`, `n_test`, `r2_train`, `r2_test`, `gain` (`r2_test` minus the
    control's `r2_test` for the same target), `weight_norm`."""
    import pandas as pd
    members = [int(m) for m in members]
    K = (max(members) + 1 if members else 0) if n_members is None else int(n_members)
    labels = list(range(K)) if labels is None else list(labels)
    names = list(names)
    rows = []

    def add(fit, b, member, label, layer):
        for q, name in enumerate(names):
            r2 = float(fit["r2_test"][b, q])
            rows.append(dict(member=member, label=label, layer=layer, target=name, rows_of=int(rows_of), n_train=int(fit["n_train"]),
                             n_test=int(fit["n_test"]), r2_train=float(fit["r2_train"][b, q]), r2_test=r2, gain=r2 - float(obs_fit["r2_test"][0, q]),
                             weight_norm=float(fit["weight_norm"][b, q])))

    add(obs_fit, 0, -1, OBS_LAYER, OBS_LAYER)
    for a, m in enumerate(members):
        for li, layer in enumerate(LAYERS):
            add(hidden_fit, 2 * a + li, m, labels[m], layer)
    return pd.DataFrame(rows)


def probe_matrix(frame, n_members=None):
    """`r2_test` of a `probe_frame` as a table: one row per (member, layer), one column per target (what `evaluate --probe` prints)."""
    import pandas as pd
    index, cols = list(dict.fromkeys(zip(frame["member"], frame["layer"]))), list(dict.fromkeys(frame["target"]))
    m = np.full((len(index), len(cols)), np.nan)
    for member, layer, target, v in zip(frame["member"], frame["layer"], frame["target"], frame["r2_test"]):
        m[index.index((member, layer)), cols.index(target)] = float(v)
    return pd.DataFrame(m, index=pd.MultiIndex.from_tuples(index, names=["member", "layer"]), columns=cols)


def probe_rows(algo, env, weights_list, rows_of=None, members=None, ridge=1e-4, folds=None, share=0.5, scenes_per_pair=4, num_agents=40, steps=1000,
               seed=0, labels=None, max_bytes=1 << 30, **extra):
    """The K populations `weights_list` (one layout) on the `SeatPlan.pairs` layout of `cross_play_rows`, their hidden layers probed for
    the eight `TARGETS` on the states the scenes visit: every acted row of every pair's scenes, or with `rows_of` = k only the rows member
    k drives, for `steps` env steps (rounded up to whole fragments).  The scenes of a pair alternate between the train and the test fold
    (`default_folds`; `scenes_per_pair` >= 2), unless `folds` [E] says otherwise.  `members`: the panel (default: all).  Returns the
    `probe_frame`."""
    def check():
        K = len(list(weights_list))
        if rows_of is not None and not 0 <= int(rows_of) < K:
            raise ValueError("probe_rows: rows_of = %r of %d members" % (rows_of, K))
        if not np.isfinite(float(ridge)) or float(ridge) < 0.0:
            raise ValueError("probe_rows: ridge = %r, a finite number >= 0 wanted" % (ridge,))

    weights_list = list(weights_list)
    return run_pairs("probe_rows", algo, env, weights_list,
                     lambda t, bank, seats, use_graph: ProbeSeatSampler(
                         t.env, t.policy, bank, seats, ProbePlan(seats, members, rows_of, folds, max_bytes=max_bytes), t.sampler.T, use_graph=use_graph,
                         ridge=ridge),
                     lambda smp, seats, labels: smp.frame(labels),
                     share=share, scenes_per_pair=scenes_per_pair, num_agents=num_agents, steps=steps, seed=seed, labels=labels, extra=extra,
                     check=check)


def probe_of(bank, obs, targets, folds, members=None, ridge=1e-4, names=None):
    """Probes of CALLER-SUPPLIED targets on plain arrays: `obs` float32 [n][O] on the bank's device, `targets` [n][Q <= 15] (any quantity
    a user can compute per row), `folds` [n] of 0 / 1 / 255 PER ROW.  One hidden launch, one accumulate on the hidden blocks of `members`
    (default: all), one on the zero-padded observation, and the fit.  Returns dict(frame, hidden, obs): the `probe_frame` (targets named
    `names`, default t0, t1, ...) and the two `probe_fit` results."""
    import torch
    n, O = (int(v) for v in obs.shape)
    targets, folds = np.asarray(targets, np.float32), np.asarray(folds)
    if targets.ndim != 2 or targets.shape[0] != n or not 1 <= targets.shape[1] <= MAX_TARGETS:
        raise ValueError("probe_of: targets of shape %s, [%d][Q] with Q in 1..%d wanted" % (targets.shape, n, MAX_TARGETS))
    if folds.shape != (n,):
        raise ValueError("probe_of: a fold table of shape %s, one entry per row [%d] wanted" % (folds.shape, n))
    Q = targets.shape[1]
    names = ["t%d" % q for q in range(Q)] if names is None else list(names)
    if len(names) != Q:
        raise ValueError("probe_of: %d names for %d targets" % (len(names), Q))
    # one scene per row: the kernel's fold table is per scene
    plan = ProbePlan(SeatPlan(np.zeros((n, 1), np.int32), bank.K), members, folds=folds)
    H, Op = int(bank.cfg.hidden), padded_width(O)
    plan.check_bytes(H, O)
    dev = obs.device
    hidden = hidden_activations(bank, obs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    panel = np.zeros((n, PANEL), np.float32)
    panel[:, :Q], panel[:, PANEL - 1] = targets, 1.0
    xobs = torch.zeros(n, Op, dtype=torch.float32, device=dev)
    xobs[:, :O] = obs
    acc = ProbeAccumulators(plan.M, H, plan.planes(H), Op, plan.planes(Op, 1), dev)
    rows, count, flags, seat, rows_of = every_row(n, dev)
    shared = (up(panel), rows, count, flags, seat, up(plan.folds), rows_of)
    base = up(np.array([(int(m) * n * 2 + layer) * H for m in plan.members for layer in range(2)], np.int64))
    probe_accumulate(hidden, base, 2 * H, H, *shared, *acc.hidden.tensors())
    probe_accumulate(xobs, up(np.zeros(1, np.int64)), Op, Op, *shared, *acc.obs.tensors())
    torch.cuda.current_stream().synchronize()
    r = acc.read()
    fit_h, fit_o = probe_fit(r["hidden"], ridge, Q), probe_fit(r["obs"], ridge, Q)
    return dict(frame=probe_frame(fit_h, fit_o, plan.members, -1, None, names, n_members=bank.K), hidden=fit_h, obs=fit_o)
