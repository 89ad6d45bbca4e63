"""Input attribution: which observation columns a checkpoint's action rests on, by integrated gradients (IG) in seated evaluation.

The other studies of `eval/` corrupt the sensors, bound the damage, compare members, remove a neighbour or lower the precision.  This one
answers the first question asked of a checkpoint: which inputs is it driving on?  The raw gradient of `adversary.beam_saliency` is local,
saturates with tanh and is not comparable across checkpoints.  IG (Sundararajan et al., 2017) integrates the gradient of an action mean
along the straight line from a BASELINE row b to the true row o and multiplies by o - b: the attributions of a row sum to
mu_a(o) - mu_a(b), so the table is in units of action per input column and checks itself.

The reference tree has no counterpart of this study; nothing here is taken from it.

A LEVEL (`points`, `baseline`) is chosen per (scene group, bank member), the keys of the seat tally.  `points` = m is the number of
midpoint-rule quadrature points, 1 .. 32.  The baseline is a row of the observation's width whose NaN entries mean "this column keeps
the row's own value": such a column gets an attribution of exactly 0.  `AttributionLevel.clear_road(cfg)` sets the LiDAR block to 1.0,
the hit fraction of a beam without a return (SPEC.md section 3.4: a beam's value is the minimum of its hits and the range), and masks
everything else -- "which beams matter"; `zeros(cfg)` sets every column to 0; `row(array)` is any row.  `AttributionLevel()` is the
identity: its rows are listed and not attributed.

`copo_ig_obs_seats_f32` (csrc/learn_attrib.inc) keeps a 16-row tile resident and runs, per quadrature point, one
forward and the backward pass of BOTH action heads down to the whole input row, the running sums on chip; it writes `attr`
[rows][2][O] and `heads` [rows][8] (`HEAD_WORDS`: the means at o and at b, the quadrature residual `gap` of either head, valid, m).
`copo_attrib_tally` folds a step's outputs into integers per (group, member): `words` [G][K][8] (`ATTRIB_WORDS`) and `cols`
[G][K][2][O], sums of |value| in 2^-32 steps (`Q32`).  Attribution changes nobody's driving: the policy acts on the true observation.

Pieces, each on its base in `levels.py`: `AttributionLevel` / `AttributionPlan` (numpy only), `AttributionBuffers`,
`AttributionSeatSampler` (whose `_policy_obs` launches the kernel inside the captured fragment), `attribution_rows` (checkpoints x levels
as a pandas frame; `evaluate --attribution`) and `load_levels`; its own: `attrib_tally`, `attribution_frame`, `attribution_profile` and
`integrated_gradients` (one launch on a plain observation array).
"""
from dataclasses import dataclass

import numpy as np

from .crossplay import SEAT_WORDS, tally_rates
from .levels import LevelBuffers, LevelPlan, LevelSeatSampler, lidar_columns, run_sweep

LEVEL_WORDS = 4
MAX_POINTS = 32
HEADS = ("steer", "throttle")
HEAD_WORDS = ("mu_steer", "mu_throttle", "mu_base_steer", "mu_base_throttle", "gap_steer", "gap_throttle", "valid", "points")
ATTRIB_WORDS = ("rows", "abs_delta_steer_q32", "abs_delta_throttle_q32", "abs_gap_steer_q32", "abs_gap_throttle_q32", "max_gap_q32", "unattributed",
                "reserved")
BLOCKS = ("ego", "navi", "lidar_front", "lidar_left", "lidar_rear", "lidar_right")
NAMED_BASELINES = ("clear_road", "zeros")
CLEAR_BEAM = 1.0          # the hit fraction of a beam without a return
Q32 = 4294967296.0


@dataclass(frozen=True, eq=False)
class AttributionLevel:
    """One level of attribution.  `points`: quadrature points, 1 .. 32; `baseline`: "clear_road" or "zeros" (made into a row by the
    plan's `resolve`, which knows the simulator's columns) or a row of floats whose NaN entries keep the row's own value.
    `AttributionLevel()` (points 0, no baseline) is the identity."""
    points: int = 0
    baseline: object = None

    def __post_init__(self):
        p = self.points
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p <= MAX_POINTS:
            raise ValueError("AttributionLevel: points = %r, an integer in [1, %d] wanted" % (p, MAX_POINTS))
        object.__setattr__(self, "points", int(p))
        b = self.baseline
        if (b is None) != (self.points == 0):
            raise ValueError("AttributionLevel: points = %r with baseline %s: points in [1, %d] and a baseline, or neither (the identity)" % (
                p, "None" if b is None else "given", MAX_POINTS))
        if b is None or isinstance(b, str):
            if b is not None and b not in NAMED_BASELINES:
                raise ValueError("AttributionLevel: baseline = %r, one of %s or a row wanted" % (b, ", ".join(repr(n) for n in NAMED_BASELINES)))
            return
        # (a JSON null inside a row is a masked column)
        row = np.array([np.nan if v is None else v for v in b] if isinstance(b, (list, tuple)) else b, np.float64)
        if row.ndim != 1 or row.size < 1:
            raise ValueError("AttributionLevel: a baseline of shape %s, one row wanted" % (row.shape,))
        if np.isinf(row).any() or (np.abs(row[~np.isnan(row)]) > np.finfo(np.float32).max).any():
            raise ValueError("AttributionLevel: a baseline entry is neither a finite number nor a NaN mask")
        row = row.astype(np.float32)
        row.setflags(write=False)
        object.__setattr__(self, "baseline", row)

    @classmethod
    def clear_road(cls, cfg, points=8):
        """Every LiDAR beam of `cfg` (a `SimConfig`) reads "nothing in range"; every other column keeps the row's own value."""
        lidar_columns(cfg)
        return cls(points, "clear_road")

    @classmethod
    def zeros(cls, cfg, points=8):
        return cls(points, "zeros")

    @classmethod
    def row(cls, array, points=8):
        return cls(points, np.asarray(array))

    @property
    def is_identity(self):
        return self.points == 0

    @property
    def baseline_name(self):
        return "none" if self.baseline is None else self.baseline if isinstance(self.baseline, str) else "row"

    def baseline_row(self, cfg, in_dim):
        """The baseline as float32 [in_dim]; the identity's is all NaN.  A row of another width is refused."""
        b = self.baseline
        if b is None:
            return np.full(in_dim, np.nan, np.float32)
        if isinstance(b, str) and b == "zeros":
            return np.zeros(in_dim, np.float32)
        if isinstance(b, str):
            lo, hi = lidar_columns(cfg)
            if not 0 <= lo <= hi <= in_dim:
                raise ValueError("AttributionLevel: LiDAR columns [%d, %d) of an observation of %d" % (lo, hi, in_dim))
            out = np.full(in_dim, np.nan, np.float32)
            out[lo:hi] = CLEAR_BEAM
            return out
        if b.shape[0] != in_dim:
            raise ValueError("AttributionLevel: a baseline of %d columns for an observation of %d" % (b.shape[0], in_dim))
        return np.array(b, np.float32)

    def words(self):
        """The level as the four 32-bit words the kernel reads: points, flags (0), 0, 0."""
        return np.array([self.points, 0, 0, 0], np.int32)

    def as_dict(self):
        return dict(points=self.points, baseline=self.baseline_name)

    def _key(self):
        b = self.baseline
        return self.points, (b if b is None or isinstance(b, str) else b.view(np.uint32).tobytes())

    def __eq__(self, other):
        return isinstance(other, AttributionLevel) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


class AttributionPlan(LevelPlan):
    """`LevelPlan` of `AttributionLevel`s; `words` int32 [L][4], `max_points` (the largest `points`, at least 1: the launch's bound) and,
    once `resolve(cfg, in_dim)` has run, `base` float32 [L][in_dim] and `in_dim`."""
    LEVEL = AttributionLevel

    def __init__(self, levels, level_of):
        super().__init__(levels, level_of)
        self.max_points = max(1, max(lv.points for lv in self.levels))
        self.base = self.in_dim = None

    def resolve(self, cfg, in_dim):
        """The baselines as rows of an observation of `in_dim` columns of the simulator `cfg` (named baselines read its columns)."""
        self.base = np.stack([lv.baseline_row(cfg, int(in_dim)) for lv in self.levels])
        self.in_dim = int(in_dim)
        return self

    @classmethod
    def sweep(cls, K, levels, scenes_per_cell, N):
        """(seat plan, attribution plan) of K checkpoints x L levels on the cell layout of `LevelPlan.sweep` at share 1: every slot of
        cell (k, l) is member k, attributed at level l.  There are no roles: nobody is impaired."""
        return super().sweep(K, levels, scenes_per_cell, N, 1.0)


class AttributionBuffers(LevelBuffers):
    """A resolved attribution plan's tables on the device; the bound on the points and the row width are part of the shape key."""
    KEY = ("L", "G", "K", "max_points", "in_dim")

    @classmethod
    def tables(cls, plan):
        if plan.base is None:
            raise ValueError("AttributionBuffers: the plan's baselines are not rows yet (AttributionPlan.resolve)")
        return dict(level_of=plan.level_of, levels=plan.words, base=plan.base), tuple(getattr(plan, name) for name in cls.KEY)


def attrib_tally(flags, attr, heads, plan_buffers, words, cols):
    """One step's `flags` uint8 [E][N], `attr` float32 [E N][2][O] and `heads` float32 [E N][8] added to `words` int64 [G][K][8]
    (`ATTRIB_WORDS`) and `cols` int64 [G][K][2][O] by the seat plan's seat and group tables.  Both accumulate (the max word keeps the
    largest); the caller clears them.  One launch on the current stream."""
    from .. import _capi
    pb = plan_buffers
    _capi.check(_capi.lib.copo_attrib_tally(flags.data_ptr(), attr.data_ptr(), heads.data_ptr(), pb.seat.data_ptr(), pb.group.data_ptr(), pb.E, pb.N,
                                            pb.K, pb.G, int(cols.shape[-1]), words.data_ptr(), cols.data_ptr(), _capi.current_stream()))


class AttributionSeatSampler(LevelSeatSampler):
    """`SeatSampler` with attribution: per env step `attribute_seats` on the true observation into `attr[t]` / `heads[t]`, the seated
    forward on the SAME true observation, the simulator step, the seat tally and the attribution tally -- the whole fragment is still one
    captured graph.  Actions, flags and the seat tally are a plain `SeatSampler`'s.  `attr` [T][E][N][2][O] and `heads` [T][E][N][8]
    (also in the batch, zero-initialised: rows of seats that nobody drives are never written and read as invalid); `attrib_words` int64
    [G][K][8] (`ATTRIB_WORDS`) and `attrib_cols` int64 [G][K][2][O] accumulate until `clear_tally()`.  Cells of a `sweep` plan share
    their action noise.  A plan whose baselines are still names is resolved against the simulator's columns here."""

    BUFFERS = AttributionBuffers
    SEEN = False          # (nothing is perturbed: the policy reads the true observation)
    attrib_buffers = property(lambda self: self.level_buffers)
    attribution = property(lambda self: self.level_plan)

    def __init__(self, vec_env, policy, bank, plan, attribution, T, use_graph=True):
        import torch
        attribution.resolve(vec_env.sim.cfg, int(bank.cfg.pol.in_dim))
        super().__init__(vec_env, policy, bank, plan, attribution, T, use_graph=use_graph)
        self.attr = torch.zeros(self.T, self.E, self.N, 2, self.O, dtype=torch.float32, device=self.device)
        self.heads = torch.zeros(self.T, self.E, self.N, len(HEAD_WORDS), dtype=torch.float32, device=self.device)
        self.attrib_words = torch.zeros(plan.n_groups, bank.K, len(ATTRIB_WORDS), dtype=torch.int64, device=self.device)
        self.attrib_cols = torch.zeros(plan.n_groups, bank.K, 2, self.O, dtype=torch.int64, device=self.device)

    def set_levels(self, levels):
        super().set_levels(levels.resolve(self.sim.cfg, self.O))

    def clear_tally(self):
        super().clear_tally()
        self.attrib_words.zero_()
        self.attrib_cols.zero_()

    def sample(self):
        batch = super().sample()
        batch["attr"], batch["heads"] = self.attr, self.heads
        return batch

    def _policy_obs(self, t):
        self.seated.attribute_seats(self.attrib_buffers, self.obs[t].view(-1, self.O), self.attr[t].view(-1, 2, self.O),
                                    self.heads[t].view(-1, len(HEAD_WORDS)))
        return self.obs[t]

    def _step(self, t):
        super()._step(t)
        attrib_tally(self.flags[t], self.attr[t], self.heads[t], self.seated.buffers, self.attrib_words, self.attrib_cols)


def column_blocks(cfg, in_dim):
    """`BLOCKS` as index arrays into an observation row of `in_dim` columns: the first `ego_dim` columns, the next `navi_dim`, and the
    LiDAR block in quadrants BY BEAM INDEX -- beam 0 looks ahead and beam k is turned clockwise, so with n beams the front quadrant is
    the beams within n / 8 of beam 0 on either side, then right, rear and left follow in index order.  Columns behind the LiDAR block
    belong to no block: the shares are over the six blocks' total."""
    ego, navi, n = int(cfg.ego_dim), int(cfg.navi_dim), int(cfg.num_lasers)
    lo = ego + navi
    if lo + n > int(in_dim):
        raise ValueError("column_blocks: %d + %d + %d columns in an observation of %d" % (ego, navi, n, in_dim))
    beams = np.arange(n)
    quadrant = ((beams + n // 8) % n) * 4 // max(n, 1)          # 0 front, 1 right, 2 rear, 3 left
    at = dict(front=0, right=1, rear=2, left=3)
    out = dict(ego=np.arange(ego), navi=np.arange(ego, lo))
    for name in BLOCKS[2:]:
        out[name] = lo + beams[quadrant == at[name.split("_")[1]]]
    return out


def attrib_rates(words, cols, blocks):
    """The derived columns of one cell: `share_<block>_<head>` (the block's sum of `cols` over the six blocks' total; they sum to 1 per
    head), `mean_abs_delta_<head>`, `mean_gap_<head>` over the attributed rows and `max_gap`; NaN where there is nothing to divide by."""
    w = dict(zip(ATTRIB_WORDS, (int(v) for v in words)))
    n = w["rows"]
    mean = lambda q: q / Q32 / n if n > 0 else float("nan")  # noqa: E731
    out = {}
    for a, head in enumerate(HEADS):
        sums = {name: int(sum(int(v) for v in cols[a][idx])) for name, idx in blocks.items()}
        total = sum(sums.values())
        for name in BLOCKS:
            out["share_%s_%s" % (name, head)] = sums[name] / total if total > 0 else float("nan")
    for head in HEADS:
        out["mean_abs_delta_" + head] = mean(w["abs_delta_%s_q32" % head])
        out["mean_gap_" + head] = mean(w["abs_gap_%s_q32" % head])
    out["max_gap"] = w["max_gap_q32"] / Q32 if n > 0 else float("nan")
    return out


def attribution_frame(words, cols, tally, seats, plan, cfg, labels=None):
    """The attribution tally (`words` [G][K][8], `cols` [G][K][2][O], numpy int64) and the seat tally [G][K][8] of a `sweep` plan as a
    frame: one row per (checkpoint, level) with the level's fields, the raw words, the block shares per head (`column_blocks` of the
    `SimConfig` `cfg`), `mean_abs_delta_*`, `mean_gap_*`, `max_gap`, then the seat tally's words and rates."""
    import pandas as pd
    labels = list(range(plan.n_checkpoints)) if labels is None else list(labels)
    blocks = column_blocks(cfg, cols.shape[-1])
    rows = []
    for g in range(seats.n_groups):
        k, lv = int(plan.checkpoint[g]), int(plan.level[g])
        aw, sw = [int(v) for v in words[g, k]], [int(v) for v in tally[g, k]]
        rows.append(dict(checkpoint=k, label=labels[k], level=lv, member=k, seats=seats.N, **plan.levels[lv].as_dict(), **dict(zip(ATTRIB_WORDS, aw)),
                         **attrib_rates(aw, cols[g, k], blocks), **dict(zip(SEAT_WORDS, sw)), **tally_rates(sw)))
    return pd.DataFrame(rows)


def attribution_profile(words, cols, seats, plan, labels=None):
    """The per-column means behind the shares, for plots: one row per (checkpoint, level, head, column) with `mean_abs_attr` = the
    column's sum over the attributed rows (NaN without one)."""
    import pandas as pd
    labels = list(range(plan.n_checkpoints)) if labels is None else list(labels)
    rows = []
    for g in range(seats.n_groups):
        k, lv = int(plan.checkpoint[g]), int(plan.level[g])
        n = int(words[g, k][0])
        for a, head in enumerate(HEADS):
            for j, q in enumerate(cols[g, k, a]):
                rows.append(dict(checkpoint=k, label=labels[k], level=lv, head=head, column=j, mean_abs_attr=int(q) / Q32 / n if n > 0 else float("nan")))
    return pd.DataFrame(rows)


def attribution_rows(algo, env, weights_list, levels, scenes_per_cell=4, num_agents=40, steps=1000, seed=0, labels=None, **extra):
    """K populations `weights_list` (one layout) x the attribution `levels`, `scenes_per_cell` scenes per cell, the same scenes and the
    same action noise for every cell, for `steps` env steps (rounded up to whole fragments).  Every slot of a cell is driven by the
    cell's checkpoint on the true observation and attributed at the cell's level (`AttributionPlan.sweep`).  Returns
    `attribution_frame`'s table, one row per (checkpoint, level)."""
    def some_levels():          # (no level-0 rule: nobody is impaired, so there is no baseline to carry)
        checked = AttributionPlan.as_levels(levels)
        if not checked:
            raise ValueError("attribution_rows: no levels")
        return checked

    def frame(smp, seats, plan, labels):
        return attribution_frame(smp.attrib_words.cpu().numpy(), smp.attrib_cols.cpu().numpy(), smp.tally.cpu().numpy(), seats, plan, smp.sim.cfg, labels)

    return run_sweep("attribution_rows", AttributionPlan, algo, env, weights_list, some_levels,
                     lambda t, bank, seats, plan, use_graph: AttributionSeatSampler(t.env, t.policy, bank, seats, plan, t.sampler.T, use_graph=use_graph),
                     frame, labels=labels, scenes_per_cell=scenes_per_cell, num_agents=num_agents, steps=steps, seed=seed, extra=extra)


def load_levels(path):
    """A JSON list of objects {points, baseline} -> [AttributionLevel]; `baseline` is "clear_road", "zeros" or a list of numbers in which
    null masks a column; {} is the identity."""
    from . import levels as _levels
    return _levels.load_levels(path, AttributionLevel)


def integrated_gradients(bank_or_policy, obs, baseline, points=8, member=0):
    """(attr [n][2][O], heads [n][8]) of every row of obs [n][O] (a float32 tensor on the bank's device) under member `member`, from the
    baseline row `baseline` [O] (NaN entries keep the row's own value) with `points` quadrature points: one launch.
    `bank_or_policy`: a `PolicyBank`, or a trainer policy with a fused learner, whose current weights become a bank of one."""
    import torch
    from types import SimpleNamespace
    from .bank import PolicyBank
    bank = bank_or_policy
    if not isinstance(bank, PolicyBank):
        bank = PolicyBank(bank, [{k: v.detach().cpu().numpy() for k, v in bank.model.state_dict().items()}])
    if not 0 <= int(member) < bank.K:
        raise ValueError("integrated_gradients: member %r of a bank of %d" % (member, bank.K))
    n, O = int(obs.shape[0]), int(bank.cfg.pol.in_dim)
    plan = AttributionPlan([AttributionLevel.row(baseline, points)], np.zeros((1, bank.K), np.int32)).resolve(None, O)
    rows = np.zeros((bank.K, n), np.int64)
    rows[int(member)] = np.arange(n)
    counts = np.zeros(bank.K, np.int32)
    counts[int(member)] = n
    dev = lambda a: torch.from_numpy(a).to(obs.device)  # noqa: E731
    pb = SimpleNamespace(K=bank.K, G=1, N=1, E=n, cap=n, n_out=n, rows=dev(rows), counts=dev(counts), group=dev(np.zeros(n, np.int32)))
    attr = torch.zeros(n, 2, O, dtype=torch.float32, device=obs.device)
    heads = torch.zeros(n, len(HEAD_WORDS), dtype=torch.float32, device=obs.device)
    bank.sync_mirror()
    bank.attribute_seats(pb, AttributionBuffers(plan, obs.device), obs, attr, heads)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return attr, heads
