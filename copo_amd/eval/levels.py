"""What the LiDAR studies of seated evaluation share: `faults.py`, `adversary.py`, `pgd.py` and `certify.py` each choose a LEVEL per (scene
group, bank member), the keys of the seat tally, and differ in what a level holds and in what their launch does with it.

Pieces: `finite_fields` (the number check of every level dataclass), `LevelPlan` (levels + `level_of`, numpy only; a study's plan is a
subclass that names its level class in `LEVEL`), `sweep_plan` / `sweep_members` / `sweep_frame` (the checkpoints x levels x roles layout
of `SeatPlan.cells`, its bank and its frame), `lidar_columns`, `LevelBuffers` (a plan's tables on the device), `LevelSeatSampler` (the
`SeatSampler` that owns the buffers, the LiDAR columns, the shared cell noise and `obs_seen`; a study adds its `_policy_obs` / `_step`
launches and its own state), `run_sweep` (the session of the four `*_sweep_rows`) and `load_levels`.
"""
import numpy as np

from .bank import DeviceTables, draw_cell_noise
from .crossplay import SEAT_WORDS, SeatPlan, SeatSampler, tally_rates


def finite_fields(level, names):
    """The fields `names` of the frozen dataclass `level` as floats; anything but a finite number is refused."""
    for name in names:
        v = getattr(level, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s: %s = %r, a finite number wanted" % (type(level).__name__, name, v))
        object.__setattr__(level, name, float(v))


class LevelPlan:
    """`levels`: a sequence of `LEVEL` (or dicts of its fields); `level_of`: int [G][K], the level of bank member k in scene group g (an
    index outside [0, L) leaves the member's rows alone).  Derived: `words` [L][the level's words], in the dtype the kernels read.
    Nothing here touches a device."""
    LEVEL = None          # the level dataclass of the subclass

    @classmethod
    def as_levels(cls, levels):
        return [lv if isinstance(lv, cls.LEVEL) else cls.LEVEL(**lv) for lv in levels]

    def __init__(self, levels, level_of):
        who = type(self).__name__
        self.levels = self.as_levels(levels)
        if not self.levels:
            raise ValueError("%s: no levels" % who)
        self.level_of = np.ascontiguousarray(level_of, np.int32)
        if self.level_of.ndim != 2 or self.level_of.shape[0] < 1 or self.level_of.shape[1] < 1:
            raise ValueError("%s: level_of of shape %s, [groups][members] wanted" % (who, self.level_of.shape,))
        self.L, (self.G, self.K) = len(self.levels), self.level_of.shape
        self.words = np.stack([lv.words() for lv in self.levels])
        self.checkpoint = self.level = None
        self.share = self.scenes_per_cell = None          # (`sweep` sets them: cells of that many scenes share their action noise)

    def check(self, seat_plan):
        if (seat_plan.n_groups, seat_plan.K) != (self.G, self.K):
            raise ValueError("%s: level_of is %d groups x %d members, the seat plan has %d x %d" % (
                type(self).__name__, self.G, self.K, seat_plan.n_groups, seat_plan.K))
        return self

    @classmethod
    def sweep(cls, K, levels, scenes_per_cell, N, share=1.0):
        """(seat plan, level plan) of K checkpoints x L levels: one scene group per cell, group k * L + l = scenes [g S, (g + 1) S), S =
        `scenes_per_cell`.  share == 1: every slot of the cell is member k at level l, a bank of K members.  share < 1: the bank holds
        every checkpoint TWICE, members k and K + k with the same weights (`sweep_members`); the first round(share * N) slots are member
        K + k at level l, the rest member k at level 0, which must then be an identity: the tally keeps the impaired and the healthy
        drivers of a scene apart.  The seat plan declares `replica_scenes` = S, so `SeatSampler.reset` gives every cell the same scenes."""
        return sweep_plan(cls, cls.__name__ + ".sweep", K, cls.as_levels(levels), scenes_per_cell, N, share)


def sweep_plan(cls, who, K, levels, scenes_per_cell, N, share):
    """(seat plan, `cls(levels, level_of)`) on the cell layout of `SeatPlan.cells`, the layout's attributes on the level plan.  With
    share < 1 the healthy seats drive at level 0, which must be the identity."""
    seats, level_of, attrs = SeatPlan.cells(K, len(levels), scenes_per_cell, N, share, who)
    if attrs["doubled"] and not levels[0].is_identity:
        raise ValueError("%s: with share < 1 the healthy seats drive at level 0, which must be the identity" % who)
    plan = cls(levels, level_of)
    vars(plan).update(attrs)
    return seats, plan


def sweep_members(weights_list, plan):
    """The bank of a `sweep` plan: the checkpoints, twice where the plan doubles them."""
    weights_list = list(weights_list)
    return weights_list + weights_list if plan.doubled else weights_list


def lidar_columns(cfg):
    """[col_lo, col_hi) of the LiDAR block in the observation row of a `SimConfig`."""
    lo = int(cfg.ego_dim) + int(cfg.navi_dim)
    return lo, lo + int(cfg.num_lasers)


class LevelBuffers(DeviceTables):
    """A level plan's tables on the device: `level_of` and the level words as `levels`; the shape key is the plan's attributes `KEY`."""
    KEY = ("L", "G", "K")

    @classmethod
    def tables(cls, plan):
        return dict(level_of=plan.level_of, levels=plan.words), tuple(getattr(plan, name) for name in cls.KEY)


class LevelSeatSampler(SeatSampler):
    """`SeatSampler` with a level plan: the plan's tables on the device (`level_buffers`, a `BUFFERS`; replacing them with other shapes
    drops the captured graph), the LiDAR columns of the observation, and the action noise of a `sweep` plan: ordinary noise, then the
    first cell's draw is copied to every cell, as `BankSampler` copies one member's -- the cells already share their scene seeds, so at
    the identity level two cells differ by their checkpoint only.  `SEEN`: the sampler keeps `obs_seen` [T][E][N][O] (also
    `batch["obs_seen"]`, zero-initialised), what the policy was given; the batch's `obs` stays the TRUE observation."""
    BUFFERS = LevelBuffers
    SEEN = True

    def __init__(self, vec_env, policy, bank, plan, levels, T, use_graph=True):
        import torch
        levels.check(plan)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.col_lo, self.col_hi = lidar_columns(self.sim.cfg)
        if not 0 <= self.col_lo <= self.col_hi <= self.O:
            raise ValueError("%s: LiDAR columns [%d, %d) of an observation of %d" % (type(self).__name__, self.col_lo, self.col_hi, self.O))
        self.level_buffers = self.BUFFERS(levels, self.device)
        self.level_buffers.on_replace.append(self._loop.reset)
        if self.SEEN:
            self.obs_seen = torch.zeros(self.T, self.E, self.N, self.O, dtype=torch.float32, device=self.device)

    @property
    def level_plan(self):
        return self.level_buffers.source

    def set_levels(self, levels):
        """Another level plan, OUTSIDE captured graphs: the same shapes (the buffers' `KEY`) are copied into the tables the captured
        fragment reads, other shapes allocate new ones and drop the graph."""
        self.level_buffers.replace(levels.check(self.seated.plan))

    def _draw_noise(self):
        draw_cell_noise(self.eps, self.level_plan.scenes_per_cell)

    def sample(self):
        batch = super().sample()
        if self.SEEN:
            batch["obs_seen"] = self.obs_seen
        return batch


def sweep_frame(tally, seats, plan, labels=None):
    """The tally [G][K][8] (numpy int64) of a `sweep` plan as a frame: one row per (checkpoint, level, role), the columns of
    `fault_sweep_rows`; the level's columns are whatever its levels' `as_dict()` names."""
    import pandas as pd
    labels = list(range(plan.n_checkpoints)) if labels is None else list(labels)
    K, N, n_imp = plan.n_checkpoints, seats.N, plan.n_impaired
    rows = []
    for g in range(seats.n_groups):
        k, lv = int(plan.checkpoint[g]), int(plan.level[g])
        roles = ([("impaired", k + K if plan.doubled else k, lv)] if n_imp > 0 else []) + ([("healthy", k, 0)] if n_imp < N else [])
        for role, member, own in roles:
            w = [int(v) for v in tally[g, member]]
            rows.append(dict(checkpoint=k, label=labels[k], level=lv, role=role, member=member, share=plan.share, seats=n_imp if role == "impaired"
                             else N - n_imp, own_level=own, **plan.levels[lv].as_dict(), **dict(zip(SEAT_WORDS, w)), **tally_rates(w)))
    return pd.DataFrame(rows)


def baseline_levels(who, plan_cls, levels, what):
    """`levels` as `plan_cls`'s levels; a sweep with roles wants level 0 to be `what`, an identity: every table carries its own baseline."""
    levels = plan_cls.as_levels(levels)
    if not levels or not levels[0].is_identity:
        raise ValueError("%s: level 0 must be %s, the table's own baseline" % (who, what))
    return levels


def run_sweep(who, plan_cls, algo, env, weights_list, levels, sampler, frame, *, labels, scenes_per_cell, num_agents, steps, seed, extra, **sweep_args):
    """The session of a `*_sweep_rows`: K populations `weights_list` (one layout) x the levels on `plan_cls.sweep`'s cells, the bank
    of `sweep_members`, `sampler(t, bank, seats, plan, use_graph)` run for `steps` env steps (rounded up to whole fragments), then
    `frame(sampler, seats, plan, labels)` while the session is still open.  `levels`: a callable that returns the study's checked
    levels (its level-0 rule, or none); it is called behind the member count and in front of the labels, the order the four functions
    always refused in."""
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    K = len(weights_list)
    if K < 1:
        raise ValueError("%s: no members" % who)
    levels = levels()
    labels = check_labels(labels, K)
    seats, plan = plan_cls.sweep(K, levels, scenes_per_cell, num_agents, **sweep_args)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        smp = sampler(t, PolicyBank(t.policy, sweep_members(weights_list, plan)), seats, plan, graph_flag(t))
        return frame(run_steps(smp, steps), seats, plan, labels)


def role_frame(smp, seats, plan, labels):
    """`run_sweep`'s frame of the studies with roles: `sweep_frame` of the seat tally."""
    return sweep_frame(smp.tally.cpu().numpy(), seats, plan, labels)


def load_levels(path, level_cls):
    """A JSON list of objects with `level_cls`'s fields (missing fields take their defaults) -> [level_cls]."""
    import json
    with open(path) as f:
        raw = json.load(f)
    if not isinstance(raw, list) or not all(isinstance(r, dict) for r in raw):
        raise ValueError("%s: a JSON list of objects wanted" % path)
    return [level_cls(**r) for r in raw]
