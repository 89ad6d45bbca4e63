"""Iterated adversarial LiDAR: projected gradient descent (PGD) on the LiDAR block of the observation, chosen against the policy that
reads it.

`adversary.py` takes ONE gradient-sign step, a first-order estimate of the worst case inside an L-infinity budget that under-states what
an iterated attack does at the same `eps`, and it needs a hand-chosen direction.  Here a LEVEL (`eps`, `steer`, `throttle`, `alpha`,
`iters`, `random_start`, `untargeted`) is chosen per (scene group, bank member), the keys of the seat tally.  For a row o driven by
member k at that level:

    x_0      o; with `random_start` every LiDAR beam starts at clamp(o[j] + eps * u, 0, 1), u uniform in (-1, 1)
    J(x)     steer * mu_0(x) + throttle * mu_1(x), or, `untargeted`, |mu(x) - mu(o)|^2 / 2: "move the action as far as it goes"
    x_{i+1}  clamp(project(x_i + alpha * sign(dJ/dx at x_i)), 0, 1) on the LiDAR columns, `project` onto [o - eps, o + eps]
    seen     x_iters; every other column is o bit for bit

Rows whose level index is outside [0, L), whose `eps` or `iters` is 0, or whose level is targeted without a direction pass through
bit for bit.  An untargeted level needs `random_start`: at x_0 = o its gradient is zero.  `iters = 1, alpha = eps` without flags is
`adversary.py`'s step; `alpha = 0` with `random_start` (on an untargeted level, or one with a direction, so that the row is not an
identity) is uniform noise of the same budget, the baseline an attack is read against.
`copo_pgd_obs_seats_f32` (csrc/learn_pgd.inc) keeps a 16-row tile resident and runs forward, backward to the
input, step and projection `iters` times in one launch; the random start is drawn from (seed, row, tick, beam), `tick` counting the
launches since `reset`, so a captured graph draws fresh starts at every replay.

An L-infinity budget, the LiDAR block, fp32 operands; the ego / navigation columns, other norms, momentum and restarts and the bfloat16
operand mode are out of scope.

Pieces: `PGDLevel` / `PGDPlan` (numpy only), `PGDBuffers`, `PGDSeatSampler` (the `SeatSampler` whose `_policy_obs` launches the kernel
inside the captured fragment) and `pgd_sweep_rows` (checkpoints x levels x roles as a pandas frame; `evaluate --pgd-sweep`).
"""
from dataclasses import dataclass

import numpy as np

from .bank import DeviceTables, draw_cell_noise
from .crossplay import SeatSampler
from .faults import lidar_columns, sweep_frame, sweep_members, sweep_plan

LEVEL_WORDS = 8
LEVEL_FIELDS = ("eps", "steer", "throttle", "alpha", "iters", "random_start", "untargeted")
MAX_ITERS = 16
RANDOM_START, UNTARGETED = 1, 2


@dataclass(frozen=True)
class PGDLevel:
    """One level of attack.  `eps`: the L-infinity budget on every LiDAR beam (beams are in [0, 1]); `alpha`: the step; `iters`: steps,
    0 .. 16; (`steer`, `throttle`): the direction the mean action is pushed along, unless `untargeted`; `random_start`: start from a
    uniform draw inside the budget.  `PGDLevel()` is the identity, as every level with eps == 0, iters == 0 or, targeted, without a
    direction: rows at it pass through bit for bit.  An untargeted level without a random start is refused: its gradient is zero."""
    eps: float = 0.0
    steer: float = 0.0
    throttle: float = 0.0
    alpha: float = 0.0
    iters: int = 0
    random_start: bool = False
    untargeted: bool = False

    def __post_init__(self):
        for name in ("eps", "steer", "throttle", "alpha"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError("PGDLevel: %s = %r, a finite number wanted" % (name, v))
            object.__setattr__(self, name, float(v))
        if isinstance(self.iters, bool) or not isinstance(self.iters, (int, np.integer)) or not 0 <= self.iters <= MAX_ITERS:
            raise ValueError("PGDLevel: iters = %r, an integer in [0, %d] wanted" % (self.iters, MAX_ITERS))
        object.__setattr__(self, "iters", int(self.iters))
        for name in ("random_start", "untargeted"):
            v = getattr(self, name)
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("PGDLevel: %s = %r, a bool wanted" % (name, v))
            object.__setattr__(self, name, bool(v))
        if self.eps < 0.0 or self.alpha < 0.0:
            raise ValueError("PGDLevel: eps = %r, alpha = %r: neither may be negative" % (self.eps, self.alpha))
        if self.untargeted and not self.random_start:
            raise ValueError("PGDLevel: an untargeted level needs random_start: at the true observation its gradient is zero")

    @property
    def flags(self):
        return (RANDOM_START if self.random_start else 0) | (UNTARGETED if self.untargeted else 0)

    @property
    def is_identity(self):
        return self.eps == 0.0 or self.iters == 0 or (not self.untargeted and self.steer == 0.0 and self.throttle == 0.0)

    def words(self):
        """The level as the eight 32-bit words the kernel reads (int32 bits): eps, steer, throttle, alpha, iters, flags, 0, 0."""
        w = np.zeros(LEVEL_WORDS, np.int32)
        w[:4] = np.array([self.eps, self.steer, self.throttle, self.alpha], np.float32).view(np.int32)
        w[4], w[5] = self.iters, self.flags
        return w

    def as_dict(self):
        return {name: getattr(self, name) for name in LEVEL_FIELDS}


def _levels(levels):
    return [lv if isinstance(lv, PGDLevel) else PGDLevel(**lv) for lv in levels]


class PGDPlan:
    """`levels`: a sequence of `PGDLevel` (or dicts of its fields); `level_of`: int [G][K], the level of bank member k in scene group g
    (an index outside [0, L) leaves the member's rows alone).  Derived: `words` int32 [L][8], `max_iters` (the largest `iters`, at
    least 1: the launch's bound).  Nothing here touches a device."""

    def __init__(self, levels, level_of):
        self.levels = _levels(levels)
        if not self.levels:
            raise ValueError("PGDPlan: no levels")
        self.level_of = np.ascontiguousarray(level_of, np.int32)
        if self.level_of.ndim != 2 or self.level_of.shape[0] < 1 or self.level_of.shape[1] < 1:
            raise ValueError("PGDPlan: level_of of shape %s, [groups][members] wanted" % (self.level_of.shape,))
        self.L, (self.G, self.K) = len(self.levels), self.level_of.shape
        self.words = np.stack([lv.words() for lv in self.levels])
        self.max_iters = max(1, max(lv.iters for lv in self.levels))
        self.checkpoint = self.level = None
        self.share = self.scenes_per_cell = None          # (`sweep` sets them: cells of that many scenes share their action noise)

    def check(self, seat_plan):
        if (seat_plan.n_groups, seat_plan.K) != (self.G, self.K):
            raise ValueError("PGDPlan: level_of is %d groups x %d members, the seat plan has %d x %d" % (
                self.G, self.K, seat_plan.n_groups, seat_plan.K))
        return self

    @classmethod
    def sweep(cls, K, levels, scenes_per_cell, N, share=1.0):
        """(seat plan, PGD plan) of K checkpoints x L levels on the cell layout of `AdversaryPlan.sweep` (`SeatPlan.cells`): with share
        < 1 the bank is doubled, the first round(share * N) slots of a cell are attacked at the cell's level and the rest drive at level
        0, which must then be an identity."""
        return sweep_plan(cls, "PGDPlan.sweep", K, _levels(levels), scenes_per_cell, N, share)


class PGDBuffers(DeviceTables):
    """A PGD plan's tables on the device.  The iteration bound is part of the shape key: it is an argument of the captured launch."""
    KEY = ("L", "G", "K", "max_iters")
    pgd = property(lambda self: self.source)

    @staticmethod
    def tables(plan):
        return dict(level_of=plan.level_of, levels=plan.words), (plan.L, plan.G, plan.K, plan.max_iters)


class PGDSeatSampler(SeatSampler):
    """`SeatSampler` under an iterated attack: per env step `pgd_seats` on the true observation, the seated forward on `obs_seen[t]`,
    the simulator step, the seat tally -- the whole fragment is still one captured graph.  The batch's `obs` stays the TRUE observation;
    `obs_seen` [T][E][N][O] (also `batch["obs_seen"]`, zero-initialised: rows of seats that nobody drives are never written) is what
    the policy was given.  State: `tick` int32 [E N], the launches a seated row has seen since `reset` -- the counter of the random
    starts, advanced by the kernel itself, so every replay of the graph draws new ones; `seed` keys them.  Cells of a `sweep` plan share
    their action noise, as in `AdversarialSeatSampler`."""

    def __init__(self, vec_env, policy, bank, plan, pgd, T, use_graph=True, seed=0):
        import torch
        pgd.check(plan)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.col_lo, self.col_hi = lidar_columns(self.sim.cfg)
        if not 0 <= self.col_lo <= self.col_hi <= self.O:
            raise ValueError("PGDSeatSampler: LiDAR columns [%d, %d) of an observation of %d" % (self.col_lo, self.col_hi, self.O))
        self.pgd_buffers = PGDBuffers(pgd, self.device)
        self.pgd_buffers.on_replace.append(self._loop.reset)
        self.obs_seen = torch.zeros(self.T, self.E, self.N, self.O, dtype=torch.float32, device=self.device)
        self.tick = torch.zeros(self.E * self.N, dtype=torch.int32, device=self.device)

    @property
    def pgd(self):
        return self.pgd_buffers.pgd

    def set_pgd(self, pgd):
        """Another PGD plan, OUTSIDE captured graphs: the same shapes (levels, groups, members, iteration bound) are copied into the
        tables the captured fragment reads, other shapes allocate new ones and drop the graph."""
        self.pgd_buffers.replace(pgd.check(self.seated.plan))

    def reset(self, seeds=None):
        super().reset(seeds)
        self.tick.zero_()

    def _draw_noise(self):
        draw_cell_noise(self.eps, self.pgd.scenes_per_cell)

    def sample(self):
        batch = super().sample()
        batch["obs_seen"] = self.obs_seen
        return batch

    def _policy_obs(self, t):
        self.seated.pgd_seats(self.pgd_buffers, self.obs[t].view(-1, self.O), self.obs_seen[t].view(-1, self.O), self.col_lo, self.col_hi,
                              self.seed, self.tick)
        return self.obs_seen[t]


def pgd_sweep_rows(algo, env, weights_list, levels, share=1.0, scenes_per_cell=4, num_agents=40, steps=1000, seed=0, labels=None,
                   pgd_seed=None, **extra):
    """K populations `weights_list` (one layout) x the attack `levels` (level 0 must be an identity, so that every table carries its
    own baseline), `scenes_per_cell` scenes per cell, the same scenes and the same action noise for every cell, for `steps` env steps
    (rounded up to whole fragments).  The first round(share * num_agents) slots of a scene are attacked at the cell's level, the rest
    are unattacked drivers of the same checkpoint (`PGDPlan.sweep`).  Returns a pandas frame, one row per (checkpoint, level, role),
    with the columns of `adversary_sweep_rows` and the level's seven parameters in the place of its three.  `pgd_seed` (the random
    starts) defaults to `seed`."""
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    K = len(weights_list)
    if K < 1:
        raise ValueError("pgd_sweep_rows: no members")
    levels = _levels(levels)
    if not levels or not levels[0].is_identity:
        raise ValueError("pgd_sweep_rows: level 0 must be an identity (eps 0, iters 0 or no direction), the table's own baseline")
    labels = check_labels(labels, K)
    seats, pgd = PGDPlan.sweep(K, levels, scenes_per_cell, num_agents, share)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        bank = PolicyBank(t.policy, sweep_members(weights_list, pgd))
        smp = PGDSeatSampler(t.env, t.policy, bank, seats, pgd, t.sampler.T, use_graph=graph_flag(t), seed=seed if pgd_seed is None else pgd_seed)
        tally = run_steps(smp, steps).tally.cpu().numpy()
    return sweep_frame(tally, seats, pgd, labels)


def load_levels(path):
    """A JSON list of objects with `PGDLevel`'s fields (missing fields are 0 / false) -> [PGDLevel]."""
    import json
    with open(path) as f:
        raw = json.load(f)
    if not isinstance(raw, list) or not all(isinstance(r, dict) for r in raw):
        raise ValueError("%s: a JSON list of objects wanted" % path)
    return [PGDLevel(**r) for r in raw]
