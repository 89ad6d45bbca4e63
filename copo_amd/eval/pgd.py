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

Pieces, each on its base in `levels.py`: `PGDLevel` / `PGDPlan` (numpy only), `PGDBuffers`, `PGDSeatSampler` (whose `_policy_obs` launches
the kernel inside the captured fragment) and `pgd_sweep_rows` (checkpoints x levels x roles as a pandas frame; `evaluate --pgd-sweep`).
"""
from dataclasses import dataclass

import numpy as np

from . import levels as _levels
from .levels import LevelBuffers, LevelPlan, LevelSeatSampler, baseline_levels, finite_fields, role_frame, run_sweep

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
        finite_fields(self, ("eps", "steer", "throttle", "alpha"))
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


class PGDPlan(LevelPlan):
    """`LevelPlan` of `PGDLevel`s; `words` int32 [L][8], and `max_iters` (the largest `iters`, at least 1: the launch's bound)."""
    LEVEL = PGDLevel

    def __init__(self, levels, level_of):
        super().__init__(levels, level_of)
        self.max_iters = max(1, max(lv.iters for lv in self.levels))


class PGDBuffers(LevelBuffers):
    """A PGD plan's tables on the device.  The iteration bound is part of the shape key: it is an argument of the captured launch."""
    KEY = ("L", "G", "K", "max_iters")
    pgd = property(lambda self: self.source)


class PGDSeatSampler(LevelSeatSampler):
    """`SeatSampler` under an iterated attack: per env step `pgd_seats` on the true observation, the seated forward on `obs_seen[t]`,
    the simulator step, the seat tally -- the whole fragment is still one captured graph.  The batch's `obs` stays the TRUE observation;
    `obs_seen` [T][E][N][O] (also `batch["obs_seen"]`, zero-initialised: rows of seats that nobody drives are never written) is what
    the policy was given.  State: `tick` int32 [E N], the launches a seated row has seen since `reset` -- the counter of the random
    starts, advanced by the kernel itself, so every replay of the graph draws new ones; `seed` keys them.  Cells of a `sweep` plan share
    their action noise, as in `AdversarialSeatSampler`."""

    BUFFERS = PGDBuffers
    pgd_buffers = property(lambda self: self.level_buffers)
    pgd = property(lambda self: self.level_plan)
    set_pgd = LevelSeatSampler.set_levels

    def __init__(self, vec_env, policy, bank, plan, pgd, T, use_graph=True, seed=0):
        import torch
        super().__init__(vec_env, policy, bank, plan, pgd, T, use_graph=use_graph)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.tick = torch.zeros(self.E * self.N, dtype=torch.int32, device=self.device)

    def reset(self, seeds=None):
        super().reset(seeds)
        self.tick.zero_()

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
    return run_sweep("pgd_sweep_rows", PGDPlan, algo, env, weights_list,
                     lambda: baseline_levels("pgd_sweep_rows", PGDPlan, levels, "an identity (eps 0, iters 0 or no direction)"),
                     lambda t, bank, seats, pgd, use_graph: PGDSeatSampler(t.env, t.policy, bank, seats, pgd, t.sampler.T, use_graph=use_graph,
                                                                           seed=seed if pgd_seed is None else pgd_seed),
                     role_frame, labels=labels, scenes_per_cell=scenes_per_cell, num_agents=num_agents, steps=steps, seed=seed, extra=extra, share=share)


def load_levels(path):
    """A JSON list of objects with `PGDLevel`'s fields (missing fields are 0 / false) -> [PGDLevel]."""
    return _levels.load_levels(path, PGDLevel)
