"""Adversarial LiDAR: one gradient-sign step (FGSM) on the LiDAR block of the observation, chosen against the policy that reads it.

`faults.py` asks how a population drives when its LiDAR is noisy; noise is the weak form of that question.  Here the perturbation of
the same size is the worst one inside an L-infinity budget, to first order.  A LEVEL (`eps`, `steer`, `throttle`) is chosen per (scene
group, bank member), the keys of the seat tally.  For a row driven by member k at that level:

    mu(o)   the first two outputs of member k's policy net on the TRUE observation row o (the action means, before sampling)
    J(o)    steer * mu_0(o) + throttle * mu_1(o): a targeted attack, (0, +1) = "make it accelerate"
    g       dJ / do
    seen[j] clamp(o[j] + eps * sign(g[j]), 0, 1) on the LiDAR columns (sign(0) = 0), o[j] bit for bit on every other column

Rows whose level index is outside [0, L), whose `eps` is 0 or whose `steer` and `throttle` are both 0 pass through bit for bit.  The
policy then acts on `seen` through the unchanged seat forward.  `copo_adv_obs_seats_f32` (csrc/learn_inputgrad.inc, DESIGN.md section
8m) does forward and backward-to-input of a seated bank in one launch; its raw gradient is an optional output, the per-beam saliency
of a checkpoint (`beam_saliency`).

One step, an L-infinity budget, the LiDAR block, fp32 operands.  Multi-step PGD and untargeted objectives are `pgd.py`'s; the ego /
navigation columns and the bfloat16 operand mode are out of scope.

Pieces, each on its base in `levels.py`: `AdversaryLevel` / `AdversaryPlan` (numpy only), `AdversaryBuffers`, `AdversarialSeatSampler`
(whose `_policy_obs` launches the kernel inside the captured fragment), `adversary_sweep_rows` (checkpoints x levels x roles as a pandas
frame; `evaluate --adversary-sweep`); and `beam_saliency`.
"""
from dataclasses import dataclass

import numpy as np

from . import levels as _levels
from .levels import LevelBuffers, LevelPlan, LevelSeatSampler, baseline_levels, finite_fields, role_frame, run_sweep

LEVEL_WORDS = 4
LEVEL_FIELDS = ("eps", "steer", "throttle")


@dataclass(frozen=True)
class AdversaryLevel:
    """One level of attack.  `eps`: the L-infinity budget on every LiDAR beam (beams are in [0, 1]); (`steer`, `throttle`): the direction
    the mean action is pushed along.  `AdversaryLevel()` is the identity, as every level with eps == 0 or steer == throttle == 0: rows at
    it pass through bit for bit."""
    eps: float = 0.0
    steer: float = 0.0
    throttle: float = 0.0

    def __post_init__(self):
        finite_fields(self, LEVEL_FIELDS)
        if self.eps < 0.0:
            raise ValueError("AdversaryLevel: eps = %r is negative" % self.eps)

    @property
    def is_identity(self):
        return self.eps == 0.0 or (self.steer == 0.0 and self.throttle == 0.0)

    def words(self):
        """The level as the four floats the kernel reads: eps, steer, throttle, 0."""
        return np.array([self.eps, self.steer, self.throttle, 0.0], np.float32)

    def as_dict(self):
        return {name: getattr(self, name) for name in LEVEL_FIELDS}


class AdversaryPlan(LevelPlan):
    """`LevelPlan` of `AdversaryLevel`s; `words` float32 [L][4]."""
    LEVEL = AdversaryLevel


class AdversaryBuffers(LevelBuffers):
    """An adversary plan's tables on the device."""
    adversary = property(lambda self: self.source)


class AdversarialSeatSampler(LevelSeatSampler):
    """`SeatSampler` under attack: per env step `perturb_seats` on the true observation, the seated forward on `obs_seen[t]`, the
    simulator step, the seat tally -- the whole fragment is still one captured graph.  The batch's `obs` stays the TRUE observation;
    `obs_seen` [T][E][N][O] (also `batch["obs_seen"]`, zero-initialised: rows of seats that nobody drives are never written) is what
    the policy was given.  Cells of a `sweep` plan share their action noise, as in `FaultySeatSampler`."""
    BUFFERS = AdversaryBuffers
    adv_buffers = property(lambda self: self.level_buffers)
    adversary = property(lambda self: self.level_plan)
    set_adversary = LevelSeatSampler.set_levels

    def _policy_obs(self, t):
        self.seated.perturb_seats(self.adv_buffers, self.obs[t].view(-1, self.O), self.obs_seen[t].view(-1, self.O), self.col_lo, self.col_hi)
        return self.obs_seen[t]


def adversary_sweep_rows(algo, env, weights_list, levels, share=1.0, scenes_per_cell=4, num_agents=40, steps=1000, seed=0, labels=None,
                         **extra):
    """K populations `weights_list` (one layout) x the attack `levels` (level 0 must be an identity, so that every table carries its
    own baseline), `scenes_per_cell` scenes per cell, the same scenes and the same action noise for every cell, for `steps` env steps
    (rounded up to whole fragments).  The first round(share * num_agents) slots of a scene are attacked at the cell's level, the rest
    are unattacked drivers of the same checkpoint (`AdversaryPlan.sweep`).  Returns a pandas frame, one row per (checkpoint, level,
    role), with the columns of `fault_sweep_rows` and the level's three parameters in the place of the fault level's five."""
    return run_sweep("adversary_sweep_rows", AdversaryPlan, algo, env, weights_list,
                     lambda: baseline_levels("adversary_sweep_rows", AdversaryPlan, levels, "an identity (eps 0 or no direction)"),
                     lambda t, bank, seats, adversary, use_graph: AdversarialSeatSampler(t.env, t.policy, bank, seats, adversary, t.sampler.T,
                                                                                         use_graph=use_graph),
                     role_frame, labels=labels, scenes_per_cell=scenes_per_cell, num_agents=num_agents, steps=steps, seed=seed, extra=extra, share=share)


def load_levels(path):
    """A JSON list of objects with `AdversaryLevel`'s fields (missing fields are 0) -> [AdversaryLevel]."""
    return _levels.load_levels(path, AdversaryLevel)


def beam_saliency(bank, plan_buffers, obs, steer, throttle):
    """dJ/do of every seated row of obs [n_out][O], J = steer * mu_0 + throttle * mu_1 of the member that drives the row: which
    entries of its observation a checkpoint steers by.  One launch at eps = 0, so nothing is perturbed.  Rows in no list hold zeros."""
    import torch
    pb = plan_buffers
    plan = AdversaryPlan([AdversaryLevel(0.0, steer, throttle)], np.zeros((pb.G, pb.K), np.int32))
    grad, seen = torch.zeros_like(obs), torch.empty_like(obs)
    bank.sync_mirror()
    bank.perturb_seats(pb, AdversaryBuffers(plan, obs.device), obs, seen, 0, 0, grad=grad)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return grad
