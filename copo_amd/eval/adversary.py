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

Pieces: `AdversaryLevel` / `AdversaryPlan` (numpy only), `AdversaryBuffers`, `AdversarialSeatSampler` (the `SeatSampler` whose
`_policy_obs` launches the kernel inside the captured fragment), `adversary_sweep_rows` (checkpoints x levels x roles as a pandas frame;
`evaluate --adversary-sweep`) and `beam_saliency`.
"""
from dataclasses import dataclass

import numpy as np

from .bank import DeviceTables, draw_cell_noise
from .crossplay import SeatSampler
from .faults import lidar_columns, sweep_frame, sweep_members, sweep_plan

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
        for name in LEVEL_FIELDS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError("AdversaryLevel: %s = %r, a finite number wanted" % (name, v))
            object.__setattr__(self, name, float(v))
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


def _levels(levels):
    return [lv if isinstance(lv, AdversaryLevel) else AdversaryLevel(**lv) for lv in levels]


class AdversaryPlan:
    """`levels`: a sequence of `AdversaryLevel` (or dicts of its fields); `level_of`: int [G][K], the level of bank member k in scene
    group g (an index outside [0, L) leaves the member's rows alone).  Derived: `words` float32 [L][4].  Nothing here touches a device."""

    def __init__(self, levels, level_of):
        self.levels = _levels(levels)
        if not self.levels:
            raise ValueError("AdversaryPlan: no levels")
        self.level_of = np.ascontiguousarray(level_of, np.int32)
        if self.level_of.ndim != 2 or self.level_of.shape[0] < 1 or self.level_of.shape[1] < 1:
            raise ValueError("AdversaryPlan: level_of of shape %s, [groups][members] wanted" % (self.level_of.shape,))
        self.L, (self.G, self.K) = len(self.levels), self.level_of.shape
        self.words = np.stack([lv.words() for lv in self.levels])
        self.checkpoint = self.level = None
        self.share = self.scenes_per_cell = None          # (`sweep` sets them: cells of that many scenes share their action noise)

    def check(self, seat_plan):
        if (seat_plan.n_groups, seat_plan.K) != (self.G, self.K):
            raise ValueError("AdversaryPlan: level_of is %d groups x %d members, the seat plan has %d x %d" % (
                self.G, self.K, seat_plan.n_groups, seat_plan.K))
        return self

    @classmethod
    def sweep(cls, K, levels, scenes_per_cell, N, share=1.0):
        """(seat plan, adversary plan) of K checkpoints x L levels on the cell layout of `FaultPlan.sweep` (`SeatPlan.cells`): with share
        < 1 the bank is doubled, the first round(share * N) slots of a cell are attacked at the cell's level and the rest drive at level
        0, which must then be an identity."""
        return sweep_plan(cls, "AdversaryPlan.sweep", K, _levels(levels), scenes_per_cell, N, share)


class AdversaryBuffers(DeviceTables):
    """An adversary plan's tables on the device."""
    KEY = ("L", "G", "K")
    adversary = property(lambda self: self.source)

    @staticmethod
    def tables(plan):
        return dict(level_of=plan.level_of, levels=plan.words), (plan.L, plan.G, plan.K)


class AdversarialSeatSampler(SeatSampler):
    """`SeatSampler` under attack: per env step `perturb_seats` on the true observation, the seated forward on `obs_seen[t]`, the
    simulator step, the seat tally -- the whole fragment is still one captured graph.  The batch's `obs` stays the TRUE observation;
    `obs_seen` [T][E][N][O] (also `batch["obs_seen"]`, zero-initialised: rows of seats that nobody drives are never written) is what
    the policy was given.  Cells of a `sweep` plan share their action noise, as in `FaultySeatSampler`."""

    def __init__(self, vec_env, policy, bank, plan, adversary, T, use_graph=True):
        import torch
        adversary.check(plan)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.col_lo, self.col_hi = lidar_columns(self.sim.cfg)
        if not 0 <= self.col_lo <= self.col_hi <= self.O:
            raise ValueError("AdversarialSeatSampler: LiDAR columns [%d, %d) of an observation of %d" % (self.col_lo, self.col_hi, self.O))
        self.adv_buffers = AdversaryBuffers(adversary, self.device)
        self.adv_buffers.on_replace.append(self._loop.reset)
        self.obs_seen = torch.zeros(self.T, self.E, self.N, self.O, dtype=torch.float32, device=self.device)

    @property
    def adversary(self):
        return self.adv_buffers.adversary

    def set_adversary(self, adversary):
        """Another adversary plan, OUTSIDE captured graphs: the same shapes (levels, groups, members) are copied into the tables the
        captured fragment reads, other shapes allocate new ones and drop the graph."""
        self.adv_buffers.replace(adversary.check(self.seated.plan))

    def _draw_noise(self):
        draw_cell_noise(self.eps, self.adversary.scenes_per_cell)

    def sample(self):
        batch = super().sample()
        batch["obs_seen"] = self.obs_seen
        return batch

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
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    K = len(weights_list)
    if K < 1:
        raise ValueError("adversary_sweep_rows: no members")
    levels = _levels(levels)
    if not levels or not levels[0].is_identity:
        raise ValueError("adversary_sweep_rows: level 0 must be an identity (eps 0 or no direction), the table's own baseline")
    labels = check_labels(labels, K)
    seats, adversary = AdversaryPlan.sweep(K, levels, scenes_per_cell, num_agents, share)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        bank = PolicyBank(t.policy, sweep_members(weights_list, adversary))
        smp = AdversarialSeatSampler(t.env, t.policy, bank, seats, adversary, t.sampler.T, use_graph=graph_flag(t))
        tally = run_steps(smp, steps).tally.cpu().numpy()
    return sweep_frame(tally, seats, adversary, labels)


def load_levels(path):
    """A JSON list of objects with `AdversaryLevel`'s fields (missing fields are 0) -> [AdversaryLevel]."""
    import json
    with open(path) as f:
        raw = json.load(f)
    if not isinstance(raw, list) or not all(isinstance(r, dict) for r in raw):
        raise ValueError("%s: a JSON list of objects wanted" % path)
    return [AdversaryLevel(**r) for r in raw]


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
