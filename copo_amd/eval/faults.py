"""Fault injection: noisy sensors and actuators in batched evaluation.

Every policy of the evaluation pipeline sees a perfect LiDAR and every action reaches the wheels as chosen.  Here a fault LEVEL is
chosen per (scene group, bank member), the keys of the seat tally (`crossplay.py`), and applied between the simulator and the policy:

* `copo_fault_obs` writes what the policy sees, `obs_seen`, from the true observation: per LiDAR beam a dropout draw (the beam reads
  `dropout_value`) or Gaussian-like noise of `lidar_sigma`, clamped to [0, 1]; every other column is copied.
* `copo_fault_act` works on the clipped action the step will read: with probability `sticky` the action of the previous step is
  repeated (only while the slot holds the agent it held a step ago), then noise of `act_sigma` per component, clamped to [-1, 1].

The simulator, its oracle and the learner know nothing of this: a fault is not part of the scene.  The draws are the simulator's
counter-based hash on (fault seed, row, the row's step count since `reset`, beam or component, stream), so a run does not depend on how
its steps are cut into fragments or on whether they are replayed from a graph.  The normal stand-in `z` is the centred, scaled sum of
four 16-bit uniform halves of two hashes: mean 0, variance 1, and its tails END at +-3.46 (|z| <= 131070 sqrt(3) / 65536): a level of
`lidar_sigma` s never moves a beam by more than 3.47 s.

Pieces, each on its base in `levels.py` (plan, buffers, sampler and sweep session shared with `adversary.py`, `pgd.py` and `certify.py`):
`FaultLevel` / `FaultPlan` (numpy only), `FaultBuffers`, `FaultySeatSampler` (the two launches inside its captured fragment: it keeps no
loop, `_policy_obs` launches `copo_fault_obs` in front of the forward of `VecSampler._act` and `_step` launches `copo_fault_act` in front
of the step and its tally) and `fault_sweep_rows` (checkpoints x levels x roles as a pandas frame; `evaluate --fault-sweep`).
"""
from dataclasses import dataclass

import numpy as np

from . import levels as _levels
from .levels import LevelBuffers, LevelPlan, LevelSeatSampler, baseline_levels, finite_fields, role_frame, run_sweep
from .levels import lidar_columns, sweep_frame, sweep_members, sweep_plan  # noqa: F401  (they lived here first: importable from here as before)

LEVEL_WORDS = 8
LEVEL_FIELDS = ("lidar_sigma", "lidar_dropout", "dropout_value", "act_sigma", "sticky")
PROB_ONE = 1 << 24              # a Bernoulli draw is (hash >> 8) < rint(p * 2^24)


@dataclass(frozen=True)
class FaultLevel:
    """One level of impairment.  `lidar_sigma`: standard deviation of the noise on every LiDAR beam (beams are in [0, 1], 1 = nothing
    in range); `lidar_dropout`: probability per beam and step that the beam reads `dropout_value` instead; `act_sigma`: standard
    deviation of the noise on each component of the clipped action; `sticky`: probability per step that the previous action is repeated.
    `FaultLevel()` is the identity: rows at it pass through bit for bit."""
    lidar_sigma: float = 0.0
    lidar_dropout: float = 0.0
    dropout_value: float = 0.0
    act_sigma: float = 0.0
    sticky: float = 0.0

    def __post_init__(self):
        finite_fields(self, LEVEL_FIELDS)
        for name in ("lidar_sigma", "act_sigma"):
            if getattr(self, name) < 0.0:
                raise ValueError("FaultLevel: %s = %r is negative" % (name, getattr(self, name)))
        for name in ("lidar_dropout", "sticky"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError("FaultLevel: %s = %r is no probability" % (name, getattr(self, name)))

    @property
    def is_identity(self):
        return self.lidar_sigma == 0.0 and self.lidar_dropout == 0.0 and self.act_sigma == 0.0 and self.sticky == 0.0

    def words(self):
        """The level as the eight 32-bit words the kernels read."""
        w = np.zeros(LEVEL_WORDS, np.uint32)
        w[[0, 2, 3]] = np.array([self.lidar_sigma, self.dropout_value, self.act_sigma], np.float32).view(np.uint32)
        w[1], w[4] = int(np.rint(self.lidar_dropout * PROB_ONE)), int(np.rint(self.sticky * PROB_ONE))
        return w

    def as_dict(self):
        return {name: getattr(self, name) for name in LEVEL_FIELDS}


class FaultPlan(LevelPlan):
    """`LevelPlan` of `FaultLevel`s; `words` uint32 [L][8]."""
    LEVEL = FaultLevel


class FaultBuffers(LevelBuffers):
    """A fault plan's tables on the device."""
    faults = property(lambda self: self.source)

    @staticmethod
    def tables(faults):          # (the level words as bits; torch has no uint32 arithmetic to need)
        return dict(level_of=faults.level_of, words=faults.words.view(np.int32)), (faults.L, faults.G, faults.K)


def _fault_launch(name, head, pb, fb, tick, fault_seed):
    """Entry point `name` on its own arguments `head` and on what both launches end in: the seat and group tables, the levels, the tick,
    the seed and the current stream."""
    from .. import _capi
    _capi.check(getattr(_capi.lib, name)(*head, pb.seat.data_ptr(), pb.group.data_ptr(), pb.K, pb.G, fb.level_of.data_ptr(), fb.words.data_ptr(),
                                         fb.L, tick.data_ptr(), fault_seed, _capi.current_stream()))


def fault_obs(obs, obs_seen, col_lo, col_hi, plan_buffers, fault_buffers, tick, fault_seed):
    """`copo_fault_obs` on the current stream: obs [E N][O] -> obs_seen."""
    pb = plan_buffers
    _fault_launch("copo_fault_obs", (obs.data_ptr(), obs_seen.data_ptr(), pb.E, pb.N, int(obs.shape[-1]), col_lo, col_hi), pb, fault_buffers,
                  tick, fault_seed)


def fault_act(act, prev, flags_prev, plan_buffers, fault_buffers, tick, fault_seed):
    """`copo_fault_act` on the current stream: act [E N][2] in place; `flags_prev` = the previous step's flags or None."""
    pb = plan_buffers
    _fault_launch("copo_fault_act", (act.data_ptr(), prev.data_ptr(), None if flags_prev is None else flags_prev.data_ptr(), pb.E, pb.N), pb,
                  fault_buffers, tick, fault_seed)


class FaultySeatSampler(LevelSeatSampler):
    """`SeatSampler` with faults: per env step fault_obs, the seated forward on `obs_seen[t]`, fault_act on `clipped[t]`, the simulator
    step, the seat tally -- the whole fragment is still one captured graph.  The batch's `obs` stays the TRUE observation, so recorders
    and observers are unaffected; `obs_seen` [T][E][N][O] (also `batch["obs_seen"]`) is what the policy was given.  `actions` and `logp`
    are the policy's own, `clipped` is what reached the simulator.

    State: `prev` [E][N][2] (the action that reached the simulator a step ago), `tick` int32 [E N] (steps since `reset`, the draws'
    counter).  The previous step's flags are `flags[t - 1]`; for t = 0 they are `flags[T - 1]`, which still holds the last step of the
    previous fragment.  `reset` zeroes `tick`, `prev` and `flags[T - 1]`: flags of zero say that nobody acted, so nothing sticks in the
    first step, as if no flags were given.  (The fault draws themselves are keyed by the absolute row, so two impaired cells of a `sweep`
    plan never share those, as they share their action noise.)"""

    BUFFERS = FaultBuffers
    fault_buffers = property(lambda self: self.level_buffers)
    faults = property(lambda self: self.level_plan)
    set_faults = LevelSeatSampler.set_levels

    def __init__(self, vec_env, policy, bank, plan, faults, T, use_graph=True, fault_seed=0):
        import torch
        super().__init__(vec_env, policy, bank, plan, faults, T, use_graph=use_graph)
        self.fault_seed = int(fault_seed) & (2 ** 64 - 1)
        self.prev = torch.zeros(self.E, self.N, 2, dtype=torch.float32, device=self.device)
        self.tick = torch.zeros(self.E * self.N, dtype=torch.int32, device=self.device)

    def reset(self, seeds=None):
        super().reset(seeds)
        self.tick.zero_()
        self.prev.zero_()
        self.flags[self.T - 1].zero_()

    def _policy_obs(self, t):
        fault_obs(self.obs[t], self.obs_seen[t], self.col_lo, self.col_hi, self.seated.buffers, self.fault_buffers, self.tick, self.fault_seed)
        return self.obs_seen[t]

    def _step(self, t):
        fault_act(self.clipped[t], self.prev, self.flags[t - 1 if t else self.T - 1], self.seated.buffers, self.fault_buffers, self.tick,
                  self.fault_seed)
        super()._step(t)


def fault_sweep_rows(algo, env, weights_list, levels, share=1.0, scenes_per_cell=4, num_agents=40, steps=1000, seed=0, labels=None,
                     fault_seed=None, **extra):
    """K populations `weights_list` (one layout) x the fault `levels` (level 0 must be the identity, so that every table carries its
    own baseline), `scenes_per_cell` scenes per cell, the same scenes and the same action noise for every cell, for `steps` env steps
    (rounded up to whole fragments).  The first round(share * num_agents) slots of a scene are impaired at the cell's level, the rest are healthy drivers of
    the same checkpoint (`FaultPlan.sweep`).  Returns a pandas frame, one row per (checkpoint, level, role): `checkpoint`, `label`,
    `level`, `role` ("impaired" / "healthy"; a role without seats has no row), `member`, `share`, `seats`, `own_level` (the level the
    row's drivers are at: 0 for the healthy), the five parameters of the CELL's level, the eight raw words of the seat tally and
    `success`, `crash_rate`, `out_rate`, `reward_per_step` as in `cross_play_rows`.  `fault_seed` defaults to `seed`."""
    return run_sweep("fault_sweep_rows", FaultPlan, algo, env, weights_list,
                     lambda: baseline_levels("fault_sweep_rows", FaultPlan, levels, "the identity FaultLevel()"),
                     lambda t, bank, seats, faults, use_graph: FaultySeatSampler(
                         t.env, t.policy, bank, seats, faults, t.sampler.T, use_graph=use_graph, fault_seed=seed if fault_seed is None else fault_seed),
                     role_frame, labels=labels, scenes_per_cell=scenes_per_cell, num_agents=num_agents, steps=steps, seed=seed, extra=extra, share=share)


def load_levels(path):
    """A JSON list of objects with `FaultLevel`'s fields (missing fields are 0) -> [FaultLevel]."""
    return _levels.load_levels(path, FaultLevel)
