"""Certified LiDAR bounds: interval bound propagation (IBP) through the policy net and, tighter, one linear relaxation per tanh unit
carried backward from each action mean (`method="linear"`): the guarantee that the attacks cannot give.

`faults.py`, `adversary.py` and `pgd.py` each SHOW a perturbation of the LiDAR block that moves the action: lower bounds on the worst
case inside an L-infinity budget `eps`.  A table that reads "PGD moved the mean throttle by 0.08 at eps = 0.02" does not say whether
the checkpoint is robust or the attack is weak.  Here the other side: a box [lo_a, hi_a] that holds the action mean mu_a(x) for EVERY x
with |x[j] - o[j]| <= eps on the LiDAR columns (and 0 <= x[j] <= 1), x = o elsewhere.  The policy net is two tanh layers (monotone) and a
linear head, so intervals propagate exactly: a centre c and a radius r per unit, W c + b and |W| r per layer, tanh of both ends.

The certificate is on the action MEANS, `dist_inputs[:, :2]`, before sampling and clipping: what the policy decides, not what the noise
and the actuator limits make of it.  fp32 sums are not rounded outward, so the bounds are sound up to fp32 rounding; `pad` >= 0 widens
every bound by that much (DESIGN.md section 8o records the measured deviation from a float64 model, so that a user can set it).

A LEVEL (`eps`, `delta_steer`, `delta_throttle`) is chosen per (scene group, bank member), the keys of the seat tally.  A row is
CERTIFIED at its level when dev_a = max(hi_a - mu_a(o), mu_a(o) - lo_a) <= delta_a on both axes: no perturbation inside the budget moves
the mean action by more than the deltas.  `copo_cert_obs_seats_f32` (csrc/learn_certify.inc) writes, per seated row, `bounds` = lo_0,
hi_0, lo_1, hi_1, mu_0(o), mu_1(o), valid, eps in one launch that costs about a seat forward (clean row, centre and radius are three
16-row tiles against one weight stream); `copo_certify_tally` folds a step's bounds into eight int64 words per (group, member),
`CERT_WORDS`.  Certification changes nobody's driving: the policy acts on the true observation.

The bracket: join `certify_sweep_rows` with `pgd.pgd_sweep_rows` on (checkpoint, eps) --

    cert = certify_sweep_rows(algo, env, ws, [dict(eps=e, delta_steer=d, delta_throttle=d) for e in budgets])
    pgd = pgd_sweep_rows(algo, env, ws, [{}] + [dict(eps=e, alpha=e / 4, iters=8, random_start=True, untargeted=True) for e in budgets])
    both = cert.merge(pgd[pgd.role == "impaired"], on=["checkpoint", "eps"], suffixes=("", "_pgd"))

-- then the attack's outcome (from below) and `max_dev` / `certified_rate` (from above) stand in one row: the true worst case lies
between them.

METHODS.  `method="interval"` (the default, every path and every bit as before) is the pass above.  Its box widens by about 0.8 sqrt(H)
per hidden layer and turns trivial (2 |W3[a]|_1) near eps = 0.01, below the budgets at which the attacks move anything.
`method="linear"` (`copo_lin_obs_seats_f32`, csrc/learn_linbound.inc) bounds every tanh unit on its interval [l, u]
by two parallel lines of slope lam = min(tanh'(l), tanh'(u)) -- lam z + betaL <= tanh z <= lam z + betaU -- and carries W3[a] backward
through those lines and the weights to the input box: mu_a(x) lies in [base - rad, base + rad] plus the beta terms.  One slope for
both sides makes the upper and the lower bound share their backward coefficients, so a head costs one backward pass.  The result is
intersected with the interval box of the same launch (never looser than it), lands in the same `bounds` layout, and is folded by the
same `copo_certify_tally`.  On the test nets the box is 8 to 40 times narrower at eps = 0.0005 .. 0.002 and still informative at
eps = 0.01 for hidden 256; at eps = 0.05 both boxes are trivial.  The launch costs about 2.4 interval launches (DESIGN.md section 8p
has the measurement and what it is made of).

An L-infinity budget, the LiDAR block, fp32 operands.  Backward bounds for layer 2's pre-activations (full CROWN), per-unit optimised
slopes, chord / tangent relaxations, zonotopes, branch and bound, the ego / navigation columns, other norms, the bfloat16 operand mode
and bounds on the sampled or clipped action are out of scope.

Pieces, each on its base in `levels.py`: `CertifyLevel` / `CertifyPlan` (numpy only), `CertifyBuffers`, `CertifySeatSampler` (whose
`_policy_obs` launches the kernel inside the captured fragment), `certify_sweep_rows` (checkpoints x levels as a pandas frame; `evaluate
--certify-sweep`) and `load_levels`; its own: `certify_tally`, `certify_frame` and `certified_bounds`.
"""
from dataclasses import dataclass

import numpy as np

from . import levels as _levels
from .bank import check_certify_method
from .crossplay import SEAT_WORDS, tally_rates
from .levels import LevelBuffers, LevelPlan, LevelSeatSampler, finite_fields, run_sweep

LEVEL_WORDS = 4
LEVEL_FIELDS = ("eps", "delta_steer", "delta_throttle")
PART_WORDS = ("lo_lin_steer", "hi_lin_steer", "lo_lin_throttle", "hi_lin_throttle", "lo_int_steer", "hi_int_steer", "lo_int_throttle", "hi_int_throttle")
BOUND_WORDS = ("lo_steer", "hi_steer", "lo_throttle", "hi_throttle", "mu_steer", "mu_throttle", "valid", "eps")
CERT_WORDS = ("rows", "certified", "certified_steer", "certified_throttle", "width_steer_q16", "width_throttle_q16", "max_dev_q16", "nonfinite")
Q16 = 65536.0


@dataclass(frozen=True)
class CertifyLevel:
    """One level of certification.  `eps`: the L-infinity budget on every LiDAR beam (beams are in [0, 1]; 0 is a legitimate level: width
    0); (`delta_steer`, `delta_throttle`): how far the mean action may move for a row to count as certified."""
    eps: float = 0.0
    delta_steer: float = 0.0
    delta_throttle: float = 0.0

    def __post_init__(self):
        finite_fields(self, LEVEL_FIELDS)
        for name in LEVEL_FIELDS:
            if getattr(self, name) < 0:
                raise ValueError("CertifyLevel: %s = %r is negative" % (name, getattr(self, name)))

    def words(self):
        """The level as the four floats the kernels read: eps, delta_steer, delta_throttle, 0."""
        return np.array([self.eps, self.delta_steer, self.delta_throttle, 0.0], np.float32)

    def as_dict(self):
        return {name: getattr(self, name) for name in LEVEL_FIELDS}


class CertifyPlan(LevelPlan):
    """`LevelPlan` of `CertifyLevel`s; `words` float32 [L][4].  A `level_of` index outside [0, L): the member's rows there are not
    certified, `valid` = 0."""
    LEVEL = CertifyLevel

    @classmethod
    def sweep(cls, K, levels, scenes_per_cell, N):
        """(seat plan, certify plan) of K checkpoints x L levels on the cell layout of `LevelPlan.sweep` at share 1: every slot of cell
        (k, l) is member k, certified at level l.  There are no roles: nobody is impaired."""
        return super().sweep(K, levels, scenes_per_cell, N, 1.0)


class CertifyBuffers(LevelBuffers):
    """A certify plan's tables on the device."""
    certify = property(lambda self: self.source)


def certify_tally(flags, bounds, plan_buffers, cert_buffers, out):
    """One step's `flags` uint8 [E][N] and `bounds` float32 [E][N][8] added to `out` int64 [G][K][8] (`CERT_WORDS`) by the seat plan's
    seat and group tables and the certify plan's levels.  `out` accumulates (its max word keeps the largest); the caller clears it.  One
    launch on the current stream."""
    from .. import _capi
    pb, cb = plan_buffers, cert_buffers
    if (cb.G, cb.K) != (pb.G, pb.K):
        raise ValueError("certify_tally: a plan of %d groups x %d members, levels for %d x %d" % (pb.G, pb.K, cb.G, cb.K))
    _capi.check(_capi.lib.copo_certify_tally(flags.data_ptr(), bounds.data_ptr(), pb.seat.data_ptr(), pb.group.data_ptr(), cb.level_of.data_ptr(),
                                             cb.levels.data_ptr(), pb.E, pb.N, pb.K, pb.G, cb.L, out.data_ptr(), _capi.current_stream()))


class CertifySeatSampler(LevelSeatSampler):
    """`SeatSampler` with certificates: per env step `certify_seats` on the true observation into `bounds[t]`, the seated forward on the
    SAME true observation, the simulator step, the seat tally and the certify tally -- the whole fragment is still one captured graph.
    Actions, flags and the seat tally are a plain `SeatSampler`'s.  `bounds` [T][E][N][8] (also `batch["bounds"]`, zero-initialised: rows
    of seats that nobody drives are never written and read as invalid); `cert_tally` int64 [G][K][8] (`CERT_WORDS`) accumulates until
    `clear_tally()`.  Cells of a `sweep` plan share their action noise, as in `AdversarialSeatSampler`.  `method`: "interval" or "linear"
    (the module docstring); the launch is the only difference, the fold and everything else are the same."""

    BUFFERS = CertifyBuffers
    SEEN = False          # (nothing is perturbed: the policy reads the true observation)
    cert_buffers = property(lambda self: self.level_buffers)
    certify = property(lambda self: self.level_plan)
    set_certify = LevelSeatSampler.set_levels

    def __init__(self, vec_env, policy, bank, plan, certify, T, use_graph=True, pad=0.0, method="interval"):
        import torch
        self.method = check_certify_method("CertifySeatSampler", method)
        super().__init__(vec_env, policy, bank, plan, certify, T, use_graph=use_graph)
        self.pad = float(pad)
        if not (self.pad >= 0.0 and np.isfinite(self.pad)):
            raise ValueError("CertifySeatSampler: pad = %r, a finite number >= 0 wanted" % (pad,))
        self.bounds = torch.zeros(self.T, self.E, self.N, len(BOUND_WORDS), dtype=torch.float32, device=self.device)
        self.cert_tally = torch.zeros(plan.n_groups, bank.K, len(CERT_WORDS), dtype=torch.int64, device=self.device)

    def clear_tally(self):
        super().clear_tally()
        self.cert_tally.zero_()

    def sample(self):
        batch = super().sample()
        batch["bounds"] = self.bounds
        return batch

    def _policy_obs(self, t):
        self.seated.certify_seats(self.cert_buffers, self.obs[t].view(-1, self.O), self.bounds[t].view(-1, len(BOUND_WORDS)), self.col_lo,
                                  self.col_hi, self.pad, self.method)
        return self.obs[t]

    def _step(self, t):
        super()._step(t)
        certify_tally(self.flags[t], self.bounds[t], self.seated.buffers, self.cert_buffers, self.cert_tally)


def cert_rates(words):
    """The derived columns of one certify-tally cell (the eight `CERT_WORDS`): `certified_rate` (both axes), `certified_rate_steer`,
    `certified_rate_throttle` over the rows with finite bounds, `mean_width_steer` / `mean_width_throttle` over the same rows and
    `max_dev`; NaN where there is no such row."""
    w = dict(zip(CERT_WORDS, (int(v) for v in words)))
    good = w["rows"] - w["nonfinite"]
    ratio = lambda a: float(a) / float(good) if good > 0 else float("nan")  # noqa: E731
    return dict(certified_rate=ratio(w["certified"]), certified_rate_steer=ratio(w["certified_steer"]),
                certified_rate_throttle=ratio(w["certified_throttle"]), mean_width_steer=ratio(w["width_steer_q16"] / Q16),
                mean_width_throttle=ratio(w["width_throttle_q16"] / Q16), max_dev=w["max_dev_q16"] / Q16 if good > 0 else float("nan"))


def certify_frame(cert_tally, tally, seats, certify, labels=None, method=None):
    """Both tallies [G][K][8] (numpy int64) of a `sweep` plan as a frame: one row per (checkpoint, level), the columns of
    `certify_sweep_rows`; `method` (not None): a `method` column behind `level`."""
    import pandas as pd
    labels = list(range(certify.n_checkpoints)) if labels is None else list(labels)
    rows = []
    for g in range(seats.n_groups):
        k, lv = int(certify.checkpoint[g]), int(certify.level[g])
        cw, sw = [int(v) for v in cert_tally[g, k]], [int(v) for v in tally[g, k]]
        rows.append(dict(checkpoint=k, label=labels[k], level=lv, **({} if method is None else dict(method=method)), member=k, seats=seats.N, **certify.levels[lv].as_dict(), **dict(zip(CERT_WORDS, cw)),
                         **cert_rates(cw), **dict(zip(SEAT_WORDS, sw)), **tally_rates(sw)))
    return pd.DataFrame(rows)


def certify_sweep_rows(algo, env, weights_list, levels, scenes_per_cell=4, num_agents=40, steps=1000, seed=0, labels=None, pad=0.0,
                       method="interval", **extra):
    """K populations `weights_list` (one layout) x the certification `levels`, `scenes_per_cell` scenes per cell, the same scenes and the
    same action noise for every cell, for `steps` env steps (rounded up to whole fragments).  Every slot of a cell is driven by the
    cell's checkpoint on the true observation and certified at the cell's level (`CertifyPlan.sweep`).  Returns a pandas frame, one
    row per (checkpoint, level): `checkpoint`, `label`, `level`, `member`, `seats`, the level's `eps`, `delta_steer`, `delta_throttle`,
    the eight raw words of the certify tally (`CERT_WORDS`), `certified_rate`, `certified_rate_steer`, `certified_rate_throttle`,
    `mean_width_steer`, `mean_width_throttle`, `max_dev`, then the eight raw words of the seat tally and its rates as in
    `cross_play_rows`.  Joined with `pgd_sweep_rows` on (checkpoint, eps) it brackets the worst case (see the module docstring).
    `method="linear"`: the tighter bounds, and a `method` column behind `level` (an interval frame keeps today's columns)."""
    check_certify_method("certify_sweep_rows", method)
    def some_levels():          # (no level-0 rule: nobody is impaired, so there is no baseline to carry)
        checked = CertifyPlan.as_levels(levels)
        if not checked:
            raise ValueError("certify_sweep_rows: no levels")
        return checked

    def frame(smp, seats, certify, labels):
        return certify_frame(smp.cert_tally.cpu().numpy(), smp.tally.cpu().numpy(), seats, certify, labels, None if method == "interval" else method)

    return run_sweep("certify_sweep_rows", CertifyPlan, algo, env, weights_list, some_levels,
                     lambda t, bank, seats, certify, use_graph: CertifySeatSampler(t.env, t.policy, bank, seats, certify, t.sampler.T,
                                                                                   use_graph=use_graph, pad=pad, method=method),
                     frame, labels=labels, scenes_per_cell=scenes_per_cell, num_agents=num_agents, steps=steps, seed=seed, extra=extra)


def load_levels(path):
    """A JSON list of objects with `CertifyLevel`'s fields (missing fields are 0) -> [CertifyLevel]."""
    return _levels.load_levels(path, CertifyLevel)


def certified_bounds(bank, plan_buffers, obs, eps, pad=0.0, *, columns, method="interval", parts=False):
    """`bounds` [n_out][8] (`BOUND_WORDS`) of every seated row of obs [n_out][O] at one budget `eps` for every (group, member): one
    launch, like `adversary.beam_saliency`.  `columns` = (col_lo, col_hi), the LiDAR block (`levels.lidar_columns(sim.cfg)`): unlike the
    saliency, the box needs to know where the beams are.  Rows in no list hold zeros (`valid` = 0).  `method="linear"`: the tighter
    bounds; with `parts=True` (linear only) returns (bounds, parts), parts [n_out][8] (`PART_WORDS`): the linear and the interval box
    before the intersection and the pad."""
    import torch
    check_certify_method("certified_bounds", method)
    if parts and method != "linear":
        raise ValueError("certified_bounds: parts=True needs method=\"linear\"")
    pb = plan_buffers
    plan = CertifyPlan([CertifyLevel(eps)], np.zeros((pb.G, pb.K), np.int32))
    col_lo, col_hi = (int(v) for v in columns)
    bounds = torch.zeros(int(obs.shape[0]), len(BOUND_WORDS), dtype=torch.float32, device=obs.device)
    second = torch.zeros_like(bounds) if parts else None
    bank.sync_mirror()
    if method == "interval":
        bank.certify_seats(pb, CertifyBuffers(plan, obs.device), obs, bounds, col_lo, col_hi, pad)
    else:
        bank.certify_seats(pb, CertifyBuffers(plan, obs.device), obs, bounds, col_lo, col_hi, pad, method, second)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return (bounds, second) if parts else bounds
