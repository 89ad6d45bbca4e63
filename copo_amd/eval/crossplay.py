"""Cross-play: the slots ("seats") of ONE scene driven by different members of a policy bank, and the outcomes folded per member.

A `PolicyBank` gives every scene to one checkpoint.  Here a seat table [E][N] names, for every slot of every scene, the member that
drives whatever agent sits in it (-1: nobody; the slot's action is left alone): CoPO next to IPPO in one scene, an early checkpoint
next to a late one, one seed next to another.  Three pieces:

* `SeatPlan` (numpy only, pure): the seat table turned into what the forward kernel reads -- per member the ascending list of its rows
  e * N + n, the counts and the lists' capacity -- with the builders `pairs` (one scene group per ordered pair of members) and `uniform`
  (whole scenes per member: the dense bank).
* `SeatedBank` / `SeatSampler`: the bank in the policy's place of `VecSampler`, acting through `copo_mlp_forward_seats_f32` (the seat
  mode of the bank kernels: the member is the grid's second dimension and owns a row list; always the one-tile kernel, so a member's
  rows hold the bits `FusedLearner.act` writes for it below 2 * 32 * 256 rows), and after every simulator step `copo_seat_tally`,
  which adds the step's flags and rewards to eight int64 words per (scene group, member).  Forward, step and tally of a fragment are
  one captured graph where the sampler captures.  The loop is `VecSampler._rollout`: `_BankPolicy` makes its `_act` call
  `SeatedBank.act`, and `SeatSampler._step` is the base's step followed by the tally.
* `cross_play_rows`: every ordered pair (focal, partner) of K populations on the same scenes, as a pandas frame.

Rewards and termination are decided per agent in the simulator, so nothing there knows about seats.  One bank is one layout, as in
`bank.py`: members of other observation widths are refused by `PolicyBank`.  LCF is out of scope: the simulator draws an agent's LCF
from its SCENE's distribution (`VecSim.set_lcf_dist` / `set_lcf_table`), whichever member drives the slot; setting it is the caller's
business, as with banks.
"""
import numpy as np

from ..trainer import VecSampler
from .bank import DeviceTables, _BankPolicy, replica_seeds

SEAT_WORDS = ("acted", "done", "arrive", "crash", "out", "maxstep", "reward_q16", "spawned")
REWARD_SCALE = 65536.0


class SeatPlan:
    """`seat`: int [E][N], the member of every slot, -1 = nobody.  `n_members`: K (default: the largest member + 1); members beyond K
    - 1 are refused.  Derived: `rows` int64 [K][cap], row e * N + n in the list of member seat[e][n], ascending, unused tail 0;
    `counts` int32 [K]; `cap` = the largest count, at least 1.  `group`: int32 [E], the scene group of the tally (default: all 0) and
    `n_groups`.  `replica_scenes` = S declares that scenes [r S, (r + 1) S) of every replica r are the same scenes (`SeatSampler.reset`
    seeds them so); None: every scene its own.  Nothing here touches a device."""

    def __init__(self, seat, n_members=None, group=None, n_groups=None, replica_scenes=None):
        seat = np.ascontiguousarray(seat, np.int32)
        if seat.ndim != 2 or seat.shape[0] < 1 or seat.shape[1] < 1:
            raise ValueError("SeatPlan: seat table of shape %s, [E][N] wanted" % (seat.shape,))
        top = int(seat.max())
        K = max(top + 1, 1) if n_members is None else int(n_members)
        if K < 1 or K > 65535 or top >= K or int(seat.min()) < -1:
            raise ValueError("SeatPlan: members %d .. %d in a table for %d members (-1 = nobody)" % (int(seat.min()), top, K))
        self.seat, self.E, self.N, self.K = seat, seat.shape[0], seat.shape[1], K
        flat = seat.reshape(-1)
        self.counts = np.bincount(flat[flat >= 0], minlength=K).astype(np.int32)
        self.cap = max(int(self.counts.max()), 1)
        self.rows = np.zeros((K, self.cap), np.int64)
        for k in range(K):
            self.rows[k, :self.counts[k]] = np.nonzero(flat == k)[0]
        self.group = np.zeros(self.E, np.int32) if group is None else np.ascontiguousarray(group, np.int32)
        if self.group.shape != (self.E,):
            raise ValueError("SeatPlan: group of shape %s for %d scenes" % (self.group.shape, self.E))
        self.n_groups = max(int(self.group.max()) + 1, 1) if n_groups is None else int(n_groups)
        self.replica_scenes = None if replica_scenes is None else int(replica_scenes)
        if self.replica_scenes is not None and (self.replica_scenes < 1 or self.E % self.replica_scenes):
            raise ValueError("SeatPlan: replicas of %d scenes in %d scenes" % (self.replica_scenes, self.E))
        self.focal = self.partner = None
        self.share = None

    @classmethod
    def pairs(cls, K, scenes_per_pair, N, share=0.5):
        """One scene group per ORDERED pair (i, j) of K members, i = j included: group i * K + j holds scenes [g S, (g + 1) S), S =
        `scenes_per_pair`; in each the first round(share * N) seats belong to the focal member i, the rest to the partner j."""
        K, S, N = int(K), int(scenes_per_pair), int(N)
        if K < 1 or S < 1 or N < 1 or not 0.0 <= float(share) <= 1.0:
            raise ValueError("SeatPlan.pairs: K=%d scenes_per_pair=%d N=%d share=%r" % (K, S, N, share))
        nf = int(round(float(share) * N))
        seat = np.empty((K * K * S, N), np.int32)
        pair = np.repeat(np.arange(K * K, dtype=np.int32), S)
        seat[:, :nf] = (pair // K)[:, None]
        seat[:, nf:] = (pair % K)[:, None]
        plan = cls(seat, K, pair, K * K, replica_scenes=S)
        plan.focal, plan.partner = np.arange(K * K) // K, np.arange(K * K) % K
        plan.share, plan.n_focal = float(share), nf
        return plan

    @classmethod
    def cells(cls, K, L, scenes_per_cell, N, share=1.0, who="SeatPlan.cells"):
        """The seat layout of a sweep of K checkpoints x L levels (`FaultPlan.sweep`, `AdversaryPlan.sweep`): one scene group per cell,
        group k * L + l = scenes [g S, (g + 1) S), S = `scenes_per_cell`.  share == 1: every slot of the cell is member k, a bank of K
        members.  share < 1: the bank holds every checkpoint TWICE, members k and K + k; the first round(share * N) slots are member K +
        k (at the cell's level), the rest member k (at level 0).  Returns (plan, level_of int32 [K L][bank members], attrs): `attrs` is
        what a level plan keeps of the layout (`checkpoint`, `level` per group, `share`, `n_checkpoints`, `doubled`, `n_impaired`,
        `scenes_per_cell`).  The plan declares `replica_scenes` = S."""
        K, L, S, N, share = int(K), int(L), int(scenes_per_cell), int(N), float(share)
        if K < 1 or S < 1 or N < 1 or L < 1 or not 0.0 <= share <= 1.0:
            raise ValueError("%s: K=%d levels=%d scenes_per_cell=%d N=%d share=%r" % (who, K, L, S, N, share))
        doubled = share < 1.0
        n_imp = int(round(share * N))
        cell = np.repeat(np.arange(K * L, dtype=np.int32), S)
        k_of, l_of = np.arange(K * L) // L, np.arange(K * L) % L
        seat = np.empty((K * L * S, N), np.int32)
        seat[:, :n_imp] = ((cell // L) + (K if doubled else 0))[:, None]
        seat[:, n_imp:] = (cell // L)[:, None]
        KB = 2 * K if doubled else K
        level_of = np.zeros((K * L, KB), np.int32)
        level_of[np.arange(K * L), k_of + (K if doubled else 0)] = l_of
        attrs = dict(checkpoint=k_of, level=l_of, share=share, n_checkpoints=K, doubled=doubled, n_impaired=n_imp, scenes_per_cell=S)
        return cls(seat, KB, cell, K * L, replica_scenes=S), level_of, attrs

    @classmethod
    def uniform(cls, member_of_scene, N, n_members=None):
        """Every seat of scene e belongs to member_of_scene[e]: with e // (E / K) the ownership of the dense bank.  Group = member."""
        m = np.ascontiguousarray(member_of_scene, np.int32).reshape(-1)
        return cls(np.repeat(m[:, None], int(N), axis=1), n_members, m, n_members)


class PlanBuffers(DeviceTables):
    """A plan's tables on the device, uploaded once: what `PolicyBank.act_seats` and `seat_tally` read."""
    KEY = ("K", "cap", "E", "N", "G")
    plan = property(lambda self: self.source)
    n_out = property(lambda self: self.E * self.N)

    @staticmethod
    def tables(plan):
        return dict(rows=plan.rows, counts=plan.counts, seat=plan.seat, group=plan.group), (plan.K, plan.cap, plan.E, plan.N, plan.n_groups)


def seat_tally(flags, rew, buffers, out):
    """One step's `flags` uint8 [E][N] and `rew` float32 [E][N] (or None) added to `out` int64 [G][K][8] (`SEAT_WORDS`) by the plan's
    seat and group tables.  `out` accumulates; the caller clears it.  One launch on the current stream."""
    from .. import _capi
    _capi.check(_capi.lib.copo_seat_tally(flags.data_ptr(), _capi.ptr(rew), buffers.seat.data_ptr(), buffers.group.data_ptr(), buffers.E,
                                          buffers.N, buffers.K, buffers.G, out.data_ptr(), _capi.current_stream()))


class SeatedBank:
    """A `PolicyBank` with a seat plan: `.act` has `FusedLearner.act`'s signature over the [E * N] rows of the plan.  The plan's device
    buffers are uploaded once; `set_plan` replaces them OUTSIDE captured graphs by `DeviceTables.replace`: a plan of the same shapes (K,
    cap, E, N, groups) is copied into the tensors a captured graph reads, any other allocates new ones and calls `on_replace` (a sampler
    drops its graph)."""

    def __init__(self, bank, plan):
        if plan.K != bank.K:
            raise ValueError("SeatedBank: a plan for %d members and a bank of %d" % (plan.K, bank.K))
        self.bank, self.K = bank, bank.K
        self.buffers = PlanBuffers(plan, bank.theta.device)
        self.on_replace = self.buffers.on_replace

    @property
    def plan(self):
        return self.buffers.plan

    @property
    def can_forward(self):
        return True

    def invalidate_mirror(self):
        self.bank.invalidate_mirror()

    def sync_mirror(self):
        self.bank.sync_mirror()

    def set_plan(self, plan):
        if plan.K != self.K:
            raise ValueError("SeatedBank: a plan for %d members and a bank of %d" % (plan.K, self.K))
        self.buffers.replace(plan)

    def act(self, obs, eps, action, logp, dist_inputs, clipped=None):
        self.bank.act_seats(self.buffers, obs, eps, action, logp, dist_inputs, clipped)

    def perturb_seats(self, adv_buffers, obs, obs_seen, col_lo, col_hi, grad=None):
        """`PolicyBank.perturb_seats` over the plan's own buffers (eval/adversary.py)."""
        self.bank.perturb_seats(self.buffers, adv_buffers, obs, obs_seen, col_lo, col_hi, grad)

    def pgd_seats(self, pgd_buffers, obs, obs_seen, col_lo, col_hi, seed=0, tick=None, trace=None, max_iters=None):
        """`PolicyBank.pgd_seats` over the plan's own buffers (eval/pgd.py)."""
        self.bank.pgd_seats(self.buffers, pgd_buffers, obs, obs_seen, col_lo, col_hi, seed, tick, trace, max_iters)

    def certify_seats(self, cert_buffers, obs, bounds, col_lo, col_hi, pad=0.0, method="interval", parts=None):
        """`PolicyBank.certify_seats` over the plan's own buffers (eval/certify.py)."""
        self.bank.certify_seats(self.buffers, cert_buffers, obs, bounds, col_lo, col_hi, pad, method, parts)

    def attribute_seats(self, attrib_buffers, obs, attr, heads, max_points=None):
        """`PolicyBank.attribute_seats` over the plan's own buffers (eval/attribution.py)."""
        self.bank.attribute_seats(self.buffers, attrib_buffers, obs, attr, heads, max_points)

    def jury_seats(self, jury_buffers, obs, verdict):
        """`PolicyBank.jury_seats` on the rows of the plan (eval/jury.py): the judges' lists must cover the plan's [E * N] rows."""
        if jury_buffers.n_out != self.buffers.n_out:
            raise ValueError("SeatedBank.jury_seats: judges' lists over %d rows, the plan has %d" % (jury_buffers.n_out, self.buffers.n_out))
        self.bank.jury_seats(jury_buffers, obs, verdict)

    def hidden_seats(self, jury_buffers, obs, hidden):
        """`PolicyBank.hidden_seats` on the rows of the plan (eval/similarity.py): the judges' lists must cover the plan's [E * N] rows."""
        if jury_buffers.n_out != self.buffers.n_out:
            raise ValueError("SeatedBank.hidden_seats: judges' lists over %d rows, the plan has %d" % (jury_buffers.n_out, self.buffers.n_out))
        self.bank.hidden_seats(jury_buffers, obs, hidden)


class SeatSampler(VecSampler):
    """`VecSampler` with a `SeatedBank` in the policy's place, as `BankSampler` puts a bank there, and the seat tally behind every
    simulator step: `tally` int64 [groups][K][8] accumulates until `clear_tally()`.  Forward, step and tally of the fragment's T env
    steps are one captured graph where the sampler captures.  Ordinary noise (every seat its own draw).  A plan that declares
    `replica_scenes` = S (`pairs` does) has `reset` seed the scenes `replica_seeds(start_seed, S, E)`: every pair sees the same scenes."""

    def __init__(self, vec_env, policy, bank, plan, T, use_graph=True):
        import torch
        if (plan.E, plan.N) != (vec_env.sim.E, vec_env.sim.N):
            raise ValueError("SeatSampler: a plan of %d x %d seats for %d scenes of %d slots" % (plan.E, plan.N, vec_env.sim.E, vec_env.sim.N))
        self.seated = SeatedBank(bank, plan)
        super().__init__(vec_env, _BankPolicy(policy, self.seated), T, use_graph=use_graph, stagger_episodes=False)
        self.seated.on_replace.append(self._loop.reset)
        self.tally = torch.zeros(plan.n_groups, bank.K, len(SEAT_WORDS), dtype=torch.int64, device=self.device)

    def set_plan(self, plan):
        if plan.n_groups != self.seated.buffers.G:
            raise ValueError("SeatSampler.set_plan: %d scene groups, the tally holds %d" % (plan.n_groups, self.seated.buffers.G))
        self.seated.set_plan(plan)

    def clear_tally(self):
        self.tally.zero_()

    def reset(self, seeds=None):
        S = self.seated.plan.replica_scenes
        if seeds is None and S:
            seeds = replica_seeds(self.sim.cfg.start_seed, S, self.E)
        super().reset(seeds)

    def _step(self, t):
        super()._step(t)
        seat_tally(self.flags[t], self.rew3[0, t], self.seated.buffers, self.tally)


def tally_rates(words):
    """The derived columns of one tally cell (the eight `SEAT_WORDS`): `success` = arrive / done, `crash_rate`, `out_rate`,
    `reward_per_step` = reward_q16 / 65536 / acted; NaN where a denominator is 0."""
    w = dict(zip(SEAT_WORDS, (int(v) for v in words)))
    ratio = lambda a, b: float(a) / float(b) if b else float("nan")  # noqa: E731
    return dict(success=ratio(w["arrive"], w["done"]), crash_rate=ratio(w["crash"], w["done"]), out_rate=ratio(w["out"], w["done"]),
                reward_per_step=ratio(w["reward_q16"] / REWARD_SCALE, w["acted"]))


def tally_frame(tally, plan, labels=None):
    """The tally [G][K][8] (numpy int64) of a `pairs` plan as a frame: one row per (pair group, member seated in it), the columns of
    `cross_play_rows`."""
    import pandas as pd
    labels = list(range(plan.K)) if labels is None else list(labels)
    rows = []
    for g in range(plan.n_groups):
        i, j = int(plan.focal[g]), int(plan.partner[g])
        for k in ([i] if i == j else [i, j]):
            w = [int(v) for v in tally[g, k]]
            rows.append(dict(focal=i, partner=j, member=k, label=labels[k], share=plan.share, **dict(zip(SEAT_WORDS, w)), **tally_rates(w)))
    return pd.DataFrame(rows)


def run_pairs(who, algo, env, weights_list, sampler, frame, *, share, scenes_per_pair, num_agents, steps, seed, labels, extra, check=None):
    """The session of the studies on `SeatPlan.pairs` (`cross_play_rows`, `jury_rows`, `influence_rows`), as `levels.run_sweep` is the level
    studies': the K populations `weights_list` (one layout), one bank, `sampler(t, bank, seats, use_graph)` run for `steps` env steps
    (rounded up to whole fragments), then `frame(sampler, seats, labels)` while the session is still open.  `check`: the study's own
    argument checks; it is called behind the member count and in front of the labels, the order the three functions always refused in."""
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    K = len(weights_list)
    if K < 1:
        raise ValueError("%s: no members" % who)
    if check is not None:
        check()
    labels = check_labels(labels, K)
    seats = SeatPlan.pairs(K, scenes_per_pair, num_agents, share)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        smp = sampler(t, PolicyBank(t.policy, weights_list), seats, graph_flag(t))
        return frame(run_steps(smp, steps), seats, labels)


def cross_play_rows(algo, env, weights_list, share=0.5, scenes_per_pair=4, num_agents=40, steps=1000, seed=0, labels=None, **extra):
    """Every ordered pair (focal i, partner j) of the K populations `weights_list` (one layout: one algorithm's observation) on
    `scenes_per_pair` scenes each, the same scenes for every pair: the first round(share * num_agents) slots of a scene are driven by
    i, the rest by j, for `steps` env steps (rounded up to whole fragments of the sampler).  Returns a pandas frame, one row per (pair
    group, member seated in it): `focal`, `partner`, `member`, `label`, `share`, the eight raw words of the tally (`SEAT_WORDS`),
    `success` = arrive / done, `crash_rate`, `out_rate`, `reward_per_step` = reward_q16 / 65536 / acted; NaN where a denominator is 0."""
    return run_pairs("cross_play_rows", algo, env, weights_list,
                     lambda t, bank, seats, use_graph: SeatSampler(t.env, t.policy, bank, seats, t.sampler.T, use_graph=use_graph),
                     lambda smp, seats, labels: tally_frame(smp.tally.cpu().numpy(), seats, labels),
                     share=share, scenes_per_pair=scenes_per_pair, num_agents=num_agents, steps=steps, seed=seed, labels=labels, extra=extra)
