"""A policy jury: every checkpoint's verdict on the states another one drives.

`crossplay.py` seats K bank members in one scene and folds what happens to each; the LiDAR studies impair, attack and bound the member
that drives a row.  All of those answer for the DRIVER.  Here the question a comparison of two populations starts with: on the states
this member actually visits, what would the others have done, and how far apart are they?  How far a partner is from the focal policy's
convention in cross-play, how much a policy drifts between an early and a late checkpoint, how close CoPO is to IPPO on the
Intersection, which checkpoints of a sweep are behaviourally the same.

A seat plan says who DRIVES a row; a `JuryPlan` adds who JUDGES it: a table `judges` [G][K], nonzero where member j judges the seated
rows of scene group g.  `copo_jury_obs_seats_f32` (csrc/learn_jury.inc, the third mode of the bank's forward) runs every judge's policy
net on the true observation of the rows in its list and writes the four distribution inputs -- mu_steer, mu_throttle, logstd_steer,
logstd_throttle -- to `verdict[row][judge]`, the bits the seat forward writes for that member on that row.  `copo_jury_tally` folds a
step's verdicts against the driver's own `dist_inputs` into eight int64 words per (group, driver, judge), `JURY_WORDS`: integer sums,
so nothing depends on the order.  Judging changes nobody's driving: the drive and the seat tally are a plain `SeatSampler`'s, bit for bit.

The divergences are between the Gaussians BEFORE sampling and clipping, (mean, log-std) per action axis; KL in float64 on the device:
    KL(p || q) = sum_a (s_q - s_p) + (0.5 (exp(2 (s_p - s_q)) + (m_p - m_q)^2 exp(-2 s_q)) - 0.5)
A judge that is the driver has distance zero in every word: the diagonal is the bit-equality of the two forwards.

Pieces: `JuryPlan` (numpy only), `JuryBuffers`, `PolicyBank.jury_seats` / `SeatedBank.jury_seats`, `jury_tally`, `JurySeatSampler`
(forward, step, seat tally, jury launch and jury fold of a fragment stay one captured graph), `jury_rates` / `jury_frame` /
`jury_matrix`, `jury_rows` (`evaluate --jury`) and `jury_verdicts` (one launch on a plain observation array).
"""
import numpy as np

from .bank import DeviceTables
from .crossplay import SeatPlan, SeatSampler, run_pairs

JURY_WORDS = ("pairs", "disagree", "d_steer_q16", "d_throttle_q16", "d_logstd_q16", "kl_driver_judge_q16", "kl_judge_driver_q16", "max_dev_q16")
VERDICT_WORDS = ("mu_steer", "mu_throttle", "logstd_steer", "logstd_throttle")
Q16 = 65536.0
PLANS = ("everyone", "seated")


def check_deltas(who, deltas):
    """(delta_steer, delta_throttle) as two finite floats >= 0."""
    d = tuple(float(v) for v in deltas)
    if len(d) != 2 or not all(np.isfinite(v) and v >= 0.0 for v in d):
        raise ValueError("%s: deltas = %r, two finite numbers >= 0 wanted (steer, throttle)" % (who, deltas))
    return d


class JuryPlan:
    """`judges`: int [G][K], nonzero where bank member j judges the rows of scene group g of the seat plan `seats`.  Derived, as
    `SeatPlan` derives its lists: `rows` int64 [K][cap], judge j's ascending list of the SEATED rows e * N + n (seat >= 0, 0 <= group[e]
    < G) of the groups it judges, unused tail 0; `counts` int32 [K]; `cap` = the largest count, at least 1.  A row stands in the list of
    every one of its judges.  Nothing here touches a device."""

    def __init__(self, seats, judges):
        judges = np.ascontiguousarray(np.asarray(judges) != 0, np.int32)
        if judges.ndim != 2 or judges.shape != (seats.n_groups, seats.K):
            raise ValueError("JuryPlan: judges of shape %s, the seat plan has %d groups x %d members" % (judges.shape, seats.n_groups, seats.K))
        self.judges, (self.G, self.K) = judges, judges.shape
        self.E, self.N, self.n_out = seats.E, seats.N, seats.E * seats.N
        ok = (seats.group >= 0) & (seats.group < self.G)
        of_scene = np.where(ok[:, None], judges[np.clip(seats.group, 0, self.G - 1)], 0)          # [E][K]
        listed = (seats.seat >= 0)[:, :, None] & (of_scene != 0)[:, None, :]                       # [E][N][K]
        flat = listed.reshape(self.n_out, self.K)
        self.counts = flat.sum(axis=0).astype(np.int32)
        self.cap = max(int(self.counts.max()), 1)
        self.rows = np.zeros((self.K, self.cap), np.int64)
        for j in range(self.K):
            self.rows[j, :self.counts[j]] = np.nonzero(flat[:, j])[0]
        self.kind = None

    def check(self, seats):
        if (seats.n_groups, seats.K, seats.E, seats.N) != (self.G, self.K, self.E, self.N):
            raise ValueError("JuryPlan: built for %d groups x %d members on %d x %d seats, the seat plan has %d x %d on %d x %d" % (
                self.G, self.K, self.E, self.N, seats.n_groups, seats.K, seats.E, seats.N))
        return self

    @classmethod
    def _named(cls, seats, judges, kind):
        plan = cls(seats, judges)
        plan.kind = kind
        return plan

    @classmethod
    def everyone(cls, seats):
        """Every member judges every group."""
        return cls._named(seats, np.ones((seats.n_groups, seats.K), np.int32), "everyone")

    @classmethod
    def seated(cls, seats):
        """The judges of a group are the members with a seat in it: for `SeatPlan.pairs` focal and partner, two forwards per row."""
        judges = np.zeros((seats.n_groups, seats.K), np.int32)
        ok = (seats.group >= 0) & (seats.group < seats.n_groups)
        for e in np.nonzero(ok)[0]:
            s = seats.seat[e]
            judges[seats.group[e], s[s >= 0]] = 1
        return cls._named(seats, judges, "seated")

    @classmethod
    def panel(cls, seats, members):
        """A fixed panel: the `members` judge every group."""
        members = [int(m) for m in members]
        if not members or min(members) < 0 or max(members) >= seats.K or len(set(members)) != len(members):
            raise ValueError("JuryPlan.panel: members %r of a bank of %d" % (members, seats.K))
        judges = np.zeros((seats.n_groups, seats.K), np.int32)
        judges[:, members] = 1
        return cls._named(seats, judges, "panel")

    @classmethod
    def named(cls, seats, kind):
        if kind not in PLANS:
            raise ValueError("JuryPlan: plan = %r, one of %s wanted" % (kind, ", ".join(repr(p) for p in PLANS)))
        return cls.everyone(seats) if kind == "everyone" else cls.seated(seats)


class JuryBuffers(DeviceTables):
    """A jury plan's tables on the device: the judges' row lists, their counts and the judge table."""
    KEY = ("K", "cap", "G", "n_out")
    jury = property(lambda self: self.source)

    @staticmethod
    def tables(plan):
        return dict(rows=plan.rows, counts=plan.counts, judges=plan.judges), (plan.K, plan.cap, plan.G, plan.n_out)


def jury_tally(flags, dist, verdict, plan_buffers, jury_buffers, deltas, out):
    """One step's `flags` uint8 [E][N], the drivers' `dist` float32 [E][N][4] and `verdict` float32 [E N][K][4] added to `out` int64
    [G][K][K][8] (`JURY_WORDS`; [group][driver][judge]) by the seat plan's seat and group tables and the jury plan's judge table;
    `deltas` = (delta_steer, delta_throttle), the disagreement thresholds on the two means.  `out` accumulates (its max word keeps the
    largest); the caller clears it.  One launch on the current stream."""
    from .. import _capi
    pb, jb = plan_buffers, jury_buffers
    if (jb.G, jb.K, jb.n_out) != (pb.G, pb.K, pb.n_out):
        raise ValueError("jury_tally: a plan of %d groups x %d members on %d rows, judges for %d x %d on %d" % (pb.G, pb.K, pb.n_out, jb.G, jb.K, jb.n_out))
    for name, t, shape in (("dist", dist, (pb.n_out * 4,)), ("verdict", verdict, (pb.n_out * pb.K * 4,)), ("out", out, (pb.G * pb.K * pb.K * 8,))):
        if t.numel() != shape[0] or not t.is_contiguous():
            raise ValueError("jury_tally: %s of shape %s, %d contiguous elements wanted" % (name, tuple(t.shape), shape[0]))
    _capi.check(_capi.lib.copo_jury_tally(flags.data_ptr(), dist.data_ptr(), verdict.data_ptr(), pb.seat.data_ptr(), pb.group.data_ptr(),
                                          jb.judges.data_ptr(), pb.E, pb.N, pb.K, pb.G, float(deltas[0]), float(deltas[1]), out.data_ptr(),
                                          _capi.current_stream()))


class JurySeatSampler(SeatSampler):
    """`SeatSampler` with a jury: per env step `jury_seats` on the observation the policy reads into `verdict[t]`, the seated forward on
    the same observation, the simulator step, the seat tally and the jury fold of the step's flags -- the whole fragment is still one
    captured graph.  Actions, flags and the seat tally are a plain `SeatSampler`'s.  `verdict` [T][E][N][K][4] (also `batch["verdict"]`,
    zero-initialised: entries that no judge's list names are never written); `jury_tally` int64 [G][K][K][8] (`JURY_WORDS`) accumulates
    until `clear_tally()`."""

    def __init__(self, vec_env, policy, bank, plan, jury, T, use_graph=True, deltas=(0.05, 0.05)):
        import torch
        jury.check(plan)
        self.deltas = check_deltas("JurySeatSampler", deltas)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.jury_buffers = JuryBuffers(jury, self.device)
        self.jury_buffers.on_replace.append(self._loop.reset)
        self.verdict = torch.zeros(self.T, self.E, self.N, bank.K, len(VERDICT_WORDS), dtype=torch.float32, device=self.device)
        self.jury_tally = torch.zeros(plan.n_groups, bank.K, bank.K, len(JURY_WORDS), dtype=torch.int64, device=self.device)

    @property
    def jury(self):
        return self.jury_buffers.source

    def set_jury(self, jury):
        """Another jury plan, OUTSIDE captured graphs (`DeviceTables.replace`: other shapes drop the graph)."""
        self.jury_buffers.replace(jury.check(self.seated.plan))

    def clear_tally(self):
        super().clear_tally()
        self.jury_tally.zero_()

    def sample(self):
        batch = super().sample()
        batch["verdict"] = self.verdict
        return batch

    def _policy_obs(self, t):
        obs = super()._policy_obs(t)
        self.seated.jury_seats(self.jury_buffers, obs.view(-1, self.O), self.verdict[t].view(-1, self.seated.K, len(VERDICT_WORDS)))
        return obs

    def _step(self, t):
        super()._step(t)
        jury_tally(self.flags[t], self.dist_inputs[t], self.verdict[t], self.seated.buffers, self.jury_buffers, self.deltas, self.jury_tally)


def jury_rates(words):
    """The derived columns of one jury-tally cell (the eight `JURY_WORDS`): `disagree_rate` = disagree / pairs, the means `d_steer`,
    `d_throttle`, `d_logstd`, `kl_driver_judge`, `kl_judge_driver` over the pairs, `sym_kl` = their mean, and `max_dev`; NaN where
    there is no pair."""
    w = dict(zip(JURY_WORDS, (int(v) for v in words)))
    n = w["pairs"]
    ratio = lambda a: float(a) / float(n) if n > 0 else float("nan")  # noqa: E731
    kl_dj, kl_jd = ratio(w["kl_driver_judge_q16"] / Q16), ratio(w["kl_judge_driver_q16"] / Q16)
    return dict(disagree_rate=ratio(w["disagree"]), d_steer=ratio(w["d_steer_q16"] / Q16), d_throttle=ratio(w["d_throttle_q16"] / Q16),
                d_logstd=ratio(w["d_logstd_q16"] / Q16), kl_driver_judge=kl_dj, kl_judge_driver=kl_jd, sym_kl=0.5 * (kl_dj + kl_jd),
                max_dev=w["max_dev_q16"] / Q16 if n > 0 else float("nan"))


def jury_frame(tally, seats, jury, labels=None, deltas=None):
    """The jury tally [G][K][K][8] (numpy int64) as a frame: one row per (group, driver, judge) with the driver seated in the group and
    the judge on its panel.  Columns: `group` (a `pairs` plan: also `focal`, `partner`), `driver`, `judge`, `driver_label`,
    `judge_label`, `delta_steer` / `delta_throttle` where `deltas` is given, the eight raw words (`JURY_WORDS`) and `jury_rates`."""
    import pandas as pd
    labels = list(range(seats.K)) if labels is None else list(labels)
    rows = []
    for g in range(seats.n_groups):
        in_group = seats.seat[seats.group == g]
        drivers = [k for k in range(seats.K) if (in_group == k).any()]
        pair = {} if seats.focal is None else dict(focal=int(seats.focal[g]), partner=int(seats.partner[g]))
        for k in drivers:
            for j in np.nonzero(jury.judges[g])[0]:
                w = [int(v) for v in tally[g, k, j]]
                rows.append(dict(group=g, **pair, driver=k, judge=int(j), driver_label=labels[k], judge_label=labels[int(j)],
                                 **({} if deltas is None else dict(delta_steer=float(deltas[0]), delta_throttle=float(deltas[1]))),
                                 **dict(zip(JURY_WORDS, w)), **jury_rates(w)))
    return pd.DataFrame(rows)


def jury_matrix(frame, n_members=None):
    """The K x K symmetric-KL table of a `jury_frame` over all groups: entry (a, b) pools the pairs (driver a, judge b) and (driver b,
    judge a) and is (sum of both KL words) / (2 * 65536 * pairs): the mean of 0.5 (KL(a || b) + KL(b || a)) on the states either drives.
    NaN where neither judged the other.  Symmetric by construction; the diagonal is 0 wherever a member judged itself."""
    import pandas as pd
    K = int(max(frame["driver"].max(), frame["judge"].max())) + 1 if n_members is None else int(n_members)
    kl, pairs = np.zeros((K, K), np.float64), np.zeros((K, K), np.int64)
    for k, j, n, a, b in zip(frame["driver"], frame["judge"], frame["pairs"], frame["kl_driver_judge_q16"], frame["kl_judge_driver_q16"]):
        kl[int(k), int(j)] += float(int(a) + int(b))
        pairs[int(k), int(j)] += int(n)
    kl, pairs = kl + kl.T, pairs + pairs.T
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(pairs > 0, kl / (2.0 * Q16 * pairs), np.nan)
    return pd.DataFrame(m, index=range(K), columns=range(K))


def jury_rows(algo, env, weights_list, plan="everyone", share=0.5, deltas=(0.05, 0.05), scenes_per_pair=4, num_agents=40, steps=1000, seed=0,
              labels=None, **extra):
    """The K populations `weights_list` (one layout) on the `SeatPlan.pairs` layout of `cross_play_rows` -- every ordered pair (focal,
    partner) on the same `scenes_per_pair` scenes, the first round(share * num_agents) slots driven by the focal member -- with a jury:
    `plan` = "everyone" (all K members judge every row) or "seated" (focal and partner judge the rows of their pair), for `steps` env
    steps (rounded up to whole fragments).  Returns the `jury_frame`: one row per (pair, driver, judge)."""
    def check():
        if plan not in PLANS:
            raise ValueError("jury_rows: plan = %r, one of %s wanted" % (plan, ", ".join(repr(p) for p in PLANS)))
        check_deltas("jury_rows", deltas)

    return run_pairs("jury_rows", algo, env, weights_list,
                     lambda t, bank, seats, use_graph: JurySeatSampler(t.env, t.policy, bank, seats, JuryPlan.named(seats, plan), t.sampler.T,
                                                                       use_graph=use_graph, deltas=deltas),
                     lambda smp, seats, labels: jury_frame(smp.jury_tally.cpu().numpy(), seats, smp.jury, labels, smp.deltas),
                     share=share, scenes_per_pair=scenes_per_pair, num_agents=num_agents, steps=steps, seed=seed, labels=labels, extra=extra,
                     check=check)


def jury_verdicts(bank, obs):
    """`verdict` [n][K][4] (`VERDICT_WORDS`) of every member of `bank` on every row of obs [n][O]: one launch with every member judging
    every row."""
    import torch
    n = int(obs.shape[0])
    seats = SeatPlan(np.zeros((1, n), np.int32), bank.K)
    jb = JuryBuffers(JuryPlan.everyone(seats), obs.device)
    verdict = torch.zeros(n, bank.K, len(VERDICT_WORDS), dtype=torch.float32, device=obs.device)
    bank.sync_mirror()
    bank.jury_seats(jb, obs, verdict)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return verdict
