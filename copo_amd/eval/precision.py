"""Precision sweeps: what a checkpoint loses when its policy runs in the precision it will be deployed in.

`faults.py` impairs what a driver sees, `adversary.py` / `pgd.py` attack it, `certify.py` bounds it and `jury.py` / `influence.py` compare
drivers.  Here the driver itself is rounded: a bank member drives with its policy net in bfloat16 or in OCP float8 e4m3 -- weights packed
once (`copo_lowp_pack`), both hidden layers on the matrix instructions of that format (`copo_lowp_forward_seats`, csrc/lowp_kernels.hip,
DESIGN.md section 8t) -- and its float32 twin, the same checkpoint through the unchanged seat forward, judges the rows it drives
(`copo_jury_obs_seats_f32`, `copo_jury_tally`, unchanged).  So a table carries outcome columns (the seat tally) and per-state drift
columns (the jury tally) and no fold of its own.

One launch serves one format: a fragment's forward is `PolicyBank.act_seats` on the float32 members' lists plus one launch per
low-precision format, each on the seat plan's row lists with the counts of the members of other formats at zero.

Pieces: `PrecisionPlan` (numpy only), `LowpBank` (the packed images of a `PolicyBank`'s members in one format), `MixedBank` (a bank whose
members each drive in their own precision; it stands where `SeatSampler` expects a `PolicyBank`), `PrecisionSeatSampler` (forwards,
simulator step, seat tally, jury launch and jury fold of a fragment stay one captured graph), `precision_sweep_rows` (`evaluate
--precision-sweep`) and `lowp_forward` (one launch on a plain observation array).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from .bank import draw_cell_noise
from .crossplay import SEAT_WORDS, SeatPlan, tally_rates
from .jury import JURY_WORDS, JuryPlan, JurySeatSampler, check_deltas, jury_rates

PRECISIONS = ("float32", "bfloat16", "float8_e4m3")
LOWP_FORMATS = {"bfloat16": 1, "float8_e4m3": 2}          # COPO_LOWP_BF16, COPO_LOWP_E4M3
DRIFT_WORDS = tuple("drift_" + w for w in JURY_WORDS)


def check_precisions(who, precisions):
    """`precisions` as a tuple of names of `PRECISIONS`, no name twice, "float32" first: every table carries its own baseline, and the
    float32 member is the judge of its low-precision twins."""
    ps = tuple(precisions)
    bad = [p for p in ps if p not in PRECISIONS]
    if not ps or bad or len(set(ps)) != len(ps) or ps[0] != "float32":
        raise ValueError("%s: precisions = %r; names of %s wanted, none twice, \"float32\" first (the baseline and the judge)" % (
            who, list(precisions), ", ".join(PRECISIONS)))
    return ps


def packed_bytes(hidden, in_dim, fmt):
    """Bytes of one member's packed image (include/copo_hip.h, copo_lowp_pack)."""
    esz = 1 if LOWP_FORMATS[fmt] == 2 else 2
    k1p = (int(in_dim) + 31) // 32 * 32
    return int(hidden) * (k1p + int(hidden)) * esz + 4 * (8 * int(hidden) + 8)


class PrecisionPlan:
    """The layout of a sweep of C checkpoints x P precisions.  The bank holds every checkpoint once per precision: member p * C + c is
    checkpoint c in `precisions[p]` (the float32 bank holds the same weights P times; the low-precision members drive from their packed
    images).  `member_precision` [P C]: index into `precisions`; `counts` {precision: int32 [P C]}: the seat plan's counts with the
    members of every other precision at zero, what each forward launch is given; `jury`: the `JuryPlan` in which the only judge of the
    rows of cell (c, p) is member c, the float32 twin; `checkpoint`, `precision` per scene group.  Nothing here touches a device."""

    def __init__(self, seats, precisions, n_checkpoints, share, scenes_per_cell):
        self.precisions, self.n_checkpoints, self.P = tuple(precisions), int(n_checkpoints), len(precisions)
        self.K = self.P * self.n_checkpoints
        self.share, self.scenes_per_cell = float(share), int(scenes_per_cell)
        self.n_lowp = int(round(self.share * seats.N))
        self.member_precision = np.repeat(np.arange(self.P, dtype=np.int32), self.n_checkpoints)
        self.member_checkpoint = np.tile(np.arange(self.n_checkpoints, dtype=np.int32), self.P)
        self.checkpoint = np.arange(seats.n_groups) // self.P
        self.precision = np.arange(seats.n_groups) % self.P
        self.counts = {p: np.where(self.member_precision == i, seats.counts, 0).astype(np.int32) for i, p in enumerate(self.precisions)}
        judges = np.zeros((seats.n_groups, self.K), np.int32)
        judges[np.arange(seats.n_groups), self.checkpoint] = 1
        self.jury = JuryPlan._named(seats, judges, "panel")

    @classmethod
    def sweep(cls, n_checkpoints, precisions, scenes_per_cell, N, share=1.0):
        """(seat plan, precision plan): one scene group per cell, group c * P + p = scenes [g S, (g + 1) S), S = `scenes_per_cell`, the
        same scenes for every cell (`replica_scenes`).  share == 1: every slot of cell (c, p) is member p * C + c.  share < 1: the first
        round(share * N) slots are that member and the rest its float32 twin, member c, in the same scene."""
        who = "PrecisionPlan.sweep"
        ps = check_precisions(who, precisions)
        Cn, S, N, share = int(n_checkpoints), int(scenes_per_cell), int(N), float(share)
        if Cn < 1 or S < 1 or N < 1 or not 0.0 <= share <= 1.0 or Cn * len(ps) > 65535:
            raise ValueError("%s: n_checkpoints=%d scenes_per_cell=%d N=%d share=%r" % (who, Cn, S, N, share))
        P = len(ps)
        cell = np.repeat(np.arange(Cn * P, dtype=np.int32), S)
        c_of, p_of = cell // P, cell % P
        n_lowp = int(round(share * N))
        seat = np.empty((Cn * P * S, N), np.int32)
        seat[:, :n_lowp] = (p_of * Cn + c_of)[:, None]
        seat[:, n_lowp:] = c_of[:, None]
        seats = SeatPlan(seat, Cn * P, cell, Cn * P, replica_scenes=S)
        return seats, cls(seats, ps, Cn, share, S)

    def check(self, seats):
        if (seats.n_groups, seats.K) != (self.n_checkpoints * self.P, self.K):
            raise ValueError("PrecisionPlan: %d cells x %d members, the seat plan has %d groups x %d members" % (
                self.n_checkpoints * self.P, self.K, seats.n_groups, seats.K))
        return self

    def members(self, weights_list):
        """The float32 bank of the plan: the checkpoints, once per precision."""
        weights_list = list(weights_list)
        if len(weights_list) != self.n_checkpoints:
            raise ValueError("PrecisionPlan: %d populations for %d checkpoints" % (len(weights_list), self.n_checkpoints))
        return weights_list * self.P


class LowpBank:
    """The packed images of the members of a `PolicyBank` in `fmt` ("bfloat16" or "float8_e4m3"): `packed` uint8 [K][stride].  `pack()`
    rebuilds them from the bank's parameters, OUTSIDE captured graphs (the constructor packs once); `act_seats` has `PolicyBank.act_seats`'s
    signature.  There is no framework fallback."""

    def __init__(self, bank, fmt):
        import torch
        if fmt not in LOWP_FORMATS:
            raise ValueError("LowpBank: fmt = %r, one of %s wanted" % (fmt, ", ".join(repr(f) for f in LOWP_FORMATS)))
        self.bank, self.fmt, self.code, self.K, self.cfg, self._capi = bank, fmt, LOWP_FORMATS[fmt], bank.K, bank.cfg, bank._capi
        self.image_bytes = packed_bytes(self.cfg.hidden, self.cfg.pol.in_dim, fmt)
        self.stride = (self.image_bytes + 255) // 256 * 256
        self.packed = torch.zeros(self.K, self.stride, dtype=torch.uint8, device=bank.theta.device)
        self.pack()

    def pack(self):
        self._capi.check(self._capi.lib.copo_lowp_pack(C.byref(self.cfg), self.bank.theta.data_ptr(), self.bank.stride, self.K, self.code,
                                                       self.packed.data_ptr(), self.stride, self._capi.current_stream()))

    def act_seats(self, plan_buffers, obs, eps, action, logp, dist_inputs, clipped=None):
        """`PolicyBank.act_seats` in this bank's format: member k reads and writes the rows of its list in `plan_buffers` (rows [K][cap],
        counts [K] on the device), rows in no list are left alone.  `eps` None: no sampling, `dist_inputs` only."""
        pb = plan_buffers
        if pb.K != self.K or int(obs.shape[0]) != pb.n_out or int(obs.shape[-1]) != int(self.cfg.pol.in_dim):
            raise ValueError("LowpBank.act_seats: a plan of %d members over %d rows and obs %s for a bank of %d members and %d inputs" % (
                pb.K, pb.n_out, tuple(obs.shape), self.K, int(self.cfg.pol.in_dim)))
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._capi.check(self._capi.lib.copo_lowp_forward_seats(
            C.byref(self.cfg), self.packed.data_ptr(), self.stride, self.code, self.K, pb.rows.data_ptr(), pb.counts.data_ptr(), pb.cap, pb.n_out,
            obs.data_ptr(), p(dist_inputs), p(eps), p(action), p(logp), p(clipped), self._capi.current_stream()))


def lowp_forward(bank, fmt, obs, member=0):
    """`dist_inputs` [n][4] of member `member` of `bank` in `fmt` on every row of obs [n][O]: one launch, no sampling."""
    import torch
    n = int(obs.shape[0])
    if not 0 <= int(member) < bank.K or n < 1:
        raise ValueError("lowp_forward: member %r of a bank of %d, %d rows" % (member, bank.K, n))
    counts = np.zeros(bank.K, np.int32)
    counts[int(member)] = n
    lists = SimpleNamespace(K=bank.K, cap=n, n_out=n, rows=torch.arange(n, dtype=torch.int64, device=obs.device).repeat(bank.K, 1).contiguous(),
                            counts=torch.from_numpy(counts).to(obs.device))
    out = torch.zeros(n, 4, dtype=torch.float32, device=obs.device)
    LowpBank(bank, fmt).act_seats(lists, obs.contiguous(), None, None, None, out)
    torch.cuda.current_stream().synchronize()          # (the lists and the images die with this call)
    return out


class MixedBank:
    """A `PolicyBank` whose members each drive in a precision of their own: `member_precision[k]` names member k's among `precisions`.
    It stands where `SeatedBank` / `SeatSampler` expect a `PolicyBank`: `act_seats` is the float32 seat forward on the float32 members'
    lists plus one `LowpBank.act_seats` per low-precision format in use; everything else (the mirror, the jury pass) is the float32
    bank's.  `bind(plan_buffers)` OUTSIDE captured graphs puts the per-format counts of a plan on the device; a captured `act_seats`
    reads them."""

    def __init__(self, bank, precisions, member_precision):
        self.bank, self.K, self.cfg, self.theta = bank, bank.K, bank.cfg, bank.theta
        self.precisions = tuple(precisions)
        self.member_precision = np.ascontiguousarray(member_precision, np.int32)
        if self.member_precision.shape != (bank.K,) or self.member_precision.min() < 0 or self.member_precision.max() >= len(self.precisions) \
                or any(p not in PRECISIONS for p in self.precisions):
            raise ValueError("MixedBank: member_precision %s over %r for a bank of %d" % (self.member_precision.shape, self.precisions, bank.K))
        self.lowp = {p: LowpBank(bank, p) for i, p in enumerate(self.precisions) if p != "float32" and (self.member_precision == i).any()}
        self._bound = {}

    can_forward = property(lambda self: True)

    def invalidate_mirror(self):
        self.bank.invalidate_mirror()

    def sync_mirror(self):
        self.bank.sync_mirror()

    def pack(self):
        for lb in self.lowp.values():
            lb.pack()

    def bind(self, plan_buffers):
        """The masked counts of `plan_buffers`' plan, per precision in use, on the device; rebinding a plan of the same member count
        copies into the tensors a captured graph already reads."""
        import torch
        pb = plan_buffers
        counts = np.ascontiguousarray(pb.source.counts, np.int32)
        if counts.shape != (self.K,):
            raise ValueError("MixedBank.bind: a plan of %d members for a bank of %d" % (counts.shape[0], self.K))
        _, lists = self._bound.setdefault(id(pb), (pb, {}))          # (the buffers are kept: their id stays theirs)
        for i, p in enumerate(self.precisions):
            if not (self.member_precision == i).any():
                continue
            masked = torch.from_numpy(np.where(self.member_precision == i, counts, 0).astype(np.int32))
            if p in lists:
                lists[p].counts.copy_(masked)
                lists[p].rows, lists[p].cap, lists[p].n_out = pb.rows, pb.cap, pb.n_out
            else:
                lists[p] = SimpleNamespace(K=self.K, cap=pb.cap, n_out=pb.n_out, rows=pb.rows, counts=masked.to(pb.rows.device))

    def act_seats(self, plan_buffers, obs, eps, action, logp, dist_inputs, clipped=None):
        if id(plan_buffers) not in self._bound:
            self.bind(plan_buffers)
        lists = self._bound[id(plan_buffers)][1]
        if "float32" in lists:
            self.bank.act_seats(lists["float32"], obs, eps, action, logp, dist_inputs, clipped)
        for p, lb in self.lowp.items():
            lb.act_seats(lists[p], obs, eps, action, logp, dist_inputs, clipped)

    def jury_seats(self, jury_buffers, obs, verdict):
        self.bank.jury_seats(jury_buffers, obs, verdict)


class PrecisionSeatSampler(JurySeatSampler):
    """`JurySeatSampler` on a `MixedBank`: per env step the float32 twins' verdicts on the observation, the float32 seat forward on the
    float32 members' lists, one low-precision launch per format, the simulator step, the seat tally and the jury fold -- one captured
    graph per fragment.  All cells share their scene seeds (`replica_scenes`) and their action noise (`draw_cell_noise`), so two cells
    differ by precision only.  `bank`: the float32 `PolicyBank` of `plan.members(...)`."""

    def __init__(self, vec_env, policy, bank, seats, plan, T, use_graph=True, deltas=(0.05, 0.05)):
        plan.check(seats)
        self.precision_plan = plan
        self.mixed = MixedBank(bank, plan.precisions, plan.member_precision)
        super().__init__(vec_env, policy, self.mixed, seats, plan.jury, T, use_graph=use_graph, deltas=deltas)
        self.mixed.bind(self.seated.buffers)

    def set_plan(self, plan):
        super().set_plan(plan)
        self.mixed.bind(self.seated.buffers)

    def _draw_noise(self):
        draw_cell_noise(self.eps, self.precision_plan.scenes_per_cell)


def precision_frame(tally, jury_tally, seats, plan, labels=None, deltas=None):
    """The seat tally [G][K][8] and the jury tally [G][K][K][8] (numpy int64) of a precision sweep as a frame: one row per (checkpoint,
    precision).  Columns: `checkpoint`, `label`, `precision`, `member`, `share`, `seats`, the thresholds where `deltas` is given, the eight
    raw words of the seat tally and its rates (`success`, `crash_rate`, `out_rate`, `reward_per_step`), the eight raw words of the jury
    tally of (cell, that member, its float32 twin) as `drift_<word>`, and `drift_steer`, `drift_throttle`, `drift_kl` (KL(driver || float32
    twin), the mean over the judged states), `drift_max`, `disagree_rate`.  The float32 rows' drift words are zeros."""
    import pandas as pd
    labels = list(range(plan.n_checkpoints)) if labels is None else list(labels)
    rows = []
    for g in range(seats.n_groups):
        c, p = int(plan.checkpoint[g]), int(plan.precision[g])
        m = p * plan.n_checkpoints + c
        w, j = [int(v) for v in tally[g, m]], [int(v) for v in jury_tally[g, m, c]]
        r = jury_rates(j)
        rows.append(dict(checkpoint=c, label=labels[c], precision=plan.precisions[p], member=m, share=plan.share,
                         seats=plan.n_lowp if p else seats.N, **({} if deltas is None else dict(delta_steer=float(deltas[0]), delta_throttle=float(deltas[1]))),
                         **dict(zip(SEAT_WORDS, w)), **tally_rates(w), **dict(zip(DRIFT_WORDS, j)), drift_steer=r["d_steer"], drift_throttle=r["d_throttle"],
                         drift_kl=r["kl_driver_judge"], drift_max=r["max_dev"], disagree_rate=r["disagree_rate"]))
    return pd.DataFrame(rows)


def precision_sweep_rows(algo, env, weights_list, precisions=PRECISIONS, share=1.0, deltas=(0.05, 0.05), scenes_per_cell=4, num_agents=40,
                         steps=1000, seed=0, labels=None, **extra):
    """The C populations `weights_list` (one layout) x `precisions` ("float32" first) on `PrecisionPlan.sweep`'s cells, the same scenes
    and the same action noise for every cell, for `steps` env steps (rounded up to whole fragments).  The first round(share *
    num_agents) slots of a cell drive in the cell's precision, the rest are float32 drivers of the same checkpoint.  Returns
    `precision_frame`: one row per (checkpoint, precision)."""
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    if len(weights_list) < 1:
        raise ValueError("precision_sweep_rows: no members")
    precisions = check_precisions("precision_sweep_rows", precisions)
    deltas = check_deltas("precision_sweep_rows", deltas)
    labels = check_labels(labels, len(weights_list))
    seats, plan = PrecisionPlan.sweep(len(weights_list), precisions, scenes_per_cell, num_agents, share)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        smp = PrecisionSeatSampler(t.env, t.policy, PolicyBank(t.policy, plan.members(weights_list)), seats, plan, t.sampler.T,
                                   use_graph=graph_flag(t), deltas=deltas)
        run_steps(smp, steps)
        return precision_frame(smp.tally.cpu().numpy(), smp.jury_tally.cpu().numpy(), seats, plan, labels, deltas)
