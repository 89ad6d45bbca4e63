"""A critic audit: the value heads of seated checkpoints against the returns their agents went on to realise.

Every other study of the seated evaluation reads the policy net.  The value nets are what make CoPO CoPO -- ego, neighbourhood and global
critics mixed by the LCF -- and here they are read: does a checkpoint's neighbourhood critic predict the neighbourhood return at all, is
a late checkpoint's ego critic better calibrated than an early one's, does a critic stay accurate when its policy drives beside a
partner from another population (`SeatPlan.pairs`)?

Pieces:

* `PolicyBank(..., values=True)` (eval/bank.py) loads every member's value nets; `PolicyBank.value_seats` is `copo_value_obs_seats_f32`
  (csrc/value_kernels.hip): the value nets of the member that owns a row, all heads, one launch, the bits `FusedLearner.values(rows=...)`
  writes for that member alone.
* `copo_audit_record` (csrc/audit_kernels.hip) compares V(s_t) with the discounted return that FOLLOWS it without storing a trajectory
  and without a backward pass: per (scene, slot, head) a float64 state carries c = sum gamma^(k-t), z = sum gamma^(k-t) V_t,
  q = sum gamma^(2(k-t)) and u = sum gamma^(k-t) G_t, and every reward r_k adds r_k c to sum G_t, r_k z to sum V_t G_t and
  r_k (r_k q + 2 gamma u) to sum G_t^2; the same per value bin gives a reliability diagram.  A finished agent's sums are quantised once
  to 2^-16 steps and added with 64-bit integer atomics per (scene group, member, head): 56 words, `SCALAR_WORDS` and three planes of
  16 bins.  G_t runs to the agent's last step, no bootstrap; an agent that ends by the max-step flag alone is truncated and counted
  only in `truncated` unless `count_truncated`; agents still open are never counted.  tests/critic_numpy.py restates the rules and
  proves the forward form against the backward recursion.
* `CriticSeatSampler`: per env step the value launch on the observation next to the seat forward, and after the step and the seat
  tally the audit record -- all of it in the fragment's one captured graph.  The drive and the seat tally are a plain `SeatSampler`'s,
  bit for bit.
* `critic_frame` / `calibration_frame`, `critic_audit_rows` (`evaluate --critic-audit`), `critic_values` (one launch on a plain array).

Scope: configurations whose critic reads the observation row (`fuse_mode = "none"`: CoPO's default, and IPPO).  A centralised `mf` /
`concat` critic is refused: feeding it means running `copo_cc_fuse_*` on the neighbour lists in front of the value launch, which this
module does not do.  fp32 operands only.
"""
import ctypes as C

import numpy as np

from .._handle import Handle
from .crossplay import PlanBuffers, SeatPlan, SeatSampler

SCALAR_WORDS = ("agents", "steps", "truncated", "sum_v_q16", "sum_vv_q16", "sum_g_q16", "sum_vg_q16", "sum_gg_q16")
MAX_BINS, N_WORDS, BIN_COUNT, BIN_VALUE, BIN_RETURN = 16, 56, 8, 24, 40
Q16 = 65536.0
HEAD_NAMES = ("ego", "neighbourhood", "global")
DEFAULT_RANGE = (-20.0, 20.0)


class CriticAudit:
    """What the audit folds with (numpy only): `gammas`, the discount per head (the trainer's own list: `[gamma]` for IPPO, `[gamma,
    gamma, 1.0]` for CoPO, `policy.gae_gammas()`); `value_range` (lo, hi) per head or one pair for all, the range the `bins` (1..16)
    equal value bins divide, values outside land in the end bins; `count_truncated`: count agents that ended by the max-step flag alone."""

    def __init__(self, gammas, value_range=DEFAULT_RANGE, bins=8, count_truncated=False):
        self.gammas = tuple(float(g) for g in gammas)
        H = len(self.gammas)
        if not 1 <= H <= 3 or not all(0.0 <= g <= 1.0 for g in self.gammas):
            raise ValueError("CriticAudit: gammas = %r, one to three discounts in [0, 1] wanted" % (gammas,))
        vr = np.asarray(value_range, np.float64)
        if vr.shape == (2,):
            vr = np.tile(vr, (H, 1))
        if vr.shape != (H, 2) or not np.isfinite(vr).all() or not (vr[:, 0] < vr[:, 1]).all():
            raise ValueError("CriticAudit: value_range = %r, finite (lo, hi) with lo < hi wanted, one pair or one per head (%d)" % (value_range, H))
        self.value_range = tuple((float(lo), float(hi)) for lo, hi in vr)
        self.bins = int(bins)
        if not 1 <= self.bins <= MAX_BINS or self.bins != bins:
            raise ValueError("CriticAudit: bins = %r, 1..%d wanted" % (bins, MAX_BINS))
        self.count_truncated = bool(count_truncated)

    heads = property(lambda self: len(self.gammas))

    def bin_edges(self, head):
        lo, hi = self.value_range[head]
        return np.linspace(lo, hi, self.bins + 1)


class AuditFold(Handle):
    """Host side of `copo_audit_*`: the per-slot state and the accumulator int64 [G][K][heads][56] of one plan shape on one device."""
    _prefix = "copo_audit_"

    def __init__(self, E, N, K, G, audit, device):
        import torch
        from .. import _capi
        self._capi, self._torch, self.sim, self.audit = _capi, torch, None, audit
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.shape = (int(G), int(K), audit.heads, N_WORDS)
        cfg = _capi.AuditCfg(E=int(E), N=int(N), K=int(K), G=int(G), heads=audit.heads, bins=audit.bins, count_truncated=int(audit.count_truncated))
        for h in range(audit.heads):
            cfg.gamma[h], (cfg.lo[h], cfg.hi[h]) = audit.gammas[h], audit.value_range[h]
        with torch.cuda.device(self.device):
            self._create(_capi.lib.copo_audit_create, C.byref(cfg))

    def record(self, flags, values, rew, nei_rew, glob_rew, seat, group):
        """One env step, on the current stream: flags uint8 [E][N], values [E N][heads], rew / nei_rew [E][N], glob_rew [E] (the last two
        may be None where the audit has fewer heads), seat int32 [E][N], group int32 [E]."""
        p = self._capi.ptr
        self._capi.check(self._capi.lib.copo_audit_record(self._h, p(flags), p(values), p(rew), p(nei_rew), p(glob_rew), p(seat), p(group),
                                                          self._stream()))

    def words(self):
        """The accumulator, device int64 [G][K][heads][56] (a copy; no host read)."""
        out = self._torch.empty(self.shape, dtype=self._torch.int64, device=self.device)
        self._call("read", out.data_ptr())
        return out

    def reset(self):
        self._call("reset")


def check_critic_input(who, policy, bank, O):
    """The configurations this module runs: a bank with value nets whose critic reads the observation row."""
    if not getattr(bank, "has_values", False):
        raise ValueError("%s: the bank holds no value nets (PolicyBank(layout_from, weights, values=True))" % who)
    cfg = getattr(policy, "config", None) or {}
    mode = cfg.get("fuse_mode", "none")
    if int(bank.cfg.val[0].in_dim) != int(O) or mode not in (None, "none"):
        raise ValueError("%s: a centralised critic (fuse_mode = %r, critic input %d wide, observation %d) is out of scope: only critics that read "
                         "the observation row (fuse_mode = \"none\": CoPO's default, IPPO) are audited" % (who, mode, int(bank.cfg.val[0].in_dim), int(O)))


class CriticSeatSampler(SeatSampler):
    """`SeatSampler` with a critic audit: per env step `value_seats` on the observation the policy reads into `values[t]`, the seated
    forward, the simulator step, the seat tally and `copo_audit_record` of the step's flags and rewards -- the whole fragment is still
    one captured graph.  Actions, flags and the seat tally are a plain `SeatSampler`'s.  `values` [T][E][N][heads] (also
    `batch["critic_values"]`; zero where no member is seated); `audit_words()` int64 [G][K][heads][56] accumulates until
    `clear_tally()`, which also forgets every open agent.  A centralised (`mf` / `concat`) critic is refused: out of scope here."""

    def __init__(self, vec_env, policy, bank, plan, audit, T, use_graph=True):
        import torch
        check_critic_input("CriticSeatSampler", policy, bank, vec_env.sim.O)
        if audit.heads != int(bank.cfg.n_value_heads):
            raise ValueError("CriticSeatSampler: an audit of %d heads for a model with %d value heads" % (audit.heads, int(bank.cfg.n_value_heads)))
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.audit = audit
        self.values = torch.zeros(self.T, self.E, self.N, audit.heads, dtype=torch.float32, device=self.device)
        self.fold = AuditFold(self.E, self.N, bank.K, plan.n_groups, audit, self.device)

    def clear_tally(self):
        super().clear_tally()
        self.fold.reset()

    def audit_words(self):
        return self.fold.words()

    def sample(self):
        batch = super().sample()
        batch["critic_values"] = self.values
        return batch

    def _policy_obs(self, t):
        obs = super()._policy_obs(t)
        self.seated.bank.value_seats(self.seated.buffers, obs.view(-1, self.O), self.values[t].view(-1, self.audit.heads))
        return obs

    def _step(self, t):
        super()._step(t)
        pb, nh = self.seated.buffers, self.audit.heads
        self.fold.record(self.flags[t], self.values[t], self.rew3[0, t], self.rew3[1, t] if nh > 1 else None, self.glob[t] if nh > 2 else None,
                         pb.seat, pb.group)


def critic_stats(words):
    """The derived columns of one cell's 56 words, over the steps of its counted agents: `mean_value`, `mean_return`, `bias` = mean(V -
    G), `rmse`, `corr`, `explained_variance` = 1 - Var(G - V) / Var(G); NaN where a denominator is 0."""
    w = [int(v) for v in words]
    n = w[1]
    nan = float("nan")
    if n <= 0:
        return dict(mean_value=nan, mean_return=nan, bias=nan, rmse=nan, corr=nan, explained_variance=nan)
    sv, svv, sg, svg, sgg = (w[i] / Q16 for i in range(3, 8))
    mv, mg = sv / n, sg / n
    var_v, var_g, cov = svv / n - mv * mv, sgg / n - mg * mg, svg / n - mv * mg
    var_d = var_g + var_v - 2.0 * cov
    return dict(mean_value=mv, mean_return=mg, bias=mv - mg, rmse=float(np.sqrt(max((svv - 2.0 * svg + sgg) / n, 0.0))),
                corr=cov / float(np.sqrt(var_v * var_g)) if var_v > 0.0 and var_g > 0.0 else nan,
                explained_variance=1.0 - var_d / var_g if var_g > 0.0 else nan)


def _cells(words, plan, audit, labels):
    labels = list(range(plan.K)) if labels is None else list(labels)
    words = np.asarray(words)
    if words.shape != (plan.n_groups, plan.K, audit.heads, N_WORDS):
        raise ValueError("critic words of shape %s, [%d][%d][%d][%d] wanted" % (words.shape, plan.n_groups, plan.K, audit.heads, N_WORDS))
    for g in range(plan.n_groups):
        in_group = plan.seat[plan.group == g]
        pair = {} if plan.focal is None else dict(focal=int(plan.focal[g]), partner=int(plan.partner[g]))
        for k in range(plan.K):
            if not (in_group == k).any():
                continue
            for h in range(audit.heads):
                yield dict(group=g, **pair, member=k, label=labels[k], head=h, head_name=HEAD_NAMES[h], gamma=audit.gammas[h]), words[g, k, h]


def critic_frame(words, plan, audit, labels=None):
    """The audit words [G][K][heads][56] (numpy int64) as a frame: one row per (scene group, member seated in it, head) with the eight
    scalar words (`SCALAR_WORDS`) and `critic_stats`."""
    import pandas as pd
    return pd.DataFrame([dict(key, **dict(zip(SCALAR_WORDS, (int(v) for v in w[:8]))), **critic_stats(w)) for key, w in _cells(words, plan, audit, labels)])


def calibration_frame(words, plan, audit, labels=None):
    """The reliability diagram: one row per (scene group, member, head, bin) with the bin's value range, `count`, `mean_value` and
    `mean_return` (NaN for an empty bin)."""
    import pandas as pd
    rows = []
    for key, w in _cells(words, plan, audit, labels):
        edges = audit.bin_edges(key["head"])
        for b in range(audit.bins):
            n = int(w[BIN_COUNT + b])
            rows.append(dict(key, bin=b, value_lo=float(edges[b]), value_hi=float(edges[b + 1]), count=n,
                             mean_value=int(w[BIN_VALUE + b]) / Q16 / n if n else float("nan"),
                             mean_return=int(w[BIN_RETURN + b]) / Q16 / n if n else float("nan")))
    return pd.DataFrame(rows)


def calibration_of(frame, n_members=None):
    """The calibration frame that `critic_audit_rows` attached to its table."""
    return frame.attrs["calibration"]


def audit_plan(K, scenes, N, pairs=False, share=None):
    """The seat plan of `critic_audit_rows`: `SeatPlan.pairs` (the cross-play question; `share` defaults to 0.5), or whole scenes per
    member, `scenes` each, group = member, every member on the same scenes.  Whole scenes have no share: one given there is refused."""
    if pairs:
        return SeatPlan.pairs(K, scenes, N, 0.5 if share is None else share)
    if share is not None:
        raise ValueError("audit_plan: share = %r goes with pairs (whole scenes per member have no share)" % (share,))
    K, S, N = int(K), int(scenes), int(N)
    if K < 1 or S < 1 or N < 1:
        raise ValueError("audit_plan: K=%d scenes=%d N=%d" % (K, S, N))
    member = np.repeat(np.arange(K, dtype=np.int32), S)
    return SeatPlan(np.repeat(member[:, None], N, axis=1), K, member, K, replica_scenes=S)


def critic_audit_rows(algo, env, weights_list, pairs=False, share=None, bins=8, value_range=DEFAULT_RANGE, count_truncated=False, gammas=None,
                      scenes_per_pair=4, num_agents=40, steps=1000, seed=0, labels=None, **extra):
    """The K populations `weights_list` (one layout, value nets included: `load_members(paths, values=True)`) audited for `steps` env steps
    (rounded up to whole fragments): every member on `scenes_per_pair` scenes of its own (the same scenes for every member), or with
    `pairs` on the `SeatPlan.pairs` layout of `cross_play_rows` (`share`: the focal member's, default 0.5; refused without `pairs`),
    which shows a critic beside every partner.  `gammas` defaults to the
    trainer's own list.  Returns the `critic_frame`; its `attrs["calibration"]` is the `calibration_frame`."""
    from .bank import PolicyBank
    from .evaluate import check_labels, eval_session, graph_flag, run_steps
    weights_list = list(weights_list)
    K = len(weights_list)
    if K < 1:
        raise ValueError("critic_audit_rows: no members")
    vr = np.asarray(value_range, np.float64)      # the argument checks, before a device is touched (the trainer's discounts come later)
    CriticAudit([1.0] * (vr.shape[0] if vr.ndim == 2 else 1) if gammas is None else gammas, value_range, bins, count_truncated)
    labels = check_labels(labels, K)
    seats = audit_plan(K, scenes_per_pair, num_agents, pairs, share)
    with eval_session(algo, env, seats.E, num_agents, seed, **extra) as t:
        audit = CriticAudit(t.policy.gae_gammas() if gammas is None else gammas, value_range, bins, count_truncated)
        bank = PolicyBank(t.policy, weights_list, values=True)
        smp = run_steps(CriticSeatSampler(t.env, t.policy, bank, seats, audit, t.sampler.T, use_graph=graph_flag(t)), steps)
        words = smp.audit_words().cpu().numpy()
        smp.fold.close()
    df = critic_frame(words, seats, audit, labels)
    df.attrs["calibration"] = calibration_frame(words, seats, audit, labels)
    return df


def critic_values(bank, obs, member):
    """values [n][n_value_heads] of member `member` of `bank` (built with `values=True`) on every row of obs [n][O]: one launch."""
    import torch
    n, member = int(obs.shape[0]), int(member)
    if not 0 <= member < bank.K:
        raise ValueError("critic_values: member %d of a bank of %d" % (member, bank.K))
    check_critic_input("critic_values", None, bank, obs.shape[1])
    pb = PlanBuffers(SeatPlan(np.full((1, n), member, np.int32), bank.K), obs.device)
    values = torch.zeros(n, int(bank.cfg.n_value_heads), dtype=torch.float32, device=obs.device)
    bank.sync_mirror()
    bank.value_seats(pb, obs, values)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return values
