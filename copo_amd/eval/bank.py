"""A bank of K policies of one layout that act in one batch: the rollout side of a checkpoint sweep.

The reference's `copo/eval.py:93-241` evaluates every checkpoint of every trial one after the other.  Here K checkpoints of one algorithm
and scene drive E / K scenes each of ONE simulator batch: `PolicyBank` holds their flat parameter sets (and transposed mirrors) in one
buffer and acts through `copo_mlp_forward_bank_f32`, in which row m belongs to member m / rows_per_member and no tile of rows spans two
members; `BankSampler` is `VecSampler` with the bank in the policy's place, so the rollout stays one captured graph of one forward and
one step per env step.  Every member sees the same scene seeds and the same action noise: two members differ by their weights (and,
with `VecSim.set_lcf_table`, their LCF distribution) only.

One bank is one layout: members of other observation widths or algorithms belong to another bank (`evaluate.sweep_trials` groups by it).

The samplers of `eval/` keep no rollout loop of their own.  `VecSampler._rollout` is the one loop, `for t: _act(t); _step(t)`, with three
hooks: `_policy_obs(t)` (what the policy reads), `_act(t)` (the forward) and `_step(t)` (the simulator step).  `BankSampler` overrides
none of them: `_BankPolicy` puts the bank where `_act` looks for the fused learner.  Helpers that every sampler here shares also live
in this module: `replica_seeds` (replicas of S scenes see the same scenes), `DeviceTables` (tables that a captured graph reads) and
`draw_cell_noise`; what the samplers of the LiDAR studies share on top of `crossplay.SeatSampler` is `levels.LevelSeatSampler`.  The
bank's three seat passes (`perturb_seats`, `pgd_seats`, `certify_seats`) go through one checked launch, `_seat_pass`.
"""
import ctypes as C

import numpy as np
import torch

from ..trainer import VecSampler

CERTIFY_METHODS = ("interval", "linear")      # `certify_seats`: copo_cert_obs_seats_f32, copo_lin_obs_seats_f32


def check_certify_method(who, method):
    if method not in CERTIFY_METHODS:
        raise ValueError("%s: method = %r, one of %s wanted" % (who, method, ", ".join(repr(m) for m in CERTIFY_METHODS)))
    return method


class PolicyBank:
    """K flat parameter sets of `layout_from`'s model.  `layout_from`: a trainer policy with a fused learner (`policy.fused`), whose
    model each member is loaded into once, as `load_policy_weights` loads it (either reference key layout), and copied out of; the
    model's own weights are put back afterwards.  Members whose shapes differ from the model's are refused.  A member is the model's
    whole flat buffer, so that the policy's own layout and `copo_transpose_weights_f32` serve it unchanged; the value nets in it
    are never read, unless `values=True` (eval/critics.py): then every member's value nets are loaded into its slice too, from the
    full state-dict keys `checkpoint_io.value_state_dict` finds, a member that lacks one of the model's value entries or has it in
    another shape is refused by member and key, and `value_seats` runs them."""

    def __init__(self, layout_from, weights, values=False):
        from .. import _capi
        from .checkpoint_io import is_value_key, load_policy_state_dict, policy_state_dict, value_state_dict
        weights = list(weights)
        if not weights:
            raise ValueError("PolicyBank: no members")
        fz = getattr(layout_from, "fused", None)
        if fz is None or not fz.can_forward:
            raise ValueError("PolicyBank needs a policy with a fused learner whose layout the forward kernel covers (hidden 64 / 128 / "
                             "256 / 512): there is no framework fallback")
        model = layout_from.model
        own = model.state_dict()
        sds = [policy_state_dict(w) for w in weights]
        self.has_values = bool(values)
        if values:
            wanted = [name for name in own if is_value_key(name)]
            for k, w in enumerate(weights):
                vsd = value_state_dict(w)
                for name in wanted:
                    if name not in vsd:
                        raise ValueError("PolicyBank member %d: no value entry %s (a policy-only file? `load_members(paths, values=True)` keeps "
                                         "a checkpoint's value nets)" % (k, name))
                sds[k] = dict(sds[k], **{name: vsd[name] for name in wanted})
        for k, sd in enumerate(sds):             # every member is checked before the first is loaded
            for name, v in sd.items():
                if name not in own or tuple(own[name].shape) != tuple(v.shape):
                    raise ValueError("PolicyBank member %d: %s has shape %s, the model's is %s" % (
                        k, name, tuple(v.shape), tuple(own[name].shape) if name in own else None))
        self._capi, self.cfg, self.K = _capi, fz.cfg, len(weights)
        self.stride = int(fz.flat.numel)
        flat = fz.flat.flat
        self.theta = torch.empty(self.K, self.stride, dtype=torch.float32, device=flat.device)
        self.theta_t = torch.zeros_like(self.theta)
        keep = flat.clone()
        for k, sd in enumerate(sds):
            load_policy_state_dict(model, sd)
            self.theta[k].copy_(flat)
        with torch.no_grad():
            flat.copy_(keep)
        fz.invalidate_mirror()
        self._mirror_ok = False

    @property
    def can_forward(self):
        return True

    def invalidate_mirror(self):
        self._mirror_ok = False

    def sync_mirror(self):
        """The transposed mirror of every member: `copo_transpose_weights_f32` once per member on its slice.  Outside captured graphs."""
        if self._mirror_ok:
            return
        st = self._capi.current_stream()
        for k in range(self.K):
            self._capi.check(self._capi.lib.copo_transpose_weights_f32(C.byref(self.cfg), self.theta[k].data_ptr(),
                                                                      self.theta_t[k].data_ptr(), st))
        self._mirror_ok = True

    def act(self, obs, eps, action, logp, dist_inputs, clipped=None):
        """`FusedLearner.act` for dense obs [K * R, O]: rows [k R, (k + 1) R) are member k's."""
        rows = int(obs.shape[0])
        if rows % self.K:
            raise ValueError("PolicyBank.act: %d rows for %d members" % (rows, self.K))
        self._capi.check(self._capi.lib.copo_mlp_forward_bank_f32(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, rows // self.K, obs.data_ptr(),
            dist_inputs.data_ptr(), eps.data_ptr(), action.data_ptr(), logp.data_ptr(),
            None if clipped is None else clipped.data_ptr(), self._capi.current_stream()))

    def act_seats(self, plan_buffers, obs, eps, action, logp, dist_inputs, clipped=None):
        """`FusedLearner.act` with a member per ROW (eval/crossplay.py): obs [n_out, O]; member k reads and writes the rows of its list
        in `plan_buffers` (`crossplay.PlanBuffers`: rows [K][cap], counts [K] on the device), rows in no list are left alone."""
        pb = plan_buffers
        if pb.K != self.K or int(obs.shape[0]) != pb.n_out:
            raise ValueError("PolicyBank.act_seats: a plan of %d members over %d rows for a bank of %d and %d rows" % (
                pb.K, pb.n_out, self.K, int(obs.shape[0])))
        self._capi.check(self._capi.lib.copo_mlp_forward_seats_f32(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, pb.rows.data_ptr(), pb.counts.data_ptr(),
            pb.cap, pb.n_out, obs.data_ptr(), dist_inputs.data_ptr(), eps.data_ptr(), action.data_ptr(), logp.data_ptr(),
            None if clipped is None else clipped.data_ptr(), self._capi.current_stream()))

    def _seat_pass(self, who, entry, pb, lb, tensors, col_lo, col_hi, middle, extra=(), dtype_text=lambda dtype: str(dtype).replace("torch.", "")):
        """One launch of a seat pass on the current stream (csrc/learn_fused.hip, seat_pass_launch): `entry`(the bank, the plan's row
        lists, obs, *middle, the columns, the plan's groups, the level tables of `lb`, *extra, stream).  `tensors`: rows (name, tensor or
        None, shape, dtype), `obs` first, every tensor given must be contiguous of that shape and dtype; `who` opens the messages, `dtype_text`
        is how they name the dtype that was wanted."""
        if pb.K != self.K or (lb.G, lb.K) != (pb.G, pb.K):
            raise ValueError("%s: a bank of %d, a plan of %d groups x %d members, levels for %d x %d" % (who, self.K, pb.G, pb.K, lb.G, lb.K))
        for name, t, shape, dtype in tensors:
            if t is not None and (tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != dtype):
                raise ValueError("%s: %s of shape %s, contiguous %s %s wanted" % (
                    who, name, tuple(t.shape), dtype_text(dtype), list(shape)))
        self._capi.check(getattr(self._capi.lib, entry)(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, pb.rows.data_ptr(), pb.counts.data_ptr(),
            pb.cap, pb.n_out, tensors[0][1].data_ptr(), *(None if t is None else t.data_ptr() for t in middle), int(col_lo), int(col_hi), pb.N,
            pb.group.data_ptr(), pb.G, lb.level_of.data_ptr(), lb.levels.data_ptr(), lb.L, *extra, self._capi.current_stream()))

    def perturb_seats(self, plan_buffers, adv_buffers, obs, obs_seen, col_lo, col_hi, grad=None):
        """`copo_adv_obs_seats_f32` (eval/adversary.py) on the current stream: obs [n_out, O] -> obs_seen, one gradient-sign step on
        the columns [col_lo, col_hi) of every seated row against the member that drives it, at the level `adv_buffers`
        (`adversary.AdversaryBuffers`) gives (scene group, member); `grad` [n_out, O]: the raw gradient, if wanted.  Needs the mirror
        (`sync_mirror`), as `act_seats`."""
        row = (plan_buffers.n_out, int(self.cfg.pol.in_dim))
        self._seat_pass("PolicyBank.perturb_seats", "copo_adv_obs_seats_f32", plan_buffers, adv_buffers,
                        [(name, t, row, torch.float32) for name, t in (("obs", obs), ("obs_seen", obs_seen), ("grad", grad))], col_lo, col_hi,
                        (obs_seen, grad))

    def pgd_seats(self, plan_buffers, pgd_buffers, obs, obs_seen, col_lo, col_hi, seed=0, tick=None, trace=None, max_iters=None):
        """`copo_pgd_obs_seats_f32` (eval/pgd.py) on the current stream: obs [n_out, O] -> obs_seen, the iterated attack on the columns
        [col_lo, col_hi) of every seated row against the member that drives it, at the level `pgd_buffers` (`pgd.PGDBuffers`) gives
        (scene group, member).  `tick` int32 [n_out]: the launch counter of the random starts, advanced by the kernel (None: 0);
        `trace` [max_iters, n_out, O]: the gradient of every iteration, if wanted; `max_iters` defaults to the plan's.  Needs the
        mirror (`sync_mirror`), as `act_seats`."""
        max_iters = int(pgd_buffers.max_iters if max_iters is None else max_iters)
        row = (plan_buffers.n_out, int(self.cfg.pol.in_dim))
        self._seat_pass("PolicyBank.pgd_seats", "copo_pgd_obs_seats_f32", plan_buffers, pgd_buffers,
                        (("obs", obs, row, torch.float32), ("obs_seen", obs_seen, row, torch.float32),
                         ("trace", trace, (max_iters,) + row, torch.float32), ("tick", tick, row[:1], torch.int32)), col_lo, col_hi, (obs_seen,),
                        (int(seed) & (2 ** 64 - 1), None if tick is None else tick.data_ptr(), max_iters, None if trace is None else trace.data_ptr()), dtype_text=str)

    def certify_seats(self, plan_buffers, cert_buffers, obs, bounds, col_lo, col_hi, pad=0.0, method="interval", parts=None):
        """`copo_cert_obs_seats_f32` (eval/certify.py) on the current stream: obs [n_out, O] -> bounds [n_out, 8], the interval bounds
        of the two action means of every seated row over the L-infinity box of its level's `eps` on the columns [col_lo, col_hi), at
        the level `cert_buffers` (`certify.CertifyBuffers`) gives (scene group, member); `pad` >= 0 widens every bound.  Nothing is
        perturbed.  Needs the mirror (`sync_mirror`), as `act_seats`.  `method="linear"`: `copo_lin_obs_seats_f32` instead, the linear
        bounds intersected with the interval box into the same `bounds` layout; `parts` [n_out, 8] (linear only): both boxes before
        the pad, if wanted."""
        check_certify_method("PolicyBank.certify_seats", method)
        if parts is not None and method != "linear":
            raise ValueError("PolicyBank.certify_seats: `parts` is an output of method=\"linear\" only")
        n_out, linear = plan_buffers.n_out, method == "linear"
        self._seat_pass("PolicyBank.certify_seats", "copo_lin_obs_seats_f32" if linear else "copo_cert_obs_seats_f32", plan_buffers, cert_buffers,
                        (("obs", obs, (n_out, int(self.cfg.pol.in_dim)), torch.float32), ("bounds", bounds, (n_out, 8), torch.float32),
                         ("parts", parts, (n_out, 8), torch.float32)), col_lo, col_hi, (bounds, parts) if linear else (bounds,), (float(pad),))

    def attribute_seats(self, plan_buffers, attrib_buffers, obs, attr, heads, max_points=None):
        """`copo_ig_obs_seats_f32` (eval/attribution.py) on the current stream: obs [n_out, O] -> attr [n_out, 2, O] and heads [n_out, 8],
        the integrated gradients of the two action means of every seated row against the member that drives it, from the baseline and
        with the quadrature points of the level `attrib_buffers` (`attribution.AttributionBuffers`) gives (scene group, member);
        `max_points` defaults to the plan's.  Nothing is perturbed.  Needs the mirror (`sync_mirror`), as `act_seats`."""
        max_points = int(attrib_buffers.max_points if max_points is None else max_points)
        n_out, O = plan_buffers.n_out, int(self.cfg.pol.in_dim)
        self._seat_pass("PolicyBank.attribute_seats", "copo_ig_obs_seats_f32", plan_buffers, attrib_buffers,
                        (("obs", obs, (n_out, O), torch.float32), ("attr", attr, (n_out, 2, O), torch.float32), ("heads", heads, (n_out, 8), torch.float32),
                         ("base", attrib_buffers.base, (attrib_buffers.L, O), torch.float32)), 0, 0, (attr, heads),
                        (attrib_buffers.base.data_ptr(), max_points))

    def jury_seats(self, jury_buffers, obs, verdict):
        """`copo_jury_obs_seats_f32` (eval/jury.py) on the current stream: obs [n_out, O] -> verdict [n_out, K, 4], the four
        distribution inputs of every JUDGE j on the rows of its list in `jury_buffers` (`jury.JuryBuffers`: rows [K][cap], counts [K]
        on the device; a row may stand in many lists), the bits `act_seats` writes to `dist_inputs` for that member on that row.
        Entries that no list names are left alone.  Needs the mirror (`sync_mirror`), as `act_seats`."""
        jb = jury_buffers
        if jb.K != self.K:
            raise ValueError("PolicyBank.jury_seats: judges' lists for %d members and a bank of %d" % (jb.K, self.K))
        for name, t, shape in (("obs", obs, (jb.n_out, int(self.cfg.pol.in_dim))), ("verdict", verdict, (jb.n_out, self.K, 4))):
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("PolicyBank.jury_seats: %s of shape %s, contiguous float32 %s wanted" % (name, tuple(t.shape), list(shape)))
        self._capi.check(self._capi.lib.copo_jury_obs_seats_f32(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, jb.rows.data_ptr(), jb.counts.data_ptr(),
            jb.cap, jb.n_out, obs.data_ptr(), verdict.data_ptr(), self._capi.current_stream()))

    def value_seats(self, plan_buffers, obs, values, cc_obs=None):
        """`copo_value_obs_seats_f32` (eval/critics.py) on the current stream: obs [n_out, O] -> values [n_out, n_value_heads], every
        value net of the member that owns a row in `plan_buffers` (anything with rows [K][cap], counts [K], cap, n_out, K on the
        device) on `cc_obs` [n_out, value input width] (None: the observation itself), the bits `FusedLearner.values(rows=...)` writes
        for that member alone.  Rows in no list are left alone.  Needs a bank built with `values=True` and the mirror (`sync_mirror`)."""
        pb, nv = plan_buffers, int(self.cfg.n_value_heads)
        if not self.has_values:
            raise ValueError("PolicyBank.value_seats: the bank was built without value nets (PolicyBank(..., values=True))")
        if pb.K != self.K:
            raise ValueError("PolicyBank.value_seats: lists for %d members and a bank of %d" % (pb.K, self.K))
        src = obs if cc_obs is None else cc_obs
        for name, t, shape in (("obs", obs, (pb.n_out, int(self.cfg.pol.in_dim))), ("values", values, (pb.n_out, nv)),
                               ("cc_obs", src, (pb.n_out, int(self.cfg.val[0].in_dim)))):
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("PolicyBank.value_seats: %s of shape %s, contiguous float32 %s wanted" % (name, tuple(t.shape), list(shape)))
        self._capi.check(self._capi.lib.copo_value_obs_seats_f32(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, pb.rows.data_ptr(), pb.counts.data_ptr(),
            pb.cap, pb.n_out, obs.data_ptr(), None if cc_obs is None else cc_obs.data_ptr(), values.data_ptr(), self._capi.current_stream()))

    def hidden_seats(self, jury_buffers, obs, hidden):
        """`copo_hidden_obs_seats_f32` (eval/similarity.py) on the current stream: obs [n_out, O] -> hidden [K, cap, 2, H], both tanh
        layers of every JUDGE j on the rows of its list in `jury_buffers`, at the POSITION of the row in the list: the bits the jury
        pass holds before its heads.  Positions at or past a judge's count are left alone.  Needs the mirror (`sync_mirror`), as
        `act_seats`."""
        jb = jury_buffers
        if jb.K != self.K:
            raise ValueError("PolicyBank.hidden_seats: judges' lists for %d members and a bank of %d" % (jb.K, self.K))
        for name, t, shape in (("obs", obs, (jb.n_out, int(self.cfg.pol.in_dim))), ("hidden", hidden, (self.K, jb.cap, 2, int(self.cfg.hidden)))):
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("PolicyBank.hidden_seats: %s of shape %s, contiguous float32 %s wanted" % (name, tuple(t.shape), list(shape)))
        self._capi.check(self._capi.lib.copo_hidden_obs_seats_f32(
            C.byref(self.cfg), self.theta.data_ptr(), self.theta_t.data_ptr(), self.stride, self.K, jb.rows.data_ptr(), jb.counts.data_ptr(),
            jb.cap, jb.n_out, obs.data_ptr(), hidden.data_ptr(), self._capi.current_stream()))


class _BankPolicy:
    """What `VecSampler` reads of a policy, with the bank as its fused learner."""

    def __init__(self, policy, bank):
        self.fused, self.config, self.device = bank, {"use_fused_inference": True}, policy.device


class DeviceTables:
    """Tables of a numpy-only `source` (a plan) on the device, where a captured graph may read them.  A subclass declares `tables(source)`
    -> (named numpy arrays, shape key) and `KEY`, the names under which the key's entries become attributes.  `replace` is the one
    protocol, OUTSIDE captured graphs: a source of the same shape key is copied into the existing tensors (their addresses are what a
    graph holds), any other key allocates new tensors and calls the `on_replace` callbacks (a sampler drops its graph)."""
    KEY = ()

    def __init__(self, source, device):
        self.device, self.on_replace = torch.device(device), []
        self.load(source)

    def load(self, source):
        arrays, key = self.tables(source)
        self.key, self.source = tuple(key), source
        for name, v in zip(self.KEY, self.key):
            setattr(self, name, v)
        for name, a in arrays.items():
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(a)).to(self.device, copy=True))      # (never the source's own memory)

    def same_shape(self, key):
        return tuple(key) == self.key

    def copy_in(self, source):
        for name, a in self.tables(source)[0].items():
            getattr(self, name).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.source = source

    def replace(self, source):
        if self.same_shape(self.tables(source)[1]):
            return self.copy_in(source)
        self.load(source)
        for fn in self.on_replace:
            fn()


def replica_seeds(start_seed, S, E):
    """Scene seeds start_seed + arange(S), tiled E // S times: scenes [r S, (r + 1) S) of every replica r are the same scenes."""
    return np.tile(np.arange(S, dtype=np.uint64) + np.uint64(start_seed), E // S)


def draw_cell_noise(eps, scenes_per_cell):
    """Action noise eps [T][E][N][2] of a sweep whose cells are `scenes_per_cell` scenes each: ordinary noise, then the first cell's draw
    is copied to every cell, as `BankSampler` copies one member's -- the cells already share their scene seeds, so at the identity
    level two cells differ by their checkpoint only.  `scenes_per_cell` None (a hand-built plan): every scene its own draw."""
    eps.normal_()
    T, E, N = eps.shape[:3]
    per = scenes_per_cell
    if per and E > per and E % per == 0:
        cells = eps.view(T, E // per, per, N, 2)
        cells[:, 1:].copy_(cells[:, :1])


def members_of_scenes(num_envs, n_members):
    """Scenes per member; scene e belongs to member e // that."""
    if n_members < 1 or num_envs % n_members:
        raise ValueError("num_envs=%d is not a multiple of the %d members of the bank" % (num_envs, n_members))
    return num_envs // n_members


class BankSampler(VecSampler):
    """`VecSampler` whose scenes [k E / K, (k + 1) E / K) are driven by member k of `bank`.  Every fragment draws noise for
    [T, E / K, N, 2] and copies it to every member's scenes, and `reset` gives every member the seeds start_seed + arange(E / K)."""

    def __init__(self, vec_env, policy, bank, T, use_graph=True):
        self.bank = bank
        self.per_member = members_of_scenes(vec_env.sim.E, bank.K)
        super().__init__(vec_env, _BankPolicy(policy, bank), T, use_graph=use_graph, stagger_episodes=False)
        self._eps_member = torch.zeros(self.T, self.per_member, self.N, 2, dtype=torch.float32, device=self.device)

    def reset(self, seeds=None):
        if seeds is None:
            seeds = replica_seeds(self.sim.cfg.start_seed, self.per_member, self.E)
        super().reset(seeds)

    def _draw_noise(self):
        self._eps_member.normal_()
        self.eps.view(self.T, self.bank.K, self.per_member, self.N, 2).copy_(self._eps_member.unsqueeze(1))
