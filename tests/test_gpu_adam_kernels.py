"""The learner's hand-written Adam updates against an independent float64 evaluation (tests/adam_numpy.py), element by element, and the
data-parallel gradient -- the sum of the shard gradients, each taken with the GLOBAL denominator -- against the float64 gradient of the
global minibatch.  One process, one GPU: ranks are shard policies in this process, no collective, no peer wait.

Adam is nearly invariant to a constant factor on the gradient, and its first steps are lr * sign(g), so a comparison of trajectories
(test_gpu_fused_learner.py) has to allow whole steps of difference; here the kernels get a KNOWN gradient and every element of `flat`,
`adam_m`, `adam_v` is held to float64 in units of u = 2^-24:
    e_m = |m - m64| / (|m_in| + |g|),  e_v = |v - v64| / v64,  e_theta = |theta - theta64| / (kappa(t) |step64| + |theta64|)
with the limit e_hip <= 3 x the figure of a plain numpy float32 evaluation of the same formula on the same inputs (which
test_adam_numpy_cpu.py bounds by 3.5 u on the generator's inputs, so <= ~10 u there).  The factor covers what the kernels may do
differently from numpy: learn_fused.hip is compiled under `#pragma clang fp contract(fast)`, so the compiler may fuse multiply-adds
(adam_flat_kernel's m', v' and theta' are one FMA each in the gfx950 code, the epilogue of wgrad_adam_kernel reproduces numpy's
figures, so the two kernels are not bit-equal on the same gradient), and the device powf of the bias corrections is not correctly
rounded.  A bias correction at t +- 1, an eps inside the bias correction, a skipped or doubled element or a wrong moment coefficient
is off by hundreds to millions of units.  A failure names the tensor and the element.

Which Adam kernel runs (from launch_fused_step / launch_adam_flat, csrc/learn_fused.hip): the shipped library has g_use_wgrad = true as
a constant, so every call of copo_ppo_fused_step_f32 with apply_adam ends in wgrad_adam_kernel, whatever the hidden size; the Adam
branch of reduce_adam_kernel is reached only by a profiling build (COPO_FUSED_WGRAD=0) that the package never loads, and the meta
modes call reduce_adam_kernel with apply_adam = 0.  No hidden size of the shipped library reaches it, so no case here does.
  case                  in front of the update                          fused update                       FusedLearner.adam
  ccppo_mf_h48_mb72     tile-GEMM forward / head / backward (no row     wgrad_adam_kernel<1>               adam_flat_kernel, ragged
                        pass: hidden 48)                                                                   32 x 32 tiles (48 = 32 + 16)
  copo_h64_mb128        rowpass_kernel<1, 4>, four nets                 wgrad_adam_kernel<1>               adam_flat_kernel
  ippo_o91_h256_mb512   rowpass_kernel<2, 8, .., 8> (8-row tiles)       wgrad_adam_kernel<1, false, true>  adam_flat_kernel, W1 tiles
                                                                        (buffer-load operand ring)         ragged in the 91 inputs
  ccppo_mf_bf16_o156    rowpass8_kernel<4, true>                        wgrad_adam_kernel<1, true, true>   adam_flat_kernel, mirror in
                                                                                                           bfloat16-rounded W1 / W2

Measured on an MI355X, worst over the step numbers t = 1, 2, 10, 1000, 200 000, HIP e_m / e_v / e_theta | numpy float32:
  (a) adam_flat_kernel on the generator's gradient (all calling forms give the same bits)
      ccppo_mf_h48_mb72     0.94 / 2.32 / 1.98  | 1.00 / 2.32 / 2.82
      copo_h64_mb128        0.92 / 2.50 / 2.50  | 1.02 / 2.50 / 2.55
      ippo_o91_h256_mb512   0.94 / 2.63 / 2.64  | 1.01 / 2.63 / 3.40
      ccppo_mf_bf16_o156    0.94 / 2.76 / 3.23  | 1.02 / 2.79 / 3.36
  (b) wgrad_adam_kernel on the gradient it computed (adam_flat_kernel on the same gradient: e_theta 2.29, 2.02, 83.46, 3.63)
      ccppo_mf_h48_mb72     0.63 / 2.52 / 2.41  | 0.63 / 2.52 / 2.53
      copo_h64_mb128        0.76 / 2.68 / 2.76  | 0.76 / 2.68 / 2.63
      ippo_o91_h256_mb512   0.93 / 2.62 / 67.84 | 0.93 / 2.62 / 68.26
      ccppo_mf_bf16_o156    0.91 / 1.94 / 3.76  | 0.91 / 1.94 / 3.75
  (c) adam on the rank-ordered sum, t = 10: copo_h64_mb128 0.81 / 2.79 / 0.97 | 0.82 / 2.79 / 0.97, ccppo_mf_h48_mb72 0.72 / 2.66 / 0.96 |
      0.72 / 2.66 / 0.96; summed shard gradient against float64, worst tensor, relative to its largest element (HIP / torch fp32):
      copo_h64_mb128 kb = 0 8.4e-7 / 6.5e-7, kb = 2 5.9e-7 / 6.2e-7; ccppo_mf_h48_mb72 kb = 0 7.7e-7 / 6.0e-7, kb = 2 6.0e-7 / 3.7e-7.
The 68 u of ippo_o91_h256_mb512 in (b) (t = 1000 and 200 000 only) is the float32 FORMULA's error, numpy's as much as the kernels': with a
real gradient of the moments' size, m' = m + (g - m)(1 - beta1) cancels in some element, its relative error is then u (|m_in| + |g|) /
|m'| instead of u, and e_theta -- which allows kappa(t) u |step| -- shows it where |theta| is smaller than the step and kappa is near 1.
The generator cannot produce it (its gradient magnitudes stay away from the moments'), so (a) and the CPU test stay under 3.5 u; the
test prints the element whenever the numpy figure exceeds 3.5.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_numpy as an  # noqa: E402
from copo_amd.engine import SampleBatch  # noqa: E402
from test_gpu_fused_dispatch import _assert_mirror_is_the_transposed_parameters, _where  # noqa: E402
from test_gpu_fused_learner import _copy_weights, _dense_batch, _make  # noqa: E402

# (id, policy, fuse mode, observation width, _make overrides, rows R ~ 3 mb, valid rows B): the smallest shapes at which each kernel
# instantiation is still selected; B gives three minibatches that all end in zero-weight padding
CASES = [
    ("ccppo_mf_h48_mb72", "ccppo", "mf", 91, dict(hiddens=(48, 48), mb=72), 220, 190),          # 64 / 63 / 63 rows
    ("copo_h64_mb128", "copo", "none", 92, dict(hiddens=(64, 64), mb=128), 390, 340),           # 114 / 113 / 113 rows
    ("ippo_o91_h256_mb512", "ippo", "none", 91, {}, 1500, 1337),                                # 446 / 446 / 445 rows
    ("ccppo_mf_bf16_o156", "ccppo", "mf", 156, dict(policy_dtype="bfloat16"), 1500, 1337),
]
IDS = [c[0] for c in CASES]
STEP0 = tuple(t - 1 for t in an.STEPS)      # step_count in front of the update: t = 1, 2, 10, 1000, 200 000
KB = 1                                      # the minibatch the gradient passes of (a) and (b) run on
W = 3                                       # simulated ranks of (c)
FACTOR = 3.0                                # limit: FACTOR x the numpy float32 evaluation's own error
STATE_NAMES = ("adam_m", "adam_v", "flat")  # the order of adam_numpy's error triples


def _mb(case):
    return case[4].get("mb", 512)


def _policy(case, fused=True):
    _id, name, fuse, odim, over, _R, _B = case
    return _make(name, fuse, odim, fused=fused, num_sgd_iter=1, **over)


def _perturbed(case, fused=True):
    pol = _policy(case, fused)
    torch.manual_seed(29)
    with torch.no_grad():                       # move off the near-zero head init
        for p in pol.model.parameters():
            if p.dtype == torch.float32:
                p.add_(torch.randn_like(p) * 0.05)
    if pol.fused is not None:
        pol.fused.invalidate_mirror()
    return pol


def _ready(case):
    """A fused policy with perturbed weights, its batch bound and one epoch planned: three minibatches, each ending in padding."""
    _id, _name, _fuse, odim, _over, R, B = case
    pol, mb = _perturbed(case), _mb(case)
    assert pol.fused is not None
    batch = _dense_batch(pol, R, odim)
    g = torch.Generator(device="cuda").manual_seed(17)
    idx = torch.randperm(R, device="cuda", generator=g)[:B].sort().values.contiguous()
    pol.prepare_sgd(batch, R, mb)
    torch.manual_seed(5)
    assert pol.plan_epoch(idx, B, [B], mb) == 3
    rs = pol._row_sources
    assert rs["rows_all"].shape[0] >= 3 and bool((rs["w_all"][:3, -1] == 0).all()) and bool((rs["w_all"][:3, 0] == 1).all())
    return pol, rs


def _slots(pol):
    """Mask of the flat buffers' elements that belong to a parameter (the others: 16-byte alignment padding between tensors)."""
    fz = pol.fused
    slot = np.zeros(fz.flat.numel, bool)
    for p in fz.flat.params:
        o = fz.flat.offset[id(p)]
        slot[o:o + p.numel()] = True
    c, H = fz.cfg, int(fz.cfg.hidden)
    nets = sum(H * int(L.in_dim) + H + H * H + H + int(L.out_dim) * H + int(L.out_dim)
               for L in [c.pol] + [c.val[v] for v in range(int(c.n_value_heads))])
    assert nets == int(slot.sum()) and 0 < int((~slot).sum()) < 64      # every fp32 parameter is in a net the step updates; there IS padding
    return slot


def _hyper(fz):
    """(lr, beta1, beta2, eps) as the kernels read them: the fp32 fields of copo_ppo_cfg, widened."""
    c = fz.cfg
    h = tuple(float(v) for v in (c.lr, c.beta1, c.beta2, c.eps))
    assert h[1:] == (an.stored(an.BETA1), an.stored(an.BETA2), an.stored(an.EPS)) and h[0] == an.stored(h[0]) and h[0] > 0
    return h


def _generated(slot, seed):
    """adam_numpy's generator in every parameter slot; the padding stays zero in all four, as the library leaves it."""
    x = an.make_inputs(np.random.default_rng(seed), slot.size)
    x = {k: np.where(slot, v, np.float32(0)) for k, v in x.items()}
    assert all(v.dtype == np.float32 for v in x.values())
    return x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load_state(pol, theta, m, v, step0, kb):
    fz = pol.fused
    fz.flat.flat.copy_(theta)
    fz.adam_m.copy_(m)
    fz.adam_v.copy_(v)
    fz.step_count.fill_(step0)
    pol._row_sources["k"].fill_(kb)
    fz.invalidate_mirror()


def _read(fz):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (fz.flat.flat, fz.adam_m, fz.adam_v))


def _references(fz, x, t):
    args = (x["theta"], x["m"], x["v"], x["g"], t) + _hyper(fz)
    return an.adam_step(*args, np.float64), an.adam_step(*args, np.float32)


def _assert_adam(pol, slot, got, refs, x, t, what):
    """Every element of (theta, m, v) = `got` against float64, limit FACTOR x the numpy float32 evaluation's worst element.  Returns
    (HIP figures, numpy float32 figures), each (e_m, e_v, e_theta)."""
    want, np32 = refs
    inputs = dict(x, t=t)
    e_np = tuple(float(e[slot].max()) for e in an.elementwise_errors(np32, want, inputs))
    e_el = an.elementwise_errors(got, want, inputs)
    order = (1, 2, 0)          # (theta, m, v) tuples -> the (m, v, theta) order of the error triples
    for name, e, lim, j in zip(STATE_NAMES, e_el, e_np, order):
        bad = np.flatnonzero(~(e <= FACTOR * lim))
        if bad.size:
            i = int(bad[np.argmax(e[bad])])
            raise AssertionError("%s, t = %d: %s is off in %d of %d elements, worst at flat index %d = %s: got %r, float64 %r, numpy float32 %r: "
                                 "%.3g units of 2^-24, limit %g x %.2f (inputs theta %r m %r v %r g %r)"
                                 % (what, t, name, bad.size, e.size, i, _where(pol, i), got[j][i], want[j][i], np32[j][i], e[i], FACTOR, lim,
                                    x["theta"][i], x["m"][i], x["v"][i], x["g"][i]))
    e_hip = tuple(float(e[slot].max()) for e in e_el)
    # an element with g = m = v = 0 keeps theta bit for bit
    dead = (x["g"] == 0) & (x["m"] == 0) & (x["v"] == 0)
    moved = np.flatnonzero(dead & (got[0].view(np.uint32) != x["theta"].view(np.uint32)))
    assert moved.size == 0, "%s, t = %d: %d elements with g = m = v = 0 moved, first %s" % (what, t, moved.size, _where(pol, int(moved[0])))
    print("%s, t = %d: HIP e_m %.2f e_v %.2f e_theta %.2f | numpy float32 %.2f %.2f %.2f" % ((what, t) + e_hip + e_np))
    if e_np[2] > 3.5:      # beyond what the generator's inputs give (test_adam_numpy_cpu.py): say which element and why
        e_th = np.where(slot, an.elementwise_errors(np32, want, inputs)[2], 0.0)
        i = int(e_th.argmax())
        print("    numpy float32 e_theta %.2f at %s: theta %r m %r v %r g %r -> m' %r (|m_in| + |g| = %.1f |m'|), step %r"
              % (e_th[i], _where(pol, i), x["theta"][i], x["m"][i], x["v"][i], x["g"][i], want[1][i],
                 (abs(float(x["m"][i])) + abs(float(x["g"][i]))) / abs(want[1][i]), want[0][i] - float(x["theta"][i])))
    return e_hip, e_np


def _assert_padding_is_zero(pol, slot, what, mirror=True):
    fz = pol.fused
    pad = _dev(~slot)
    for name, buf in (("flat", fz.flat.flat), ("adam_m", fz.adam_m), ("adam_v", fz.adam_v)) + ((("flat_t", fz.flat_t),) if mirror else ()):
        nz = torch.nonzero((buf != 0) & pad).reshape(-1)
        assert nz.numel() == 0, "%s: %s has %d non-zero padding slots, first at %d: %r" % (what, name, nz.numel(), int(nz[0]), buf[int(nz[0])].item())


def _assert_same_bits(pol, names, got, want, what):
    for name, a, b in zip(names, got, want):
        if not torch.equal(a, b):
            bad = torch.nonzero(a != b).reshape(-1)
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d of %d elements, first at %d = %s: %r != %r"
                                 % (what, name, bad.numel(), a.numel(), i, _where(pol, i), a[i].item(), b[i].item()))


def _grad_pass(pol, prefill=0.0):
    """The trainer's gradient pass (`_fused_grads`): publishes the Adam step number and the next minibatch index in the workspace
    slots, moves no counter and no state.  Returns (gradient, statistics)."""
    fz, rs = pol.fused, pol._row_sources
    k0, s0 = int(rs["k"]), int(fz.step_count)
    fz.grad.fill_(prefill)
    fz.stats.zero_()
    fz.step(rs, apply_adam=False, stats=fz.stats, bump_index=False)
    torch.cuda.synchronize()
    assert int(rs["k"]) == k0 and int(fz.step_count) == s0        # bump_index=False / apply_adam=False: neither counter moves
    return fz.grad.clone(), fz.stats.clone()


def _adam_call(pol, workspace, mirror, index):
    """copo_adam_step_f32 in one of its calling forms (FusedLearner.adam is workspace + mirror + index)."""
    from copo_amd import _capi
    fz, rs = pol.fused, pol._row_sources
    _capi.check(_capi.lib.copo_adam_step_f32(
        C.byref(fz.cfg), fz.flat.flat.data_ptr(), fz.adam_m.data_ptr(), fz.adam_v.data_ptr(), fz.grad.data_ptr(), fz.flat.numel,
        fz.step_count.data_ptr(), rs["k"].data_ptr() if index else None, fz.flat_t.data_ptr() if mirror else None,
        fz.workspace.data_ptr() if workspace else None, _capi.current_stream()))


# (name, workspace, theta_t, mb_index)
FORMS = [
    ("as the trainer calls it", True, True, True),       # step number / next index from the slots the gradient pass published
    ("workspace NULL", False, True, True),               # the kernel takes step[0] + 1, a trailing launch bumps both counters
    ("theta_t NULL, mb_index NULL", True, False, False),      # no tiled workgroups: the sweep takes every element; k untouched
    ("workspace NULL, mb_index NULL", False, True, False),    # the trailing launch bumps the step counter only
]
SENTINEL = 123.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adam_flat_kernel_on_a_known_gradient(case):
    """(a) adam_flat_kernel (copo_adam_step_f32 / FusedLearner.adam), the update every rank applies after the gradient all-reduce: its
    tiled workgroups (W1 / W2 blocks, Adam + mirror through an LDS tile) and its sweep workgroups (everything else) partition the flat
    buffer by hand.  Generator-filled state and gradient, every calling form of the C entry point, t = 1, 2, 10, 1000, 200 000."""
    pol, rs = _ready(case)
    fz = pol.fused
    slot = _slots(pol)
    x = _generated(slot, 1000 + IDS.index(case[0]))
    dx = {k: _dev(v) for k, v in x.items()}
    worst_hip, worst_np = np.zeros(3), np.zeros(3)
    for step0 in STEP0:
        t = step0 + 1
        refs = _references(fz, x, t)
        first = None
        for name, workspace, mirror, index in FORMS:
            what = "%s: adam_flat_kernel, %s" % (case[0], name)
            _load_state(pol, dx["theta"], dx["m"], dx["v"], step0, KB)
            if workspace:
                _grad_pass(pol)                  # (on the generator's parameters: only the slots it publishes matter here)
            fz.grad.copy_(dx["g"])
            fz.flat_t.fill_(SENTINEL)            # whatever the mirror held: the update must rewrite ALL of it, or none of it
            if workspace and mirror and index:
                fz.adam(rs)
            else:
                _adam_call(pol, workspace, mirror, index)
            got = _read(fz)
            e_hip, e_np = _assert_adam(pol, slot, got, refs, x, t, what)
            worst_hip, worst_np = np.maximum(worst_hip, e_hip), np.maximum(worst_np, e_np)
            _assert_padding_is_zero(pol, slot, what, mirror=mirror)
            if mirror:
                _assert_mirror_is_the_transposed_parameters(fz)
            else:
                assert bool((fz.flat_t == SENTINEL).all()), what
            assert int(fz.step_count) == step0 + 1, (what, int(fz.step_count), step0)
            assert int(rs["k"]) == (KB + 1 if index else KB), (what, int(rs["k"]))
            assert torch.equal(fz.grad, dx["g"]), what
            state = [t_.clone() for t_ in (fz.flat.flat, fz.adam_m, fz.adam_v)]
            if first is None:
                first = state
            else:       # the same arithmetic per element, only the partition into workgroups differs: the same bits
                _assert_same_bits(pol, ("flat", "adam_m", "adam_v"), state, first, "%s vs %s, t = %d" % (name, FORMS[0][0], t))
    print("%s adam_flat_kernel, worst over t: HIP e_m %.2f e_v %.2f e_theta %.2f | numpy float32 %.2f %.2f %.2f"
          % ((case[0],) + tuple(worst_hip) + tuple(worst_np)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_epilogue_applies_adam_to_the_gradient_it_computed(case):
    """(b) The production epilogue (wgrad_adam_kernel) on the gradient it computed.  G = `fused.grad` of step(apply_adam=False) from the
    same state: the code in front of `if (adam)` is the same for both values of apply_adam and adds no floats with atomics, so G is, bit
    for bit, the gradient the fused update applies.  The state after step(apply_adam=True) must be float64 Adam of G; the same G
    through FusedLearner.adam must land within the same limits of the same float64 result (no bit equality is asserted between the two
    kernels; whether they were bit-equal is printed)."""
    pol, rs = _ready(case)
    fz = pol.fused
    slot = _slots(pol)
    gen = _generated(slot, 2000 + IDS.index(case[0]))
    theta0 = fz.flat.flat.clone()
    assert bool((theta0[_dev(~slot)] == 0).all())
    m0, v0 = _dev(gen["m"]), _dev(gen["v"])
    G0 = None
    worst_hip, worst_np = np.zeros(3), np.zeros(3)
    for step0 in STEP0:
        t = step0 + 1
        _load_state(pol, theta0, m0, v0, step0, KB)
        G, stats_g = _grad_pass(pol, prefill=float("nan"))
        pad = _dev(~slot)
        assert bool(torch.isfinite(G[~pad]).all())      # the pass wrote every parameter's gradient
        G[pad] = 0.0
        fz.grad.copy_(G)
        _assert_same_bits(pol, ("flat", "adam_m", "adam_v"), (fz.flat.flat, fz.adam_m, fz.adam_v), (theta0, m0, v0), "gradient pass left the state")
        if G0 is None:
            G0 = G
            assert float(G.abs().max()) > 1e-4
        assert torch.equal(G, G0)                   # (the gradient does not depend on the step number)
        x = dict(theta=theta0.cpu().numpy(), m=gen["m"], v=gen["v"], g=G.cpu().numpy())
        refs = _references(fz, x, t)
        # the same G through adam_flat_kernel, as the trainer issues it behind this very gradient pass
        fz.adam(rs)
        got_flat = _read(fz)
        _assert_adam(pol, slot, got_flat, refs, x, t, "%s: adam_flat_kernel on the step's gradient" % case[0])
        _assert_mirror_is_the_transposed_parameters(fz)
        assert int(fz.step_count) == step0 + 1 and int(rs["k"]) == KB + 1
        # the fused update
        _load_state(pol, theta0, m0, v0, step0, KB)
        fz.stats.zero_()
        fz.step(rs, stats=fz.stats)
        got = _read(fz)
        what = "%s: wgrad_adam_kernel epilogue" % case[0]
        e_hip, e_np = _assert_adam(pol, slot, got, refs, x, t, what)
        worst_hip, worst_np = np.maximum(worst_hip, e_hip), np.maximum(worst_np, e_np)
        _assert_padding_is_zero(pol, slot, what)
        _assert_mirror_is_the_transposed_parameters(fz)
        assert int(fz.step_count) == step0 + 1 and int(rs["k"]) == KB + 1, (int(fz.step_count), int(rs["k"]))
        assert torch.equal(fz.stats, stats_g)       # the statistics of the two passes: the same code in front of the update
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, got_flat))
        print("%s t = %d: wgrad_adam_kernel and adam_flat_kernel bit-equal on the same gradient: %s" % (case[0], t, same))
    print("%s wgrad_adam_kernel, worst over t: HIP e_m %.2f e_v %.2f e_theta %.2f | numpy float32 %.2f %.2f %.2f"
          % ((case[0],) + tuple(worst_hip) + tuple(worst_np)))


DP_CASES = [CASES[1], CASES[0]]


@pytest.mark.parametrize("case", DP_CASES, ids=[c[0] for c in DP_CASES])
def test_shard_gradients_sum_to_the_global_minibatch_gradient(case):
    """(c) W = 3 ranks as three fused policies of identical weights on three different batches with B_all = [2 mb + 37, mb + 5, 1] valid
    rows: three minibatches, rank 2's minibatches 1 and 2 hold only zero-weight padding.  Every rank plans with the GLOBAL denominators;
    the rank-ordered fp32 sum of the shard gradients and statistics (what the all-reduce loop and the tile exchange both compute) is
    held to the float64 gradient of the global minibatch: the sum over the ranks of torch autograd in float64 on each rank's
    `_gather_minibatch()`, which carries `valid_denominator`.  Bounds of test_fused_gradients_against_a_float64_evaluation, relative to
    the largest float64 element of each tensor: e_hip <= 1e-5 and e_hip <= 3 e_t32 + W mb 2^-24 (a sum over up to W mb rows).  Then all
    three ranks apply `adam` to the sum: identical bits, float64 Adam of that sum."""
    _id, name, _fuse, odim, _over, _R, _B = case
    mb = _mb(case)
    R, B_all = 3 * mb, [2 * mb + 37, mb + 5, 1]
    refs = [_perturbed(case, fused=False)] + [_policy(case, fused=False) for _ in range(W - 1)]
    pols = [_policy(case) for _ in range(W)]
    for pol in refs[1:] + pols:
        _copy_weights(pol, refs[0])
        if pol.fused is not None:
            pol.fused.invalidate_mirror()
    assert all(p.fused is not None for p in pols) and all(p.fused is None for p in refs)
    for r in range(W):
        batch = _dense_batch(refs[0], R, odim, seed=r)
        g = torch.Generator(device="cuda").manual_seed(40 + r)
        idx = torch.randperm(R, device="cuda", generator=g)[:B_all[r]].sort().values.contiguous()
        for pol in (refs[r], pols[r]):
            pol.prepare_sgd(batch, R, mb)
            torch.manual_seed(50 + r)
            assert pol.plan_epoch(idx, B_all[r], B_all, mb) == 3
        for key in ("rows_all", "w_all", "denom_all"):
            assert torch.equal(refs[r]._row_sources[key], pols[r]._row_sources[key]), (r, key)
    # the denominators are the global ones: the sum of the ranks' minibatch sizes
    sizes = torch.stack([pols[r]._row_sources["w_all"][:3].sum(1) for r in range(W)])
    assert sizes.tolist() == [[float(B // 3 + (k < B % 3)) for k in range(3)] for B in B_all], sizes.tolist()
    assert sizes[2].tolist() == [1.0, 0.0, 0.0]
    for r in range(W):
        d = pols[r]._row_sources["denom_all"][:3]
        assert torch.equal(d, sizes.sum(0)), "rank %d: denominators %r, sum of the ranks' minibatch sizes %r" % (r, d.tolist(), sizes.sum(0).tolist())
    slot = _slots(pols[0])
    pad = _dev(~slot)
    off = pols[0].fused.flat.offset
    names = [(n, p) for n, p in pols[0].model.named_parameters() if p.dtype == torch.float32]
    # generator-filled moments and a preset step counter on every rank (the gradient passes leave them alone): the update below is t = 10
    gen = _generated(slot, 3000)
    theta0 = pols[0].fused.flat.flat.clone()
    m0, v0 = _dev(gen["m"]), _dev(gen["v"])
    for pol in pols:
        assert torch.equal(pol.fused.flat.flat, theta0)
        _load_state(pol, theta0, m0, v0, 9, 0)
    kbs = (0, 2)
    hip, hip_stats, t32 = {}, {}, {}
    for r in range(W):
        refs[r]._ensure_flat_grads()
    for kb in kbs:
        gsum, ssum, tsum = None, None, None
        for r in range(W):
            pols[r]._row_sources["k"].fill_(kb)
            g_r, s_r = _grad_pass(pols[r], prefill=float("nan"))
            assert bool(torch.isfinite(g_r[~pad]).all()) and bool(torch.isfinite(s_r).all()), (kb, r)
            g_r[pad] = 0.0
            if r == 2 and kb == 2:      # every row weight is 0: every term carries a factor w / denom = 0
                nz = torch.nonzero(g_r).reshape(-1)
                assert nz.numel() == 0, "rank 2, kb = 2: %d non-zero gradient elements, first %s" % (nz.numel(), _where(pols[r], int(nz[0])))
                assert not bool(s_r.any()), s_r.tolist()
            if r == 2 and kb == 0:      # one live row
                assert float(g_r.abs().max()) > 0.0 and float(s_r.abs().max()) > 0.0
            # rank order, fp32
            gsum = g_r.clone() if gsum is None else gsum.add_(g_r)
            ssum = s_r.clone() if ssum is None else ssum.add_(s_r)
            refs[r]._row_sources["k"].fill_(kb)
            refs[r]._row_sources["stats"].zero_()
            refs[r]._forward_backward()
            g32 = {n: p.grad.detach().clone() for n, p in refs[r].model.named_parameters() if p.dtype == torch.float32 and p.grad is not None}
            tsum = g32 if tsum is None else {n: tsum[n] + g32[n] for n in tsum}
        hip[kb], hip_stats[kb], t32[kb] = gsum, ssum, tsum
    # the same minibatches and loss in float64
    for r in range(W):
        kl32 = refs[r].kl_coeff
        refs[r].model.double()
        refs[r].kl_coeff = kl32.double()
    n_stats = len(refs[0].STAT_KEYS)
    assert n_stats == (8 if name == "copo" else 5)
    for kb in kbs:
        g64, s64 = None, torch.zeros(n_stats, dtype=torch.float64, device="cuda")
        for r in range(W):
            ref = refs[r]
            ref._row_sources["k"].fill_(kb)
            tb = ref._gather_minibatch()
            assert float(tb["valid_denominator"]) == float(sizes.sum(0)[kb])
            tb64 = SampleBatch({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tb.items()})
            for p in ref.model.parameters():
                p.grad = None
            ref.loss(ref.model, ref.dist_class, tb64).backward()
            gr = {n: p.grad.detach().clone() for n, p in ref.model.named_parameters() if n in t32[kb] and p.grad is not None}
            g64 = gr if g64 is None else {n: g64[n] + gr[n] for n in g64}
            s64 += torch.stack([ref.model.tower_stats[k].detach().double().reshape(()) for k in ref.STAT_KEYS])
        worst_hip, worst_t32 = 0.0, 0.0
        for n, p in names:
            if n not in g64:
                continue
            want = g64[n]
            scale = float(want.abs().max())
            if scale == 0.0:
                continue
            d_hip = (hip[kb][off[id(p)]:off[id(p)] + p.numel()].view_as(p).double() - want).abs()
            e_hip = float(d_hip.max()) / scale
            e_t32 = float((t32[kb][n].double() - want).abs().max()) / scale
            worst_hip, worst_t32 = max(worst_hip, e_hip), max(worst_t32, e_t32)
            print("%s kb=%d %s: e_hip %.2e, e_t32 %.2e" % (case[0], kb, n, e_hip, e_t32))
            at = "%s[%d]" % (n, int(d_hip.reshape(-1).argmax()))
            assert e_hip <= 1e-5, (kb, at, e_hip, e_t32)
            assert e_hip <= 3.0 * e_t32 + W * mb * 2.0 ** -24, (kb, at, e_hip, e_t32)
        assert worst_hip > 0.0 and worst_t32 > 0.0
        print("%s kb=%d: max error / largest gradient element per tensor: HIP %.2e, torch fp32 %.2e" % (case[0], kb, worst_hip, worst_t32))
        fs, st = hip_stats[kb].tolist(), s64.tolist()
        np.testing.assert_allclose(fs[:5], st[:5], rtol=2e-4, atol=1e-5, err_msg="kb = %d" % kb)
        if name == "copo":
            np.testing.assert_allclose(fs[5:8], st[5:8], rtol=2e-4, atol=1e-5, err_msg="kb = %d" % kb)
    # every rank applies Adam to the same sum, behind its own gradient pass of kb = 2 (whose slots say: step 10, next minibatch 3)
    gsum = hip[kbs[-1]]
    assert not bool(gsum[pad].any())
    for pol in pols:
        pol.fused.grad.copy_(gsum)
        pol.fused.flat_t.fill_(SENTINEL)
        pol.fused.adam(pol._row_sources)
    torch.cuda.synchronize()
    state_names = ("flat", "adam_m", "adam_v", "flat_t")
    states = [[getattr(p.fused, n) if n != "flat" else p.fused.flat.flat for n in state_names] for p in pols]
    for r in range(1, W):
        _assert_same_bits(pols[r], state_names, states[r], states[0], "rank %d vs rank 0 after adam on the summed gradient" % r)
    x = dict(theta=theta0.cpu().numpy(), m=gen["m"], v=gen["v"], g=gsum.cpu().numpy())
    refs_adam = _references(pols[0].fused, x, 10)
    for r, pol in enumerate(pols):
        what = "%s: rank %d, adam on the summed gradient" % (case[0], r)
        if r == 0:
            _assert_adam(pol, slot, _read(pol.fused), refs_adam, x, 10, what)
        _assert_padding_is_zero(pol, slot, what)
        _assert_mirror_is_the_transposed_parameters(pol.fused)
        assert int(pol.fused.step_count) == 10 and int(pol._row_sources["k"]) == kbs[-1] + 1, what
