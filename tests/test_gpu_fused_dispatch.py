"""The fused SGD step as the trainer drives it (`PPOPolicyBase.run_sgd_fused`): rows gathered into minibatch order (`rows` = NULL in
the C ABI), every epoch planned up front, captured chains of 16 steps and single-step graphs, the one-rank data-parallel entry point.

tests/test_gpu_fused_learner.py pins the EAGER step that reads its rows THROUGH THE TABLE to torch and to float64.  The launcher picks
the same kernel instantiation whether a row table is given or not, and no kernel of the step adds floating-point numbers with atomics
(the one atomicAdd is an integer completion counter), so every other way of issuing the same steps must give the SAME BITS: the
comparisons below are `torch.equal`, a derived expectation and not a measured tolerance.  Any mistake in the addressing of the
gathered layout, in the hand-over of the device-side minibatch counter or in the order of the planned epochs shows up as a mismatch
(DESIGN.md section 7)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from copo_amd.engine import SampleBatch  # noqa: E402
from test_gpu_fused_learner import _copy_weights, _dense_batch, _make  # noqa: E402

EPOCHS, CALLS = 7, 4      # 7 epochs x 3 minibatches = 21 steps per call: one 16-step chain + 5 single steps; the chain graph is
#                           captured by the third call and REPLAYED by the fourth

# (id, policy, fuse mode, observation width, _make overrides, rows R, valid rows B): the smallest shapes at which each kernel
# instantiation is still selected; B gives 3 minibatches per epoch that all end in zero-weight padding
CASES = [
    # production: 8-row-tile row pass, buffer-load weight gradient, 4 nets; 446 / 446 / 445 rows
    ("copo_o92", "copo", "none", 92, {}, 1500, 1337),
    # input width not a multiple of 4 (scalar input gather), 2 nets
    ("ippo_o91", "ippo", "none", 91, {}, 1500, 1337),
    # general weight-gradient instantiation (mb != 512), ragged 16-row tiles, critic input 184 wide; 179 / 178 / 178 rows
    ("ccppo_mf_h128_mb200", "ccppo", "mf", 91, dict(hiddens=(128, 128), mb=200), 600, 535),
    # no row pass: the tile-GEMM forward / head / backward-input kernels in front of the general weight-gradient kernel (the shipped
    # library ends every PPO step in wgrad_adam_kernel: reduce_adam_kernel and the mirror refresh launch serve the meta modes only);
    # 64 / 63 / 63 rows
    ("ccppo_mf_h48_mb72", "ccppo", "mf", 91, dict(hiddens=(48, 48), mb=72), 220, 190),
    # bfloat16 operands: buffer-load instantiation whose layer 1 rounds the gathered inputs
    ("ccppo_mf_bf16_o156", "ccppo", "mf", 156, dict(policy_dtype="bfloat16"), 1500, 1337),
]
STATE = ("flat", "adam_m", "adam_v", "step_count", "flat_t")
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "mean_nei_vf_loss", "mean_global_vf_loss",
             "normalized_advantages")          # positions 0..7 of FusedLearner.stats


def _policy(case, fused=True):
    _id, name, fuse, odim, over, _R, _B = case
    return _make(name, fuse, odim, fused=fused, num_sgd_iter=EPOCHS, **over)


def _setup(case, fused_first=True):
    """(first policy with perturbed weights, batch, sorted valid row indices, mb)."""
    _id, _name, _fuse, odim, over, R, B = case
    src = _policy(case, fused=fused_first)
    with torch.no_grad():                       # move off the near-zero head init
        for p in src.model.parameters():
            if p.dtype == torch.float32:
                p.add_(torch.randn_like(p) * 0.05)
    if src.fused is not None:
        src.fused.invalidate_mirror()
    batch = _dense_batch(src, R, odim)
    g = torch.Generator(device="cuda").manual_seed(17)
    idx = torch.randperm(R, device="cuda", generator=g)[:B].sort().values.contiguous()
    mb = over.get("mb", 512)
    assert -(-B // mb) == 3 and B % mb != 0 and 3 * EPOCHS % 16 != 0 and 3 * EPOCHS > 16
    return src, batch, idx, mb


def _clone_of(case, src, batch, mb):
    pol = _policy(case)
    assert pol.fused is not None
    _copy_weights(pol, src)
    pol.fused.invalidate_mirror()
    pol.prepare_sgd(batch, case[5], mb)
    return pol


def _state(fz):
    return [t.clone() for t in (fz.flat.flat, fz.adam_m, fz.adam_v, fz.step_count, fz.flat_t)]


def _where(pol, i):
    """Name of the parameter that element i of the flat buffers belongs to: net and layer of a mismatch."""
    off = pol.fused.flat.offset
    for n, p in pol.model.named_parameters():
        if id(p) in off and off[id(p)] <= i < off[id(p)] + p.numel():
            return "%s[%d]" % (n, i - off[id(p)])
    return "padding[%d]" % i


def _assert_same_state(pol, got, want, what):
    for name, a, b in zip(STATE, got, want):
        if not torch.equal(a, b):
            bad = torch.nonzero(a != b).reshape(-1)
            first = int(bad[0])
            where = _where(pol, first) if a.numel() > 1 else ""
            raise AssertionError("%s: %s differs in %d of %d elements, first at %d %s: %r != %r"
                                 % (what, name, bad.numel(), a.numel(), first, where, a[first].item(), b[first].item()))


def _reference_call(pol, idx, B, mb, seed):
    """Variant A, the path that test_gpu_fused_learner.py pins to torch: eager steps that read their rows through the table, one
    plan per epoch, the minibatch counter bumped by every step."""
    fz = pol.fused
    torch.manual_seed(seed)
    fz.stats.zero_()
    steps = 0
    for _ in range(EPOCHS):
        n_mb = pol.plan_epoch(idx, B, [B], mb)
        for _k in range(n_mb):
            fz.step(pol._row_sources, stats=fz.stats)
        steps += n_mb
    assert int(pol._row_sources["k"]) == n_mb
    return steps, (fz.stats / steps).tolist()


def _assert_mirror_is_the_transposed_parameters(fz):
    """`flat_t` (written by the Adam epilogue, read by the next row pass) against a fresh transposition of the parameters."""
    from copo_amd import _capi
    fresh = torch.zeros_like(fz.flat_t)
    _capi.check(_capi.lib.copo_transpose_weights_f32(C.byref(fz.cfg), fz.flat.flat.data_ptr(), fresh.data_ptr(), _capi.current_stream()))
    torch.cuda.synchronize()
    c, H = fz.cfg, int(fz.cfg.hidden)
    for g, L in enumerate([c.pol] + [c.val[v] for v in range(int(c.n_value_heads))]):
        for name, o, n in (("w1", int(L.w1), H * int(L.in_dim)), ("w2", int(L.w2), H * H)):
            assert torch.equal(fresh[o:o + n], fz.flat_t[o:o + n]), ("net %d %s" % (g, name), int((fresh[o:o + n] != fz.flat_t[o:o + n]).sum()))
    # outside those ranges the mirror is a plain copy (biases, head layers, alignment padding): the kernels write those too, and
    # copo_transpose_weights_f32 copies them, so the whole buffer must agree
    assert torch.equal(fresh, fz.flat_t)


def _configure(pol, variant):
    if variant == "B":          # eager steps on rows gathered once per epoch
        pol.use_graphs = False
    elif variant == "C":        # production: graphs, gather, all epochs planned up front
        pol.use_graphs = True
    elif variant == "D":        # graphs on the row tables, one plan per epoch
        pol.use_graphs = True
        pol.config["plan_all_epochs"] = False
        pol.config["gather_epoch_rows"] = False
    elif variant == "E":        # as C through copo_ppo_fused_step_dp_f32 with a world of one (step_dp(rs, None))
        pol.use_graphs = True
        pol._dp_mode = "tile"
        pol._tile = None


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_sgd_path_gives_the_bits_of_the_eager_table_path(case):
    B = case[6]
    ref, batch, idx, mb = _setup(case)
    ref.prepare_sgd(batch, case[5], mb)
    lr = float(ref.config["lr"])
    start = ref.fused.flat.flat.clone()
    # identical policies, one per variant; "A" repeats the reference: the premise that the path itself is deterministic
    pols = {variant: _clone_of(case, ref, batch, mb) for variant in "ABCDE"}
    want_state, want_stats = [], []
    for call in range(CALLS):
        steps, st = _reference_call(ref, idx, B, mb, 100 + call)
        assert steps == 3 * EPOCHS and int(ref.fused.step_count) == (call + 1) * steps
        assert all(np.isfinite(st)), st
        want_state.append(_state(ref.fused))
        want_stats.append(st)
        if call == 0:
            moved = float((ref.fused.flat.flat - start).abs().max())
            assert moved > 10 * lr, moved
    _assert_mirror_is_the_transposed_parameters(ref.fused)
    for variant, pol in pols.items():
        assert pol.fused.cfg.operand_dtype == ref.fused.cfg.operand_dtype and torch.equal(pol.fused.flat.flat, start)
        _configure(pol, variant)
        for call in range(CALLS):
            what = "variant %s, call %d" % (variant, call)
            if variant == "A":
                steps, st = _reference_call(pol, idx, B, mb, 100 + call)
            else:
                torch.manual_seed(100 + call)
                out = pol.run_sgd(idx, B, [B], mb, EPOCHS)
                steps, st = out["num_sgd_steps"], [out[k] for k in STAT_KEYS]
                assert int(pol._row_sources["k"]) == (3 * EPOCHS if variant in "CE" else 3), what
            torch.cuda.synchronize()
            assert steps == 3 * EPOCHS, what
            _assert_same_state(pol, _state(pol.fused), want_state[call], what)
            assert st == want_stats[call], (what, st, want_stats[call])
        if variant in "CE":     # the test went where it claims: the 16-step chain is a replayed graph, the kernels got rows = NULL
            assert pol._sgd_chain.graph is not None and pol._sgd.graph is not None and pol._rs_step["rows_all"] is None
        if variant == "B":
            assert pol._sgd_chain.graph is None and pol._rs_step["rows_all"] is None
        if variant == "D":
            assert pol._sgd.graph is not None and pol._rs_step is None
        if variant == "C":
            _assert_mirror_is_the_transposed_parameters(pol.fused)


@pytest.mark.parametrize("case", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_gathered_gradients_of_later_minibatches_against_float64(case):
    """`test_fused_gradients_against_a_float64_evaluation` for minibatches kb = 1 and kb = n_mb - 1 of rows in minibatch order
    (`gather_epoch`, rows = NULL): the layer-1 weight gradient then finds its inputs at kb * mb * K.  Same bounds as there (DESIGN.md
    section 7), relative to the largest float64 gradient element of each tensor: e_hip <= 1e-5 and e_hip <= 3 e_t32 + mb 2^-24; the
    gathered gradient equals the table gradient of the same minibatch bit for bit.  Measured, worst tensor over both minibatches
    (e_hip / e_t32): copo 2.1e-6 / 1.6e-6, ippo 7.7e-7 / 1.6e-6, ccppo mean-field hidden 128 mb 200 7.7e-7 / 8.0e-7."""
    B = case[6]
    ref, batch, idx, mb = _setup(case, fused_first=False)
    assert ref.fused is None
    fz = _policy(case)
    _copy_weights(fz, ref)
    fz.fused.invalidate_mirror()
    for pol in (ref, fz):
        pol.prepare_sgd(batch, case[5], mb)
        torch.manual_seed(5)
        n_mb = pol.plan_epoch(idx, B, [B], mb)
    assert n_mb == 3 and torch.equal(ref._row_sources["rows_all"], fz._row_sources["rows_all"])
    f = fz.fused
    rs_g = f.gather_epoch(fz._row_sources, n_mb)
    assert rs_g["rows_all"] is None and rs_g["k"] is fz._row_sources["k"]
    off = f.flat.offset
    names = [(n, p) for n, p in fz.model.named_parameters() if p.dtype == torch.float32]
    ref._ensure_flat_grads()
    kbs = sorted({1, n_mb - 1})
    ghip, g32 = {}, {}
    for kb in kbs:
        for pol in (ref, fz):
            pol._row_sources["k"].fill_(kb)
        grads = []
        for rs in (rs_g, fz._row_sources):
            f.stats.zero_()
            f.grad.zero_()
            f.step(rs, apply_adam=False, stats=f.stats, bump_index=False)
            assert int(fz._row_sources["k"]) == kb and int(f.step_count) == 0      # bump_index=False / apply_adam=False: neither counter moves
            grads.append((f.grad.clone(), f.stats.clone()))
        assert torch.equal(grads[0][0], grads[1][0]), ("gathered vs table gradient, kb = %d" % kb, int((grads[0][0] != grads[1][0]).sum()))
        assert torch.equal(grads[0][1], grads[1][1]), ("gathered vs table statistics, kb = %d" % kb)
        ghip[kb] = {n: grads[0][0][off[id(p)]:off[id(p)] + p.numel()].view_as(p).double().clone() for n, p in names}
        ref._row_sources["stats"].zero_()
        ref._forward_backward()
        g32[kb] = {n: p.grad.detach().double().clone() for n, p in ref.model.named_parameters() if p.dtype == torch.float32 and p.grad is not None}
        st, fs = ref._row_sources["stats"].tolist(), grads[0][1].tolist()
        np.testing.assert_allclose(fs[:5], st[:5], rtol=2e-4, atol=1e-5)
    # the same minibatches and loss in float64
    kl32 = ref.kl_coeff
    ref.model.double()
    ref.kl_coeff = kl32.double()
    for kb in kbs:
        ref._row_sources["k"].fill_(kb)
        tb = ref._gather_minibatch()
        tb64 = SampleBatch({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tb.items()})
        for p in ref.model.parameters():
            p.grad = None
        ref.loss(ref.model, ref.dist_class, tb64).backward()
        worst_hip, worst_t32 = 0.0, 0.0
        for n, p in ref.model.named_parameters():
            if n not in g32[kb] or p.grad is None:
                continue
            g64 = p.grad.detach()
            scale = float(g64.abs().max())
            if scale == 0.0:
                continue
            e_hip = float((ghip[kb][n] - g64).abs().max()) / scale
            e_t32 = float((g32[kb][n] - g64).abs().max()) / scale
            worst_hip, worst_t32 = max(worst_hip, e_hip), max(worst_t32, e_t32)
            print("%s kb=%d %s: e_hip %.2e, e_t32 %.2e" % (case[0], kb, n, e_hip, e_t32))
            assert e_hip <= 1e-5, (kb, n, e_hip, e_t32)
            assert e_hip <= 3.0 * e_t32 + mb * 2.0 ** -24, (kb, n, e_hip, e_t32)
        assert worst_hip > 0.0 and worst_t32 > 0.0
        print("%s kb=%d: max error / largest gradient element per tensor: HIP %.2e, torch fp32 %.2e" % (case[0], kb, worst_hip, worst_t32))
