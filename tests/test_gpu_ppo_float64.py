"""The fused PPO step against its float64 model (tests/ppo_numpy.py, pinned to the torch policies by
tests/test_ppo_cpu.py) at every kernel instantiation the PPO modes of the shipped library select (tests/ppo_cases.py): every
parameter gradient of every net on its own scale and all eight loss statistics, on the first and the last minibatch of a real
`plan_epoch`, with ~10 % of the rows outside the plan, rows crafted onto every branch of the surrogate and of both value-loss forms,
and the padded slots of the row table pointed at poisoned rows; then one real Adam step per shape.

Measured on an MI355X (`python -m pytest -s` prints every figure): DESIGN.md section 7, "The referee of the PPO step"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_cases as PC  # noqa: E402
import ppo_numpy as P  # noqa: E402
from copo_amd.engine import SampleBatch  # noqa: E402
from test_gpu_fused_dispatch import _assert_mirror_is_the_transposed_parameters  # noqa: E402
from test_gpu_fused_learner import _make  # noqa: E402

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The policies and batches of the cases live for this module only."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _setup(shape, conf):
    """One fused policy, poisoned batch and real plan per case, built once per module."""
    if (shape, conf) in _CACHE:
        return _CACHE[(shape, conf)]
    case = PC.SHAPE_CASES[shape]
    mb, R = case["mb"], case["R"]
    fz = _make(case["policy"], case["fuse"], case["odim"], fused=True, hiddens=(case["hidden"],) * 2, mb=mb, **case["over"], **PC.CONFIGS[conf])
    assert fz.fused is not None
    PC.perturb(fz.model)
    fz.fused.invalidate_mirror()
    PC.assert_selected(fz.fused.cfg, case)                  # the case covers the kernels it claims, for the cfg the kernels get
    batch, idx, _blocks, theta, cf = PC.build_inputs(fz, case)
    cols = PC.host_columns(batch, case)
    # The kernels multiply a row's terms by w / denom, as torch does (head_row_terms: `wgt * ...`); they do not skip a row of weight 0.
    # So the rows outside the plan are poisoned with huge FINITE values, not NaN: 0 x finite = 0, and anything else swamps the sums.
    bad_batch, bad = PC.poisoned(batch, idx)
    dev = SampleBatch({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in bad_batch.items()})
    fz.prepare_sgd(dev, R, mb)
    B = int(idx.numel())
    # `plan_epoch` with the permutation of `ppo_cases.host_plan`: the device tables must be the host's, so that the minibatches judged
    # here are the ones whose fp32 yardstick tests/test_ppo_cpu.py asserts
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(PC.PLAN_SEED)).cuda()
    n_mb = fz.plan_epoch(idx.cuda().contiguous(), B, [B] + list(case["others"]), mb, perm=perm)
    rs = fz._row_sources
    assert n_mb == max(1, -(-max([B] + list(case["others"])) // mb)) <= rs["rows_all"].shape[0]
    h_rows, h_w, h_denom = PC.host_plan(idx, case)
    assert np.array_equal(rs["w_all"][:n_mb].cpu().numpy(), h_w) and np.array_equal(rs["denom_all"][:n_mb].cpu().numpy(), h_denom)
    assert np.array_equal(rs["rows_all"][:n_mb].cpu().numpy()[h_w > 0], h_rows[h_w > 0])
    pad = rs["w_all"][:n_mb] == 0
    fill = bad.cuda()[torch.arange(int(pad.sum()), device="cuda") % bad.numel()]
    rows_k = rs["rows_all"][:n_mb]
    rows_k[pad] = fill                                      # every padded slot reads a poisoned row
    assert float(dev[SampleBatch.OBS][fill].abs().min()) > 0.99 * PC.POISON
    # the plans asserted above are those of 16-byte aligned sources with the mirror present
    for t in (rs["obs"], rs["pack"], fz.fused.flat.flat, fz.fused.flat_t, fz.fused.workspace, fz.fused.grad) + (() if rs["cc_obs"] is None else (rs["cc_obs"],)):
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    tabs = {k: rs[k][:n_mb].cpu().numpy() for k in ("rows_all", "w_all", "denom_all")}
    assert sorted(tabs["rows_all"][tabs["w_all"] > 0].tolist()) == idx.tolist()       # every valid row exactly once
    S = dict(case=case, shape=shape, conf_name=conf, fz=fz, theta=theta, conf=cf, cols=cols, n_mb=n_mb, tabs=tabs, dev=dev)
    _CACHE[(shape, conf)] = S
    return S


def _hip_grads(fz):
    off = fz.fused.flat.offset
    return [{name: fz.fused.grad[off[id(p)]:off[id(p)] + p.numel()].view_as(p).double().cpu().numpy() for name, p in net.items()}
            for net in PC.params_of(fz.model)]


@pytest.mark.parametrize("shape,conf", PC.CASES, ids=PC.CASE_IDS)
def test_gradients_and_statistics_against_float64(shape, conf):
    """`copo_ppo_fused_step_f32` without Adam on the first and on the last minibatch of the plan.  Per gradient tensor of every net,
    relative to the float64 tensor's largest element: e_hip <= 3 e_t32 + mb 2^-24 and e_hip <= 1e-5 (e_t32: torch fp32 autograd on the
    host, the same minibatch; a tensor whose exact gradient is identically 0 must be exactly 0).  Per statistic: |s_hip - s64| <=
    3 |s_t32 - s64| + mb 2^-24 x the mean absolute row term.  The padded slots point at poisoned rows."""
    S = _setup(shape, conf)
    fz, case, tabs = S["fz"], S["case"], S["tabs"]
    mb, rs = case["mb"], S["fz"]._row_sources
    worst, ratios, missed = [0.0, 0.0], np.zeros(8), []
    for k in sorted({0, S["n_mb"] - 1}):
        m = PC.minibatch(S["cols"], tabs["rows_all"][k], tabs["w_all"][k], tabs["denom_all"][k])
        assert 0 < m["w"].size < mb
        r64, r32 = P.step(S["theta"], m, S["conf"]), P.step(S["theta"], m, S["conf"], dtype=torch.float32)
        rs["k"].fill_(k)
        fz.fused.stats.zero_()
        fz.fused.step(rs, apply_adam=False, stats=fz.fused.stats, bump_index=False)
        torch.cuda.synchronize()
        got = _hip_grads(fz)
        stats = fz.fused.stats.double().cpu().numpy()
        assert all(np.all(np.isfinite(g[t])) for g in got for t in P.TENSORS) and np.all(np.isfinite(stats)), (shape, conf, k)
        e_hip, e_t32 = PC.tensor_errors(got, r64["grads"]), PC.tensor_errors(r32["grads"], r64["grads"])
        for key in e_hip:
            if not r64["grads"][key[0]][key[1]].any():
                assert not got[key[0]][key[1]].any(), (shape, conf, k, key)
                continue
            worst[0], worst[1] = max(worst[0], e_hip[key]), max(worst[1], e_t32[key])
            if not (e_hip[key] <= PC.GRAD_REL and e_t32[key] <= PC.GRAD_REL and e_hip[key] <= 3.0 * e_t32[key] + mb * 2.0 ** -24):
                missed.append(("minibatch %d net %d %s" % (k, key[0], key[1]), e_hip[key], e_t32[key]))
        for i, name in enumerate(P.STAT_NAMES):
            err, allowed = abs(stats[i] - r64["stats"][i]), 3.0 * abs(r32["stats"][i] - r64["stats"][i]) + mb * 2.0 ** -24 * r64["scales"][i]
            if not err <= allowed:
                missed.append(("minibatch %d statistic %s" % (k, name), stats[i], r64["stats"][i], err, allowed))
            if allowed > 0:
                ratios[i] = max(ratios[i], err / allowed)
        assert int(rs["k"]) == k and int(fz.fused.step_count) == 0
    rs["k"].zero_()
    print("[%s-%s] worst tensor: HIP %.2e  torch fp32 %.2e (of the tensor's largest element); statistics error / allowed %s" % (
        shape, conf, worst[0], worst[1], " ".join("%s %.2f" % (n, x) for n, x in zip(P.STAT_NAMES, ratios))))
    assert not missed, (shape, conf, missed)


@pytest.mark.parametrize("shape", list(PC.SHAPE_CASES))
def test_one_adam_step_leaves_a_finite_state_and_a_true_mirror(shape):
    """One real step (`apply_adam=True`) on the poisoned plan: parameters, moments and the transposed mirror stay finite, the mirror is
    the transposition of the parameters bit for bit, the step and minibatch counters advanced.  (The arithmetic of the update belongs
    to tests/test_gpu_adam_kernels.py.)"""
    S = _setup(shape, "default")
    fz, rs = S["fz"].fused, S["fz"]._row_sources
    _CACHE.pop((shape, "default"))                          # the weights move: nobody reuses this case
    before = fz.flat.flat.clone()
    rs["k"].zero_()
    fz.stats.zero_()
    fz.step(rs, stats=fz.stats)
    torch.cuda.synchronize()
    assert int(fz.step_count) == 1 and int(rs["k"]) == 1
    for t in (fz.flat.flat, fz.adam_m, fz.adam_v, fz.flat_t, fz.stats):
        assert bool(torch.isfinite(t).all())
    moved = (fz.flat.flat - before).abs()
    lr = float(S["fz"].config["lr"])
    assert 0.0 < float(moved.max()) <= 1.01 * lr             # Adam's first step: lr g / (|g| + eps)
    _assert_mirror_is_the_transposed_parameters(fz)
