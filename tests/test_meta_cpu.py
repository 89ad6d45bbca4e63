"""CPU: the float64 / 40-digit model of the LCF meta step (tests/meta_numpy.py) against the torch statement of the same step
(CoPOPolicy._meta_pieces / _meta_finish) evaluated in float64, the launch plans of the referee's shape cases, and the conditions the
referee puts on its inputs (crafted ratios clear of the clip thresholds, decidable dot products).  No device is touched."""
import numpy as np
import pytest
import torch

import meta_cases as MC
import meta_numpy as M
from copo_amd.engine import Box, SampleBatch
from copo_amd.fused import FlatParams
from test_learner_plan_cpu import make_cfg


def _cpu_policy(hidden, odim, mb):
    from copo_amd.torch_copo import algo_copo as A
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv, get_lcf_env, get_rllib_compatible_env
    cfg = A.CoPOConfig()
    cfg.update_from_dict(dict(env=get_rllib_compatible_env(get_lcf_env(MultiAgentIntersectionEnv)), device="cpu", use_hip_graphs=False,
                              use_fused_learner=False, seed=3, sgd_minibatch_size=mb, model={"fcnet_hiddens": [hidden, hidden]}))
    cfg.fuse_mode = "none"
    cfg.validate()
    return A.CoPOPolicy(Box(-1, 1, (odim,)), Box(-1, 1, (2,)), cfg)


def _cpu_batch(R, odim, seed):
    """The columns of `_dense_batch` (tests/test_gpu_fused_learner.py) that the meta step reads, same distributions, host generator."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    b = {"obs": torch.rand(R, odim, generator=g) * 2 - 1, "actions": rn(R, 2) * 0.8}
    di = torch.cat([rn(R, 2) * 0.3, rn(R, 2) * 0.2 - 0.2], 1)
    z = (b["actions"] - di[:, :2]) / torch.exp(di[:, 2:])
    b["action_logp"] = (-0.5 * z * z - di[:, 2:] - 0.5 * np.log(2 * np.pi)).sum(-1)
    b["advantages"], b["nei_advantage"], b["global_advantages"] = rn(R) * 2, rn(R) * 2, rn(R)
    return b


@pytest.fixture(scope="module")
def small():
    """The 64-hidden shape case on the host: policy in float64, thetas, batch with the row edges, the plan's first minibatches."""
    case = MC.SHAPE_CASES[MC.SMALL]
    H, odim, mb, R = (case[k] for k in ("hidden", "odim", "mb", "R"))
    pol = _cpu_policy(H, odim, mb)
    with torch.no_grad():
        for p in list(pol.model.parameters()) + list(pol.target_model.parameters()):
            if p.dtype == torch.float32:
                p.add_(torch.randn_like(p) * 0.05)
    tn, to = MC.thetas(pol, FlatParams(pol.model, "cpu"), FlatParams(pol.target_model, "cpu"))
    assert tn["n"] == to["n"] == case["hidden"] * (odim + 1) + H * (H + 1) + 4 * (H + 1)
    clip = float(pol.config["clip_param"])
    batch = _cpu_batch(R, odim, seed=5)
    idx = MC.valid_rows(R, seed=5)
    logp64 = M.log_prob(tn["layers"], batch["obs"].double(), batch["actions"].double()).numpy()
    blocks = MC.add_row_edges(batch, idx, logp64, clip, seed=5)
    cols = MC.host_columns(batch)
    # the plan of one pass: near-equal minibatches of the shuffled valid rows, padded with zero-weight rows to mb
    perm = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(7))].numpy()
    n_mb = -(-perm.size // mb)
    mbs, g = [], torch.Generator().manual_seed(8)
    for k, part in enumerate(np.array_split(perm, n_mb)):
        rows, w = np.zeros(mb, np.int64), np.zeros(mb)
        rows[:part.size], w[:part.size] = part, 1.0
        mbs.append(MC.minibatch(cols, rows, w, part.size, torch.randn(mb, generator=g, dtype=torch.float64).numpy()))
    pol.model.double()
    pol.target_model.double()
    return dict(case=case, pol=pol, tn=tn, to=to, clip=clip, cols=cols, idx=idx.numpy(), blocks=blocks, mbs=mbs)


def _train_batch(mbk):
    t = lambda x: torch.as_tensor(x, dtype=torch.float64)  # noqa: E731
    return SampleBatch({"obs": t(mbk["obs"]), "actions": t(mbk["act"]), "action_logp": t(mbk["old_logp"]),
                        "global_advantages": t(mbk["glob_adv"]), "advantages": t(mbk["ego"]), "nei_advantage": t(mbk["nei"]),
                        SampleBatch.VALID: t(mbk["w"]), "valid_denominator": t(mbk["denom"])})


@pytest.mark.parametrize("name", list(MC.SHAPE_CASES))
def test_shape_cases_select_the_kernels_they_claim(name):
    case = MC.SHAPE_CASES[name]
    MC.assert_selected(make_cfg(mb=case["mb"], hidden=case["hidden"], in_pol=case["odim"], in_val=(case["odim"],) * 3), case)
    # what only the meta modes reach: the non-mirror row passes, and the scalar chain / the bias-column tiles under META heads
    pair = case["kernels"]["pair"][0]
    assert pair.startswith("rowpass_kernel<") and pair.endswith(", false>") or pair.startswith("gemm_kernel<FwdOpT<1>")


def test_torch_clamp_passes_the_gradient_on_the_bound():
    """What the kernels' `>=` / `<=` are held to: on the bound itself torch.clamp's autograd passes the gradient, outside it is 0."""
    for x, lo, hi, want in ((2.0, -20.0, 2.0, 1.0), (-20.0, -20.0, 2.0, 1.0), (2.5, -20.0, 2.0, 0.0), (-21.0, -20.0, 2.0, 0.0),
                            (M.LIM, -M.LIM, M.LIM, 1.0), (-M.LIM, -M.LIM, M.LIM, 1.0)):
        t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        torch.clamp(t, lo, hi).backward()
        assert float(t.grad) == want, (x, float(t.grad))
    for i, (p0, p1) in enumerate(MC.LCF_CASES):
        d0, d1, _s, _a = M.lcf_terms((p0, p1), (0.0, 1.0), [1.0, -2.0], [0.5, 3.0], [0.3, -1.1], [1.0, 1.0], 2.0)
        assert (d0 == 0) == (i in MC.ZERO_D0) and (d1 == 0) == (i in MC.ZERO_D1), (i, d0, d1)


def test_policy_gradients_match_torch_float64(small):
    """g_new / g_old of the model == CoPOPolicy._meta_pieces in float64, every minibatch of the pass: 1e-12 of the largest element."""
    pol = small["pol"]
    for mbk in small["mbs"]:
        flat, stats = pol._meta_pieces(_train_batch(mbk), torch.as_tensor(mbk["eps"]))
        n = small["tn"]["n"]
        t = M.policy_terms(small["tn"], small["to"], mbk["obs"], mbk["act"], mbk["old_logp"], mbk["glob_adv"], mbk["w"], mbk["denom"], small["clip"])
        # hidden 64: no tensor is padded, the fold layout is the concatenation of the policy parameters
        for got, want in ((t["g_new"], flat[:n].numpy()), (t["g_old"], flat[n:2 * n].numpy())):
            assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        np.testing.assert_allclose([t["new_loss"], t["old_loss"], t["global_adv"]],
                                   [float(stats[k]) for k in ("new_policy_ego_loss", "old_policy_logp_loss", "global_adv")], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("raw", MC.RAW_MEAN_STD)
@pytest.mark.parametrize("ci", range(len(MC.LCF_CASES)))
def test_lcf_terms_and_adam_match_torch_float64(small, ci, raw):
    """The 40-digit LCF terms and three chained Adam steps == _meta_pieces / _meta_finish in float64: tail terms to 1e-13 relative, the
    clamp-branch derivatives exactly 0 on both sides, parameters after the steps to 1e-13."""
    pol, mbs = small["pol"], small["mbs"]
    pol.model.lcf_parameters.data.copy_(torch.tensor(MC.LCF_CASES[ci], dtype=torch.float64))
    pol._lcf_optimizer = torch.optim.Adam([pol.model.lcf_parameters], lr=pol.config["lcf_lr"])
    pol._raw_ms.copy_(torch.tensor(raw, dtype=torch.float64))
    n = small["tn"]["n"]
    p, adam, lr = list(MC.LCF_CASES[ci]), [0.0] * 5, float(pol.config["lcf_lr"])
    for step, mbk in enumerate(mbs):
        flat, _ = pol._meta_pieces(_train_batch(mbk), torch.as_tensor(mbk["eps"]))
        want = flat[2 * n:2 * n + 3].numpy()
        d0, d1, S, _mean_a = M.lcf_terms(p, raw, mbk["ego"], mbk["nei"], mbk["eps"], mbk["w"], mbk["denom"])
        got = np.array([float(d0), float(d1), float(S)])
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want)), (step, got, want)
        if step == 0:
            assert (want[0] == 0.0) == (ci in MC.ZERO_D0) == (got[0] == 0.0) and (want[1] == 0.0) == (ci in MC.ZERO_D1) == (got[1] == 0.0)
        gv = float((flat[:n] * flat[n:2 * n]).sum())
        pol._meta_finish(flat, {})
        p, adam = M.lcf_adam(p, adam, [gv * d0, gv * d1], lr)
        np.testing.assert_allclose([float(x) for x in p], pol.model.lcf_parameters.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert float(adam[4]) == len(mbs)
    st = pol._lcf_optimizer.state[pol.model.lcf_parameters]
    np.testing.assert_allclose([float(x) for x in adam[:4]], np.concatenate([st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()]), rtol=1e-12, atol=1e-300)
    # the float64 restatement of the same formulas stays within fp64 rounding of the 40-digit values (what a bound on an fp64 KERNEL may
    # be derived from): a sum of mb terms, each carrying a few roundings
    f64 = M.lcf_terms_float64(MC.LCF_CASES[ci], raw, mbs[0]["ego"], mbs[0]["nei"], mbs[0]["eps"], mbs[0]["w"], mbs[0]["denom"])
    mpv = M.lcf_terms(MC.LCF_CASES[ci], raw, mbs[0]["ego"], mbs[0]["nei"], mbs[0]["eps"], mbs[0]["w"], mbs[0]["denom"])
    for a, b in zip(f64, mpv):
        assert abs(a - float(b)) <= 1e-12 * abs(float(b)) + 1e-15, (a, float(b))          # the bound the GPU test puts on the kernels


def test_row_edges_stay_clear_of_the_clip_thresholds(small):
    """The crafted rows land where they were sent: no valid row within CLIP_MARGIN of a threshold, every block beyond its threshold with
    its sign of advantage; the blocks that min(A r, A clip(r)) clips and the block of zero advantage contribute exactly no gradient to
    g_new, the two blocks whose clamp is out of range on the side min does not take contribute theirs."""
    tn, to, cols, clip = small["tn"], small["to"], small["cols"], small["clip"]
    idx = small["idx"]
    ones = np.ones(idx.size)
    t = M.policy_terms(tn, to, cols["obs"][idx], cols["actions"][idx], cols["action_logp"][idx], cols["global_advantages"][idx], ones, idx.size, clip, grads=False)
    assert MC.ratio_margin(t["ratio"], clip) >= MC.CLIP_MARGIN
    zero, neg, pos, pos_hi, neg_lo = (b.numpy() for b in small["blocks"])
    ratio = dict(zip(idx.tolist(), t["ratio"]))
    assert all(cols["global_advantages"][r] == 0.0 for r in zero) and len(zero) >= 4
    assert all(ratio[r] > 1 + clip and cols["global_advantages"][r] < 0 for r in neg)
    assert all(ratio[r] < 1 - clip and cols["global_advantages"][r] > 0 for r in pos)
    assert all(ratio[r] > 1 + clip and cols["global_advantages"][r] > 0 for r in pos_hi)
    assert all(ratio[r] < 1 - clip and cols["global_advantages"][r] < 0 for r in neg_lo)
    for blk in (zero, neg, pos, pos_hi, neg_lo):
        g_new, g_old = M.policy_grads(tn, to, cols["obs"][blk], cols["actions"][blk], cols["action_logp"][blk], cols["global_advantages"][blk],
                                      np.ones(blk.size), blk.size, clip)
        assert bool(g_new.any()) == (blk is neg or blk is pos) and g_old.any()
    # and rows of every branch are in every minibatch's neighbourhood: unclipped rows carry the gradient
    assert sum(1 for r in idx if 1 - clip < ratio[r] < 1 + clip) > idx.size // 4


def test_dot_products_of_the_case_are_decidable(small):
    terms = [M.policy_terms(small["tn"], small["to"], m["obs"], m["act"], m["old_logp"], m["glob_adv"], m["w"], m["denom"], small["clip"])
             for m in small["mbs"]]
    share, bounds = MC.decidable_share(terms, (small["tn"], small["to"]))
    assert share >= MC.DECIDABLE_SHARE, (share, bounds, [float(np.dot(t["g_new"], t["g_old"])) for t in terms])
