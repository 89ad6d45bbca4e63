"""Shapes, configurations and row edges of the PPO-step referee (tests/test_ppo_cpu.py, tests/test_gpu_ppo_float64.py).

Every shape case is the smallest one that still selects its kernels; the kernels a case launches are written down in the case and
asserted against the library's launch plan, so a case cannot silently stop covering what its comment claims."""
import numpy as np
import torch

import ppo_numpy as P
from copo_amd.engine import Postprocessing, SampleBatch, TorchDiagGaussian
from test_learner_plan_cpu import ALL, PPO_GRADS, PPO_STEP, make_cfg, query

RP8 = "rowpass8_kernel<4>"
RP_HO = "rowpass_kernel<2, 8, true, false, true>"
RP_TW = {64: "rowpass_kernel<1, 4, true>", 128: "rowpass_kernel<2, 4, true>", 256: "rowpass_kernel<2, 8, true>", 512: "rowpass_kernel<4, 8, true>"}
WG, WG_FAST = "wgrad_adam_kernel<1>", "wgrad_adam_kernel<1, false, true>"
GEMM_VEC = ["gemm_kernel<FwdOpT<1>, true>", "gemm_kernel<FwdOpT<2>, true>", "head_kernel", "gemm_kernel<BxOp, true>"]
GEMM_SCALAR = ["gemm_kernel<FwdOpT<1>, false>", "gemm_kernel<FwdOpT<2>, false>", "head_kernel", "gemm_kernel<BxOp, false>"]
# every fp32 entry of the kernel table that plan_step can choose in the PPO modes of the shipped library (DESIGN.md section 7 lists what
# stays out of reach); test_ppo_cpu.py checks the union of the cases' plans against this list
REACHABLE = {RP8, RP_HO, WG, WG_FAST, *RP_TW.values(), *GEMM_VEC, *GEMM_SCALAR}


def _case(policy, fuse, odim, hidden, mb, R, kernels, others=(), over=None, seed=5):
    """policy / fuse / odim: what `_make` takes; R rows of which ~10 % stay out of the valid list; `others`: valid counts of further
    (imagined) ranks, which enter the number of minibatches and the denominators as `plan_epoch` computes them; `over`: config keys."""
    return dict(policy=policy, fuse=fuse, odim=odim, hidden=hidden, mb=mb, R=R, kernels=kernels, others=tuple(others), over=dict(over or {}), seed=seed)


SHAPE_CASES = {
    # the production shape: four nets on 8-row tiles (32 x 4 = 128 workgroups), the buffer-load weight-gradient kernel of mb = 512
    "prod": _case("copo", "none", 92, 256, 512, 1200, [RP8, WG_FAST]),
    # the same kernels with a 260-wide layer 1 (the 8-row kernel pads it to 320 columns)
    "k260": _case("copo", "none", 260, 256, 512, 640, [RP8, WG_FAST]),
    # hidden 256 beyond head_tiles x G = 160 (41 x 4): 16-row tiles with the hand-over of layer 1; 648 is no multiple of 16 or 64
    "ho_mb648": _case("copo", "none", 92, 256, 648, 800, [RP_HO, WG]),
    # ... without the hand-over for the 260-wide input.  (Seed: with the seed of the other cases the 360 terms of the neighbour head's
    # one-element b3 gradient cancel to 1e-3 of their size and torch fp32 on the host misses its own 1e-5 there, 2.6e-5: the inputs
    # change, not the bound)
    "tw_k260_mb648": _case("copo", "none", 260, 256, 648, 800, [RP_TW[256], WG], seed=7),
    # a 91-wide observation: no vector rows, the scalar input gather of the row pass through the mirror; G = 2
    "ippo_k91": _case("ippo", "none", 91, 256, 512, 640, [RP8, WG_FAST]),
    # CCPPO mean-field, critic input 184 wide next to the 91-wide policy input; mb = 200 is no multiple of 8 x 16 or 64
    "ccppo_mf_mb200": _case("ccppo", "mf", 91, 256, 200, 450, [RP8, WG]),
    # CCPPO concat with three neighbours of a 77-wide observation: critic input 314 wide; RP_TW_2_4; mb = 72
    "ccppo_concat_h128": _case("ccppo", "concat", 77, 128, 72, 200, [RP_TW[128], WG], over=dict(num_neighbours=3)),
    # RP_TW_1_4 and the buffer-load weight-gradient kernel at a hidden width other than 256 (`fastk` depends on mb == 512 alone).  A
    # second rank of 1800 rows makes four minibatches of this rank's ~157 rows: every minibatch, the last included, is mostly
    # padding, and the denominators (global counts) are not the sums of this rank's weights
    "h64": _case("copo", "none", 92, 64, 512, 700, [RP_TW[64], WG_FAST], others=(1800,)),
    # RP_TW_4_8, G = 4
    "h512_mb200": _case("copo", "none", 92, 512, 200, 450, [RP_TW[512], WG]),
    # a hidden width without a row pass: the vector tile-GEMM chain with head_kernel under PPO heads
    "h48": _case("copo", "none", 92, 48, 72, 200, GEMM_VEC + [WG]),
    # ... and the scalar chain (inputs 91 and 184 wide)
    "h48_k91": _case("ccppo", "mf", 91, 48, 72, 200, GEMM_SCALAR + [WG]),
}
PROD, SMALL = "prod", "h64"
CONFIGS = {
    "default": {},                                                  # kl_coeff 0.2, old_value_loss, vf_clip_param 100
    "kl0": dict(kl_coeff=0.0),
    "newvf": dict(old_value_loss=False, vf_clip_param=10.0),
    "ent": dict(entropy_coeff=0.01),
}
CASES = [(s, "default") for s in SHAPE_CASES] + [(s, c) for s in (PROD, SMALL) for c in ("kl0", "newvf", "ent")]
CASE_IDS = ["%s-%s" % sc for sc in CASES]
MARGIN = 1e-3                   # relative; meta_cases.CLIP_MARGIN
GRAD_REL = 1e-5                 # an fp32 gradient element against the exact one, relative to its tensor's largest
STAT_REL = 2e-5                 # ... and a statistic against the exact one, relative to the mean absolute row term
VP = ("vf_preds", "nei_values", "global_values")
VT = ("value_targets", "nei_target", "global_target")
POISON = 1e30                   # see `poisoned`
PLAN_SEED = 7                   # of the permutation that `host_plan` and the GPU test's `plan_epoch` cut into minibatches


def critic_dim(case):
    o = case["odim"]
    if case["policy"] != "ccppo" or case["fuse"] == "none":
        return o
    k = 1 if case["fuse"] == "mf" else int(case["over"].get("num_neighbours", 4))
    return (k + 1) * o + 2 * k


def n_heads(case):
    return 3 if case["policy"] == "copo" else 1


def plan_cfg(case):
    """The case's PpoCfg as far as the launch plan reads it (the GPU test asserts the plan of the learner's own cfg)."""
    return make_cfg(mb=case["mb"], hidden=case["hidden"], in_pol=case["odim"], in_val=(critic_dim(case),) * n_heads(case))


def selected(cfg, mode):
    rc, _geo, launches = query(cfg, mode, facts=ALL)
    assert rc == 0, rc
    return [name for name, *_ in launches]


def assert_selected(cfg, case):
    """Gradients only and the step with Adam launch exactly the kernels the case lists (aligned sources, the mirror present)."""
    for mode in (PPO_GRADS, PPO_STEP):
        assert selected(cfg, mode) == case["kernels"], (mode, selected(cfg, mode), case["kernels"])


def dense_batch(pol, R, odim, seed=0, device="cuda"):
    """A dense train batch of R rows with every column the PPO and the meta steps read (all rows valid).  The critics' targets are off
    by ~150 on 30 % of the rows and by ~120 on the global head: the value nets' gradients dwarf the policy net's."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)  # noqa: E731
    b = SampleBatch()
    b[SampleBatch.OBS] = torch.rand(R, odim, device=device, generator=g) * 2 - 1
    cdim = pol.model.value_input_dim()
    if cdim != odim:
        b["centralized_critic_obs"] = torch.cat([b[SampleBatch.OBS], rn(R, cdim - odim) * 0.5], 1)
    b[SampleBatch.ACTIONS] = rn(R, 2) * 0.8
    di = torch.cat([rn(R, 2) * 0.3, rn(R, 2) * 0.2 - 0.2], 1)
    b[SampleBatch.ACTION_DIST_INPUTS] = di
    b[SampleBatch.ACTION_LOGP] = TorchDiagGaussian(di).logp(b[SampleBatch.ACTIONS])
    for k, s in [(Postprocessing.ADVANTAGES, 2), (SampleBatch.VF_PREDS, 3), ("nei_advantage", 2), ("global_advantages", 1),
                 ("nei_values", 3), ("global_values", 30), ("normalized_advantages", 1)]:
        b[k] = rn(R) * s
    b[Postprocessing.VALUE_TARGETS] = b[SampleBatch.VF_PREDS] + rn(R) * 2 + rn(R) * 150 * (torch.rand(R, device=device, generator=g) < 0.3)
    b["nei_target"] = b["nei_values"] + rn(R) * 2
    b["global_target"] = b["global_values"] + rn(R) * 120
    b[SampleBatch.FLAGS] = torch.ones(R, dtype=torch.uint8, device=device)
    return b


def make(pcls_name, fuse, odim, fused, hiddens=(256, 256), mb=512, device="cuda", **over):
    """A policy of one of the three algorithms on `device` (`_make` of the GPU test files)."""
    from copo_amd.engine import Box
    from copo_amd.torch_copo import algo_ccppo as C, algo_copo as A, algo_ippo as I
    from copo_amd.torch_copo.utils.env_wrappers import (MultiAgentIntersectionEnv, get_ccenv, get_lcf_env,
                                                        get_rllib_compatible_env)
    pcls, ccls = dict(copo=(A.CoPOPolicy, A.CoPOConfig), ccppo=(C.CCPPOPolicy, C.CCPPOConfig),
                      ippo=(I.IPPOPolicy, I.IPPOConfig))[pcls_name]
    cfg = ccls()
    env = get_rllib_compatible_env(get_lcf_env(MultiAgentIntersectionEnv) if pcls_name == "copo"
                                   else get_ccenv(MultiAgentIntersectionEnv))
    cfg.update_from_dict(dict(env=env, device=device, use_hip_graphs=False, use_fused_learner=fused, seed=3,
                              sgd_minibatch_size=mb, model={"fcnet_hiddens": list(hiddens)}, **over))
    if "fuse_mode" in cfg:
        cfg.fuse_mode = fuse
    cfg.validate()
    return pcls(Box(-1, 1, (odim,)), Box(-1, 1, (2,)), cfg)


def make_policy(case, conf, device="cpu", fused=False):
    """The policy of a case under a configuration."""
    return make(case["policy"], case["fuse"], case["odim"], fused, hiddens=(case["hidden"],) * 2, mb=case["mb"], device=device,
                **case["over"], **CONFIGS[conf])


def perturb(model, seed=17):
    """Move the weights off the near-zero head initialisation, from a host generator (the same weights on every device)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dtype == torch.float32:
                p.add_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))


def nets_of(model):
    """Per net (policy, ego value, [neighbour value, global value]) its three nn.Linear, in the kernels' order of the nets."""
    lin = lambda seq: [m._model[0] for m in seq]  # noqa: E731
    nets = [lin(model._hidden_layers) + [model._logits._model[0]], lin(model._value_branch_separate) + [model._value_branch._model[0]]]
    for name in ("nei_value_network", "global_value_network"):
        if getattr(model, name, None) is not None:
            nets.append(lin(getattr(model, name)))
    return nets


def params_of(model):
    """[{tensor name: nn.Parameter}] per net, named as ppo_numpy names the gradients."""
    return [dict(zip(P.TENSORS, [p for lin in net for p in (lin.weight, lin.bias)])) for net in nets_of(model)]


def conf_of(policy):
    """The float64 model's view of the configuration: the numbers the step really uses (the KL coefficient is an fp32 tensor)."""
    c = policy.config
    return dict(clip=float(c["clip_param"]), vf_clip=float(c["vf_clip_param"]), old_value_loss=bool(c["old_value_loss"]),
                vf_coeff=float(c["vf_loss_coeff"]), ent_coeff=float(policy.entropy_coeff),
                kl_coeff=float(policy.kl_coeff) if c["kl_coeff"] > 0.0 else 0.0)


def adv_key(case):
    return "normalized_advantages" if case["policy"] == "copo" else Postprocessing.ADVANTAGES


def valid_rows(R, seed):
    """The valid index list: about 10 % of the rows left out (sorted, like the trainer's), so that every minibatch ends in zero-weight
    padding (meta_cases.valid_rows)."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randperm(R, generator=g)[:R - R // 10].sort().values


def _cc(batch):
    return batch["centralized_critic_obs"] if "centralized_critic_obs" in batch else batch[SampleBatch.OBS]


def add_row_edges(batch, idx, theta, conf, case, seed):
    """Row edges inside the valid rows `idx` of a host batch built by `dense_batch`, written in place.  Everything is crafted from the
    float64 model's own log-probabilities and values under the current weights `theta`, at least 5 % of a threshold away from it, so
    that the fp32 kernels and the model cannot disagree on a branch by rounding.  Returns {block name: row indices}:

      zero_obs, sat<g>   an all-zero input row; per net a row that drives unit 0 of layer 1 to a pre-activation of +24 (tanh is 1.0f,
                         its derivative underflows)
      adv_zero           advantage exactly 0
      neg_hi, pos_lo     ratio beyond 1 + clip with A < 0, below 1 - clip with A > 0: min takes the UNCLIPPED term, gradient flows
      pos_hi, neg_lo     the mirror blocks: min takes the clipped term, no gradient from the surrogate
      old form, per head h:
        v<h>_unclipped   |v - v_prev| > c and the unclipped square wins: gradient 2 (v - T)
        v<h>_clip_hi/lo  v - v_prev > c / < -c and the clipped square wins: the head gets NO gradient from the row
        v<h>_inside      |v - v_prev| = c - 5 % .. 10 %, both sides: inside the clamp the clipped value IS v, the two squares are
                         the same number up to rounding and whichever `max` takes carries the gradient 2 (v - T)
      new form, per head h:
        v<h>_above/below (v - T)^2 above c (no gradient) / below c
    Every other valid row within 2 MARGIN (relative) of a threshold -- ratio against 1 +- clip, |v - v_prev| against c, (v - T)^2 against
    c, the gap of the two squares of a row outside the clamp against 0 -- is moved to 4 MARGIN on its own side."""
    g = torch.Generator().manual_seed(3000 + seed)
    n = idx.numel()
    blk = max(4, n // 24)
    clip, c, old_form = conf["clip"], conf["vf_clip"], conf["old_value_loss"]
    heads = len(theta) - 1
    pick = idx[torch.randperm(n, generator=g)]
    blocks = {"zero_obs": pick[0:1]}
    obs, cc = batch[SampleBatch.OBS], _cc(batch)
    obs[pick[0]] = 0.0
    cc[pick[0]] = 0.0
    for gi, net in enumerate(theta):
        w1 = net[0][0][0]
        src = obs if gi == 0 else cc
        src[pick[1 + gi]] = (torch.sign(w1) * (24.0 - float(net[0][1][0])) / float(w1.abs().sum())).float()
        blocks["sat%d" % gi] = pick[1 + gi:2 + gi]
    logp, vals = P.forward_rows(theta, obs.double().numpy(), cc.double().numpy(), batch[SampleBatch.ACTIONS].double().numpy())
    lp = torch.as_tensor(logp)
    # ---- the surrogate's branches
    for i, name in enumerate(("adv_zero", "neg_hi", "pos_lo", "pos_hi", "neg_lo")):
        blocks[name] = pick[8 + i * blk:8 + (i + 1) * blk]
    ak = adv_key(case)
    adv, oldlp = batch[ak].double(), batch[SampleBatch.ACTION_LOGP].double()
    adv[blocks["adv_zero"]] = 0.0
    u = torch.rand(blk, generator=g, dtype=torch.float64)
    for name, sign, high in (("neg_hi", -1.0, True), ("pos_lo", 1.0, False), ("pos_hi", 1.0, True), ("neg_lo", -1.0, False)):
        r = blocks[name]
        adv[r] = sign * (adv[r].abs() + 0.1)
        oldlp[r] = lp[r] - torch.log((1.0 + clip + 0.05 * (1.0 + u)) if high else (1.0 - clip - 0.05 * (1.0 + u)))
    ratio = torch.exp(lp - oldlp)
    for thr in (1.0 - clip, 1.0 + clip):
        near = idx[((ratio - thr).abs() < 2 * MARGIN * thr)[idx]]
        side = torch.where(ratio[near] >= thr, 1.0, -1.0).double()
        oldlp[near] = lp[near] - torch.log(thr * (1.0 + side * 4 * MARGIN))
    batch[ak], batch[SampleBatch.ACTION_LOGP] = adv.float(), oldlp.float()
    # ---- the value losses' branches, per head on its own columns and its own draw of rows
    for h in range(heads):
        v = torch.as_tensor(vals[h])
        vp, tg = batch[VP[h]].double(), batch[VT[h]].double()
        ph = idx[torch.randperm(n, generator=g)]
        uu = [torch.rand(blk, generator=g, dtype=torch.float64) for _ in range(4)]
        alt = torch.where(torch.arange(blk) % 2 == 0, 1.0, -1.0).double()
        if old_form:
            names = ("unclipped", "clip_hi", "clip_lo", "inside")
            for i, name in enumerate(names):
                blocks["v%d_%s" % (h, name)] = ph[i * blk:(i + 1) * blk]
            d = 0.05 * c * (1.0 + uu[0])
            r = blocks["v%d_unclipped" % h]
            vp[r], tg[r] = v[r] - alt * (c + d), v[r] - 2.0 * alt * d         # v - T = 2 s d, clipped - T = s d
            for name, s, ui in (("clip_hi", 1.0, 1), ("clip_lo", -1.0, 2)):
                r, d = blocks["v%d_%s" % (h, name)], 0.05 * c * (1.0 + uu[ui])
                vp[r], tg[r] = v[r] - s * (c + d), v[r] + s * d                 # v - T = -s d, clipped - T = -2 s d
            r = blocks["v%d_inside" % h]
            vp[r] = v[r] - alt * (c - 0.05 * c * (1.0 + uu[3]))
            crafted = ph[:4 * blk]
            rest = torch.ones(vp.numel(), dtype=torch.bool)
            rest[crafted] = False
            dist = (v - vp).abs()
            near = idx[(((dist - c).abs() < 2 * MARGIN * c) & rest)[idx]]
            side = torch.where(dist[near] >= c, 1.0, -1.0).double()
            vp[near] = v[near] - torch.sign(v[near] - vp[near]) * c * (1.0 + side * 4 * MARGIN)
            # rows outside the clamp that nobody crafted (the global head's v_prev spreads over +-100): the gap of the two squares
            e = (v - vp) - torch.sign(v - vp) * c
            d1 = v - tg
            l1, l2 = d1 ** 2, (d1 - e) ** 2
            out = idx[(((v - vp).abs() > c) & rest & ((l1 - l2).abs() < 2 * MARGIN * torch.maximum(l1, l2)))[idx]]
            rho = (1.0 + 4 * MARGIN) ** 0.5
            d1_new = torch.where(l1[out] >= l2[out], e[out] * rho / (1.0 + rho), e[out] / (1.0 + rho))
            tg[out] = v[out] - d1_new
        else:
            for i, name in enumerate(("above", "below")):
                blocks["v%d_%s" % (h, name)] = ph[i * blk:(i + 1) * blk]
            r = blocks["v%d_above" % h]
            tg[r] = v[r] - alt * c ** 0.5 * (1.5 + uu[0])
            r = blocks["v%d_below" % h]
            tg[r] = v[r] - alt * c ** 0.5 * 0.4 * (1.0 + uu[1])
            l1 = (v - tg) ** 2
            near = idx[((l1 - c).abs() < 2 * MARGIN * c)[idx]]
            side = torch.where(l1[near] >= c, 1.0, -1.0).double()
            tg[near] = v[near] - torch.where(v[near] >= tg[near], 1.0, -1.0).double() * (c * (1.0 + side * 4 * MARGIN)) ** 0.5
        batch[VP[h]], batch[VT[h]] = vp.float(), tg.float()
    return blocks


def build_inputs(pol, case):
    """Host batch with the row edges for the policy's current weights: (batch of fp32 CPU tensors, valid rows, blocks, theta, conf)."""
    theta = P.theta_of_nets(nets_of(pol.model))
    conf, seed = conf_of(pol), case["seed"]
    batch = dense_batch(pol, case["R"], case["odim"], seed=seed, device="cpu")
    idx = valid_rows(case["R"], seed)
    blocks = add_row_edges(batch, idx, theta, conf, case, seed)
    return batch, idx, blocks, theta, conf


def host_columns(batch, case):
    """The columns the PPO step reads, as float64 numpy on the host (exact copies of the fp32 values the kernels read)."""
    d = lambda k: batch[k].detach().cpu().double().numpy()  # noqa: E731
    h = n_heads(case)
    return dict(obs=d(SampleBatch.OBS), cc=_cc(batch).detach().cpu().double().numpy(), act=d(SampleBatch.ACTIONS), old_logp=d(SampleBatch.ACTION_LOGP),
                dist=d(SampleBatch.ACTION_DIST_INPUTS), adv=d(adv_key(case)), vpred=np.stack([d(k) for k in VP[:h]], 1),
                vtarget=np.stack([d(k) for k in VT[:h]], 1))


def minibatch(cols, rows, w, denom):
    """The float64 model's view of one minibatch of the planned tables: the rows with w > 0."""
    rows, w = np.asarray(rows), np.asarray(w, np.float64)
    keep = w > 0
    r = rows[keep]
    return dict({k: v[r] for k, v in cols.items()}, rows=r, w=w[keep], denom=float(denom), mb=int(w.size))


def host_plan(idx, case, seed=None):
    """The tables `plan_epoch` builds, on the host: the shuffled valid rows cut into n_mb near-equal minibatches padded with zero-weight
    slots, n_mb from the largest rank, the denominators summed over the ranks (and at least 1), in fp32 as the device tables hold them."""
    mb, B = case["mb"], int(idx.numel())
    perm = idx[torch.randperm(B, generator=torch.Generator().manual_seed(PLAN_SEED if seed is None else seed))].numpy()
    n_mb = max(1, -(-max((B,) + case["others"]) // mb))
    rows, w = np.zeros((n_mb, mb), np.int64), np.zeros((n_mb, mb), np.float32)
    denom = np.zeros(n_mb)
    for k, part in enumerate(np.array_split(perm, n_mb)):
        rows[k, :part.size], w[k, :part.size] = part, 1.0
    for b in (B,) + case["others"]:
        q, r = divmod(b, n_mb)
        denom += q + (np.arange(n_mb) < r)
    return rows, w, np.maximum(denom, 1.0).astype(np.float32)


def poisoned(batch, idx):
    """A copy of the batch whose rows OUTSIDE the valid list hold values that would swamp any sum they entered: the padded slots of the
    row table are pointed at them.  The kernels (like torch) MULTIPLY a row's terms by its weight, they do not skip the row, so the
    poison is huge but finite and chosen so that every row term stays finite (0 x term = 0) and every path carries it: 1e30 in the
    inputs (the hidden units saturate, the head outputs stay ordinary), 1e25 in the advantages, 1e15 in the value columns (their
    squares are 1e30).  Actions, old log-probabilities and the behaviour policy's distribution stay as they are, so that the ratio is
    of order 1 and the surrogate term and its gradient are ~1e25 times a valid row's.  NaN, or a value whose square overflows, would
    come out of a correct kernel as NaN."""
    out = SampleBatch({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
    R = out[SampleBatch.OBS].shape[0]
    bad = torch.ones(R, dtype=torch.bool)
    bad[idx] = False
    for k, v in out.items():
        if not torch.is_tensor(v) or not v.is_floating_point():
            continue
        if k in (SampleBatch.ACTION_DIST_INPUTS, SampleBatch.ACTIONS, SampleBatch.ACTION_LOGP):
            continue
        v[bad.to(v.device)] = 1e15 if k in VP + VT else 1e25 if "advantage" in k else POISON
    return out, torch.nonzero(bad).reshape(-1)


def tolerance(e_t32, mb):
    """The GPU bound on a tensor's error relative to its largest element (the gradient row)."""
    return min(3.0 * e_t32 + mb * 2.0 ** -24, GRAD_REL)


def tensor_errors(got, ref):
    """{(net, tensor): max |got - ref| / max |ref|} over the nets' tensors; a tensor whose reference is identically 0 maps to
    max |got| (which must then be 0)."""
    out = {}
    for gi, (a, b) in enumerate(zip(got, ref)):
        for name in P.TENSORS:
            scale = float(np.abs(b[name]).max())
            out[(gi, name)] = float(np.abs(a[name] - b[name]).max()) / (scale if scale > 0.0 else 1.0)
    return out
