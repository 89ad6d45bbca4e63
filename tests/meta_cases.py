"""Shapes, row edges and LCF parameter cases of the meta-update referee (tests/test_meta_cpu.py, tests/test_gpu_meta_float64.py).

Every shape case is the smallest one that still selects its kernels; `selected()` reads the kernels a case really launches from the
library's launch plan, and the tests assert them, so a case cannot silently stop covering what its comment claims."""
import numpy as np
import torch

import meta_numpy as M
from test_learner_plan_cpu import ALIGNED, META_BATCH, META_PAIR, ROW_STORE, ROW_WGRADS, STORE_OK, query

_VEC = ["gemm_kernel<FwdOpT<1>, true>", "gemm_kernel<FwdOpT<2>, true>", "head_kernel", "gemm_kernel<BxOp, true>"]
_SCALAR = ["gemm_kernel<FwdOpT<1>, false>", "gemm_kernel<FwdOpT<2>, false>", "head_kernel", "gemm_kernel<BxOp, false>"]
_FOLD, _PAIR_FOLD = "meta_batch_fold_kernel", "reduce_adam_kernel"


def _case(hidden, odim, mb, R, pair, rows, bw, bw_store, fold_blocks):
    """pair: the row-local kernels of the step-by-step pair; rows: those of the batched pass and of the row store (always the tile-GEMM
    chain: the row pass has no batched form); bw / bw_store: the weight-gradient GEMM of a pass without / with the row store."""
    return dict(hidden=hidden, odim=odim, mb=mb, R=R, fold_blocks=fold_blocks,
                kernels=dict(pair=pair + [bw, _PAIR_FOLD], batch=rows + [bw, _FOLD],
                             store=rows, wgrads=[bw_store, _FOLD]))


SHAPE_CASES = {
    # RP_1_4 in pair mode (the PPO tests at hidden 64 take RP_TW_1_4: the meta pair has no mirror of the target net); the batched
    # vector GEMM chain at its smallest tile count: one column tile, two row tiles
    "h64": _case(64, 92, 128, 300, ["rowpass_kernel<1, 4, false>"], _VEC, "gemm_bw_kernel<true>", "gemm_bw_kernel<true, true>", 11),
    # RP_2_4; a minibatch size that is no multiple of the 16-row head tiles or the 64-row GEMM tiles; ragged minibatches (135 of 200)
    "h128_mb200": _case(128, 92, 200, 450, ["rowpass_kernel<2, 4, false>"], _VEC, "gemm_bw_kernel<true>", "gemm_bw_kernel<true, true>", 29),
    # RP_4_8; a fold of 306 workgroups (the production shape has 89), weight-gradient row split 4 in pair mode
    "h512": _case(512, 92, 512, 600, ["rowpass_kernel<4, 8, false>"], _VEC, "gemm_bw_kernel<true>", "gemm_bw_kernel<true, true>", 306),
    # an input width that is no multiple of 4: no vector rows, hence no row pass in pair mode either (it needs them without the
    # mirror) -- the scalar GEMM_F1 / F2 / BX / BW and head_kernel with META heads in pair and batched modes.  The row store is NOT
    # refused at this width: it takes the scalar gather-all GEMM_BW_GA, all of the head layer's tiles included (28 instead of 25)
    "k93": _case(256, 93, 512, 1100, _SCALAR, _SCALAR, "gemm_bw_kernel<false>", "gemm_bw_kernel<false, true>", 89),
    # a hidden width without a row-pass shape and H % 64 != 0: gemm_bw_kernel places the bias column inside the (only) column tile
    # of layers 2 / 3 instead of taking it from the row sums (BwOpT::bias_by_rowsum off)
    "h48": _case(48, 92, 72, 200, _VEC, _VEC, "gemm_bw_kernel<true>", "gemm_bw_kernel<true, true>", 7),
    # an input wider than the hidden layer: RP_2_8 with a 260-wide layer 1, five column tiles of the layer-1 weight gradient
    "k260": _case(256, 260, 512, 600, ["rowpass_kernel<2, 8, false>"], _VEC, "gemm_bw_kernel<true>", "gemm_bw_kernel<true, true>", 131),
}
SMALL = "h64"                   # the shape of the end-to-end run

# (p0, p1) of the LCF distribution: mean = clamp(tanh p0, +-(1 - 1e-6)), std = exp(clamp(p1, -20, 2))
LCF_CASES = [
    (0.05, -2.3),               # interior
    (9.0, 0.3),                 # tanh clamped high: dS/dp0 exactly 0
    (-9.0, 0.3),                # ... low
    (0.2, 2.5),                 # std clamped high: dS/dp1 exactly 0
    (0.2, -21.0),               # ... low
    (0.0, 2.0),                 # exactly ON the clamp: torch.clamp passes the gradient at equality (test_meta_cpu holds it to that)
    (0.0, -20.0),
]
ZERO_D0 = {1, 2}                # indices of LCF_CASES whose dS/dp0 / dS/dp1 must be exactly 0.0
ZERO_D1 = {3, 4}
RAW_MEAN_STD = [(0.0, 1.0), (-0.4, 0.05)]
CLIP_MARGIN = 1e-3              # no valid row's ratio lies closer than this to 1 - clip or 1 + clip
DECIDABLE_SHARE = 0.8           # share of a case's minibatches whose |gv64| must exceed the derived bound on |gv - gv64|
GRAD_REL = 1e-5                 # an fp32 gradient element against the exact one, relative to its tensor's largest


def selected(cfg, mode, n=0):
    """Kernel names of the plan the entry points walk for `cfg` in `mode` (their pointers: 16-byte aligned, no mirror)."""
    rc, geo, launches = query(cfg, mode, n=n, facts=ALIGNED | STORE_OK)
    assert rc == 0, rc
    return [name for name, *_ in launches], geo


def assert_selected(cfg, case):
    """The four meta modes of `cfg` launch exactly the kernels the case lists (batched modes at nb = 1 and 3)."""
    k = case["kernels"]
    names, geo = selected(cfg, META_PAIR)
    assert names == k["pair"] and geo["fold_blocks"] == case["fold_blocks"], (names, geo)
    for nb in (1, 3):
        assert selected(cfg, META_BATCH, nb)[0] == k["batch"], selected(cfg, META_BATCH, nb)[0]
        assert selected(cfg, ROW_WGRADS, nb)[0] == k["wgrads"], selected(cfg, ROW_WGRADS, nb)[0]
    blocks = -(-case["R"] // case["mb"])
    assert selected(cfg, ROW_STORE, blocks)[0] == k["store"], selected(cfg, ROW_STORE, blocks)[0]


def valid_rows(R, seed):
    """The valid index list: about 10 % of the rows left out (sorted, like the trainer's), so that every minibatch of the plan ends in
    zero-weight padding."""
    g = torch.Generator().manual_seed(1000 + seed)
    keep = torch.randperm(R, generator=g)[:R - R // 10]
    return keep.sort().values


def add_row_edges(batch, idx, logp_new64, clip, seed):
    """Row edges inside the valid rows `idx` (int64, CPU) of a batch built by `_dense_batch`, written in place:
      - a block with global_advantages == 0,
      - a block with negative advantage and ratio above 1 + clip, a block with positive advantage and ratio below 1 - clip: the clamp
        is out of range but min(A r, A clip(r)) takes the UNCLIPPED term, the gradient flows,
      - the two mirror blocks (positive advantage above 1 + clip, negative below 1 - clip): min takes the clipped term, the rows carry
        weight 1 and contribute NO gradient to g_new,
      - every other valid row whose ratio falls within 2 CLIP_MARGIN of a threshold is moved to 4 CLIP_MARGIN from it, on its side.
    ACTION_LOGP is crafted from `logp_new64`, the float64 model's log-probabilities of ALL rows under the current policy, so that
    the fp32 kernels and the float64 model cannot disagree on a branch because of rounding.  Returns the five blocks (row indices): zero, negative-high, positive-low, positive-high, negative-low."""
    g = torch.Generator().manual_seed(2000 + seed)
    n = idx.numel()
    blk = max(4, n // 24)
    pick = idx[torch.randperm(n, generator=g)]
    zero, neg, pos, pos_hi, neg_lo = (pick[i * blk:(i + 1) * blk] for i in range(5))
    dev = batch["global_advantages"].device
    adv = batch["global_advantages"].detach().cpu().double()
    old = batch["action_logp"].detach().cpu().double()
    lp = torch.as_tensor(logp_new64, dtype=torch.float64)
    adv[zero] = 0.0
    u = torch.rand(blk, generator=g, dtype=torch.float64)
    for rows_, sign, high in ((neg, -1.0, True), (pos, 1.0, False), (pos_hi, 1.0, True), (neg_lo, -1.0, False)):
        adv[rows_] = sign * (adv[rows_].abs() + 0.1)
        old[rows_] = lp[rows_] - torch.log((1.0 + clip + 0.05 * (1.0 + u)) if high else (1.0 - clip - 0.05 * (1.0 + u)))
    ratio = torch.exp(lp - old)
    for thr in (1.0 - clip, 1.0 + clip):
        near = ((ratio - thr).abs() < 2 * CLIP_MARGIN)
        near_idx = idx[near[idx]]
        side = torch.where(ratio[near_idx] >= thr, 1.0, -1.0).double()
        old[near_idx] = lp[near_idx] - torch.log(thr + side * 4 * CLIP_MARGIN)
    batch["global_advantages"] = adv.float().to(dev)
    batch["action_logp"] = old.float().to(dev)
    return zero, neg, pos, pos_hi, neg_lo


def ratio_margin(ratio, clip):
    """Smallest distance of a ratio from the two clip thresholds."""
    r = np.asarray(ratio, np.float64)
    return float(np.minimum(np.abs(r - (1.0 - clip)), np.abs(r - (1.0 + clip))).min())


def policy_linears(model):
    return [m._model[0] for m in model._hidden_layers] + [model._logits._model[0]]


def thetas(policy, flat_new, flat_old):
    """(theta_new, theta_old) of meta_numpy for a CoPOPolicy whose model / target model live in the FlatParams given."""
    return (M.theta_of(policy_linears(policy.model), lambda p: flat_new.offset[id(p)]),
            M.theta_of(policy_linears(policy.target_model), lambda p: flat_old.offset[id(p)]))


def minibatch(cols, rows, w, denom, eps):
    """The float64 model's view of one minibatch: the rows with w > 0 of the planned tables (numpy / CPU tensors)."""
    rows, w, eps = np.asarray(rows), np.asarray(w, np.float64), np.asarray(eps, np.float64)
    keep = w > 0
    r = rows[keep]
    return dict(rows=r, w=w[keep], denom=float(denom), eps=eps[keep], obs=cols["obs"][r], act=cols["actions"][r],
                old_logp=cols["action_logp"][r], glob_adv=cols["global_advantages"][r], ego=cols["advantages"][r],
                nei=cols["nei_advantage"][r])


def host_columns(batch):
    """The columns the meta step reads, as float64 numpy on the host (exact copies of the fp32 values the kernels read)."""
    return {k: batch[k].detach().cpu().double().numpy() for k in ("obs", "actions", "action_logp", "global_advantages", "advantages",
                                                                 "nei_advantage")}


def decidable_share(terms, thetas_):
    """Share of the minibatches whose exact dot product exceeds the derived bound on an fp32 evaluation's error (meta_numpy.dot_bound
    with GRAD_REL per element) -- a condition on the inputs, computed from the float64 model alone; also returns the bounds."""
    tn, to = thetas_
    bounds, ok = [], 0
    for t in terms:
        b = M.dot_bound(t["g_new"], t["g_old"], M.element_bounds(tn, t["g_new"], GRAD_REL), M.element_bounds(to, t["g_old"], GRAD_REL))
        bounds.append(b)
        ok += abs(float(np.dot(t["g_new"], t["g_old"]))) > b
    return ok / len(terms), bounds
