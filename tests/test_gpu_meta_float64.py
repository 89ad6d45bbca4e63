"""The LCF meta update against its float64 / 40-digit model (tests/meta_numpy.py) at every kernel shape the
meta modes select (tests/meta_cases.py): both policy gradients of the step-by-step pair, of the batched pass and of the row-store
pass against the exact gradients and against torch's own fp32 step; their dot products against a DERIVED bound; the fp64 LCF tail
and the sequential LCF kernel against mpmath at the clamp branches; one end-to-end `run_meta` against the chained model.

Measured on an MI355X (`python -m pytest -s` prints every figure).  Gradient error / largest element of the tensor, worst tensor,
minibatch and path of a case, HIP | torch fp32:  h64 6.2e-7 | 5.6e-7,  h128_mb200 1.1e-6 | 9.2e-7,  h512 3.9e-6 | 5.7e-6,
k93 1.3e-6 | 1.2e-6,  h48 5.3e-7 | 5.9e-7,  k260 1.5e-6 | 1.1e-6 (bound 1e-5).  |gv - gv64| / derived bound: 5e-5 .. 1.6e-3, every
minibatch of every case decidable.  meta_lcf tail: at most 0.071 of (1e-12 |x| + 1e-15); meta_seq_kernel after 12 steps: at most 5.3e-4
of (1e-10 |x| + 1e-12); run_meta end to end: at most 2.4e-3 of what the dot products' bounds allow.  The file takes 8 s, 3 s of it
the first policy's construction."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import meta_cases as MC  # noqa: E402
import meta_numpy as M  # noqa: E402
from test_gpu_fused_learner import _copy_weights, _dense_batch, _make  # noqa: E402

RAW = (0.3, 2.0)                # {mean, std} of the raw coordinated advantage in the gradient / end-to-end tests
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The policies, batches and meta buffers of the shape cases live for this module only."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _setup(name):
    """One policy pair (torch fp32 reference, fused), batch, plan and float64 gradients per shape case, built once per module."""
    if name in _CACHE:
        return _CACHE[name]
    t0 = time.perf_counter()
    case = MC.SHAPE_CASES[name]
    H, odim, mb, R = (case[k] for k in ("hidden", "odim", "mb", "R"))
    ref = _make("copo", "none", odim, fused=False, hiddens=(H, H), mb=mb)
    fz = _make("copo", "none", odim, fused=True, hiddens=(H, H), mb=mb)
    assert fz.fused is not None and ref.fused is None
    with torch.no_grad():
        for p in list(ref.model.parameters()) + list(ref.target_model.parameters()):
            if p.dtype == torch.float32:
                p.add_(torch.randn_like(p) * 0.05)
    _copy_weights(fz, ref)
    MC.assert_selected(fz.fused.cfg, case)                  # the case covers the kernels it claims, for the cfg the kernels get
    tn, to = MC.thetas(fz, fz.fused.flat, fz.fused.target_flat)
    nf = fz.fused.meta_fold_len()
    assert nf == tn["n"] == to["n"]
    clip = float(fz.config["clip_param"])
    batch = _dense_batch(ref, R, odim, seed=5)
    idx_h = MC.valid_rows(R, seed=5)
    logp64 = M.log_prob(tn["layers"], batch["obs"].double().cpu(), batch["actions"].double().cpu()).numpy()
    MC.add_row_edges(batch, idx_h, logp64, clip, seed=5)
    cols = MC.host_columns(batch)
    idx = idx_h.cuda()
    B = int(idx.numel())
    for pol in (ref, fz):
        pol.prepare_sgd(batch, R, mb)
        pol._raw_lcf_adv_mean.fill_(RAW[0])
        pol._raw_lcf_adv_std.fill_(RAW[1])
        torch.manual_seed(1)
        pol.use_graphs = False
        pol.run_meta(idx, B, [B], mb, 0)                    # allocates the meta buffers, no steps
        torch.manual_seed(2)
        n_mb = pol.plan_epoch(idx, B, [B], mb, bufs=pol._meta_bufs)
        pol._meta_bufs["eps_all"].normal_()
    fz._meta_bufs["eps_all"].copy_(ref._meta_bufs["eps_all"])
    assert torch.equal(ref._meta_bufs["rows_all"], fz._meta_bufs["rows_all"]) and n_mb == -(-B // mb)
    mbuf = fz._meta_bufs
    # the plans asserted above are those of 16-byte aligned pointers without a mirror (what facts_of derives from these arguments)
    for t in (fz._row_sources["obs"], fz._row_sources["pack"], fz.fused.flat.flat, fz.fused.target_flat.flat, fz.fused.workspace,
              mbuf["g_new"], mbuf["g_old"]):
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    tabs = {k: mbuf[k][:n_mb].cpu().numpy() for k in ("rows_all", "w_all", "denom_all", "eps_all")}
    mbs = [MC.minibatch(cols, tabs["rows_all"][k], tabs["w_all"][k], tabs["denom_all"][k], tabs["eps_all"][k]) for k in range(n_mb)]
    assert all(0 < m["w"].size < mb and m["w"].sum() == m["denom"] for m in mbs)      # every minibatch ends in zero-weight padding
    terms = [M.policy_terms(tn, to, m["obs"], m["act"], m["old_logp"], m["glob_adv"], m["w"], m["denom"], clip) for m in mbs]
    # conditions on the inputs, from the float64 model alone: ratios clear of the thresholds, dot products decidable
    margin = min(MC.ratio_margin(t["ratio"], clip) for t in terms)
    assert margin >= MC.CLIP_MARGIN, margin
    share, bounds = MC.decidable_share(terms, (tn, to))
    assert share >= MC.DECIDABLE_SHARE, (share, bounds)
    # torch's own fp32 evaluation of every minibatch, in the fold layout
    n_pol, lay, t32 = ref._meta_bufs["n_pol"], M.tensors_of(tn), []
    for k in range(n_mb):
        ref._meta_bufs["k"].fill_(k)
        ref._meta_step_a()
        flat = ref._meta_bufs["flat"].cpu().numpy()
        pair = []
        for part in (flat[:n_pol], flat[n_pol:2 * n_pol]):
            g, pos = np.zeros(nf), 0
            for _n, a, b in lay:
                g[a:b] = part[pos:pos + b - a]
                pos += b - a
            assert pos == n_pol
            pair.append(g)
        t32.append(pair)
    S = dict(case=case, name=name, ref=ref, fz=fz, tn=tn, to=to, nf=nf, clip=clip, batch=batch, cols=cols, idx=idx, B=B, n_mb=n_mb, mbs=mbs,
             terms=terms, bounds=bounds, share=share, t32=t32, lo=min(fz.fused.flat.offset[id(p)] for p in fz.model.policy_parameters()),
             rs=dict(fz._row_sources, **{k: mbuf[k] for k in ("rows_all", "w_all", "denom_all")}), worst={})
    print("\n[%s] setup %.2f s: %d minibatches, ratio margin %.2e, decidable %.0f %%" % (name, time.perf_counter() - t0, n_mb, margin, 100 * share))
    _CACHE[name] = S
    return S


def _check_pair(S, k, g_new, g_old, gv, path):
    """One minibatch's gradient pair (numpy float64 views of fp32 results, fold layout) and dot product against the float64 model."""
    mb = S["case"]["mb"]
    for which, got, theta in (("g_new", g_new, S["tn"]), ("g_old", g_old, S["to"])):
        g64, g32 = S["terms"][k][which], S["t32"][k][which == "g_old"]
        for tname, a, b in M.tensors_of(theta):
            scale = float(np.abs(g64[a:b]).max())
            assert scale > 0.0
            e_hip, e_t32 = float(np.abs(got[a:b] - g64[a:b]).max()) / scale, float(np.abs(g32[a:b] - g64[a:b]).max()) / scale
            w = S["worst"].setdefault(path, [0.0, 0.0, 0.0])
            w[0], w[1] = max(w[0], e_hip), max(w[1], e_t32)
            assert e_hip <= MC.GRAD_REL and e_t32 <= MC.GRAD_REL, (S["name"], path, k, which, tname, e_hip, e_t32)
            assert e_hip <= 3.0 * e_t32 + mb * 2.0 ** -24, (S["name"], path, k, which, tname, e_hip, e_t32)
    gv64 = float(np.dot(S["terms"][k]["g_new"], S["terms"][k]["g_old"]))
    S["worst"][path][2] = max(S["worst"][path][2], abs(gv - gv64) / S["bounds"][k])
    assert abs(gv - gv64) <= S["bounds"][k], (S["name"], path, k, gv, gv64, S["bounds"][k])
    if abs(gv64) > S["bounds"][k]:
        assert np.sign(gv) == np.sign(gv64)


def _report(S, path):
    w = S["worst"][path]
    print("[%s] %-12s HIP %.2e  torch fp32 %.2e  (of the tensor's largest element);  |gv - gv64| / bound %.2e" % (S["name"], path, w[0], w[1], w[2]))


@pytest.mark.parametrize("name", list(MC.SHAPE_CASES))
def test_pair_gradients_and_dot_product(name):
    """`copo_meta_grads_f32` (step-by-step pair), every minibatch of the plan: per tensor, the HIP error against the exact gradient is
    at most 3 x torch fp32's own + mb 2^-24, and both are under 1e-5 of the tensor's largest element; the dot
    product of the pair (the fold's fp64 partials) is within the bound derived from that 1e-5 (meta_numpy.dot_bound)."""
    S = _setup(name)
    fz, mbuf, nf, lo = S["fz"], S["fz"]._meta_bufs, S["nf"], S["lo"]
    for k in range(S["n_mb"]):
        mbuf["k"].fill_(k)
        mbuf["g_both"].zero_()
        fz._meta_step_a()
        torch.cuda.synchronize()
        gv = float(mbuf["dot_partials"][:S["case"]["fold_blocks"]].sum())
        _check_pair(S, k, mbuf["g_new"][lo:lo + nf].double().cpu().numpy(), mbuf["g_old"][lo:lo + nf].double().cpu().numpy(), gv, "pair")
    mbuf["k"].zero_()
    _report(S, "pair")


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", list(MC.SHAPE_CASES))
def test_batched_and_row_store_gradients_and_dot_products(name, nb):
    """`copo_meta_batch_grads_f32` and `copo_meta_rows_f32` + `copo_meta_batch_wgrads_f32` over all minibatches of one pass in chunks of
    `nb`: the exported gradient pairs (the row store's carry unit row weights: both factors 1 / D_k applied here, as `meta_batch_dot`
    documents) and `gv` against the same float64 gradients, in the same way."""
    S = _setup(name)
    fz, rs, nf, n_mb = S["fz"].fused, S["rs"], S["nf"], S["n_mb"]
    denom = rs["denom_all"][:n_mb].double().cpu().numpy()
    for path, store in (("batch nb=%d" % nb, False), ("store nb=%d" % nb, True)):
        gv = torch.full((n_mb,), float("nan"), dtype=torch.float64, device="cuda")
        stats_k = torch.zeros(n_mb, 2, 8, device="cuda")
        g_out = torch.full((n_mb, 2, nf), float("nan"), device="cuda")
        if store:
            fz.meta_rows(S["fz"]._row_sources)
        for c0 in range(0, n_mb, nb):
            (fz.meta_batch_wgrads if store else fz.meta_batch_grads)(rs, c0, min(nb, n_mb - c0), gv, stats_k, g_out=g_out[c0:])
        torch.cuda.synchronize()
        g, gvh = g_out.double().cpu().numpy(), gv.cpu().numpy()
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(gvh))
        for k in range(n_mb):
            sc = 1.0 / denom[k] if store else 1.0
            _check_pair(S, k, g[k, 0] * sc, g[k, 1] * sc, float(gvh[k]), path)
            # the loss statistics the LCF steps accumulate: fp32 sums of mb terms against the model's, 1e-5 of the terms' size
            t = S["terms"][k]
            st = stats_k[k].cpu().numpy()
            for got, want, size in ((st[0, 1], t["new_loss"], t["abs_new"]), (st[1, 1], t["old_loss"], t["abs_old"]), (st[0, 7], t["global_adv"], t["abs_adv"])):
                assert abs(got - want) <= 1e-5 * size + 1e-9, (name, path, k, got, want)
        _report(S, path)


def _close(got, want, rel, ab, what):
    got, want = np.asarray(got, np.float64), np.array([float(x) for x in want])
    err = np.abs(got - want)
    assert np.all(err <= rel * np.abs(want) + ab), (what, got.tolist(), want.tolist(), (err / (rel * np.abs(want) + ab)).max())
    return float((err / (rel * np.abs(want) + ab)).max())


@pytest.mark.parametrize("name", list(MC.SHAPE_CASES))
def test_lcf_tail_against_mpmath(name):
    """`copo_meta_lcf_f64` (tail[0:4] = dS/dp0, dS/dp1, S, mean A') on the first and the last minibatch, every LCF parameter case and
    both raw (mean, std): 1e-12 relative + 1e-15 absolute against the 40-digit terms (fp64 sums of up to 512 rows), the derivative
    of a clamped parameter exactly 0.0."""
    S = _setup(name)
    fz, mbuf = S["fz"], S["fz"]._meta_bufs
    rs = dict(S["rs"], k=mbuf["k"])
    worst = 0.0
    for ri, raw in enumerate(MC.RAW_MEAN_STD):
        raw_t = torch.tensor(raw, dtype=torch.float64, device="cuda")
        for ci, pc in enumerate(MC.LCF_CASES):
            k = 0 if (ci + ri) % 2 == 0 else S["n_mb"] - 1
            mbuf["k"].fill_(k)
            p = torch.tensor(pc, dtype=torch.float64, device="cuda")
            tail = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
            fz.fused.meta_lcf(rs, mbuf["eps_all"], p, raw_t, tail, mbuf["col_adv"], mbuf["col_nei_adv"])
            got = tail.cpu().numpy()
            m = S["mbs"][k]
            want = M.lcf_terms(pc, raw, m["ego"], m["nei"], m["eps"], m["w"], m["denom"])
            worst = max(worst, _close(got, want, 1e-12, 1e-15, (name, pc, raw, k)))
            if ci in MC.ZERO_D0:
                assert got[0] == 0.0 and want[0] == 0
            if ci in MC.ZERO_D1:
                assert got[1] == 0.0 and want[1] == 0
            assert (got[0] != 0.0 or ci in MC.ZERO_D0) and (got[1] != 0.0 or ci in MC.ZERO_D1)
    mbuf["k"].zero_()
    print("\n[%s] meta_lcf tail: worst error / (1e-12 |x| + 1e-15) = %.3f" % (name, worst))


@pytest.mark.parametrize("name", list(MC.SHAPE_CASES))
def test_sequential_lcf_kernel_against_mpmath(name):
    """`copo_meta_batch_lcf_f64` (meta_seq_kernel: sincospi, prefetched rows, expm1 forms of tanh / exp), 12 LCF steps on dense rows with
    one workgroup and with four, from every LCF parameter case, fed the MODEL's dot products so that only the fp64 kernel is under
    test: parameters, Adam state and the seven statistics to 1e-10 relative + 1e-12 absolute against mpmath (the bounds
    test_sequential_lcf_kernel_over_several_workgroups uses between kernel variants)."""
    S = _setup(name)
    fz, mb, n_mb, steps_n = S["fz"], S["case"]["mb"], S["n_mb"], 12
    lr = float(fz.config["lcf_lr"])
    g = torch.Generator().manual_seed(31)
    en, w = np.zeros((1, steps_n, mb, 2), np.float32), np.zeros((1, steps_n, mb), np.float32)
    eps = torch.randn(1, steps_n, mb, generator=g, dtype=torch.float64).numpy()
    denom, gv, stats_in, steps = np.ones(steps_n, np.float32), np.zeros(steps_n), np.zeros((steps_n, 2, 8), np.float32), []
    for s in range(steps_n):
        k = s % n_mb
        m, t = S["mbs"][k], S["terms"][k]
        n = m["w"].size
        en[0, s, :n, 0], en[0, s, :n, 1], w[0, s, :n], denom[s] = m["ego"], m["nei"], m["w"], m["denom"]
        en[0, s, n:] = 3.0 * torch.randn(mb - n, 2, generator=g).numpy()      # zero-weight slots hold values that must not be summed (eps too)
        gv[s] = float(np.dot(t["g_new"], t["g_old"])) * (1.0 + 0.25 * s) * (-1.0 if s % 5 == 3 else 1.0)
        stats_in[s, 0, 1], stats_in[s, 1, 1], stats_in[s, 0, 7] = t["new_loss"], t["old_loss"], t["global_adv"]
        steps.append(dict(gv=gv[s], ego=en[0, s, :n, 0], nei=en[0, s, :n, 1], eps=eps[0, s, :n], w=w[0, s, :n], denom=float(denom[s]),
                          new_loss=float(stats_in[s, 0, 1]), old_loss=float(stats_in[s, 1, 1]), global_adv=float(stats_in[s, 0, 7])))
    dev = [torch.as_tensor(x).cuda() for x in (en, w, eps, denom, gv, stats_in)]
    worst = 0.0
    for ci, pc in enumerate(MC.LCF_CASES):
        raw = MC.RAW_MEAN_STD[ci % 2]
        raw_t = torch.tensor(raw, dtype=torch.float64, device="cuda")
        want = M.meta_trajectory(pc, [0.0] * 5, raw, steps, lr)
        for n_wg in (1, 4):
            p = torch.tensor(pc, dtype=torch.float64, device="cuda")
            adam, st = torch.zeros(5, dtype=torch.float64, device="cuda"), torch.zeros(7, dtype=torch.float64, device="cuda")
            fz.fused.meta_batch_lcf(dict(denom_all=dev[3]), steps_n, None, dev[4], dev[5], p, raw_t, adam, lr, st, 0, 0,
                                    dense=(dev[0], dev[1], dev[2]), n_wg=n_wg)
            torch.cuda.synchronize()
            for got, exp, what in ((p, want[0], "lcf_param"), (adam, want[1], "adam"), (st, want[2], "stats")):
                worst = max(worst, _close(got.cpu().numpy(), exp, 1e-10, 1e-12, (name, pc, raw, n_wg, what)))
            assert float(adam[4]) == steps_n
    assert all(np.abs(en[0, s, int(denom[s]):]).min() > 0 and np.abs(eps[0, s, int(denom[s]):]).min() > 0 and not w[0, s, int(denom[s]):].any()
               for s in range(steps_n))
    print("\n[%s] meta_seq_kernel, 12 steps: worst error / (1e-10 |x| + 1e-12) = %.2e" % (name, worst))


def test_run_meta_end_to_end_against_the_model():
    """`run_meta(num_iters=2)` at the small shape, with the defaults (row store, LCF steps chunk by chunk on the side stream) and with
    `meta_batch_size=0` (one `copo_meta_step_f64` per minibatch), against `meta_trajectory` on the plans and eps draws of the run.
    Every link is held: each pass's dot products to their derived bound; the LCF parameters, Adam state and fp64 statistics of each
    run to 1e-10 against the model FED that run's dot products; and everything against the model fed the EXACT dot products, within twice the
    first-order effect of moving each step's dot product by its bound (computed from the model alone) -- so neither path can drift
    from the exact trajectory by more than the fp32 gradients' error allows."""
    S = _setup(MC.SMALL)
    case, tn, to, idx, B, clip = S["case"], S["tn"], S["to"], S["idx"], S["B"], S["clip"]
    mb, n_mb = case["mb"], S["n_mb"]
    pols = []
    for _ in range(2):                  # policies of this test alone: the case's cached pair, its plan and its LCF state stay as they are
        pol = _make("copo", "none", case["odim"], fused=True, hiddens=(case["hidden"],) * 2, mb=mb)
        _copy_weights(pol, S["fz"])
        pol.prepare_sgd(S["batch"], case["R"], mb)
        pol._raw_lcf_adv_mean.fill_(RAW[0])
        pol._raw_lcf_adv_std.fill_(RAW[1])
        pol.use_graphs = False
        pols.append(pol)
    a, b = pols
    b.config["meta_batch_size"] = 0
    p_init = a.model.lcf_parameters.detach().cpu().numpy().copy()
    assert not a._lcf_adam.any() and np.array_equal(p_init, b.model.lcf_parameters.detach().cpu().numpy())
    outs = []
    for pol in (a, b):
        torch.manual_seed(77)
        outs.append(pol.run_meta(idx, B, [B], mb, 2))
    torch.cuda.synchronize()
    ma = a._meta_bufs
    assert ma["pass_no"] == 2 and a._meta_row_store                 # two passes, one per set of planned tables
    assert torch.equal(b._meta_bufs["rows_all"][:n_mb], ma["sets"][1]["rows_all"][:n_mb])      # same seed, same plans in both modes
    assert torch.equal(b._meta_bufs["eps_all"][:n_mb], ma["sets"][1]["eps_all"][:n_mb])
    steps, bounds, gv_hip, gv_pair = [], [], [], []
    mbb, kk = b._meta_bufs, torch.zeros(1, dtype=torch.int64, device="cuda")
    for q in range(2):
        tabs = {k: ma["sets"][q][k][:n_mb].cpu().numpy() for k in ("rows_all", "w_all", "denom_all", "eps_all")}
        gv_hip += ma["gv2"][q][:n_mb].cpu().tolist()
        rs_q = dict(b._row_sources, k=kk, **{key: ma["sets"][q][key] for key in ("rows_all", "w_all", "denom_all")})
        for k in range(n_mb):
            # the dot product the step-by-step run took at this step: the same launch chain on the same plan again (fixed summation
            # orders: the same partials, test_fused_meta_single_call_equals_three_calls), its fp64 partials added up on the host
            kk.fill_(k)
            b.fused.meta_grads(rs_q, mbb["g_new"], mbb["g_old"], mbb["stats_new"], mbb["stats_old"], mbb["dot_partials"])
            gv_pair.append(float(mbb["dot_partials"][:case["fold_blocks"]].sum()))
            m = MC.minibatch(S["cols"], tabs["rows_all"][k], tabs["w_all"][k], tabs["denom_all"][k], tabs["eps_all"][k])
            t = M.policy_terms(tn, to, m["obs"], m["act"], m["old_logp"], m["glob_adv"], m["w"], m["denom"], clip)
            bounds.append(M.dot_bound(t["g_new"], t["g_old"], M.element_bounds(tn, t["g_new"], MC.GRAD_REL), M.element_bounds(to, t["g_old"], MC.GRAD_REL)))
            steps.append(dict(m, gv=float(np.dot(t["g_new"], t["g_old"])), **{k: t[k] for k in ("new_loss", "old_loss", "global_adv", "abs_new", "abs_old", "abs_adv")}))
    n = len(steps)
    lr = float(a.config["lcf_lr"])
    for k in range(n):
        for gvk in (gv_hip[k], gv_pair[k]):
            assert abs(gvk - steps[k]["gv"]) <= bounds[k], (k, gvk, steps[k]["gv"], bounds[k])

    def flat(tr):
        return np.array([float(x) for x in tr[0] + tr[1] + tr[2]])

    exact = flat(M.meta_trajectory(p_init, [0.0] * 5, RAW, steps, lr))
    fed = [flat(M.meta_trajectory(p_init, [0.0] * 5, RAW, [dict(s, gv=g) for s, g in zip(steps, gvs)], lr)) for gvs in (gv_hip, gv_pair)]
    allowed = np.zeros_like(exact)
    for k in range(n):
        moved = [dict(s, gv=s["gv"] + (bounds[k] if j == k else 0.0)) for j, s in enumerate(steps)]
        allowed += 2.0 * np.abs(flat(M.meta_trajectory(p_init, [0.0] * 5, RAW, moved, lr)) - exact)
    allowed += 1e-10 * np.abs(exact) + 1e-12
    # the three statistics that are fp32 sums of the policy half: 1e-5 of their terms' size per step
    for j, key in ((7, "abs_new"), (8, "abs_old"), (13, "abs_adv")):
        allowed[j] += 1e-5 * sum(s[key] for s in steps) + 1e-9
    keys = a.META_KEYS
    for pol, out, which in ((a, outs[0], "row store"), (b, outs[1], "step by step")):
        got = np.concatenate([pol.model.lcf_parameters.detach().cpu().numpy(), pol._lcf_adam.cpu().numpy(), np.array([out[k] for k in keys]) * n])
        assert got[6] == float(n)                                        # the Adam step count
        err = np.abs(got - exact)
        print("\n[%s] run_meta (%s): LCF parameters %s, error / allowed: parameters %.2e, Adam %.2e, statistics %.2e" % (
            MC.SMALL, which, got[:2].tolist(), (err[:2] / allowed[:2]).max(), (err[2:6] / allowed[2:6]).max(), (err[7:] / allowed[7:]).max()))
        assert np.all(err <= allowed), (which, got.tolist(), exact.tolist(), (err / allowed).tolist())
        assert np.all(got[:2] != p_init)                                  # both parameters moved
    # each run against the model fed ITS OWN dot products: the fp64 chain alone, what meta_finish / meta_seq_kernel make of the partials
    # they consume (the fp32 statistics excepted)
    for pol, out, fed_own in ((a, outs[0], fed[0]), (b, outs[1], fed[1])):
        got = np.concatenate([pol.model.lcf_parameters.detach().cpu().numpy(), pol._lcf_adam.cpu().numpy(), np.array([out[k] for k in keys]) * n])
        for j in list(range(7)) + [9, 10, 11, 12]:
            assert abs(got[j] - fed_own[j]) <= 1e-10 * abs(fed_own[j]) + 1e-12, (j, got[j], fed_own[j])
