"""A float64 / 40-digit model of ONE step of the LCF meta update, written from the torch statement of the
step (CoPOPolicy._meta_pieces / _meta_finish, CoPOModel.compute_coordinated / lcf_mean / lcf_std) and SPEC.md -- not from the
kernels, with which it shares no expression.

  policy_grads     the two policy gradients, torch autograd in float64 on the CPU, in the layout of `meta_fold_len()` / `g_out`
  lcf_terms        dS/dp0, dS/dp1, S, mean(A') in mpmath at 40 digits (the kernels are fp64: a numpy float64 model could not tell a
                   wrong kernel from a differently rounded one)
  lcf_adam         torch.optim.Adam's step on the two LCF scalars, in mpmath
  meta_trajectory  the pieces chained over n minibatches: parameters, Adam state, the seven accumulated statistics

`theta` is what `theta_of` returns: the three (weight, bias) pairs of a policy net as float64 tensors, their offsets in the flat
parameter buffer and the length of the span they occupy."""
import math

import mpmath as mp
import numpy as np
import torch

DIGITS = 40
LIM = 1 - 1e-6                  # the float64 number torch.clamp(tanh(p0), -1 + 1e-6, 1 - 1e-6) clamps to


def theta_of(linears, offset_of):
    """linears: the three nn.Linear of a policy net (layer 1, layer 2, head); offset_of(parameter) -> its offset in the flat buffer
    (FlatParams.offset[id(p)]).  Offsets are taken relative to the first one, the fold's `lo`."""
    lo = min(offset_of(p) for lin in linears for p in (lin.weight, lin.bias))
    layers = [(lin.weight.detach().double().cpu().clone(), lin.bias.detach().double().cpu().clone()) for lin in linears]
    offsets = [(offset_of(lin.weight) - lo, offset_of(lin.bias) - lo) for lin in linears]
    n = max(o + t.numel() for (w, b), (ow, ob) in zip(layers, offsets) for o, t in ((ow, w), (ob, b)))
    return dict(layers=layers, offsets=offsets, n=n)


def tensors_of(theta):
    """[(name, first element, one past the last)] of the six tensors inside the flat layout."""
    out = []
    for i, ((w, b), (ow, ob)) in enumerate(zip(theta["layers"], theta["offsets"])):
        out += [("w%d" % (i + 1), ow, ow + w.numel()), ("b%d" % (i + 1), ob, ob + b.numel())]
    return out


def _t(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64)


def log_prob(layers, obs, act):
    """log N(act; mean, exp(log_std)^2) of the tanh MLP's diagonal Gaussian, head output = [mean (2) | log_std (2)]."""
    h = obs
    for w, b in layers[:-1]:
        h = torch.tanh(torch.addmm(b, h, w.t()))
    out = torch.addmm(layers[-1][1], h, layers[-1][0].t())
    k = act.shape[1]
    mu, log_std = out[:, :k], out[:, k:]
    z = (act - mu) * torch.exp(-log_std)
    return -0.5 * (z * z).sum(1) - log_std.sum(1) - 0.5 * k * math.log(2.0 * math.pi)


def _flat_grads(theta, loss, leaves):
    grads = torch.autograd.grad(loss, [t for pair in leaves for t in pair])
    g = np.zeros(theta["n"])
    for i, (ow, ob) in enumerate(theta["offsets"]):
        gw, gb = grads[2 * i], grads[2 * i + 1]
        g[ow:ow + gw.numel()] = gw.reshape(-1).numpy()
        g[ob:ob + gb.numel()] = gb.reshape(-1).numpy()
    return g


def policy_terms(theta_new, theta_old, obs, act, old_logp, glob_adv, w, denom, clip, grads=True):
    """Everything of the policy half of a meta step for the rows given (padding rows may be passed with w = 0): a dict with `g_new`,
    `g_old` (float64, fold layout), the two losses, mean global advantage, the per-row `ratio` and the per-row absolute terms
    `abs_new` / `abs_old` / `abs_adv` (sum_i w_i |term_i| / denom: what an fp32 sum of the terms is accurate relative to)."""
    obs, act, old_logp, adv, w = _t(obs), _t(act), _t(old_logp).reshape(-1), _t(glob_adv).reshape(-1), _t(w).reshape(-1)
    denom = float(denom)
    new = [(a.clone().requires_grad_(grads), b.clone().requires_grad_(grads)) for a, b in theta_new["layers"]]
    old = [(a.clone().requires_grad_(grads), b.clone().requires_grad_(grads)) for a, b in theta_old["layers"]]
    ratio = torch.exp(log_prob(new, obs, act) - old_logp)
    unclipped, clipped = adv * ratio, adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surrogate = torch.where(unclipped <= clipped, unclipped, clipped)
    new_loss = (w * -surrogate).sum() / denom
    lp_old = log_prob(old, obs, act)
    old_loss = (w * lp_old).sum() / denom
    f = lambda x: float(x.detach())  # noqa: E731
    out = dict(new_loss=f(new_loss), old_loss=f(old_loss), global_adv=f((w * adv).sum() / denom), ratio=ratio.detach().numpy(),
               abs_new=f((w * surrogate.abs()).sum() / denom), abs_old=f((w * lp_old.abs()).sum() / denom),
               abs_adv=f((w * adv.abs()).sum() / denom))
    if grads:
        out["g_new"] = _flat_grads(theta_new, new_loss, new)
        out["g_old"] = _flat_grads(theta_old, old_loss, old)
    return out


def policy_grads(theta_new, theta_old, obs, act, old_logp, glob_adv, w, denom, clip):
    """g_new = d/dtheta sum_i w_i * -min(A r, A clip(r)) / denom through the current policy, g_old = d/dtheta' sum_i w_i logp'_i / denom
    through the target policy."""
    t = policy_terms(theta_new, theta_old, obs, act, old_logp, glob_adv, w, denom, clip)
    return t["g_new"], t["g_old"]


def _mpf(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def lcf_terms(p, raw_mean_std, ego, nei, eps, w, denom):
    """(dS/dp0, dS/dp1, S, mean A') as mpf, for S = sum_i w_i (A'_i - mu) / sigma / denom, A' = cos(phi) A_ego + sin(phi) A_nei,
    phi = (m + s eps) pi / 2, m = clamp(tanh p0, -LIM, LIM), s = exp(clamp(p1, -20, 2)).  torch.clamp passes the gradient where the
    input lies inside the CLOSED interval (tests/test_meta_cpu.py holds torch to that), so a derivative is exactly 0 outside it."""
    with mp.workdps(DIGITS):
        p0, p1 = _mpf(p[0]), _mpf(p[1])
        mu, sigma, D = _mpf(raw_mean_std[0]), _mpf(raw_mean_std[1]), _mpf(denom)
        lim = mp.mpf(LIM)
        th = mp.tanh(p0)
        inside0 = -lim <= th <= lim
        m = th if inside0 else (lim if th > lim else -lim)
        dm = (1 - th * th) if inside0 else mp.mpf(0)
        inside1 = -20 <= p1 <= 2
        s = mp.exp(p1 if inside1 else (mp.mpf(2) if p1 > 2 else mp.mpf(-20)))
        ds = s if inside1 else mp.mpf(0)
        half_pi = mp.pi / 2
        sum_a = sum_da = sum_dae = sum_w = mp.mpf(0)
        for a_e, a_n, e, wi in zip(np.asarray(ego, np.float64).reshape(-1), np.asarray(nei, np.float64).reshape(-1),
                                   np.asarray(eps, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)):
            if wi == 0.0:
                continue
            a_e, a_n, e, wi = mp.mpf(float(a_e)), mp.mpf(float(a_n)), mp.mpf(float(e)), mp.mpf(float(wi))
            c, sn = mp.cos_sin((m + s * e) * half_pi)
            da = (c * a_n - sn * a_e) * half_pi          # dA'/d(m + s eps)
            sum_a += wi * (c * a_e + sn * a_n)
            sum_da += wi * da
            sum_dae += wi * da * e
            sum_w += wi
        return (sum_da * dm / sigma / D, sum_dae * ds / sigma / D, (sum_a - mu * sum_w) / sigma / D, sum_a / D)


def lcf_terms_float64(p, raw_mean_std, ego, nei, eps, w, denom):
    """The same formulas in numpy float64 (libm sin / cos of phi): what a correct fp64 evaluation shows against `lcf_terms`."""
    p0, p1 = float(p[0]), float(p[1])
    mu, sigma = float(raw_mean_std[0]), float(raw_mean_std[1])
    th = math.tanh(p0)
    m = min(max(th, -LIM), LIM)
    dm = (1.0 - th * th) if -LIM <= th <= LIM else 0.0
    s = math.exp(min(max(p1, -20.0), 2.0))
    ds = s if -20.0 <= p1 <= 2.0 else 0.0
    ego, nei, eps, w = (np.asarray(x, np.float64).reshape(-1) for x in (ego, nei, eps, w))
    phi = (m + s * eps) * (np.pi / 2)
    a = np.cos(phi) * ego + np.sin(phi) * nei
    da = (np.cos(phi) * nei - np.sin(phi) * ego) * (np.pi / 2)
    D = float(denom)
    return (float(np.sum(w * da) * dm / sigma / D), float(np.sum(w * da * eps) * ds / sigma / D),
            float(np.sum(w * (a - mu) / sigma) / D), float(np.sum(w * a) / D))


def lcf_adam(p, adam, g, lr):
    """One torch.optim.Adam step (betas 0.9 / 0.999, eps 1e-8, bias-corrected, no weight decay) on the two scalars.
    adam = [m0, m1, v0, v1, step]; returns the new (p, adam) as lists of mpf."""
    with mp.workdps(DIGITS):
        b1, b2, eps = mp.mpf(0.9), mp.mpf(0.999), mp.mpf(1e-8)
        t = _mpf(adam[4]) + 1
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        p_out, m_out, v_out = [], [], []
        for j in range(2):
            gj = _mpf(g[j])
            m = b1 * _mpf(adam[j]) + (1 - b1) * gj
            v = b2 * _mpf(adam[2 + j]) + (1 - b2) * gj * gj
            p_out.append(_mpf(p[j]) - (_mpf(lr) / bc1) * m / (mp.sqrt(v) / mp.sqrt(bc2) + eps))
            m_out.append(m)
            v_out.append(v)
        return p_out, m_out + v_out + [t]


def meta_trajectory(p, adam, raw_mean_std, steps, lr):
    """`steps`: one dict per minibatch, in order, with gv, ego, nei, eps, w, denom and the three statistics of the policy half
    (new_loss, old_loss, global_adv).  Returns (p, adam, stats): stats = the sums over the steps of [new_loss, old_loss, S, gv S, gv,
    mean A', mean global advantage], the layout of MetaFinishArgs::stats (run_meta reports them divided by the step count)."""
    with mp.workdps(DIGITS):
        p, adam = [_mpf(x) for x in p], [_mpf(x) for x in adam]
        stats = [mp.mpf(0)] * 7
        for st in steps:
            d0, d1, S, mean_a = lcf_terms(p, raw_mean_std, st["ego"], st["nei"], st["eps"], st["w"], st["denom"])
            gv = _mpf(st["gv"])
            add = [_mpf(st.get("new_loss", 0.0)), _mpf(st.get("old_loss", 0.0)), S, gv * S, gv, mean_a, _mpf(st.get("global_adv", 0.0))]
            stats = [a + b for a, b in zip(stats, add)]
            p, adam = lcf_adam(p, adam, [gv * d0, gv * d1], lr)
        return p, adam, stats


def dot_bound(g_new, g_old, e_new, e_old):
    """|<a, b> - <g_new, g_old>| for any a, b with |a_i - g_new_i| <= e_new_i and |b_i - g_old_i| <= e_old_i, the dot product of a and
    b taken in float64 in any order: sum_i (e_new_i |g_old_i| + e_old_i |g_new_i| + e_new_i e_old_i) plus n 2^-53 sum_i |a_i b_i|
    for the summation (the products of two fp32 numbers are exact in fp64).  e_*: arrays (per element) or scalars."""
    gn, go = np.abs(np.asarray(g_new, np.float64)), np.abs(np.asarray(g_old, np.float64))
    first = float(np.sum(e_new * go + e_old * gn + e_new * e_old * np.ones_like(gn)))
    return first + gn.size * 2.0 ** -53 * float(np.sum((gn + e_new) * (go + e_old)))


def element_bounds(theta, g, rel):
    """Per element: `rel` x the largest element of the tensor the element belongs to (how the gradient comparisons are stated)."""
    e = np.zeros(theta["n"])
    for _name, a, b in tensors_of(theta):
        e[a:b] = rel * float(np.abs(g[a:b]).max())
    return e
