"""A float64 model of ONE minibatch of the PPO step, written from the torch statement of the step
(IPPOPolicy.loss / CCPPOPolicy.loss / CoPOPolicy.loss, clipped_value_loss, TorchDiagGaussian's logp / entropy / kl) -- it calls none
of them and shares no expression with the kernels.  The gradients are torch autograd on this restatement.

  theta   what `theta_of_nets` returns: per net (policy first, then the value nets in the kernels' order: ego, neighbour, global) the
          three (weight, bias) pairs as float64 CPU tensors
  mbatch  one minibatch, the rows with w > 0 of the planned tables (`ppo_cases.minibatch`): obs, cc (the critics' input), act,
          old_logp, dist (the [mean | log_std] of the behaviour policy), adv, vpred / vtarget (one column per value head), w, denom
  conf    clip, vf_clip, old_value_loss, vf_coeff, ent_coeff, kl_coeff (0.0: the step has no KL term at all)

`step` returns every parameter gradient per tensor, the eight statistics in the order of `FusedLearner.stats` (total, policy,
vf_ego, kl, entropy, vf_nei, vf_glob, adv), per statistic the mean of the ABSOLUTE row terms (the size an fp32 sum of the terms is
accurate relative to), per net the sum of the absolute row terms of its head-bias gradient (`head_abs`) and the per-row quantities
the branch conditions are stated on."""
import math

import numpy as np
import torch

STAT_NAMES = ("total", "policy", "vf_ego", "kl", "entropy", "vf_nei", "vf_glob", "adv")
TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3")
# the ways a step can be wrong that test_ppo_cpu.py shows the referee would notice
MUTANTS = ("no_entropy", "no_kl", "clip_wrong_side", "max_for_min", "no_value_clamp", "denominator_mb", "nei_gets_ego_targets")


def theta_of_nets(nets):
    """nets: per net its three nn.Linear (layer 1, layer 2, head)."""
    return [[(lin.weight.detach().double().cpu().clone(), lin.bias.detach().double().cpu().clone()) for lin in net] for net in nets]


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def mlp(layers, x, pre=None):
    """tanh(x W1' + b1) -> tanh(. W2' + b2) -> . W3' + b3; `pre` (a list) receives the layer-1 pre-activations."""
    z1 = x @ layers[0][0].t() + layers[0][1]
    if pre is not None:
        pre.append(z1.detach())
    h2 = torch.tanh(torch.tanh(z1) @ layers[1][0].t() + layers[1][1])
    return h2 @ layers[2][0].t() + layers[2][1]


def gaussian_logp(mean, log_std, x):
    z = (x - mean) * torch.exp(-log_std)
    return (-0.5 * z * z - log_std).sum(1) - 0.5 * x.shape[1] * math.log(2.0 * math.pi)


def gaussian_entropy(log_std):
    return log_std.sum(1) + 0.5 * log_std.shape[1] * (1.0 + math.log(2.0 * math.pi))


def gaussian_kl(mean_p, log_std_p, mean_q, log_std_q):
    """KL(p || q) of two diagonal Gaussians."""
    var_p, var_q = torch.exp(2.0 * log_std_p), torch.exp(2.0 * log_std_q)
    return (log_std_q - log_std_p + (var_p + (mean_p - mean_q) ** 2) / (2.0 * var_q) - 0.5).sum(1)


def value_loss(v, v_prev, target, c, old_form, clamp=True):
    """old form: max((v - T)^2, (v_prev + clip(v - v_prev, +-c) - T)^2); new form: clip((v - T)^2, 0, c).  Returns (loss, the unclipped
    square, the clipped square or None)."""
    l1 = (v - target) ** 2
    if old_form:
        l2 = (v_prev + torch.clamp(v - v_prev, -c, c) - target) ** 2
        return (torch.maximum(l1, l2) if clamp else l1), l1, l2
    return (torch.clamp(l1, 0.0, c) if clamp else l1), l1, None


def step(theta, mbatch, conf, dtype=torch.float64, grads=True, mutant=None):
    """One minibatch.  `dtype=torch.float32` evaluates the same statement in fp32 on the host: the yardstick `e_t32` of the referee.
    `mutant`: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    t = lambda x: _t(x, dtype)  # noqa: E731
    layers = [[(w.to(dtype).clone().requires_grad_(grads), b.to(dtype).clone().requires_grad_(grads)) for w, b in net] for net in theta]
    obs, cc, act, old_logp, dist, adv, w = (t(mbatch[k]) for k in ("obs", "cc", "act", "old_logp", "dist", "adv", "w"))
    vpred, vtarget = t(mbatch["vpred"]), t(mbatch["vtarget"])
    n_heads = len(theta) - 1
    assert vpred.shape[1] == vtarget.shape[1] == n_heads
    denom = float(mbatch["mb"]) if mutant == "denominator_mb" else float(mbatch["denom"])
    clip, c, k = float(conf["clip"]), float(conf["vf_clip"]), float(conf["vf_coeff"])
    ent_c = 0.0 if mutant == "no_entropy" else float(conf["ent_coeff"])
    kl_c = 0.0 if mutant == "no_kl" else float(conf["kl_coeff"])
    use_kl = float(conf["kl_coeff"]) > 0.0
    mean = lambda x: (x * w).sum() / denom  # noqa: E731
    pre = []
    out = mlp(layers[0], obs, pre)
    na = act.shape[1]
    mu, log_std = out[:, :na], out[:, na:]
    logp = gaussian_logp(mu, log_std, act)
    ratio = torch.exp(logp - old_logp)
    clipped = torch.clamp(ratio, 1.0 + clip, 1.0 + 2.0 * clip) if mutant == "clip_wrong_side" else torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    a, b = adv * ratio, adv * clipped
    surrogate = torch.maximum(a, b) if mutant == "max_for_min" else torch.minimum(a, b)
    entropy = gaussian_entropy(log_std)
    kl = gaussian_kl(dist[:, :na], dist[:, na:], mu, log_std) if use_kl else torch.zeros_like(logp)
    row_total = -surrogate - ent_c * entropy + kl_c * kl
    vf, values, squares, outs = [], [], [], [out]
    for g in range(n_heads):
        outs.append(mlp(layers[1 + g], cc, pre))
        v = outs[-1].reshape(-1)
        tgt = vtarget[:, 0] if (mutant == "nei_gets_ego_targets" and g == 1) else vtarget[:, g]
        l, l1, l2 = value_loss(v, vpred[:, g], tgt, c, bool(conf["old_value_loss"]), clamp=mutant != "no_value_clamp")
        vf.append(l)
        values.append(v.detach())
        squares.append((l1.detach(), None if l2 is None else l2.detach()))
        row_total = row_total + k * l
    total = mean(row_total)
    zero = torch.zeros_like(logp)
    rows = [row_total, -surrogate, vf[0], kl, entropy, vf[1] if n_heads > 1 else zero, vf[2] if n_heads > 2 else zero, adv]
    f = lambda x: float(x.detach())  # noqa: E731
    res = dict(stats=np.array([f(mean(r)) for r in rows]), scales=np.array([f(mean(r.abs())) for r in rows]),
               logp=logp.detach().numpy(), ratio=ratio.detach().numpy(), values=[v.numpy() for v in values],
               squares=[(l1.numpy(), None if l2 is None else l2.numpy()) for l1, l2 in squares], pre1=[p.numpy() for p in pre])
    if grads:
        flat = [x for net in layers for pair in net for x in pair]
        got = torch.autograd.grad(total, flat + outs, allow_unused=True)
        # b3 of a net is the sum over the rows of d total / d (head output): `head_abs` is the sum of the ABSOLUTE row terms, what the
        # largest element of a b3 gradient falls short of when its terms cancel
        res["head_abs"] = [g_.abs().sum(0).double().numpy() for g_ in got[len(flat):]]
        res["grads"] = [{name: (torch.zeros_like(p) if g_ is None else g_).double().numpy() for name, p, g_ in
                         zip(TENSORS, flat[6 * i:6 * i + 6], got[6 * i:6 * i + 6])} for i in range(len(layers))]
    return res


def forward_rows(theta, obs, cc, act):
    """(logp, [v per head]) of ALL rows in float64 under the current weights: what the crafted columns are built from."""
    with torch.no_grad():
        layers = theta
        out = mlp(layers[0], _t(obs, torch.float64))
        na = act.shape[1]
        logp = gaussian_logp(out[:, :na], out[:, na:], _t(act, torch.float64)).numpy()
        vals = [mlp(net, _t(cc, torch.float64)).reshape(-1).numpy() for net in layers[1:]]
    return logp, vals
