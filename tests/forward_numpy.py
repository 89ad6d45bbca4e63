"""The float64 model of the forward-only kernel (mlp_fwd_kernel, csrc/learn_rowpass.inc) and its fp32 yardstick: one net, the sampling
epilogue, the clip, and the kernel's tanh formula in numpy fp32.  No GPU and no native library is touched."""
import numpy as np

import adversary_cases as ac

LOG_2PI = float(np.log(2.0 * np.pi))
F = np.float32


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def forward64(weights, x):
    """[n][out] float64: W3 tanh(W2 tanh(W1 x + b1) + b2) + b3 of one net in the torch key layout on the rows of x."""
    W1, b1, W2, b2, W3, b3 = ac.net_of(weights)
    h1 = np.tanh(np.asarray(x, np.float64) @ W1.T + b1)
    return np.tanh(h1 @ W2.T + b2) @ W3.T + b3


def sample64(dist_inputs, eps):
    """(action [n][2], logp [n]) of TorchDiagGaussian on [mean | log_std]: mean + exp(log_std) eps, and its `logp` of that action."""
    d, eps = np.asarray(dist_inputs, np.float64), np.asarray(eps, np.float64)
    mean, log_std = d[:, :2], d[:, 2:]
    std = np.exp(log_std)
    action = mean + std * eps
    z = (action - mean) / std
    return action, (-0.5 * z * z - log_std - 0.5 * LOG_2PI).sum(-1)


def clip64(action):
    return np.clip(np.asarray(action, np.float64), -1.0, 1.0)


# ---- the fp32 yardstick: the same three functions through torch fp32 on the CPU ----------------------------------------------------------
def forward32(weights, x):
    import torch
    W1, b1, W2, b2, W3, b3 = (torch.from_numpy(a) for a in ac.net_of(weights, np.float32))
    h1 = torch.tanh(torch.from_numpy(np.ascontiguousarray(x, F)) @ W1.T + b1)
    return (torch.tanh(h1 @ W2.T + b2) @ W3.T + b3).numpy()


def sample32(dist_inputs, eps):
    import torch
    d, eps = torch.from_numpy(np.ascontiguousarray(dist_inputs, F)), torch.from_numpy(np.ascontiguousarray(eps, F))
    mean, log_std = torch.chunk(d, 2, dim=-1)
    std = torch.exp(log_std)
    action = mean + std * eps
    z = (action - mean) / std
    return action.numpy(), (-0.5 * z * z - log_std - 0.5 * LOG_2PI).sum(-1).numpy()


def clip32(action):
    import torch
    return torch.from_numpy(np.ascontiguousarray(action, F)).clamp(-1.0, 1.0).numpy()


def deviation(x32, x64):
    """max |x32 - x64| / max(1, |x64|), element by element: how far one fp32 evaluation lies from the float64 model."""
    x64 = np.asarray(x64, np.float64)
    if x64.size == 0:
        return 0.0
    return float((np.abs(np.asarray(x32, np.float64) - x64) / np.maximum(1.0, np.abs(x64))).max())


# ---- tanh_fast (csrc/learn_gemm.inc) ---------------------------------------------------------------------------------------------------------
def tanh_fast_formula32(x):
    """The kernel's formula, every operation rounded to fp32, with numpy's correctly rounded exp and division in the place of the
    hardware's __expf and __frcp_rn: the odd polynomial below |x| = 0.3, 1 - 2 / (exp(2 x) + 1) from there on."""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", under="ignore"):
        x2 = x * x
        p = x * (F(1.0) + x2 * (F(-0.33333334) + x2 * (F(0.13333334) + x2 * (F(-0.053968254) + x2 * F(0.021869488)))))
        # exp in float64, rounded once to fp32, is the correctly rounded fp32 exp (double rounding aside: 2^-29 of the cases)
        e = np.exp((F(2.0) * x).astype(np.float64)).astype(F)
        r = F(1.0) - F(2.0) * (F(1.0) / (e + F(1.0)))
    out = np.where(np.abs(x) < F(0.3), p, r)
    assert out.dtype == F
    return out
