"""The learner's Adam update restated in numpy: the formula that `wgrad_adam_kernel`, `adam_flat_kernel` and `reduce_adam_kernel`
(csrc/learn_update.inc) state, evaluated operation for operation in float64 (the reference) or in float32 (a plain evaluation whose own
error the tests measure and from which they take the kernels' limit).

    m' = m + (g - m) (1 - beta1)
    v' = v beta2 + g g (1 - beta2)
    theta' = theta - (lr / (1 - beta1^t)) * (m' / (sqrt(v') / sqrt(1 - beta2^t) + eps))

The hyper-parameters are the values AS STORED in `copo_ppo_cfg` (fp32 fields): `stored(x)` is that value widened to float64, so that the
comparison is one of arithmetic alone and not of 0.9 against fp32(0.9).

Errors are reported in units of u = 2^-24 (half an fp32 ulp, relative) against what the inputs allow:
  e_m      |m - m64| / (|m_in| + |g|)                     m' is a difference of the two: relative to m' itself the error is unbounded
  e_v      |v - v64| / v64                                a sum of non-negative terms
  e_theta  |theta - theta64| / (kappa(t) |step64| + |theta64|),  step64 = theta64 - theta_in
kappa(t) = 1 + beta1^t / (1 - beta1^t) + (1 / 2) beta2^t / (1 - beta2^t) is the condition number of the step size with respect to the two
bias corrections: a relative error d in beta^t moves 1 - beta^t by d beta^t / (1 - beta^t), and the second correction enters through a
square root.  509.5 at t = 1, 254.9 at t = 2, 1.3 at t = 1000, 1.0 at t = 200 000 (beta1 = 0.9, beta2 = 0.999).  An element whose
denominator is zero must match exactly: it reports 0 when it does and infinity when it does not."""
import numpy as np

U = 2.0 ** -24
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8          # what FusedLearner writes into copo_ppo_cfg
MAGNITUDES = (0.0, 1e-12, 1e-8, 1e-4, 1.0, 1e3)
STEPS = (1, 2, 10, 1000, 200000)


def stored(x):
    """An fp32 struct field read back: the fp32 value, widened to float64."""
    return float(np.float32(x))


def adam_step(theta, m, v, g, t, lr, beta1, beta2, eps, dtype=np.float64):
    """(theta', m', v') of Adam step number t (>= 1), every operation rounded to `dtype`."""
    dt = np.dtype(dtype).type
    theta, m, v, g = (np.asarray(a).astype(dt) for a in (theta, m, v, g))
    lr, beta1, beta2, eps, one, tt = dt(lr), dt(beta1), dt(beta2), dt(eps), dt(1), dt(t)
    bc1 = one - np.power(beta1, tt)
    bc2s = np.sqrt(one - np.power(beta2, tt))
    m2 = m + (g - m) * (one - beta1)
    v2 = v * beta2 + g * g * (one - beta2)
    theta2 = theta - (lr / bc1) * (m2 / (np.sqrt(v2) / bc2s + eps))
    assert theta2.dtype == dt and m2.dtype == dt and v2.dtype == dt
    return theta2, m2, v2


def kappa(t, beta1=BETA1, beta2=BETA2):
    b1, b2 = stored(beta1) ** float(t), stored(beta2) ** float(t)
    return 1.0 + b1 / (1.0 - b1) + 0.5 * b2 / (1.0 - b2)


def _ratio(err, den):
    out = np.zeros_like(err)
    pos = den > 0.0
    out[pos] = err[pos] / den[pos]
    out[~pos & (err != 0.0)] = np.inf
    return out / U


def elementwise_errors(got, want64, inputs):
    """The three normalised errors of every element, in units of 2^-24.  got, want64: (theta, m, v) after the step; inputs: dict of
    theta, m, v, g before it and the step number t (and optionally beta1 / beta2 as stored)."""
    th, m, v = (np.asarray(a, np.float64) for a in got)
    th64, m64, v64 = (np.asarray(a, np.float64) for a in want64)
    th_in, m_in, g_in = (np.asarray(inputs[k], np.float64) for k in ("theta", "m", "g"))
    k = kappa(inputs["t"], inputs.get("beta1", BETA1), inputs.get("beta2", BETA2))
    e_m = _ratio(np.abs(m - m64), np.abs(m_in) + np.abs(g_in))
    e_v = _ratio(np.abs(v - v64), v64)
    e_th = _ratio(np.abs(th - th64), k * np.abs(th64 - th_in) + np.abs(th64))
    return e_m, e_v, e_th


def normalised_errors(got, want64, inputs):
    """(e_m, e_v, e_theta): the largest element of each, in units of 2^-24."""
    return tuple(float(e.max()) if e.size else 0.0 for e in elementwise_errors(got, want64, inputs))


def make_inputs(rng, n):
    """dict(theta, m, v, g) of n fp32 elements each: g = N(0, 1) x a magnitude drawn from MAGNITUDES (exact zeros, the eps-dominated
    regime, large gradients; g g (1 - beta2) stays a normal fp32 number), m = N(0, 1e-3) or exactly 0 with probability 0.3,
    v = N(0, 1e-3)^2 or exactly 0 with probability 0.3, theta = N(0, 0.1)."""
    f32 = np.float32
    g = (rng.standard_normal(n) * np.asarray(MAGNITUDES)[rng.integers(0, len(MAGNITUDES), n)]).astype(f32)
    m = (rng.standard_normal(n) * 1e-3 * (rng.random(n) >= 0.3)).astype(f32)
    v = ((rng.standard_normal(n) * 1e-3) ** 2 * (rng.random(n) >= 0.3)).astype(f32)
    theta = (rng.standard_normal(n) * 0.1).astype(f32)
    sq = g.astype(np.float64) ** 2 * (1.0 - stored(BETA2))
    assert np.all((sq == 0.0) | (sq > 2.0 ** -126)), "the generator must not reach fp32 subnormals"
    return dict(theta=theta, m=m, v=v, g=g)
