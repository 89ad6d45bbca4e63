"""The Adam reference of tests/adam_numpy.py is itself pinned: its float64 evaluation to torch.optim.Adam in float64, and its float32
evaluation -- from whose error the GPU tests take the kernels' limit -- to a bound in units of 2^-24 on the shared input generator."""
import numpy as np
import pytest
import torch

import adam_numpy as an

B1, B2, EPS = an.stored(an.BETA1), an.stored(an.BETA2), an.stored(an.EPS)


@pytest.mark.parametrize("t0", [0, 999], ids=["fresh_state_t1", "loaded_state_t999"])
def test_float64_adam_step_equals_torch_adam_in_float64(t0):
    """Five consecutive steps of torch.optim.Adam, from a fresh optimiser (first step t = 1) and from a state loaded at step 999 with
    generator-filled moments (first step t = 1000); every step is compared with `adam_step` applied to the state torch held in front
    of it: 1e-14 relative, element by element -- relative to what each quantity is a sum of (|m_in| + |g| for m, |theta| + |step| for
    theta; v is a sum of non-negative terms), because relative to a cancelled result no bound holds (and two trajectories that each
    carried their own state would inherit such a cancelled element's error in the next step)."""
    n, lr = 4096, an.stored(5e-5)
    rng = np.random.default_rng(7)
    x = an.make_inputs(rng, n)
    th, m, v = (x[k].astype(np.float64) for k in ("theta", "m", "v"))
    if t0 == 0:
        m, v = np.zeros(n), np.zeros(n)
    p = torch.nn.Parameter(torch.from_numpy(th.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=0.0, amsgrad=False, foreach=False)
    if t0:
        opt.state[p] = dict(step=torch.tensor(float(t0)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    for i in range(5):
        g = an.make_inputs(rng, n)["g"].astype(np.float64)
        p.grad = torch.from_numpy(g.copy())
        th_in, m_in = th, m
        opt.step()
        th, m, v = an.adam_step(th_in, m_in, v, g, t0 + 1 + i, lr, B1, B2, EPS, np.float64)
        st = opt.state[p]
        assert float(st["step"]) == t0 + 1 + i
        th_t, m_t, v_t = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        assert th_t.dtype == np.float64 and th.dtype == np.float64
        for name, a, b, den in (("m", m, m_t, np.abs(m_in) + np.abs(g)), ("v", v, v_t, v_t),
                                ("theta", th, th_t, np.abs(th_t) + np.abs(th_t - th_in))):
            bad = np.flatnonzero(np.abs(a - b) > 1e-14 * den)
            assert bad.size == 0, ("step %d: %s differs in %d elements, first at %d: %r != %r" % (t0 + 1 + i, name, bad.size, bad[0], a[bad[0]], b[bad[0]]))
        th, m, v = th_t.copy(), m_t.copy(), v_t.copy()
        assert np.abs(th - th_in).max() > 0.5 * lr          # (the steps are real: Adam moves the largest element by ~lr)


def test_kappa_values():
    np.testing.assert_allclose([an.kappa(t) for t in (1, 2, 1000, 200000)], [509.5, 254.9, 1.3, 1.0], rtol=0, atol=0.06)


def test_normalised_errors_units_and_zero_denominators():
    x = dict(theta=np.array([1.0, 0.0, 0.0]), m=np.array([1.0, 0.0, 0.0]), v=np.zeros(3), g=np.array([1.0, 0.0, 0.0]), t=200000)
    want = (np.array([0.5, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]))
    assert an.normalised_errors(want, want, x) == (0.0, 0.0, 0.0)
    got = (want[0] * (1 + 3 * an.U), want[1] * (1 + 5 * an.U), want[2] * (1 + 7 * an.U))
    e_m, e_v, e_th = an.normalised_errors(got, want, x)
    # theta: |step64| = 0.5, kappa = 1, |theta64| = 0.5 -> the denominator is 1, the error 1.5 u
    np.testing.assert_allclose([e_m, e_v, e_th], [5.0, 7.0, 1.5], rtol=1e-6)
    # an element with nothing to be relative to (g = m = v = theta = 0) must match exactly
    off = (want[0].copy(), want[1].copy(), want[2].copy())
    off[0][2] = 1e-30
    assert an.normalised_errors(off, want, x)[2] == np.inf


@pytest.mark.parametrize("lr", [5e-5, 3e-4])
@pytest.mark.parametrize("t", an.STEPS)
def test_float32_evaluation_error_on_the_shared_generator(t, lr):
    """A condition on the reference and its inputs, not on the kernels: the plain float32 evaluation stays at or under 3.5 units of
    2^-24 in e_m, e_v and e_theta at every step number the GPU tests use (measured, worst over both learning rates: 1.01, 2.71, 2.94),
    so their limit of 3 x this evaluation's own figures is at most ~10 units."""
    x = an.make_inputs(np.random.default_rng(0), 200000)
    lr = an.stored(lr)
    args = (x["theta"], x["m"], x["v"], x["g"], t, lr, B1, B2, EPS)
    want = an.adam_step(*args, np.float64)
    got = an.adam_step(*args, np.float32)
    assert all(a.dtype == np.float32 for a in got) and all(a.dtype == np.float64 for a in want)
    e = an.normalised_errors(got, want, dict(x, t=t))
    print("t = %d, lr = %g: float32 evaluation e_m %.2f, e_v %.2f, e_theta %.2f (units of 2^-24)" % ((t, lr) + e))
    assert max(e) <= 3.5, e
    assert min(e) > 0.1, e           # (and it is a float32 evaluation: it does differ from float64)
    # the edge cases are there: exact zeros that must stay put, the eps-dominated regime, large gradients
    dead = (x["g"] == 0) & (x["m"] == 0) & (x["v"] == 0)
    assert dead.sum() > 1000 and np.array_equal(got[0][dead], x["theta"][dead]) and np.array_equal(want[0][dead], x["theta"][dead].astype(np.float64))
    root = np.sqrt(want[2])
    assert ((root > 0) & (root < 1e-2 * EPS)).sum() > 1000 and (np.abs(x["g"]) > 100).sum() > 1000
