"""CPU: linear LiDAR certificates (copo_lin_obs_seats_f32, copo_amd/eval/certify.py method="linear") -- the two
relaxation lines of a tanh unit, the float64 model's soundness on its own, the PREMISE of the GPU tests measured on the model alone (the
ratios are printed; DESIGN.md 8p quotes them), eps = 0, and the host side: the `method` keyword, the export, the entry's refusals (no
device is touched) and the CLI flag."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import certify_cases as cc
import certify_numpy as cz
import linbound_cases as lc
import linbound_numpy as lz
from test_learner_plan_cpu import make_cfg

from copo_amd import _capi

F = np.float32
CASES = [(h, k) for h in lc.HIDDENS for k in lc.IN_DIMS]
SLACK64 = 1e-12          # float64 sums of at most 512 terms of magnitude <= a few units: rounding stays far below this


def test_relaxation_lines_bound_tanh():
    """lam z + betaL <= tanh z <= lam z + betaU on [l, u]: 10^4 random intervals -- a quarter each of l == u, intervals that straddle 0,
    saturated ones (an end beyond |z| = 9) and ordinary ones -- on a grid of 257 points each, in float64, slack 1e-15."""
    rng = np.random.RandomState(0x11B)
    n = 10000
    a, b = rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 4.0, n)
    l, u = np.minimum(a, b), np.maximum(a, b)
    kind = np.arange(n) % 4
    u[kind == 0] = l[kind == 0]
    l[kind == 1], u[kind == 1] = -np.abs(a[kind == 1]), np.abs(b[kind == 1])
    sat = kind == 2
    far = rng.uniform(9.0, 30.0, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    l[sat], u[sat] = np.minimum(a[sat], far[sat]), np.maximum(a[sat], far[sat])
    assert (l <= u).all() and (l[kind == 1] <= 0).all() and (u[kind == 1] >= 0).all() and (np.maximum(np.abs(l[sat]), np.abs(u[sat])) >= 9.0).all()
    worst = 0.0
    for i in range(n):
        tl, tu, lam, bl, bu = lz.relax(float(l[i]), float(u[i]))
        assert 0.0 <= lam <= 1.0 and tl <= tu
        z = np.linspace(l[i], u[i], 257)
        z[0], z[-1] = l[i], u[i]
        t = np.tanh(z)
        worst = max(worst, float((lam * z + bl - t).max()), float((t - lam * z - bu).max()))
    print("largest violation of a line over %d intervals x 257 points: %.3g" % (n, worst))
    assert worst <= 1e-15


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_model_soundness(hidden, in_dim):
    """On the float64 model alone, every case at the three budgets: the means of certify_cases.box_draws (64 draws of the box per row) and
    of the observations that certify_cases.attacked reaches (+steer, +throttle, untargeted) lie inside [loL, hiL] and inside the
    intersected box on every valid row.  The smallest distance to a bound is printed."""
    c, ref = lc.inputs(hidden, in_dim), lc.reference(hidden, in_dim)
    for table, eps in lc.BUDGETS:
        t = ref["tables"][table]
        eps = float(F(eps))
        rows = np.flatnonzero(t["index"] >= 0)
        assert len(rows) == 15
        seen = [cc.attacked(hidden, in_dim, eps)["seen"]] + cc.box_draws(c["obs"], eps, 31 + hidden + in_dim)
        gap = np.inf
        for r in rows:
            net, o = c["nets"][ref["member"][int(r)]], c["obs"][r].astype(np.float64)
            b, p = t["bounds"][r], t["parts"][r]
            lo, hi, loL, hiL = b[[0, 2]], b[[1, 3]], p[[0, 2]], p[[1, 3]]
            assert (lo >= loL).all() and (hi <= hiL).all() and (lo >= p[[4, 6]]).all() and (hi <= p[[5, 7]]).all()
            for x in seen:
                x = x[r].astype(np.float64)
                assert np.abs(x - o).max() <= eps + 2.0 ** -23          # (float32 ends o +- eps are rounded once)
                m = cz.mu(net, x)
                assert (m >= lo - SLACK64).all() and (m <= hi + SLACK64).all(), (table, r, m, lo, hi)
                gap = min(gap, float(np.minimum(m - lo, hi - m).min()))
        print("hidden %d in_dim %d eps %.4g: smallest distance of a probe's mean to the intersected box %.3g" % (hidden, in_dim, eps, gap))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_premise_of_the_gpu_tests(hidden, in_dim):
    """On every valid row with eps > 0 (the three uniform tables and the main one) the intersected width is strictly smaller than the
    interval width; at EPS_WIDE it is strictly inside (0, 2 |W3[a]|_1).  The mean ratios are printed per budget."""
    c, ref = lc.inputs(hidden, in_dim), lc.reference(hidden, in_dim)
    for table in ("small", "large", "wide", "main"):
        t = ref["tables"][table]
        rows = [r for r in np.flatnonzero(t["index"] >= 0) if lc.LEVELS[t["index"][r]][0] > 0.0]
        assert len(rows) == (10 if table == "main" else 15)
        shares_i, shares_l = [], []
        for r in rows:
            b, p = t["bounds"][r], t["parts"][r]
            trivial = cz.trivial_width(c["nets"][ref["member"][int(r)]])
            w, wi = b[[1, 3]] - b[[0, 2]], p[[5, 7]] - p[[4, 6]]
            assert (w < wi).all() and (w > 0.0).all(), (table, r, w, wi)
            if table == "wide":
                assert (w < trivial).all(), (r, w, trivial)
            shares_i.append(wi / trivial)
            shares_l.append(w / trivial)
        si, sl = np.array(shares_i), np.array(shares_l)
        print("hidden %d in_dim %d table %s: width / trivial, interval mean %.4g max %.4g, linear mean %.4g max %.4g, mean ratio %.3g" % (
            hidden, in_dim, table, si.mean(), si.max(), sl.mean(), sl.max(), sl.mean() / si.mean()))
    assert 0.0 < ref["tau"] < 1e-3
    print("hidden %d in_dim %d: torch fp32 dev %.3g, tau %.3g" % (hidden, in_dim, ref["dev"], ref["tau"]))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_zero_budget(hidden, in_dim):
    """eps = 0: loL == hiL == mu(o) to 1e-12 (the lines meet at the one point of the interval), and so does the intersected box."""
    t = lc.reference(hidden, in_dim)["tables"]["zero"]
    rows = np.flatnonzero(t["index"] >= 0)
    assert len(rows) == 15
    b, p = t["bounds"][rows], t["parts"][rows]
    for a in range(2):
        for x in (p[:, 2 * a], p[:, 2 * a + 1], b[:, 2 * a], b[:, 2 * a + 1]):
            assert np.abs(x - b[:, 4 + a]).max() <= 1e-12


def test_the_case_holds_the_rows_it_says():
    ref, c = lc.reference(64, 91), lc.inputs(64, 91)
    index = ref["tables"]["main"]["index"]
    assert sorted(set(index[c["rows"][2][:16]].tolist())) == [-1, 0, 1, 3] and index[42] == -1 and index[9] == 2 and (index >= -1).sum() == 18
    for key in ("bounds", "parts"):
        b = ref["tables"]["main"][key]
        assert (b[index == -1] == 0.0).all() and np.isnan(b[index == -2]).all() and np.isfinite(b[index >= 0]).all()
    assert lc.LEVELS[3][0] == F(0.01) and [e for _, e in lc.BUDGETS] == [cc.EPS_SMALL, cc.EPS_LARGE, lc.EPS_WIDE]
    p = np.array([[0.0, 1.0, 2.0, 1.0, -1.0, 0.5, 0.0, 3.0], [0.6, 0.7, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0]], F)
    # row 0: axis 0 intersects to (0, 0.5); axis 1's linear box is empty against itself -> the interval box; row 1: disjoint boxes -> interval
    assert lc.intersect_f32(p, 0.25).tolist() == [[-0.25, 0.75, -0.25, 3.25], [-0.25, 0.75, -0.25, 0.25]]
    assert lz.intersect(0.0, 1.0, -1.0, 0.5) == (0.0, 0.5) and lz.intersect(0.6, 0.7, 0.0, 0.5) == (0.0, 0.5)


# ---- host and ABI --------------------------------------------------------------------------------------------------------------------------
def test_method_keyword_is_validated_and_defaults_to_interval():
    from types import SimpleNamespace

    from copo_amd.eval import certify as cert
    from copo_amd.eval.bank import CERTIFY_METHODS, PolicyBank, check_certify_method
    from copo_amd.eval.crossplay import SeatedBank
    assert CERTIFY_METHODS == ("interval", "linear") and check_certify_method("x", "linear") == "linear"
    for fn in (PolicyBank.certify_seats, SeatedBank.certify_seats, cert.CertifySeatSampler.__init__, cert.certify_sweep_rows, cert.certified_bounds):
        assert inspect.signature(fn).parameters["method"].default == "interval", fn
    assert inspect.signature(cert.certified_bounds).parameters["parts"].default is False
    assert inspect.signature(PolicyBank.certify_seats).parameters["parts"].default is None
    for bad in ("crown", "", None, "Linear", 1):
        with pytest.raises(ValueError):
            check_certify_method("x", bad)
        with pytest.raises(ValueError):
            PolicyBank.certify_seats(SimpleNamespace(), None, None, None, None, 0, 0, method=bad)
        with pytest.raises(ValueError):
            cert.CertifySeatSampler(None, None, None, None, None, 4, method=bad)
        with pytest.raises(ValueError):
            cert.certify_sweep_rows("copo", "inter", [{}], [{}], method=bad)
        with pytest.raises(ValueError):
            cert.certified_bounds(None, None, None, 0.01, columns=(19, 91), method=bad)
    with pytest.raises(ValueError):
        cert.certified_bounds(None, None, None, 0.01, columns=(19, 91), parts=True)          # parts belong to the linear method
    with pytest.raises(ValueError):
        PolicyBank.certify_seats(SimpleNamespace(), None, None, None, None, 0, 0, parts=object())
    assert len(cert.PART_WORDS) == 8 and "out of scope" in cert.__doc__ and "CROWN, zonotopes)" not in cert.__doc__


def test_frame_gains_the_method_column_in_linear_mode_only():
    from copo_amd.eval.certify import CERT_WORDS, LEVEL_FIELDS, CertifyLevel, CertifyPlan, certify_frame
    from copo_amd.eval.crossplay import SEAT_WORDS
    seats, plan = CertifyPlan.sweep(2, [CertifyLevel(), CertifyLevel(0.01, 0.1, 0.1)], 1, 4)
    zero = np.zeros((seats.n_groups, 2, 8), np.int64)
    plain, lin = certify_frame(zero, zero, seats, plan), certify_frame(zero, zero, seats, plan, method="linear")
    head = ["checkpoint", "label", "level", "member", "seats"] + list(LEVEL_FIELDS) + list(CERT_WORDS)
    assert list(plain.columns)[:len(head)] == head and "method" not in plain.columns and SEAT_WORDS[0] in plain.columns
    assert list(lin.columns) == list(plain.columns)[:3] + ["method"] + list(plain.columns)[3:] and (lin["method"] == "linear").all()
    assert [(r.checkpoint, r.level) for r in lin.itertuples()] == [(k, l) for k in range(2) for l in range(2)]


def test_symbol_is_exported_declared_and_the_abi_version_stays():
    assert "copo_lin_obs_seats_f32" in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, "copo_lin_obs_seats_f32")
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "copo_hip.h")).read()
    assert "int copo_lin_obs_seats_f32(const copo_ppo_cfg* cfg" in header and "float* bounds, float* parts," in header


def test_entry_refuses_before_it_touches_a_device():
    null, dim = -1, -2
    cfg = make_cfg(hidden=64, in_pol=91, in_val=())
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    good = dict(cfg=C.byref(cfg), theta=p, theta_t=p, member_stride=cfg.n_params, n_members=3, rows=p, counts=p, cap=32, n_out=48, obs_src=p,
                bounds=p, parts=p, col_lo=19, col_hi=91, n_slots=8, group=p, n_groups=3, level_of=p, levels=p, n_levels=2, pad=0.0, stream=None)
    call = lambda **kw: _capi.lib.copo_lin_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "bounds", "group", "level_of", "levels"):
        assert call(**{name: None}) == null, name
        assert call(**{name: None, "parts": None}) == null, name
    for bad in (dict(n_members=0), dict(n_members=65536), dict(cap=0), dict(n_out=0), dict(n_out=47), dict(n_slots=0), dict(n_groups=0),
                dict(n_levels=0), dict(member_stride=cfg.n_params - 4), dict(member_stride=cfg.n_params + 2), dict(col_lo=-1),
                dict(col_lo=92, col_hi=92), dict(col_hi=92), dict(col_lo=50, col_hi=49), dict(theta_t=p + 4),
                dict(pad=-1e-9), dict(pad=float("nan")), dict(pad=float("inf"))):
        assert call(**bad) == dim, bad
    assert call(cfg=C.byref(make_cfg(hidden=64, in_pol=91, in_val=(), bf16=True))) == dim          # fp32 operands only
    for hidden in (96, 32, 1024):
        c = make_cfg(hidden=hidden, in_pol=91, in_val=())
        assert call(cfg=C.byref(c), member_stride=c.n_params) == dim, hidden
    wide = make_cfg(hidden=512, in_pol=200, in_val=())          # k1p = 256 at hidden 512: the tiles and the partial sums pass the LDS ceiling
    assert call(cfg=C.byref(wide), member_stride=wide.n_params) == dim
    assert (buf == 0).all()


def test_cli_flag(tmp_path):
    from copo_amd.eval.evaluate import main
    levels = tmp_path / "levels.json"
    levels.write_text("[{}]")
    base = ["--certify-sweep", "a.npz", "--certify-levels", str(levels), "--table", str(tmp_path / "t.csv")]
    for argv in (base + ["--certify-method", "crown"], base + ["--certify-method"], ["--certify-method", "linear"],
                 base + ["--certify-method", "linear", "--pgd-sweep", "a.npz", "--pgd-levels", str(levels)],
                 base[:4] + ["--certify-method", "linear"]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2, argv
    seen = {}

    def fake(algo, env, ws, lv, **kw):
        import pandas as pd
        seen.update(kw)
        return pd.DataFrame([dict(checkpoint=0, label="a.npz", level=0)])
    import copo_amd.eval.certify as cert
    import copo_amd.eval.checkpoint_io as io
    keep = cert.certify_sweep_rows, io.load_members
    cert.certify_sweep_rows, io.load_members = fake, lambda paths: [{} for _ in paths]
    try:
        main(base + ["--certify-method", "linear"])
        assert seen["method"] == "linear"
        main(base)
        assert seen["method"] == "interval"
    finally:
        cert.certify_sweep_rows, io.load_members = keep
