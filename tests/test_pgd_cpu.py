"""CPU: iterated adversarial LiDAR (copo_amd/eval/pgd.py, copo_pgd_obs_seats_f32) -- levels and plans, the sweep
layout, the C entry's refusals (no device is touched), the CLI's clashes, the numpy model against torch autograd and against the one-step
model, the random start's moments, and the PREMISE of the GPU tests measured on the model alone."""
import ctypes as C
import json

import numpy as np
import pytest

import adversary_cases as ac
import adversary_numpy as an
import pgd_cases as pc
import pgd_numpy as pn
from test_learner_plan_cpu import make_cfg

from copo_amd import _capi
from copo_amd.eval.adversary import AdversaryLevel, AdversaryPlan
from copo_amd.eval.crossplay import SeatPlan
from copo_amd.eval.pgd import LEVEL_FIELDS, PGDLevel, PGDPlan, load_levels


def test_level_validation_and_words():
    assert PGDLevel().is_identity and PGDLevel(eps=0.1, iters=3, alpha=0.1).is_identity          # targeted, no direction
    assert PGDLevel(eps=0.1, throttle=1.0, alpha=0.1).is_identity                                 # iters 0
    assert PGDLevel(throttle=1.0, alpha=0.1, iters=2).is_identity                                 # eps 0
    lv = PGDLevel(eps=0.1, throttle=1, alpha=0.05, iters=4)
    assert not lv.is_identity and lv.flags == 0
    assert lv.as_dict() == dict(eps=0.1, steer=0.0, throttle=1.0, alpha=0.05, iters=4, random_start=False, untargeted=False)
    assert tuple(lv.as_dict()) == LEVEL_FIELDS
    w = lv.words()
    assert w.dtype == np.int32 and w.shape == (8,) and w[:4].view(np.float32).tolist() == [np.float32(0.1), 0.0, 1.0, np.float32(0.05)]
    assert w[4:].tolist() == [4, 0, 0, 0]
    un = PGDLevel(eps=0.1, alpha=0.02, iters=16, random_start=True, untargeted=True)
    assert not un.is_identity and un.flags == 3 and un.words()[4:].tolist() == [16, 3, 0, 0]
    noise = PGDLevel(eps=0.1, iters=1, random_start=True, untargeted=True)                        # alpha = 0: uniform noise of the budget
    assert not noise.is_identity and noise.flags == 3
    for bad in (dict(eps=-0.1), dict(alpha=-1.0), dict(eps=float("nan")), dict(steer=float("inf")), dict(throttle="1"), dict(eps=True),
                dict(iters=17), dict(iters=-1), dict(iters=1.5), dict(iters=True), dict(random_start=1), dict(untargeted="yes")):
        with pytest.raises(ValueError):
            PGDLevel(**bad)
    with pytest.raises(ValueError, match="random_start"):
        PGDLevel(eps=0.1, alpha=0.1, iters=2, untargeted=True)                                    # zero gradient at x_0 = o
    with pytest.raises(Exception):
        lv.eps = 0.2          # frozen


def test_plan_validation_and_check():
    plan = PGDPlan([{}, dict(eps=0.1, steer=1.0, alpha=0.05, iters=3)], np.array([[0, 1], [1, -1], [5, 0]]))
    assert (plan.L, plan.G, plan.K, plan.max_iters) == (2, 3, 2, 3) and plan.words.shape == (2, 8) and plan.words.dtype == np.int32
    assert plan.level_of.dtype == np.int32 and plan.scenes_per_cell is None
    assert PGDPlan([{}], np.zeros((1, 1))).max_iters == 1          # the launch's bound is at least 1
    seats = SeatPlan(np.array([[0, 1], [1, 0], [0, 0]]), 2, np.array([0, 1, 2]), 3)
    assert plan.check(seats) is plan
    with pytest.raises(ValueError):
        plan.check(SeatPlan(np.array([[0, 1]]), 2))
    for bad in (([], np.zeros((1, 1))), ([{}], np.zeros(3)), ([dict(eps=-1.0)], np.zeros((1, 1))), ([dict(untargeted=True)], np.zeros((1, 1)))):
        with pytest.raises(ValueError):
            PGDPlan(*bad)


def test_sweep_is_the_adversary_sweeps_layout_and_keeps_its_identity_rule():
    harsh = PGDLevel(0.1, 0.0, 1.0, 0.05, 4)
    for share in (1.0, 0.25):
        p_seats, p = PGDPlan.sweep(3, [PGDLevel(), harsh], 2, 8, share)
        a_seats, a = AdversaryPlan.sweep(3, [AdversaryLevel(), AdversaryLevel(0.1, 0.0, 1.0)], 2, 8, share)
        assert np.array_equal(p_seats.seat, a_seats.seat) and np.array_equal(p_seats.group, a_seats.group) and np.array_equal(p.level_of, a.level_of)
        assert np.array_equal(p_seats.rows, a_seats.rows) and p_seats.replica_scenes == a_seats.replica_scenes == 2
        assert (p.doubled, p.n_impaired, p.scenes_per_cell, p.n_checkpoints, p.share) == (a.doubled, a.n_impaired, 2, 3, share)
        assert p.checkpoint.tolist() == a.checkpoint.tolist() and p.level.tolist() == a.level.tolist() and p.check(p_seats) is p
    with pytest.raises(ValueError):
        PGDPlan.sweep(2, [harsh, PGDLevel()], 2, 8, 0.25)          # the unattacked seats need an identity at level 0
    seats, _ = PGDPlan.sweep(2, [PGDLevel(eps=0.3, alpha=0.1, iters=2), harsh], 2, 8, 0.25)      # no direction IS an identity
    assert seats.K == 4
    for bad in (dict(K=0), dict(scenes_per_cell=0), dict(N=0), dict(share=1.5), dict(levels=[])):
        a = dict(K=2, levels=[PGDLevel()], scenes_per_cell=1, N=4, share=1.0)
        a.update(bad)
        with pytest.raises(ValueError):
            PGDPlan.sweep(**a)


def test_load_levels(tmp_path):
    p = tmp_path / "levels.json"
    p.write_text(json.dumps([{}, dict(eps=0.1, throttle=1.0, alpha=0.05, iters=4), dict(eps=0.05, alpha=0.01, iters=8, random_start=True, untargeted=True)]))
    got = load_levels(str(p))
    assert got == [PGDLevel(), PGDLevel(0.1, 0.0, 1.0, 0.05, 4), PGDLevel(0.05, 0.0, 0.0, 0.01, 8, True, True)] and got[0].is_identity
    for bad in (dict(eps=0.1), [1, 2], [dict(sigma=1.0)], [dict(eps=-1)], [dict(iters=40)], [dict(untargeted=True)]):
        p.write_text(json.dumps(bad))
        with pytest.raises((ValueError, TypeError)):
            load_levels(str(p))


def test_symbol_is_exported_and_the_abi_version_stays():
    assert "copo_pgd_obs_seats_f32" in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, "copo_pgd_obs_seats_f32")
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION


def test_entry_refuses_before_it_touches_a_device():
    null, dim = -1, -2
    cfg = make_cfg(hidden=64, in_pol=91, in_val=())
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    good = dict(cfg=C.byref(cfg), theta=p, theta_t=p, member_stride=cfg.n_params, n_members=3, rows=p, counts=p, cap=32, n_out=48, obs_src=p,
                obs_seen=p, col_lo=19, col_hi=91, n_slots=8, group=p, n_groups=3, level_of=p, levels=p, n_levels=2, seed=7, tick=None,
                max_iters=4, trace=None, stream=None)
    call = lambda **kw: _capi.lib.copo_pgd_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "obs_seen", "group", "level_of", "levels"):
        assert call(**{name: None}) == null, name
    for bad in (dict(n_members=0), dict(n_members=65536), dict(cap=0), dict(n_out=0), dict(n_out=47), dict(n_slots=0), dict(n_groups=0),
                dict(n_levels=0), dict(member_stride=cfg.n_params - 4), dict(member_stride=cfg.n_params + 2), dict(col_lo=-1),
                dict(col_lo=92, col_hi=92), dict(col_hi=92), dict(col_lo=50, col_hi=49), dict(theta_t=p + 4),
                dict(max_iters=0), dict(max_iters=17), dict(max_iters=-3)):
        assert call(**bad) == dim, bad
    assert call(cfg=C.byref(make_cfg(hidden=64, in_pol=91, in_val=(), bf16=True))) == dim          # fp32 operands only
    for hidden in (96, 32, 1024):
        c = make_cfg(hidden=hidden, in_pol=91, in_val=())
        assert call(cfg=C.byref(c), member_stride=c.n_params) == dim, hidden


def test_cli_clashes(tmp_path):
    from copo_amd.eval.evaluate import main
    levels = tmp_path / "levels.json"
    levels.write_text("[{}]")
    base = ["--pgd-sweep", "a.npz", "--pgd-levels", str(levels), "--table", str(tmp_path / "t.csv")]
    for extra in (["--cross-play", "a.npz", "b.npz"], ["--fault-sweep", "a.npz", "--fault-levels", str(levels)],
                  ["--adversary-sweep", "a.npz", "--adversary-levels", str(levels)]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
    for cut in (base[:2] + base[4:], base[:4]):          # without the levels, without the table
        with pytest.raises(SystemExit) as e:
            main(cut)
        assert e.value.code == 2


def test_model_gradient_equals_torch_float64_autograd():
    import torch
    w = ac.bc.random_population(19, 64, 7)
    net = ac.net_of(w)
    rng = np.random.RandomState(8)
    for level in ((0.1, 0.0, 1.0, 0.05, 2, 0), (0.1, 1.0, -0.5, 0.05, 2, 1), (0.1, 0.0, 0.0, 0.05, 2, 3), (0.1, 5.0, 5.0, 0.05, 2, 3)):
        o = rng.rand(19)
        x = np.clip(o + 0.1 * (2.0 * rng.rand(19) - 1.0), 0.0, 1.0)
        g = pn.gradient(net, x, o, level)
        want = pc.torch_gradient(w, x, o, level, torch.float64)
        assert want.dtype == np.float64 and np.abs(want).max() > 0.0
        assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max(), level
    assert np.abs(pn.gradient(net, o, o, (0.1, 0.0, 0.0, 0.05, 2, 3))).max() == 0.0          # untargeted at x = o: why the level is refused


def test_random_start_moments():
    """2^16 draws of u: |u| < 1, mean within 5 standard errors of 0 (a uniform on (-1, 1) has variance 1 / 3); exact in float32."""
    n = 1 << 16
    u = np.array([pn.uniform_pm1(pn.hash_rng(pc.SEED, r, t, b, pn.STREAM)) for r in range(16) for t in range(8) for b in range(n // 128)], np.float32)
    assert u.size == n and u.dtype == np.float32 and float(np.abs(u).max()) < 1.0
    se = np.sqrt(1.0 / 3.0 / n)
    print("random start: mean %.3g (5 se = %.3g), variance %.4f, extremes %.6f %.6f" % (u.mean(dtype=np.float64), 5 * se, u.var(dtype=np.float64), u.min(), u.max()))
    assert abs(float(u.mean(dtype=np.float64))) <= 5.0 * se
    h = 0x12345678
    assert float(pn.uniform_pm1(h)) == (2 * (h >> 9) + 1 - 2 ** 23) / 2.0 ** 23          # exact: an odd integer over 2^23


@pytest.mark.parametrize("table", ac.TABLES)
def test_one_step_is_fgsm(table):
    """iters = 1, alpha = eps, flags = 0 is adversary_numpy's step on the LiDAR columns, after rounding to float32."""
    hidden, in_dim = 64, 91
    ref, c = ac.reference(hidden, in_dim, table), pc.inputs(hidden, in_dim)
    out = pn.pgd(c["nets"], c["obs"], ac.N, c["rows"], c["counts"], ac.GROUP, ac.LEVEL_OF[table], pc.fgsm_levels(), ac.COL_LO, ac.COL_HI, 0, None, 4)
    assert np.array_equal(out["its"] >= 0, ref["written"]) and np.array_equal(out["its"] == 1, ref["perturbed"])
    rows = np.flatnonzero(ref["written"])
    lo, hi = ac.COL_LO, ac.COL_HI
    assert np.array_equal(out["seen"][rows][:, lo:hi], ref["seen"][rows][:, lo:hi].astype(np.float32))
    assert np.array_equal(out["seen"][rows].view(np.uint32)[:, :lo], c["obs"][rows].view(np.uint32)[:, :lo])
    assert np.isnan(out["seen"][~ref["written"]]).all() and ref["perturbed"].sum() > 0
    assert pc.fgsm_words().view(np.float32)[:, [0, 3]].tolist() == [[e, e] for e in ac.LEVELS[:, 0].tolist()]


def test_the_case_holds_the_rows_it_says():
    m = pc.model(64, 91)
    its = m["its"]
    tile0 = pc.inputs(64, 91)["rows"][2][:16]
    assert sorted(set(its[tile0].tolist())) == [0, 1, 3, 4] and its[42] == 0 and its[9] == 2 and (its >= 0).sum() == 18
    assert [int(m["level"][r][5]) for r in (0, 16, 32, 9)] == [0, 3, 3, 1] and pc.words().shape == (5, 8)
    lo, hi = pc.COL_LO, pc.COL_HI
    for r, xs in m["iterates"].items():
        o, eps = pc.inputs(64, 91)["obs"][r], np.float32(m["level"][r][0])
        for x in xs:
            assert x.dtype == np.float32 and np.array_equal(x[:lo].view(np.uint32), o[:lo].view(np.uint32))
            assert (np.abs(x[lo:hi].astype(np.float64) - o[lo:hi]) <= float(eps) * (1 + 1e-6)).all() and x[lo:hi].min() >= 0.0 and x[lo:hi].max() <= 1.0
    assert not np.array_equal(m["iterates"][32][0], pc.inputs(64, 91)["obs"][32])          # a random start moved x_0
    assert np.array_equal(m["iterates"][32][0], m["iterates"][32][1])                      # alpha = 0: noise only
    cut = pc.model(64, 91, max_iters=1)
    assert sorted(set(cut["its"].tolist())) == [-1, 0, 1]


@pytest.mark.parametrize("in_dim", pc.IN_DIMS)
@pytest.mark.parametrize("hidden", pc.HIDDENS)
def test_premise_of_the_gpu_tests(hidden, in_dim):
    """On the model alone, for the very inputs of tests/test_gpu_pgd.py: every targeted attacked row ends with J(x_it) > J(o), every
    untargeted one with |mu(x_it) - mu(o)| > 0.  The smallest margins are printed."""
    c, m = pc.inputs(hidden, in_dim), pc.model(hidden, in_dim)
    gain, moved = [], []
    for r, xs in m["iterates"].items():
        net, o, level = c["nets"][m["member"][r]], c["obs"][r], m["level"][r]
        if int(level[5]) & pn.UNTARGETED:
            moved.append(float(np.abs(pn.mu(net, xs[-1]) - pn.mu(net, o)).max()))
        else:
            gain.append(pn.objective(net, xs[-1], o, level) - pn.objective(net, o, o, level))
    print("hidden %d in_dim %d: smallest J(x_it) - J(o) over %d targeted rows %.3g, smallest |mu(x_it) - mu(o)| over %d untargeted rows %.3g" % (
        hidden, in_dim, len(gain), min(gain), len(moved), min(moved)))
    assert len(gain) == 6 and len(moved) == 9
    assert min(gain) > 0.0 and min(moved) > 0.0
