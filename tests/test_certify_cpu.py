"""CPU: certified LiDAR bounds (copo_amd/eval/certify.py, copo_cert_obs_seats_f32, copo_certify_tally) -- levels
and plans, the sweep layout, the C entries' refusals (no device is touched), the CLI's clashes, the fold's restatement against a case
written out by hand, the float64 model's soundness on its own, and the PREMISE of the GPU tests measured on the model alone."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

import certify_cases as cc
import certify_numpy as cz
import pgd_numpy as pn
from test_learner_plan_cpu import make_cfg

from copo_amd import _capi
from copo_amd.eval.adversary import AdversaryLevel, AdversaryPlan
from copo_amd.eval.certify import BOUND_WORDS, CERT_WORDS, LEVEL_FIELDS, CertifyLevel, CertifyPlan, cert_rates, load_levels
from copo_amd.eval.crossplay import SeatPlan

F = np.float32


def test_level_validation_and_words():
    lv = CertifyLevel(0.01, 0.05, 0.1)
    assert lv.as_dict() == dict(eps=0.01, delta_steer=0.05, delta_throttle=0.1) and tuple(lv.as_dict()) == LEVEL_FIELDS
    w = lv.words()
    assert w.dtype == np.float32 and w.tolist() == [F(0.01), F(0.05), F(0.1), 0.0]
    assert CertifyLevel().words().tolist() == [0.0] * 4 and CertifyLevel(eps=1) == CertifyLevel(eps=1.0)          # eps = 0 is a level
    for bad in (dict(eps=-0.1), dict(delta_steer=-1.0), dict(delta_throttle=-1e-9), dict(eps=float("nan")), dict(delta_steer=float("inf")),
                dict(eps="1"), dict(eps=True), dict(steer=1.0)):
        with pytest.raises((ValueError, TypeError)):
            CertifyLevel(**bad)
    with pytest.raises(Exception):
        lv.eps = 0.2          # frozen
    assert len(BOUND_WORDS) == len(CERT_WORDS) == 8


def test_plan_validation_and_check():
    plan = CertifyPlan([{}, dict(eps=0.01, delta_steer=0.1)], np.array([[0, 1], [1, -1], [5, 0]]))
    assert (plan.L, plan.G, plan.K) == (2, 3, 2) and plan.words.shape == (2, 4) and plan.words.dtype == np.float32
    assert plan.level_of.dtype == np.int32 and plan.scenes_per_cell is None
    seats = SeatPlan(np.array([[0, 1], [1, 0], [0, 0]]), 2, np.array([0, 1, 2]), 3)
    assert plan.check(seats) is plan
    with pytest.raises(ValueError):
        plan.check(SeatPlan(np.array([[0, 1]]), 2))
    for bad in (([], np.zeros((1, 1))), ([{}], np.zeros(3)), ([dict(eps=-1.0)], np.zeros((1, 1)))):
        with pytest.raises(ValueError):
            CertifyPlan(*bad)


def test_sweep_is_the_adversary_sweeps_layout_at_share_one():
    levels = [CertifyLevel(0.001, 0.1, 0.1), CertifyLevel(0.002, 0.1, 0.1), CertifyLevel()]          # no identity rule: nobody is impaired
    c_seats, c = CertifyPlan.sweep(3, levels, 2, 8)
    a_seats, a = AdversaryPlan.sweep(3, [AdversaryLevel(), AdversaryLevel(0.1, 0.0, 1.0), AdversaryLevel(0.2, 1.0, 0.0)], 2, 8, 1.0)
    assert np.array_equal(c_seats.seat, a_seats.seat) and np.array_equal(c_seats.group, a_seats.group) and np.array_equal(c.level_of, a.level_of)
    assert np.array_equal(c_seats.rows, a_seats.rows) and c_seats.replica_scenes == a_seats.replica_scenes == 2 and c_seats.K == 3
    assert (c.doubled, c.n_impaired, c.scenes_per_cell, c.n_checkpoints, c.share) == (False, 8, 2, 3, 1.0)
    assert c.checkpoint.tolist() == a.checkpoint.tolist() and c.level.tolist() == a.level.tolist() and c.check(c_seats) is c
    for bad in (dict(K=0), dict(scenes_per_cell=0), dict(N=0), dict(levels=[])):
        kw = dict(K=2, levels=[CertifyLevel()], scenes_per_cell=1, N=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            CertifyPlan.sweep(**kw)


def test_load_levels(tmp_path):
    p = tmp_path / "levels.json"
    p.write_text(json.dumps([{}, dict(eps=0.001, delta_steer=0.05, delta_throttle=0.1), dict(eps=0.002)]))
    assert load_levels(str(p)) == [CertifyLevel(), CertifyLevel(0.001, 0.05, 0.1), CertifyLevel(0.002)]
    for bad in (dict(eps=0.1), [1, 2], [dict(sigma=1.0)], [dict(eps=-1)], [dict(delta_steer="x")]):
        p.write_text(json.dumps(bad))
        with pytest.raises((ValueError, TypeError)):
            load_levels(str(p))


def test_symbols_are_exported_and_the_abi_version_stays():
    for name in ("copo_cert_obs_seats_f32", "copo_certify_tally"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, name)
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION
    from copo_amd import trainer
    assert (cz.ACTED, cz.SPAWNED) == (trainer.F_ACTED, trainer.F_SPAWNED)


def test_entries_refuse_before_they_touch_a_device():
    null, dim = -1, -2
    cfg = make_cfg(hidden=64, in_pol=91, in_val=())
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    good = dict(cfg=C.byref(cfg), theta=p, theta_t=p, member_stride=cfg.n_params, n_members=3, rows=p, counts=p, cap=32, n_out=48, obs_src=p,
                bounds=p, col_lo=19, col_hi=91, n_slots=8, group=p, n_groups=3, level_of=p, levels=p, n_levels=2, pad=0.0, stream=None)
    call = lambda **kw: _capi.lib.copo_cert_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "bounds", "group", "level_of", "levels"):
        assert call(**{name: None}) == null, name
    for bad in (dict(n_members=0), dict(n_members=65536), dict(cap=0), dict(n_out=0), dict(n_out=47), dict(n_slots=0), dict(n_groups=0),
                dict(n_levels=0), dict(member_stride=cfg.n_params - 4), dict(member_stride=cfg.n_params + 2), dict(col_lo=-1),
                dict(col_lo=92, col_hi=92), dict(col_hi=92), dict(col_lo=50, col_hi=49), dict(theta_t=p + 4),
                dict(pad=-1e-9), dict(pad=float("nan")), dict(pad=float("inf"))):
        assert call(**bad) == dim, bad
    assert call(cfg=C.byref(make_cfg(hidden=64, in_pol=91, in_val=(), bf16=True))) == dim          # fp32 operands only
    for hidden in (96, 32, 1024):
        c = make_cfg(hidden=hidden, in_pol=91, in_val=())
        assert call(cfg=C.byref(c), member_stride=c.n_params) == dim, hidden
    tgood = dict(flags=p, bounds=p, seat=p, group=p, level_of=p, levels=p, E=4, N=8, K=2, G=3, L=2, out=p, stream=None)
    tally = lambda **kw: _capi.lib.copo_certify_tally(*dict(tgood, **kw).values())  # noqa: E731
    for name in ("flags", "bounds", "seat", "group", "level_of", "levels", "out"):
        assert tally(**{name: None}) == null, name
    for bad in (dict(E=-1), dict(N=0), dict(N=257), dict(K=0), dict(K=65536), dict(G=0), dict(L=0)):
        assert tally(**bad) == dim, bad
    assert tally(E=0) == 0          # nothing to do, nothing launched


def test_cli_clashes(tmp_path):
    from copo_amd.eval.evaluate import main
    levels = tmp_path / "levels.json"
    levels.write_text("[{}]")
    base = ["--certify-sweep", "a.npz", "--certify-levels", str(levels), "--table", str(tmp_path / "t.csv")]
    for extra in (["--cross-play", "a.npz", "b.npz"], ["--fault-sweep", "a.npz", "--fault-levels", str(levels)],
                  ["--adversary-sweep", "a.npz", "--adversary-levels", str(levels)], ["--pgd-sweep", "a.npz", "--pgd-levels", str(levels)]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
    for cut in (base[:2] + base[4:], base[:4]):          # without the levels, without the table
        with pytest.raises(SystemExit) as e:
            main(cut)
        assert e.value.code == 2


def hand_case():
    """Two scenes x six slots, two members, two groups (+ one out of range), written out by hand.  Level 0: deltas (0.25, 0.5).
    Scene 0 (group 0): slot 0 a bound exactly at delta on both axes; slot 1 steer just over; slot 2 NaN; slot 3 infinity; slot 4
    valid = 0; slot 5 seat -1.  Scene 1 (group 1): slot 0 SPAWNED without ACTED; slot 1 a width that quantises half-way (to even);
    slot 2 the largest deviation; slot 3 member 0 at level index -1; slots 4 / 5 ordinary.  Scene 2: group 9, out of range."""
    A, S = cz.ACTED, cz.SPAWNED
    inf, nan = float("inf"), float("nan")
    h = 2.0 ** -17          # half a quantisation step
    seat = np.array([[0, 0, 0, 1, 1, -1], [1, 1, 1, 0, 1, 1], [0, 1, 0, 1, 0, 1]], np.int32)
    flags = np.array([[A, A, A, A | S, A, A], [S, A, A | 2, A, A, A], [A] * 6], np.uint8)
    group = np.array([0, 1, 9], np.int32)
    level_of = np.array([[0, 0], [-1, 0]], np.int32)
    levels = np.array([[0.001, 0.25, 0.5, 0.0]], np.float32)
    b = np.zeros((3, 6, 8), np.float32)
    b[..., 6] = 1.0
    b[0, 0, :6] = [0.75, 1.25, -0.5, 0.5, 1.0, 0.0]            # dev (0.25, 0.5): exactly at delta -> certified
    b[0, 1, :6] = [0.75, 1.25 + 2.0 ** -20, -0.5, 0.5, 1.0, 0.0]      # steer over by an ulp: throttle alone
    b[0, 2, :6] = [nan, 1.0, 0.0, 1.0, 0.5, 0.5]
    b[0, 3, :6] = [0.0, 1.0, 0.0, inf, 0.5, 0.5]
    b[0, 4, :6], b[0, 4, 6] = [0.0, 1.0, 0.0, 1.0, 0.5, 0.5], 0.0
    b[0, 5, :6] = [0.0, 1.0, 0.0, 1.0, 0.5, 0.5]
    b[1, 0, :6] = [0.0, 0.1, 0.0, 0.1, 0.05, 0.05]
    b[1, 1, :6] = [0.0, h, 0.0, 3 * h, 0.0, 0.0]                # widths h, 3 h: q16 = 0 (half to even), 2
    b[1, 2, :6] = [0.0, 2000.0, 0.0, 1.0, 1.0, 0.5]              # dev_0 = 1999: clamps to 1024
    b[1, 3, :6] = [0.0, 1.0, 0.0, 1.0, 0.5, 0.5]
    b[1, 4, :6] = [0.0, 0.25, 0.0, 0.5, 0.125, 0.25]
    b[1, 5, :6] = [0.0, 0.5, 0.0, 1.0, 0.125, 0.25]              # dev (0.375, 0.75): neither
    want = np.zeros((2, 2, 8), np.int64)
    want[0, 0] = [3, 1, 1, 2, 2 * 32768, 2 * 65536, 32768, 1]            # slots 0, 1 (its extra 2^-20 of width rounds away), 2 (NaN)
    want[0, 1] = [1, 0, 0, 0, 0, 0, 0, 1]                                 # slot 3 (infinity); slot 4 is invalid
    want[1, 1] = [4, 2, 2, 3, 0 + 1024 * 65536 + 16384 + 32768, 2 + 65536 + 32768 + 65536, 1024 * 65536, 0]
    return flags, b, seat, group, level_of, levels, want


def test_fold_restatement_on_a_hand_made_case():
    flags, b, seat, group, level_of, levels, want = hand_case()
    assert cz.q16(F(2.0 ** -17)) == 0 and cz.q16(F(3 * 2.0 ** -17)) == 2 and cz.q16(F(2000.0)) == 1024 * 65536 and cz.q16(F(-1.0)) == 0
    got = cz.fold(flags, b, seat, group, level_of, levels, 2, 2, np.zeros((2, 2, 8), np.int64))
    assert got.tolist() == want.tolist()
    again = cz.fold(flags, b, seat, group, level_of, levels, 2, 2, got.copy())          # it accumulates; the max word keeps the largest
    assert np.array_equal(again[..., [0, 1, 2, 3, 4, 5, 7]], 2 * want[..., [0, 1, 2, 3, 4, 5, 7]]) and np.array_equal(again[..., 6], want[..., 6])
    r = cert_rates(want[1, 1])
    assert r["certified_rate"] == 0.5 and r["certified_rate_throttle"] == 0.75 and r["max_dev"] == 1024.0
    assert np.isnan(cert_rates([1, 0, 0, 0, 0, 0, 0, 1])["certified_rate"])


def test_the_case_holds_the_rows_it_says():
    ref, c = cc.reference(64, 91), cc.inputs(64, 91)
    index = ref["tables"]["main"]["index"]
    tile0 = c["rows"][2][:16]
    assert sorted(set(index[tile0].tolist())) == [-1, 0, 1, 2] and index[42] == -1 and index[9] == 2 and (index >= -1).sum() == 18
    b = ref["tables"]["main"]["bounds"]
    assert (b[index == -1] == 0.0).all() and np.isnan(b[index == -2]).all() and (b[index >= 0][:, 6] == 1.0).all()
    zero = ref["tables"]["zero"]["bounds"]
    ok = ref["tables"]["zero"]["index"] >= 0
    assert np.array_equal(zero[ok][:, 0], zero[ok][:, 4]) and np.array_equal(zero[ok][:, 3], zero[ok][:, 5]) and ok.sum() == 15


@pytest.mark.parametrize("in_dim", cc.IN_DIMS)
@pytest.mark.parametrize("hidden", cc.HIDDENS)
def test_model_soundness_and_the_premise_of_the_gpu_tests(hidden, in_dim):
    """On the float64 model alone, for the very inputs of tests/test_gpu_certify.py and both nonzero budgets.  Soundness: the means of all
    2^6 corners over six beams, of 256 uniform draws in the box and of pgd_numpy's three attacks (+steer, +throttle, untargeted) lie
    inside [lo, hi] on every valid row.  Premise: every width is strictly between 0 and the trivial 2 |W3[a]|_1, and the smallest gap
    between an attack's mean and the bound it approaches is positive.  Both margins are printed."""
    c, ref = cc.inputs(hidden, in_dim), cc.reference(hidden, in_dim)
    rng = np.random.RandomState(5 + hidden + in_dim)
    lo_c, hi_c = cc.COL_LO, cc.COL_HI
    for table, eps in (("small", cc.EPS_SMALL), ("large", cc.EPS_LARGE)):
        b, index = ref["tables"][table]["bounds"], ref["tables"][table]["index"]
        eps = float(F(eps))
        att = cc.attacked(hidden, in_dim, eps)
        width_share, gap, n = 0.0, np.inf, 0
        for r in np.flatnonzero(index >= 0):
            net, o = c["nets"][ref["member"][int(r)]], c["obs"][r].astype(np.float64)
            lo, hi = b[r][[0, 2]], b[r][[1, 3]]
            share = (hi - lo) / cz.trivial_width(net)
            assert (share > 0.0).all() and (share < 1.0).all(), (r, share)
            width_share = max(width_share, float(share.max()))
            blo, bhi = np.maximum(o - eps, 0.0), np.minimum(o + eps, 1.0)
            points = []
            beams = rng.choice(np.arange(lo_c, hi_c), 6, replace=False)
            for corner in itertools.product((0, 1), repeat=6):          # corners over six beams, the other beams at a random end
                x = np.where(rng.rand(len(o)) < 0.5, blo, bhi)
                x[beams] = np.where(np.array(corner) == 1, bhi[beams], blo[beams])
                points.append(x)
            u = rng.rand(256, len(o))
            points += list(blo + u * (bhi - blo))
            for x in points:
                x[:lo_c], x[hi_c:] = o[:lo_c], o[hi_c:]
                m = cz.mu(net, x)
                assert (m >= lo).all() and (m <= hi).all(), (r, m, lo, hi)
            xa = att["seen"][r].astype(np.float64)
            # (the attack projects onto the float32 ends o +- eps, each rounded once: up to an ulp of a beam outside the real box)
            assert np.abs(xa[lo_c:hi_c] - o[lo_c:hi_c]).max() <= eps + 2.0 ** -23 and np.abs(xa - o).max() > 0.0
            m = cz.mu(net, xa)
            assert (m >= lo).all() and (m <= hi).all(), (r, m, lo, hi)
            gap = min(gap, float(np.minimum(m - lo, hi - m).min()))
            n += 1
        print("hidden %d in_dim %d eps %.4g: %d rows, largest width / trivial %.3g, smallest gap attack-to-bound %.3g (tau %.3g)" % (
            hidden, in_dim, eps, n, width_share, gap, ref["tau"]))
        assert n == 15 and gap > 0.0 and gap > 4.0 * ref["tau"]
    assert 0.0 < ref["tau"] < 1e-3
