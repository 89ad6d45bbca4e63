"""CPU: adversarial LiDAR (copo_amd/eval/adversary.py, copo_adv_obs_seats_f32) -- levels and plans, the sweep
layout, the C entry's refusals (no device is touched), the CLI's clashes, the float64 restatement against torch autograd, and the
PREMISE of the GPU tests measured on the float64 model alone."""
import ctypes as C
import json

import numpy as np
import pytest

import adversary_cases as ac
import adversary_numpy as an
from test_learner_plan_cpu import make_cfg

from copo_amd import _capi
from copo_amd.eval.adversary import AdversaryLevel, AdversaryPlan, load_levels
from copo_amd.eval.crossplay import SeatPlan
from copo_amd.eval.faults import sweep_members


def test_level_validation_and_words():
    assert AdversaryLevel().is_identity and AdversaryLevel(eps=0.1).is_identity and AdversaryLevel(steer=1.0, throttle=-1.0).is_identity
    lv = AdversaryLevel(eps=0.1, throttle=1)
    assert not lv.is_identity and lv.as_dict() == dict(eps=0.1, steer=0.0, throttle=1.0)
    w = lv.words()
    assert w.dtype == np.float32 and w.tolist() == [np.float32(0.1), 0.0, 1.0, 0.0]
    for bad in (dict(eps=-0.1), dict(eps=float("nan")), dict(steer=float("inf")), dict(throttle="1"), dict(eps=True)):
        with pytest.raises(ValueError):
            AdversaryLevel(**bad)
    with pytest.raises(Exception):
        lv.eps = 0.2          # frozen


def test_plan_validation_and_check():
    plan = AdversaryPlan([{}, dict(eps=0.1, steer=1.0)], np.array([[0, 1], [1, -1], [5, 0]]))
    assert (plan.L, plan.G, plan.K) == (2, 3, 2) and plan.words.shape == (2, 4) and plan.words.dtype == np.float32
    assert plan.level_of.dtype == np.int32 and plan.scenes_per_cell is None
    seats = SeatPlan(np.array([[0, 1], [1, 0], [0, 0]]), 2, np.array([0, 1, 2]), 3)
    assert plan.check(seats) is plan
    with pytest.raises(ValueError):
        plan.check(SeatPlan(np.array([[0, 1]]), 2))
    with pytest.raises(ValueError):
        AdversaryPlan([], np.zeros((1, 1)))
    with pytest.raises(ValueError):
        AdversaryPlan([{}], np.zeros(3))
    with pytest.raises(ValueError):
        AdversaryPlan([dict(eps=-1.0)], np.zeros((1, 1)))


@pytest.mark.parametrize("share,n_imp", [(1.0, 8), (0.25, 2), (0.0, 0)])
def test_sweep_layout(share, n_imp):
    K, S, N = 2, 2, 8
    levels = [AdversaryLevel(), AdversaryLevel(0.1, 0.0, 1.0), AdversaryLevel(0.05, 1.0, 0.0)]
    L = len(levels)
    seats, adv = AdversaryPlan.sweep(K, levels, S, N, share)
    doubled = share < 1.0
    KB = 2 * K if doubled else K
    assert adv.check(seats) is adv and adv.doubled == doubled and adv.n_impaired == n_imp and adv.scenes_per_cell == S
    assert (seats.E, seats.N, seats.K, seats.n_groups, seats.replica_scenes) == (K * L * S, N, KB, K * L, S)
    assert adv.level_of.shape == (K * L, KB) and adv.share == share and adv.n_checkpoints == K
    for g in range(K * L):
        k, lv = g // L, g % L
        assert (adv.checkpoint[g], adv.level[g]) == (k, lv) and (seats.group[g * S:(g + 1) * S] == g).all()
        for e in range(g * S, (g + 1) * S):
            assert (seats.seat[e, :n_imp] == (K + k if doubled else k)).all() and (seats.seat[e, n_imp:] == k).all()
        assert adv.level_of[g, K + k if doubled else k] == lv and np.count_nonzero(adv.level_of[g]) == (1 if lv else 0)
    ws = [dict(a=np.zeros(1)), dict(a=np.ones(1))]
    bank = sweep_members(ws, adv)
    assert len(bank) == KB and all(bank[m] is ws[m % K] for m in range(KB))


def test_sweep_is_the_fault_sweeps_layout_and_keeps_its_identity_rule():
    from copo_amd.eval.faults import FaultLevel, FaultPlan
    harsh = AdversaryLevel(0.1, 0.0, 1.0)
    for share in (1.0, 0.25):
        a_seats, a = AdversaryPlan.sweep(3, [AdversaryLevel(), harsh], 2, 8, share)
        f_seats, f = FaultPlan.sweep(3, [FaultLevel(), FaultLevel(sticky=0.5)], 2, 8, share)
        assert np.array_equal(a_seats.seat, f_seats.seat) and np.array_equal(a_seats.group, f_seats.group) and np.array_equal(a.level_of, f.level_of)
        assert np.array_equal(a_seats.rows, f_seats.rows) and a_seats.replica_scenes == f_seats.replica_scenes
    with pytest.raises(ValueError):
        AdversaryPlan.sweep(2, [harsh, AdversaryLevel()], 2, 8, 0.25)          # the unattacked seats need an identity at level 0
    seats, adv = AdversaryPlan.sweep(2, [AdversaryLevel(eps=0.3), harsh], 2, 8, 0.25)      # eps without a direction IS an identity
    assert seats.K == 4
    seats, adv = AdversaryPlan.sweep(2, [harsh, AdversaryLevel()], 2, 8, 1.0)
    assert seats.K == 2 and adv.level_of.tolist() == [[0, 0], [1, 0], [0, 0], [0, 1]]
    for bad in (dict(K=0), dict(scenes_per_cell=0), dict(N=0), dict(share=1.5), dict(levels=[])):
        a = dict(K=2, levels=[AdversaryLevel()], scenes_per_cell=1, N=4, share=1.0)
        a.update(bad)
        with pytest.raises(ValueError):
            AdversaryPlan.sweep(**a)


def test_load_levels(tmp_path):
    p = tmp_path / "levels.json"
    p.write_text(json.dumps([{}, dict(eps=0.1, throttle=1.0), dict(eps=0.05, steer=-1, throttle=0.5)]))
    got = load_levels(str(p))
    assert got == [AdversaryLevel(), AdversaryLevel(0.1, 0.0, 1.0), AdversaryLevel(0.05, -1.0, 0.5)] and got[0].is_identity
    for bad in (dict(eps=0.1), [1, 2], [dict(sigma=1.0)], [dict(eps=-1)]):
        p.write_text(json.dumps(bad))
        with pytest.raises((ValueError, TypeError)):
            load_levels(str(p))


def test_symbol_is_exported_and_the_abi_version_stays():
    assert "copo_adv_obs_seats_f32" in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, "copo_adv_obs_seats_f32")
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION


def test_entry_refuses_before_it_touches_a_device():
    null, dim = -1, -2
    cfg = make_cfg(hidden=64, in_pol=91, in_val=())
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    good = dict(cfg=C.byref(cfg), theta=p, theta_t=p, member_stride=cfg.n_params, n_members=3, rows=p, counts=p, cap=32, n_out=48, obs_src=p,
                obs_seen=p, grad=None, col_lo=19, col_hi=91, n_slots=8, group=p, n_groups=3, level_of=p, levels=p, n_levels=2, stream=None)
    call = lambda **kw: _capi.lib.copo_adv_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "obs_seen", "group", "level_of", "levels"):
        assert call(**{name: None}) == null, name
    for bad in (dict(n_members=0), dict(n_members=65536), dict(cap=0), dict(n_out=0), dict(n_out=47), dict(n_slots=0), dict(n_groups=0),
                dict(n_levels=0), dict(member_stride=cfg.n_params - 4), dict(member_stride=cfg.n_params + 2), dict(col_lo=-1),
                dict(col_lo=92, col_hi=92), dict(col_hi=92), dict(col_lo=50, col_hi=49), dict(theta_t=p + 4)):
        assert call(**bad) == dim, bad
    assert call(cfg=C.byref(make_cfg(hidden=64, in_pol=91, in_val=(), bf16=True))) == dim          # fp32 operands only
    for hidden in (96, 32, 1024):
        c = make_cfg(hidden=hidden, in_pol=91, in_val=())
        assert call(cfg=C.byref(c), member_stride=c.n_params) == dim, hidden


def test_cli_clashes(tmp_path):
    from copo_amd.eval.evaluate import main
    levels = tmp_path / "levels.json"
    levels.write_text("[{}]")
    base = ["--adversary-sweep", "a.npz", "--adversary-levels", str(levels), "--table", str(tmp_path / "t.csv")]
    for extra in (["--cross-play", "a.npz", "b.npz"], ["--fault-sweep", "a.npz", "--fault-levels", str(levels)]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2
    for cut in (base[:2] + base[4:], base[:4]):          # without the levels, without the table
        with pytest.raises(SystemExit) as e:
            main(cut)
        assert e.value.code == 2


def test_restatement_equals_torch_float64_autograd():
    import torch
    w = ac.bc.random_population(19, 64, 7)
    net = ac.net_of(w)
    rng = np.random.RandomState(8)
    for steer, throttle in ((0.0, 1.0), (1.0, -0.5), (-2.0, 0.0)):
        o = rng.rand(19)
        g = an.input_gradient(net, o, steer, throttle)
        want = ac.torch_gradient(w, o, steer, throttle, torch.float64)
        assert want.dtype == np.float64 and np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(g).max() > 0.0


def test_restatement_rules_on_a_case_written_out_by_hand():
    """One scene of four slots, one member: a perturbed row, the clamps, sign(0) = 0 and the three pass-through cases."""
    W1 = np.zeros((2, 4))
    W1[0, 1], W1[0, 2], W1[1, 3] = 1.0, -1.0, 0.0          # J grows with column 1, falls with column 2, ignores columns 0 and 3
    net = (W1, np.zeros(2), np.eye(2), np.zeros(2), np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]), np.zeros(4))
    obs = np.array([[0.5, 0.95, 0.05, 0.5]] * 4)
    rows, counts = np.array([[0, 1, 2, 0]]), np.array([3])
    levels = [(0.1, 1.0, 0.0), (0.0, 1.0, 0.0), (0.1, 0.0, 0.0)]
    for level_of, moved in (([[0]], True), ([[1]], False), ([[2]], False), ([[3]], False), ([[-1]], False)):
        seen, grad, written, perturbed = an.adversary([net], obs, 4, rows, counts, [0], level_of, levels, 1, 4)
        assert written.tolist() == [True, True, True, False] and np.isnan(seen[3]).all() and perturbed[:3].all() == moved
        if moved:
            assert grad[0][1] > 0 > grad[0][2] and grad[0][3] == 0.0 and grad[0][0] == 0.0
            assert seen[0].tolist() == [0.5, 1.0, 0.0, 0.5]          # both clamps; the column outside the block and the zero-gradient one stay
        else:
            assert np.array_equal(seen[:3], obs[:3])


@pytest.mark.parametrize("in_dim", ac.IN_DIMS)
@pytest.mark.parametrize("hidden", ac.HIDDENS)
def test_premise_of_the_gpu_tests(hidden, in_dim):
    """On the float64 model alone, for the very inputs of tests/test_gpu_adversary.py (adversary_cases: seeds WEIGHT_SEED, OBS_SEED): the
    sign comparison may leave out the LiDAR elements with |g| <= tau max|g| of their row, and that share is at most 1 %; no row has an
    all-zero gradient.  Measured: a share of 0 in every one of the sixteen cases (792 / 504 LiDAR elements in tables A / B), with dev
    2.3e-7 .. 7.4e-7 and tau 9.1e-7 .. 3.0e-6 on the host this was written on; dev is measured where the test runs."""
    for table in ac.TABLES:
        ref = ac.reference(hidden, in_dim, table)
        share, dead = ac.small_share(ref)
        print("hidden %d in_dim %d table %s: fp32 deviation %.3g tau %.3g excluded share %.3g" % (hidden, in_dim, table, ref["dev"], ref["tau"], share))
        assert int(ref["perturbed"].sum()) == (11 if table == "A" else 7)
        assert 0.0 < ref["tau"] < 1e-3 and share <= 0.01 and dead == 0
