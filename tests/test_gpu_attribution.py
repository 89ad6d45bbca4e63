"""Input attribution on the GPU (copo_ig_obs_seats_f32, copo_attrib_tally, copo_amd/eval/attribution.py).  The
kernel cases are those of tests/attribution_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, adversary_cases' 48
rows and lists (0 / 1 / 17 rows in lists of 32), three tables of four levels -- and tests/test_attribution_cpu.py measures on the model
alone what the comparisons here rely on.  Every case launches the kernels a handful of times; outputs and references are computed once."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attribution_cases as xc
import attribution_numpy as az
import crossplay_numpy as cn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
CASES = [(h, k) for h in xc.HIDDENS for k in xc.IN_DIMS]
N_OUT = xc.E * xc.N


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plan_buffers(c, table, rows=None):
    return SimpleNamespace(K=xc.K, G=xc.G, N=xc.N, E=xc.E, cap=xc.CAP, n_out=N_OUT, rows=_dev(c["rows"] if rows is None else rows),
                           counts=_dev(c["counts"]), group=_dev(xc.GROUPS[table]), seat=_dev(c["seat"]))


def _levels(table, base, words=None):
    return SimpleNamespace(K=xc.K, G=xc.G, L=len(xc.POINTS), level_of=_dev(xc.LEVEL_OF[table]), levels=_dev(xc.level_words() if words is None else words),
                           base=_dev(base), max_points=xc.MAX_POINTS)


def _attribute(bank, pb, lb, obs):
    attr, heads = _poison(N_OUT, 2, obs.shape[1]), _poison(N_OUT, 8)
    bank.attribute_seats(pb, lb, obs, attr, heads)
    torch.cuda.synchronize()
    return attr.cpu().numpy(), heads.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    c = xc.reference(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), c["members"])
    bank.sync_mirror()
    obs = _dev(c["obs"])
    out = {t: _attribute(bank, _plan_buffers(c, t), _levels(t, c["base"]), obs) for t in xc.TABLES}
    out["again"] = _attribute(bank, _plan_buffers(c, "A"), _levels("A", c["base"]), obs)
    assert torch.equal(obs.view(torch.int32), _dev(c["obs"]).view(torch.int32))          # the true observation is left alone
    return dict(ref=c, out=out, bank=bank, obs=obs)


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_attributions_against_float64(hidden, in_dim):
    """(a) Every attributed row of the three tables: attr and heads[:6] against the float64 model as |x - x64| / max(1, |x64|); valid and
    the m bits exact.  The bound is measured per case, not fixed: `dev` = the same quantity for the same rule in torch fp32 on the CPU,
    tau = 4 dev (the rule of test_gpu_certify.py).  No row is excluded.  Every figure is printed before it is asserted."""
    c = _case(hidden, in_dim)
    ref, worst, n = c["ref"], 0.0, 0
    for t in xc.TABLES:
        m, (attr, heads) = ref["tables"][t], c["out"][t]
        rows = np.flatnonzero(m["index"] >= 0)
        assert len(rows) == xc.ATTRIBUTED[t]
        for r in rows:
            worst = max(worst, xc.rel(attr[r], m["attr"][r]), xc.rel(heads[r][:6], m["heads"][r][:6]))
            assert heads[r][6] == 1.0 and _u32(heads[r][7]).item() == int(xc.POINTS[m["index"][r]]), (t, r)
            n += 1
    print("hidden %d in_dim %d: %d rows, kernel %.3g, torch fp32 dev %.3g, tau %.3g, kernel / tau %.2f" % (
        hidden, in_dim, n, worst, ref["dev"], ref["tau"], worst / ref["tau"]))
    assert n == sum(xc.ATTRIBUTED.values()) and 0.0 < ref["tau"] < 1e-3
    assert worst <= ref["tau"], (worst, ref["tau"])


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_one_point_is_the_adversary_gradient_at_the_midpoint(hidden, in_dim):
    """(b) At m = 1 and head 0: attr against d * grad, grad from copo_adv_obs_seats_f32 with (steer, throttle) = (1, 0) on the midpoint
    rows b + (1/2) d formed in fp32 as the kernel forms them -- within tau of each other; whether the bits are equal is printed."""
    c = _case(hidden, in_dim)
    ref = c["ref"]
    obs, base = ref["obs"], ref["base"][1]
    b = np.where(np.isnan(base), obs, base).astype(np.float32)
    d = obs - b
    mid = (b + np.float32(0.5) * d).astype(np.float32)
    worst, n, same = 0.0, 0, True
    for t in ("A", "B"):
        rows = np.flatnonzero(ref["tables"][t]["index"] == 1)
        grad, seen = _poison(N_OUT, in_dim), _poison(N_OUT, in_dim)
        words = np.zeros((len(xc.POINTS), 4), np.float32)
        words[1] = (0.0, 1.0, 0.0, 0.0)
        c["bank"].perturb_seats(_plan_buffers(ref, t), _levels(t, ref["base"], words), _dev(mid), seen, xc.COL_LO, xc.COL_HI, grad)
        torch.cuda.synchronize()
        want = d[rows] * grad.cpu().numpy()[rows]
        got = c["out"][t][0][rows, 0]
        worst = max(worst, xc.rel(got, want.astype(np.float64)))
        same = same and np.array_equal(_u32(got)[d[rows] != 0], _u32(want)[d[rows] != 0])
        n += len(rows)
    print("hidden %d in_dim %d: %d one-point rows, attr against d * grad %.3g (tau %.3g), bits equal: %s" % (hidden, in_dim, n, worst, ref["tau"], same))
    assert n == 6 and worst <= ref["tau"]


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_masks_zero_rows_unlisted_rows_and_determinism(hidden, in_dim):
    """(c) In bits: a column under a NaN mask is 0.0; identity, index -1 and out-of-range-group rows hold zeros with valid = 0; rows in
    no list keep the pre-filled words; a second launch gives the same bits."""
    c = _case(hidden, in_dim)
    ref = c["ref"]
    for t in xc.TABLES:
        m, (attr, heads) = ref["tables"][t], c["out"][t]
        for r in np.flatnonzero(m["index"] >= 0):
            masked = np.isnan(ref["base"][m["index"][r]])
            assert masked.any() or m["index"][r] == 3
            assert (_u32(attr[r][:, masked]) == 0).all(), (t, r)
        zero = m["listed"] & (m["index"] < 0)
        assert zero.sum() == 18 - xc.ATTRIBUTED[t] and (_u32(attr[zero]) == 0).all() and (_u32(heads[zero]) == 0).all()
        assert (_u32(attr[~m["listed"]]) == POISON).all() and (_u32(heads[~m["listed"]]) == POISON).all() and (~m["listed"]).sum() == N_OUT - 18
    for x, y in zip(c["out"]["A"], c["out"]["again"]):
        assert np.array_equal(_u32(x), _u32(y))


def _fold_gpu(flags, attr, heads, seat, group, O):
    words = torch.zeros(xc.G, xc.K, 8, dtype=torch.int64, device="cuda")
    cols = torch.zeros(xc.G, xc.K, 2, O, dtype=torch.int64, device="cuda")
    from copo_amd.eval.attribution import attrib_tally
    pb = SimpleNamespace(K=xc.K, G=xc.G, N=xc.N, E=xc.E, seat=_dev(seat), group=_dev(group))
    for _ in range(2):          # the outputs accumulate
        attrib_tally(_dev(flags), _dev(attr), _dev(heads), pb, words, cols)
    torch.cuda.synchronize()
    return words.cpu().numpy(), cols.cpu().numpy()


def _twice(words, cols):
    w2 = np.array([[[2 * int(v) for v in cell] for cell in row] for row in words], np.int64)
    w2[..., 5] //= 2          # (the max word keeps the largest)
    return w2, (2 * cols).astype(np.int64)


@pytest.mark.parametrize("hidden,in_dim", [(64, 91), (256, 92)])
def test_fold_against_numpy(hidden, in_dim):
    """(d) The fold of the kernel's own attr / heads and a step's flags against the python integers of attribution_numpy.fold, integer for
    integer, and again with the rows of the lists permuted between the scenes of one group."""
    c = _case(hidden, in_dim)
    ref, flags = c["ref"], xc.step_flags()
    for t in xc.TABLES:
        attr, heads = (np.where(_u32(x) == POISON, np.float32(0), x) for x in c["out"][t])          # (unlisted rows: seat -1, never read)
        group = xc.GROUPS[t]
        want = _twice(*az.fold(flags, attr, heads, ref["seat"], group, xc.K, xc.G))
        got = _fold_gpu(flags, attr, heads, ref["seat"], group, in_dim)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), t
        assert want[0][..., 0].sum() > 0 and want[0][..., 6].sum() > 0 and want[1].sum() > 0
        # scenes 0 and 1 share group 0, scenes 4 and 5 group 2: exchanging them whole moves every row to another wave, not another cell
        if t != "C":
            perm = np.array([1, 0, 2, 3, 5, 4])
            sw = lambda x: x.reshape(xc.E, xc.N, *x.shape[1:])[perm].reshape(x.shape)  # noqa: E731
            moved = _fold_gpu(flags[perm], sw(attr), sw(heads), ref["seat"][perm], group[perm], in_dim)
            assert np.array_equal(moved[0], got[0]) and np.array_equal(moved[1], got[1]), t


# ---- (e) the sampler -----------------------------------------------------------------------------------------------------------------------
E2E = (8, 8, 4)          # scenes, slots, T


@pytest.fixture(scope="module")
def e2e(golden_dir):
    from copo_amd.eval.evaluate import make_eval_trainer
    t = make_eval_trainer("copo", "inter", E2E[0], E2E[1], 0)
    yield t, cn.e2e_members(golden_dir)
    t.stop()


def _fragments(smp, keys, seed=3):
    """One fragment after a reset under one torch seed (the action noise); clones of `keys`."""
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    smp.sample()
    torch.cuda.synchronize()
    return {k: getattr(smp, k).clone() for k in keys}


def test_captured_fragment_equals_eager_and_the_drive_is_untouched(e2e):
    from copo_amd.eval.attribution import AttributionLevel, AttributionPlan, AttributionSeatSampler
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(2, 2, N, 0.5)
    assert plan.E == E and plan.n_groups == 4
    cfg = t.env.sim.cfg
    levels = [AttributionLevel(), AttributionLevel.clear_road(cfg, 4), AttributionLevel.zeros(cfg, 8)]
    attribution = AttributionPlan(levels, np.array([[1, 2], [0, 1], [2, -1], [1, 1]], np.int32))
    bank = PolicyBank(t.policy, ws)
    drive = ("tally", "actions", "clipped", "flags", "obs", "dist_inputs")
    keys = ("attr", "heads", "attrib_words", "attrib_cols") + drive
    runs = {}
    for mode in (False, True):
        smp = AttributionSeatSampler(t.env, t.policy, bank, plan, attribution, T, use_graph=mode)
        smp._loop.warmup = 0          # capture at the first fragment
        runs[mode] = _fragments(smp, keys)
        assert (smp._loop.graph is not None) == mode
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a, b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)  # noqa: E731
    for k in keys:
        assert same(runs[False][k], runs[True][k]), k
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), drive)
    for k in drive:
        assert same(plain[k], runs[True][k]), k          # attribution does not touch the drive
    aw, st = runs[True]["attrib_words"].cpu().numpy(), runs[True]["tally"].cpu().numpy()
    assert np.array_equal(aw[..., 0] + aw[..., 6], st[..., 0]) and aw[..., 0].sum() > 0 and aw[..., 6].sum() > 0
    h = runs[True]["heads"]
    valid = h[..., 6] == 1
    fwd = runs[True]["dist_inputs"][:T][valid][:, :2]          # the seat forward's means: equal up to the order of the head's sum
    assert float((h[valid][:, :2] - fwd).abs().max()) <= 512 * 2.0 ** -24 * max(1.0, float(fwd.abs().max()))
    lo, hi = cfg.ego_dim + cfg.navi_dim, cfg.ego_dim + cfg.navi_dim + cfg.num_lasers
    road = valid & (h.view(torch.int32)[..., 7] == 4)
    assert int(road.sum()) > 0 and (runs[True]["attr"][road][..., :lo] == 0).all() and (runs[True]["attr"][road][..., hi:] == 0).all()
