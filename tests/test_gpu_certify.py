"""Certified LiDAR bounds on the GPU (copo_cert_obs_seats_f32, copo_certify_tally, copo_amd/eval/certify.py).  The
kernel cases are those of tests/certify_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, adversary_cases' 48 rows
and lists, the main level table and three uniform ones -- and tests/test_certify_cpu.py measures on the model alone what the comparisons
here rely on.  Every case launches the kernels a few dozen times; the outputs and the references are computed once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bank_cases as bc
import certify_cases as cc
import certify_numpy as cz
import crossplay_numpy as cn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
CASES = [(h, k) for h in cc.HIDDENS for k in cc.IN_DIMS]
N_OUT = cc.E * cc.N
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plan_buffers(c):
    seat = np.full(N_OUT, -1, np.int32)
    for k in range(cc.K):
        seat[c["rows"][k][:c["counts"][k]]] = k
    return SimpleNamespace(K=cc.K, G=cc.G, N=cc.N, E=cc.E, cap=cc.CAP, n_out=N_OUT, rows=_dev(c["rows"]), counts=_dev(c["counts"]),
                           group=_dev(cc.GROUP), seat=_dev(seat.reshape(cc.E, cc.N)))


def _levels(level_of, words):
    return SimpleNamespace(K=cc.K, G=cc.G, L=len(words), level_of=_dev(level_of), levels=_dev(words), max_iters=cc.ATTACK_ITERS)


def _certify(bank, pb, table, obs, pad=0.0):
    bounds = _poison(N_OUT, 8)
    bank.certify_seats(pb, _levels(cc.LEVEL_OF[table], cc.LEVELS), obs, bounds, cc.COL_LO, cc.COL_HI, pad)
    torch.cuda.synchronize()
    return bounds.cpu().numpy()


def _means(bank, pb, obs):
    """dist_inputs[:, :2] of the unchanged seat forward on obs [n_out][O] (numpy float32)."""
    out = dict(action=_poison(N_OUT, 2), logp=_poison(N_OUT), dist_inputs=_poison(N_OUT, 4))
    bank.act_seats(pb, _dev(obs), torch.zeros(N_OUT, 2, device="cuda"), **out)
    torch.cuda.synchronize()
    return out["dist_inputs"].cpu().numpy()[:, :2]


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    c = cc.inputs(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), c["members"])
    bank.sync_mirror()
    pb, obs = _plan_buffers(c), _dev(c["obs"])
    out = {t: _certify(bank, pb, t, obs) for t in cc.TABLES}
    out["again"], out["padded"] = _certify(bank, pb, "main", obs), _certify(bank, pb, "main", obs, cc.PAD)
    out["clean"] = _means(bank, pb, c["obs"])
    probes = {}
    for table, eps in (("small", cc.EPS_SMALL), ("large", cc.EPS_LARGE)):
        seen = _poison(N_OUT, in_dim)
        bank.pgd_seats(pb, _levels(cc.ATTACK_LEVEL_OF, cc.attack_words(eps)), obs, seen, cc.COL_LO, cc.COL_HI, cc.ATTACK_SEED, None, None, cc.ATTACK_ITERS)
        torch.cuda.synchronize()
        seen = seen.cpu().numpy()
        listed = _u32(seen)[:, 0] != POISON
        seen[~listed] = c["obs"][~listed]
        probes[table] = dict(seen=seen, attack=_means(bank, pb, seen), draws=[_means(bank, pb, x) for x in cc.box_draws(c["obs"], eps, 77 + hidden + in_dim)])
    assert _same(obs, _dev(c["obs"]))                              # the true observation is left alone
    return dict(inputs=c, out=out, probes=probes, ref=cc.reference(hidden, in_dim), bank=bank, pb=pb)


def _rel(x, x64):
    return float((np.abs(x.astype(np.float64) - x64) / np.maximum(1.0, np.abs(x64))).max())


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_bounds_against_float64(hidden, in_dim):
    """(a) Every listed valid row of the four tables: the six numbers against the float64 model as |x - x64| / max(1, |x64|); valid and
    eps in bits.  The bound is measured per case, not fixed: `dev` = the same quantity for the same rule in torch fp32 on the CPU, tau =
    4 dev (two fp32 evaluations with different summation orders land within a small multiple of each other: the rule of
    test_gpu_adversary.py).  Every figure is printed before it is asserted."""
    c = _case(hidden, in_dim)
    ref, worst, n = c["ref"], 0.0, 0
    for table in cc.TABLES:
        m, got = ref["tables"][table], c["out"][table]
        for r in np.flatnonzero(m["index"] >= 0):
            worst = max(worst, _rel(got[r][:6], m["bounds"][r][:6]))
            assert got[r][6] == 1.0 and _u32(got[r][7]) == _u32(cc.LEVELS[m["index"][r]][0]), (table, r)
            n += 1
    print("hidden %d in_dim %d: %d rows, kernel %.3g, torch fp32 dev %.3g, tau %.3g, kernel / tau %.2f" % (
        hidden, in_dim, n, worst, ref["dev"], ref["tau"], worst / ref["tau"]))
    assert n == 4 * 15 and 0.0 < ref["tau"] < 1e-3
    assert worst <= ref["tau"], (worst, ref["tau"])


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_zero_budget_is_the_clean_pass_in_bits(hidden, in_dim):
    """(b) At eps = 0: lo_a == hi_a == mu_a(o) bit for bit (the three tiles run one instruction sequence, the radius is zero and c0 = o
    exactly), in the uniform table and on the eps = 0 rows of the main table; the clean means are within tau of act_seats'."""
    c = _case(hidden, in_dim)
    ref = c["ref"]
    for table in ("zero", "main"):
        got, index = c["out"][table], ref["tables"][table]["index"]
        rows = np.flatnonzero(index == 0)
        assert len(rows) == (15 if table == "zero" else 5)
        b = _u32(got[rows])
        assert np.array_equal(b[:, 0], b[:, 4]) and np.array_equal(b[:, 1], b[:, 4]) and np.array_equal(b[:, 2], b[:, 5]) and np.array_equal(b[:, 3], b[:, 5])
    listed = np.flatnonzero(ref["tables"]["main"]["index"] >= 0)
    worst = _rel(c["out"]["main"][listed][:, 4:6], c["out"]["clean"][listed].astype(np.float64))
    print("hidden %d in_dim %d: clean means against act_seats %.3g (tau %.3g)" % (hidden, in_dim, worst, ref["tau"]))
    assert worst <= ref["tau"]


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_soundness_on_the_devices_own_numbers(hidden, in_dim):
    """(c) obs_seen of copo_pgd_obs_seats_f32 at the same budget on the same lists (+steer in group 0, +throttle in group 1, untargeted
    in group 2) and 64 host-drawn samples of the box per row, through the unchanged act_seats: every mean lies inside
    [lo - tau, hi + tau] (tau relative to max(1, |bound|)), no element excluded."""
    c = _case(hidden, in_dim)
    ref, obs = c["ref"], c["inputs"]["obs"]
    for table, eps in (("small", cc.EPS_SMALL), ("large", cc.EPS_LARGE)):
        b, p = c["out"][table].astype(np.float64), c["probes"][table]
        rows = np.flatnonzero(ref["tables"][table]["index"] >= 0)
        lo, hi = b[rows][:, [0, 2]], b[rows][:, [1, 3]]
        lo_t, hi_t = lo - ref["tau"] * np.maximum(1.0, np.abs(lo)), hi + ref["tau"] * np.maximum(1.0, np.abs(hi))
        moved = np.abs(p["seen"][rows].astype(np.float64) - obs[rows])
        assert float(moved.max()) <= float(F(eps)) + 2.0 ** -23          # (the float32 ends o +- eps are rounded once)
        assert (moved.max(axis=1) > 0.0).all() and len(rows) == 15
        gap = np.inf
        for m in [p["attack"]] + p["draws"]:
            m = m[rows].astype(np.float64)
            assert np.isfinite(m).all()
            gap = min(gap, float(np.minimum(m - lo, hi - m).min()))
            assert (m >= lo_t).all() and (m <= hi_t).all(), (table, float((lo_t - m).max()), float((m - hi_t).max()))
        print("hidden %d in_dim %d eps %.4g: smallest distance of a probe's mean to its bound %.3g (tau %.3g)" % (hidden, in_dim, eps, gap, ref["tau"]))
        assert len(p["draws"]) == cc.BOX_DRAWS


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_monotone_in_the_budget_and_the_pad(hidden, in_dim):
    """(d) The bounds at the larger budget contain those at the smaller, and those contain the clean means, within tau.  `pad` widens
    every bound by exactly pad: one fp32 addition to the unpadded value, in bits."""
    c = _case(hidden, in_dim)
    ref, out = c["ref"], c["out"]
    rows = np.flatnonzero(ref["tables"]["zero"]["index"] >= 0)
    z, s, l = (out[t][rows].astype(np.float64) for t in ("zero", "small", "large"))
    slack = lambda x: ref["tau"] * np.maximum(1.0, np.abs(x))  # noqa: E731
    for inner, outer in ((z, s), (s, l)):
        for a in (0, 2):
            assert (outer[:, a] <= inner[:, a] + slack(inner[:, a])).all() and (outer[:, a + 1] >= inner[:, a + 1] - slack(inner[:, a + 1])).all()
    assert ((l[:, 1] - l[:, 0]) > (s[:, 1] - s[:, 0])).all() and ((s[:, 1] - s[:, 0]) > 0.0).all()
    plain, padded = out["main"], out["padded"]
    listed = np.flatnonzero(ref["tables"]["main"]["index"] >= 0)
    pad = F(cc.PAD)
    for a in (0, 2):
        assert np.array_equal(_u32(padded[listed][:, a]), _u32(plain[listed][:, a] + (-pad)))
        assert np.array_equal(_u32(padded[listed][:, a + 1]), _u32(plain[listed][:, a + 1] + pad))
    assert np.array_equal(_u32(padded[listed][:, 4:]), _u32(plain[listed][:, 4:]))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_invalid_rows_unlisted_rows_and_determinism(hidden, in_dim):
    """(e) A listed row whose group is out of range holds eight zeros (in a mixed tile and in the all-invalid tile); rows in no list keep
    their poison; two launches give equal bits."""
    c = _case(hidden, in_dim)
    got, index = c["out"]["main"], c["ref"]["tables"]["main"]["index"]
    assert (_u32(got[index == -1]) == 0).all() and (index == -1).sum() == 3 and index[42] == -1
    assert (_u32(got[index == -2]) == POISON).all() and (index == -2).sum() == N_OUT - 18
    assert np.array_equal(_u32(got), _u32(c["out"]["again"]))


def test_certified_bounds_is_the_uniform_launch():
    """`certified_bounds` at one budget: the uniform table's launch in bits on the valid rows, zeros on every other row."""
    from copo_amd.eval.certify import certified_bounds
    c = _case(128, 92)
    got = certified_bounds(c["bank"], c["pb"], _dev(c["inputs"]["obs"]), cc.EPS_LARGE, columns=(cc.COL_LO, cc.COL_HI)).cpu().numpy()
    valid = c["ref"]["tables"]["large"]["index"] >= 0
    assert np.array_equal(_u32(got[valid]), _u32(c["out"]["large"][valid])) and (_u32(got[~valid]) == 0).all() and valid.sum() == 15
    padded = certified_bounds(c["bank"], c["pb"], _dev(c["inputs"]["obs"]), cc.EPS_LARGE, cc.PAD, columns=(cc.COL_LO, cc.COL_HI)).cpu().numpy()
    assert np.array_equal(_u32(padded[valid][:, 1]), _u32(got[valid][:, 1] + F(cc.PAD)))


def test_refusals():
    """(f) What the Python layer and the entries refuse; nothing is written."""
    from copo_amd.eval.bank import PolicyBank
    c = cc.inputs(64, 91)
    bank = PolicyBank(_policy("ippo", 91, 64, False), c["members"])
    bank.sync_mirror()
    pb, lv = _plan_buffers(c), _levels(cc.LEVEL_OF["main"], cc.LEVELS)
    obs, bounds = _dev(c["obs"]), _poison(N_OUT, 8)
    for pad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception):
            bank.certify_seats(pb, lv, obs, bounds, cc.COL_LO, cc.COL_HI, pad)
    with pytest.raises(Exception):
        bank.certify_seats(pb, lv, obs, bounds, cc.COL_LO, 92)
    for bad in (dict(obs=obs[:, :90].contiguous()), dict(bounds=_poison(N_OUT, 7)), dict(bounds=torch.zeros(N_OUT, 8, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError):
            bank.certify_seats(pb, lv, **dict(dict(obs=obs, bounds=bounds), **bad), col_lo=cc.COL_LO, col_hi=cc.COL_HI)
    with pytest.raises(ValueError):
        bank.certify_seats(pb, SimpleNamespace(K=2, G=cc.G, L=3, level_of=lv.level_of, levels=lv.levels), obs, bounds, cc.COL_LO, cc.COL_HI)
    torch.cuda.synchronize()
    assert (_bits(bounds) == POISON).all()


# ---- (g) the fold ------------------------------------------------------------------------------------------------------------------------
def _fold_gpu(flags, bounds, seat, group, level_of, levels, K, G):
    from copo_amd.eval.certify import certify_tally
    E, N = seat.shape
    pb = SimpleNamespace(K=K, G=G, N=N, E=E, seat=_dev(seat), group=_dev(group))
    cb = SimpleNamespace(K=K, G=G, L=len(levels), level_of=_dev(level_of), levels=_dev(levels))
    out = torch.zeros(G, K, 8, dtype=torch.int64, device="cuda")
    for _ in range(2):          # it accumulates
        certify_tally(_dev(flags), _dev(bounds), pb, cb, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _twice(want):
    want = want.copy()
    want[..., [0, 1, 2, 3, 4, 5, 7]] *= 2
    return want


def test_fold_on_the_kernels_own_bounds():
    c = _case(64, 91)
    rng = np.random.RandomState(3)
    flags = rng.choice(np.array([0, cz.ACTED, cz.ACTED | 2, cz.SPAWNED, cz.ACTED | cz.SPAWNED], np.uint8), (cc.E, cc.N))
    seat = c["pb"].seat.cpu().numpy()
    level_of = cc.LEVEL_OF["main"]
    for name in ("main", "large", "padded"):
        bounds = c["out"][name].reshape(cc.E, cc.N, 8).copy()
        bounds[_u32(bounds) == POISON] = 0.0          # rows in no list: what the sampler's zero-initialised buffer holds
        lo = cc.LEVEL_OF["large"] if name == "large" else level_of
        want = cz.fold(flags, bounds, seat, cc.GROUP, lo, cc.LEVELS, cc.K, cc.G, np.zeros((cc.G, cc.K, 8), np.int64))
        got = _fold_gpu(flags, bounds, seat, cc.GROUP, lo, cc.LEVELS, cc.K, cc.G)
        assert np.array_equal(got, _twice(want)), (name, got.tolist(), want.tolist())
        assert want[..., 0].sum() > 0 and want[..., 6].max() > 0
        if name == "main":          # its eps = 0 rows are certified at delta = 0, its other rows are not
            assert 0 < want[..., 1].sum() < want[..., 0].sum()


def test_fold_on_a_hand_made_case_and_at_scale():
    from test_certify_cpu import hand_case
    flags, b, seat, group, level_of, levels, want = hand_case()
    assert np.array_equal(_fold_gpu(flags, b, seat, group, level_of, levels, 2, 2), _twice(want))
    E, N, K, G, L = 1030, 130, 64, 5, 3          # more than one workgroup, three rounds of 64 slots, many members per round
    rng = np.random.RandomState(9)
    seat = rng.randint(-1, K, (E, N)).astype(np.int32)
    seat[rng.rand(E, N) < 0.6] = -1
    seat[7, :] = 5          # a whole scene of one member
    flags = rng.choice(np.array([0, cz.ACTED, cz.ACTED | 2, cz.SPAWNED], np.uint8), (E, N), p=[0.2, 0.6, 0.1, 0.1])
    group = rng.randint(-1, G + 1, E).astype(np.int32)
    level_of = rng.randint(-1, L + 1, (G, K)).astype(np.int32)
    levels = np.array([[0.0, 0.0, 0.0, 0.0], [0.001, 0.05, 0.08, 0.0], [0.002, 0.2, 0.1, 0.0]], np.float32)
    b = np.zeros((E, N, 8), np.float32)
    mu = rng.randn(E, N, 2).astype(np.float32)
    down, up = (rng.rand(E, N, 2) * 0.2).astype(np.float32), (rng.rand(E, N, 2) * 0.2).astype(np.float32)
    b[..., 0], b[..., 1], b[..., 2], b[..., 3] = mu[..., 0] - down[..., 0], mu[..., 0] + up[..., 0], mu[..., 1] - down[..., 1], mu[..., 1] + up[..., 1]
    b[..., 4:6] = mu
    b[..., 6] = (rng.rand(E, N) < 0.9).astype(np.float32)
    bad = rng.rand(E, N) < 0.01
    b[bad, 1] = np.nan
    b[rng.rand(E, N) < 0.01, 2] = -np.inf
    b[3, 3, :6] = [0.0, 3000.0, 0.0, 1.0, 1.0, 0.5]
    want = cz.fold(flags, b, seat, group, level_of, levels, K, G, np.zeros((G, K, 8), np.int64))
    got = _fold_gpu(flags, b, seat, group, level_of, levels, K, G)
    assert np.array_equal(got, _twice(want))
    assert want[..., 0].sum() > 10000 and want[..., 7].sum() > 0 and 0 < want[..., 1].sum() < want[..., 2].sum()


# ---- (h) the sampler ---------------------------------------------------------------------------------------------------------------------
E2E = (8, 8, 4)          # scenes, slots, T
LEVELS = [dict(), dict(eps=0.0005, delta_steer=0.05, delta_throttle=0.05), dict(eps=0.002, delta_steer=0.05, delta_throttle=0.05)]


@pytest.fixture(scope="module")
def e2e(golden_dir):
    from copo_amd.eval.evaluate import make_eval_trainer
    t = make_eval_trainer("copo", "inter", E2E[0], E2E[1], 0)
    yield t, cn.e2e_members(golden_dir)
    t.stop()


def _fragments(smp, n_frag, keys, seed=3):
    """`n_frag` fragments after a reset under one torch seed (the action noise); clones of `keys` per fragment."""
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    keep = []
    for _ in range(n_frag):
        smp.sample()
        torch.cuda.synchronize()
        keep.append({k: getattr(smp, k).clone() for k in keys})
    return keep


def _plans():
    from copo_amd.eval.certify import CertifyPlan
    from copo_amd.eval.crossplay import SeatPlan
    plan = SeatPlan.pairs(2, 2, E2E[1], 0.5)
    assert plan.E == E2E[0] and plan.n_groups == 4
    return plan, CertifyPlan(LEVELS, np.array([[1, 2], [0, 1], [2, -1], [1, 1]], np.int32))


def test_captured_fragment_equals_eager_and_the_drive_is_untouched(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.certify import CertifyPlan, CertifySeatSampler
    from copo_amd.eval.crossplay import SeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan, cert = _plans()
    bank = PolicyBank(t.policy, ws)
    keys = ("bounds", "cert_tally", "tally", "actions", "clipped", "flags", "obs", "dist_inputs")
    runs = {}
    for mode in (False, True):
        smp = CertifySeatSampler(t.env, t.policy, bank, plan, cert, T, use_graph=mode)
        smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
        runs[mode] = _fragments(smp, 2, keys)
        assert (smp._loop.graph is not None) == mode
    for f in range(2):
        for k in keys:
            assert _same(runs[False][f][k], runs[True][f][k]), (f, k)
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, ("tally", "actions", "clipped", "flags", "obs"))
    for f in range(2):
        for k in plain[f]:
            assert _same(plain[f][k], runs[True][f][k]), (f, k)          # certification does not touch the drive
    last = runs[True][1]
    assert smp.sample()["bounds"] is smp.bounds
    b, seat, group = last["bounds"], torch.from_numpy(plan.seat).cuda(), torch.from_numpy(plan.group).cuda()[:, None]
    off = (group == 2) & (seat == 1)          # level index -1: listed, invalid
    assert (b[:, off] == 0).all() and (b[:, ~off][..., 6] == 1).all() and int(off.sum()) == 2 * N // 2
    # the clean means are the seat forward's up to the order of the head's sum (at most 512 fp32 terms, each within 2^-24 relative)
    mine, fwd = b[:, ~off][..., 4:6], last["dist_inputs"][:T][:, ~off][..., :2]
    assert float((mine - fwd).abs().max()) <= 512 * 2.0 ** -24 * max(1.0, float(fwd.abs().max()))
    calm = (group == 1) & (seat == 0)         # eps = 0
    assert _same(b[:, calm][..., 0], b[:, calm][..., 4]) and _same(b[:, calm][..., 3], b[:, calm][..., 5])
    ct, st = last["cert_tally"].cpu().numpy(), last["tally"].cpu().numpy()
    lv_ok = torch.from_numpy(cert.level_of >= 0).numpy()
    assert np.array_equal(ct[..., 0][lv_ok], st[..., 0][lv_ok]) and (ct[..., 0][~lv_ok] == 0).all() and ct[..., 0].sum() > 0 and ct[..., 7].sum() == 0
    assert (ct[1, 0, 1] == ct[1, 0, 0]) and ct[1, 0, 6] == 0          # eps = 0: width 0, every row certified
    # set_certify: the same shapes are copied in and the graph stays; another L drops it
    graph = smp._loop.graph
    smp.set_certify(CertifyPlan(LEVELS, np.array([[2, 1], [1, 1], [0, 0], [1, 2]], np.int32)))
    assert smp._loop.graph is graph and graph is not None
    smp.clear_tally()
    assert int(smp.cert_tally.abs().sum()) == 0 and int(smp.tally.abs().sum()) == 0
    hot = _fragments(smp, 1, ("bounds",))
    assert not _same(hot[0]["bounds"], runs[True][0]["bounds"])
    smp.set_certify(CertifyPlan(LEVELS[:2], np.ones((4, 2), np.int32)))
    assert smp._loop.graph is None
    with pytest.raises(ValueError):
        smp.set_certify(CertifyPlan(LEVELS, np.zeros((5, 2), np.int32)))


def test_certify_sweep_rows_frame(golden_dir):
    from copo_amd.eval.certify import CERT_WORDS, LEVEL_FIELDS, CertifyLevel, certify_sweep_rows
    from copo_amd.eval.crossplay import SEAT_WORDS
    w = bc.golden_population(golden_dir, "copo_inter")
    levels = [CertifyLevel(0.0, 0.02, 0.02), CertifyLevel(0.0005, 0.02, 0.02), CertifyLevel(0.002, 0.02, 0.02)]
    N, steps, S = 8, 8, 2          # one fragment or two
    df = certify_sweep_rows("copo", "inter", [w, dict(w)], levels, scenes_per_cell=S, num_agents=N, steps=steps, seed=0, labels=["a", "b"])
    rates = ["certified_rate", "certified_rate_steer", "certified_rate_throttle", "mean_width_steer", "mean_width_throttle", "max_dev"]
    seat_rates = ["success", "crash_rate", "out_rate", "reward_per_step"]
    assert list(df.columns) == ["checkpoint", "label", "level", "member", "seats"] + list(LEVEL_FIELDS) + list(CERT_WORDS) + rates + list(SEAT_WORDS) + seat_rates
    assert [(r.checkpoint, r.level) for r in df.itertuples()] == [(k, l) for k in range(2) for l in range(3)]
    for r in df.itertuples():
        assert {k: getattr(r, k) for k in LEVEL_FIELDS} == levels[r.level].as_dict()
    assert (df["rows"] == df["acted"]).all() and (df["rows"] >= steps).all() and (df["nonfinite"] == 0).all()
    for k in range(2):
        cell = df[df.checkpoint == k].sort_values("eps")
        rate, width, dev = cell["certified_rate"].tolist(), cell["mean_width_steer"].tolist(), cell["max_dev"].tolist()
        assert rate[0] == 1.0 and rate[0] >= rate[1] >= rate[2], rate
        assert width[0] == 0.0 and width[0] < width[1] < width[2] and dev[0] == 0.0 and dev[1] < dev[2], (width, dev)
    # the same checkpoint twice on the same scenes and noise: the same table
    a, b = df[df.checkpoint == 0].drop(columns=["checkpoint", "label", "member"]), df[df.checkpoint == 1].drop(columns=["checkpoint", "label", "member"])
    assert a.reset_index(drop=True).equals(b.reset_index(drop=True))
