"""Linear LiDAR certificates on the GPU (copo_lin_obs_seats_f32, copo_amd/eval/certify.py method="linear").  The
kernel cases are those of tests/linbound_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, certify_cases' 48 rows and
lists, the main level table and four uniform ones -- and tests/test_linbound_cpu.py measures on the model alone what the comparisons here
rely on.  Every case launches the kernels a few dozen times; the outputs and the references are computed once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bank_cases as bc
import certify_cases as cc
import certify_numpy as cz
import crossplay_numpy as cn
import linbound_cases as lc

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
CASES = [(h, k) for h in lc.HIDDENS for k in lc.IN_DIMS]
N_OUT = lc.E * lc.N
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
    for k in range(lc.K):
        seat[c["rows"][k][:c["counts"][k]]] = k
    return SimpleNamespace(K=lc.K, G=lc.G, N=lc.N, E=lc.E, cap=lc.CAP, n_out=N_OUT, rows=_dev(c["rows"]), counts=_dev(c["counts"]),
                           group=_dev(lc.GROUP), seat=_dev(seat.reshape(lc.E, lc.N)))


def _levels(level_of, words):
    return SimpleNamespace(K=lc.K, G=lc.G, L=len(words), level_of=_dev(level_of), levels=_dev(words), max_iters=cc.ATTACK_ITERS)


def _linear(bank, pb, table, obs, pad=0.0, parts=True):
    """(bounds, parts) of one launch into poisoned outputs."""
    bounds, second = _poison(N_OUT, 8), _poison(N_OUT, 8) if parts else None
    bank.certify_seats(pb, _levels(lc.LEVEL_OF[table], lc.LEVELS), obs, bounds, lc.COL_LO, lc.COL_HI, pad, "linear", second)
    torch.cuda.synchronize()
    return bounds.cpu().numpy(), None if second is None else second.cpu().numpy()


def _interval(bank, pb, table, obs, pad=0.0):
    bounds = _poison(N_OUT, 8)
    bank.certify_seats(pb, _levels(lc.LEVEL_OF[table], lc.LEVELS), obs, bounds, lc.COL_LO, lc.COL_HI, pad)
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
    c = lc.inputs(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), c["members"])
    bank.sync_mirror()
    pb, obs = _plan_buffers(c), _dev(c["obs"])
    out = {t: _linear(bank, pb, t, obs) for t in lc.TABLES}
    out["again"], out["padded"] = _linear(bank, pb, "main", obs), _linear(bank, pb, "main", obs, lc.PAD)
    out["no_parts"] = _linear(bank, pb, "main", obs, parts=False)
    interval = {t: _interval(bank, pb, t, obs) for t in lc.TABLES}
    probes = {}
    for table, eps in lc.BUDGETS:
        seen = _poison(N_OUT, in_dim)
        bank.pgd_seats(pb, _levels(cc.ATTACK_LEVEL_OF, cc.attack_words(eps)), obs, seen, lc.COL_LO, lc.COL_HI, cc.ATTACK_SEED, None, None, cc.ATTACK_ITERS)
        torch.cuda.synchronize()
        seen = seen.cpu().numpy()
        listed = _u32(seen)[:, 0] != POISON
        seen[~listed] = c["obs"][~listed]
        probes[table] = dict(seen=seen, attack=_means(bank, pb, seen), draws=[_means(bank, pb, x) for x in cc.box_draws(c["obs"], eps, 77 + hidden + in_dim)],
                             padded=_linear(bank, pb, table, obs, lc.PAD, parts=False)[0])
    assert _same(obs, _dev(c["obs"]))                              # the true observation is left alone
    return dict(inputs=c, out=out, interval=interval, probes=probes, ref=lc.reference(hidden, in_dim), bank=bank, pb=pb)


def _rel(x, x64):
    return float((np.abs(x.astype(np.float64) - x64) / np.maximum(1.0, np.abs(x64))).max())


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_bounds_and_parts_against_float64(hidden, in_dim):
    """(a) Every listed valid row of the five tables: the six numbers of `bounds` and the eight of `parts` against the float64 model as
    |x - x64| / max(1, |x64|); valid and eps in bits.  The bound is measured per case, not fixed: `dev` = the same quantity for the same
    rule in torch fp32 on the CPU, tau = 4 dev (the rule of test_gpu_adversary.py and test_gpu_certify.py).  Every figure is printed
    before it is asserted."""
    c = _case(hidden, in_dim)
    ref, worst, n = c["ref"], 0.0, 0
    for table in lc.TABLES:
        m, (got, parts) = ref["tables"][table], c["out"][table]
        for r in np.flatnonzero(m["index"] >= 0):
            worst = max(worst, _rel(lc.numbers(got[r], parts[r]), lc.numbers(m["bounds"][r], m["parts"][r])))
            assert got[r][6] == 1.0 and _u32(got[r][7]) == _u32(lc.LEVELS[m["index"][r]][0]), (table, r)
            n += 1
    print("hidden %d in_dim %d: %d rows, kernel %.3g, torch fp32 dev %.3g, tau %.3g, kernel / tau %.2f" % (
        hidden, in_dim, n, worst, ref["dev"], ref["tau"], worst / ref["tau"]))
    assert n == 5 * 15 and 0.0 < ref["tau"] < 1e-3
    assert worst <= ref["tau"], (worst, ref["tau"])


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_intersection_in_bits(hidden, in_dim):
    """(b) bounds[:4] is the intersection-and-fallback rule on the kernel's own `parts`, then the pad, bit for bit, at pad = 0 and pad =
    PAD; the pad leaves `parts` and the words 4..7 alone.  At eps = 0 the box has no width."""
    c = _case(hidden, in_dim)
    for name, pad in (("main", 0.0), ("padded", lc.PAD), ("zero", 0.0), ("wide", 0.0)):
        got, parts = c["out"][name]
        index = c["ref"]["tables"]["main" if name == "padded" else name]["index"]
        rows = np.flatnonzero(index >= 0)
        assert np.array_equal(_u32(got[rows][:, :4]), _u32(lc.intersect_f32(parts[rows], pad))), name
        if name == "zero":
            assert np.array_equal(_u32(got[rows][:, 0]), _u32(got[rows][:, 1])) and np.array_equal(_u32(got[rows][:, 2]), _u32(got[rows][:, 3]))
    (plain, p0), (padded, p1) = c["out"]["main"], c["out"]["padded"]
    assert np.array_equal(_u32(p0), _u32(p1)) and np.array_equal(_u32(plain[:, 4:]), _u32(padded[:, 4:]))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_soundness_on_the_devices_own_numbers(hidden, in_dim):
    """(c) With pad = PAD: obs_seen of copo_pgd_obs_seats_f32 at the three budgets on the same lists (+steer, +throttle, untargeted) and
    64 host-drawn samples of the box per row, through the unchanged act_seats: every mean lies inside the box, no element excluded and
    no slack beyond the pad."""
    c = _case(hidden, in_dim)
    ref, obs = c["ref"], c["inputs"]["obs"]
    for table, eps in lc.BUDGETS:
        p = c["probes"][table]
        b = p["padded"].astype(np.float64)
        rows = np.flatnonzero(ref["tables"][table]["index"] >= 0)
        lo, hi = b[rows][:, [0, 2]], b[rows][:, [1, 3]]
        moved = np.abs(p["seen"][rows].astype(np.float64) - obs[rows])
        assert float(moved.max()) <= float(F(eps)) + 2.0 ** -23          # (the float32 ends o +- eps are rounded once)
        assert (moved.max(axis=1) > 0.0).all() and len(rows) == 15
        gap = np.inf
        for m in [p["attack"]] + p["draws"]:
            m = m[rows].astype(np.float64)
            assert np.isfinite(m).all()
            gap = min(gap, float(np.minimum(m - lo, hi - m).min()))
            assert (m >= lo).all() and (m <= hi).all(), (table, float((lo - m).max()), float((m - hi).max()))
        print("hidden %d in_dim %d eps %.4g: smallest distance of a probe's mean to its padded bound %.3g (pad %.3g)" % (hidden, in_dim, eps, gap, lc.PAD))
        assert len(p["draws"]) == cc.BOX_DRAWS


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_against_the_interval_kernel(hidden, in_dim):
    """(d) Never looser than copo_cert_obs_seats_f32 on the same inputs: lo >= lo_I - tau, hi <= hi_I + tau; the words 4..7 match its
    words within tau.  Whether the clean means and the interval parts came out equal in bits is printed (DESIGN.md 8p records it)."""
    c = _case(hidden, in_dim)
    ref = c["ref"]
    mu_same = box_same = True
    for table in lc.TABLES:
        (got, parts), other = c["out"][table], c["interval"][table]
        rows = np.flatnonzero(ref["tables"][table]["index"] >= 0)
        g, o = got[rows].astype(np.float64), other[rows].astype(np.float64)
        slack = lambda x: ref["tau"] * np.maximum(1.0, np.abs(x))  # noqa: E731
        for a in (0, 2):
            assert (g[:, a] >= o[:, a] - slack(o[:, a])).all() and (g[:, a + 1] <= o[:, a + 1] + slack(o[:, a + 1])).all(), table
        assert (np.abs(g[:, 4:] - o[:, 4:]) <= slack(o[:, 4:])).all()
        mu_same = mu_same and np.array_equal(_u32(got[rows][:, 4:]), _u32(other[rows][:, 4:]))
        box_same = box_same and np.array_equal(_u32(parts[rows][:, 4:]), _u32(other[rows][:, :4]))
        hot = lc.LEVELS[ref["tables"][table]["index"][rows]][:, 0] > 0.0          # strictly narrower wherever there is a budget
        assert ((g[hot, 1] - g[hot, 0]) < (o[hot, 1] - o[hot, 0])).all() and ((g[hot, 3] - g[hot, 2]) < (o[hot, 3] - o[hot, 2])).all(), table
    print("hidden %d in_dim %d: clean means equal copo_cert_obs_seats_f32's in bits: %s; interval parts equal its box in bits: %s" % (
        hidden, in_dim, mu_same, box_same))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_tile_modes_and_determinism(hidden, in_dim):
    """(e), (f) A listed row whose group is out of range holds eight zeros in both outputs (in a mixed tile and in the all-invalid tile);
    rows in no list keep their poison in both; the masked one-row tile is certified; parts = NULL gives the same `bounds` bits; two
    launches give equal bits."""
    c = _case(hidden, in_dim)
    index = c["ref"]["tables"]["main"]["index"]
    for got in c["out"]["main"]:
        assert (_u32(got[index == -1]) == 0).all() and (index == -1).sum() == 3 and index[42] == -1
        assert (_u32(got[index == -2]) == POISON).all() and (index == -2).sum() == N_OUT - 18
    assert c["out"]["main"][0][9][6] == 1.0 and index[9] == 2
    for a, b in zip(c["out"]["main"], c["out"]["again"]):
        assert np.array_equal(_u32(a), _u32(b))
    assert np.array_equal(_u32(c["out"]["main"][0]), _u32(c["out"]["no_parts"][0]))


def test_certified_bounds_linear():
    """`certified_bounds(method="linear")` at one budget: the uniform table's launch in bits on the valid rows, zeros on every other row;
    `parts=True` returns the second array."""
    from copo_amd.eval.certify import certified_bounds
    c = _case(128, 92)
    obs = _dev(c["inputs"]["obs"])
    got = certified_bounds(c["bank"], c["pb"], obs, lc.EPS_WIDE, columns=(lc.COL_LO, lc.COL_HI), method="linear").cpu().numpy()
    valid = c["ref"]["tables"]["wide"]["index"] >= 0
    want, want_parts = c["out"]["wide"]
    assert np.array_equal(_u32(got[valid]), _u32(want[valid])) and (_u32(got[~valid]) == 0).all() and valid.sum() == 15
    b, p = certified_bounds(c["bank"], c["pb"], obs, lc.EPS_WIDE, lc.PAD, columns=(lc.COL_LO, lc.COL_HI), method="linear", parts=True)
    assert np.array_equal(_u32(p.cpu().numpy()[valid]), _u32(want_parts[valid])) and (_u32(p.cpu().numpy()[~valid]) == 0).all()
    assert np.array_equal(_u32(b.cpu().numpy()[valid][:, :4]), _u32(lc.intersect_f32(want_parts[valid], lc.PAD)))
    plain = certified_bounds(c["bank"], c["pb"], obs, lc.EPS_WIDE, columns=(lc.COL_LO, lc.COL_HI)).cpu().numpy()
    assert np.array_equal(_u32(plain[valid]), _u32(c["interval"]["wide"][valid]))          # the default is the interval launch


def test_refusals():
    """(g) What the Python layer and the entry refuse; nothing is written."""
    from copo_amd.eval.bank import PolicyBank
    c = lc.inputs(64, 91)
    bank = PolicyBank(_policy("ippo", 91, 64, False), c["members"])
    bank.sync_mirror()
    pb, lv = _plan_buffers(c), _levels(lc.LEVEL_OF["main"], lc.LEVELS)
    obs, bounds, parts = _dev(c["obs"]), _poison(N_OUT, 8), _poison(N_OUT, 8)
    for pad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception):
            bank.certify_seats(pb, lv, obs, bounds, lc.COL_LO, lc.COL_HI, pad, "linear", parts)
    with pytest.raises(Exception):
        bank.certify_seats(pb, lv, obs, bounds, lc.COL_LO, 92, 0.0, "linear", parts)
    for bad in (dict(obs=obs[:, :90].contiguous()), dict(bounds=_poison(N_OUT, 7)), dict(parts=_poison(N_OUT, 7)), dict(parts=_poison(N_OUT - 1, 8)),
                dict(bounds=torch.zeros(N_OUT, 8, dtype=torch.float64, device="cuda")), dict(method="crown"), dict(method="interval")):
        with pytest.raises(ValueError):
            bank.certify_seats(pb, lv, **dict(dict(obs=obs, bounds=bounds, parts=parts, method="linear"), **bad), col_lo=lc.COL_LO, col_hi=lc.COL_HI)
    with pytest.raises(ValueError):
        bank.certify_seats(pb, SimpleNamespace(K=2, G=lc.G, L=4, level_of=lv.level_of, levels=lv.levels), obs, bounds, lc.COL_LO, lc.COL_HI, 0.0, "linear")
    torch.cuda.synchronize()
    assert (_bits(bounds) == POISON).all() and (_bits(parts) == POISON).all()


# ---- (h) the sampler ---------------------------------------------------------------------------------------------------------------------
E2E = (8, 8, 4)          # scenes, slots, T
LEVELS = [dict(), dict(eps=0.0005, delta_steer=0.05, delta_throttle=0.05), dict(eps=0.01, delta_steer=0.05, delta_throttle=0.05)]


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


def test_linear_sampler(e2e):
    """The captured fragment equals the eager run in bits; actions, flags and the seat tally are a plain SeatSampler's in bits; cert_tally
    is certify_numpy.fold of the kernel's own bounds; method="interval" is today's CertifySeatSampler in bits."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.certify import CertifyPlan, CertifySeatSampler
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(2, 2, N, 0.5)
    assert plan.E == E and plan.n_groups == 4
    cert = CertifyPlan(LEVELS, np.array([[1, 2], [0, 1], [2, -1], [1, 1]], np.int32))
    bank = PolicyBank(t.policy, ws)
    keys = ("bounds", "cert_tally", "tally", "actions", "clipped", "flags", "obs", "dist_inputs")
    runs = {}
    for mode in (False, True):
        smp = CertifySeatSampler(t.env, t.policy, bank, plan, cert, T, use_graph=mode, method="linear")
        smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
        runs[mode] = _fragments(smp, 2, keys)
        assert (smp._loop.graph is not None) == mode and smp.method == "linear"
    for f in range(2):
        for k in keys:
            assert _same(runs[False][f][k], runs[True][f][k]), (f, k)
    drive = ("tally", "actions", "clipped", "flags", "obs")
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, drive)
    for f in range(2):
        for k in drive:
            assert _same(plain[f][k], runs[True][f][k]), (f, k)          # certification does not touch the drive
    # the fold of one more fragment from a cleared tally, restated on the kernel's own bounds
    smp.clear_tally()
    smp.sample()
    torch.cuda.synchronize()
    flags, bounds = smp.flags.cpu().numpy(), smp.bounds.cpu().numpy()
    want = np.zeros((plan.n_groups, bank.K, 8), np.int64)
    for s in range(T):
        cz.fold(flags[s], bounds[s], plan.seat, plan.group, cert.level_of, cert.words, bank.K, plan.n_groups, want)
    got = smp.cert_tally.cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert want[..., 0].sum() > 0 and want[..., 7].sum() == 0 and want[..., 4].sum() > 0
    # the interval method through the new keyword is the old sampler in bits, and the linear box is inside it
    old = _fragments(CertifySeatSampler(t.env, t.policy, bank, plan, cert, T, use_graph=False), 1, keys)
    new = _fragments(CertifySeatSampler(t.env, t.policy, bank, plan, cert, T, use_graph=False, method="interval"), 1, keys)
    for k in keys:
        assert _same(old[0][k], new[0][k]), k
    assert not _same(old[0]["bounds"], runs[False][0]["bounds"])
    lin, itv = runs[False][0]["bounds"], old[0]["bounds"]
    on = lin[..., 6] == 1
    assert torch.equal(on, itv[..., 6] == 1) and int(on.sum()) > 0
    assert bool(((lin[on][:, 1] - lin[on][:, 0]) <= (itv[on][:, 1] - itv[on][:, 0]) + 1e-5).all())


def test_certify_sweep_rows_linear_frame(golden_dir):
    from copo_amd.eval.certify import CERT_WORDS, LEVEL_FIELDS, CertifyLevel, certify_sweep_rows
    from copo_amd.eval.crossplay import SEAT_WORDS
    w = bc.golden_population(golden_dir, "copo_inter")
    levels = [CertifyLevel(0.0, 0.02, 0.02), CertifyLevel(0.0005, 0.02, 0.02), CertifyLevel(0.01, 0.02, 0.02)]
    N, steps, S = 8, 8, 2
    kw = dict(scenes_per_cell=S, num_agents=N, steps=steps, seed=0, labels=["a", "b"])
    df = certify_sweep_rows("copo", "inter", [w, dict(w)], levels, method="linear", **kw)
    rates = ["certified_rate", "certified_rate_steer", "certified_rate_throttle", "mean_width_steer", "mean_width_throttle", "max_dev"]
    seat_rates = ["success", "crash_rate", "out_rate", "reward_per_step"]
    assert list(df.columns) == ["checkpoint", "label", "level", "method", "member", "seats"] + list(LEVEL_FIELDS) + list(CERT_WORDS) + rates + list(SEAT_WORDS) + seat_rates
    assert [(r.checkpoint, r.level) for r in df.itertuples()] == [(k, l) for k in range(2) for l in range(3)] and (df["method"] == "linear").all()
    assert (df["rows"] == df["acted"]).all() and (df["rows"] >= steps).all() and (df["nonfinite"] == 0).all()
    ref = certify_sweep_rows("copo", "inter", [w, dict(w)], levels, **kw)
    assert "method" not in ref.columns and list(ref.columns) == [c for c in df.columns if c != "method"]
    for k in range(2):
        cell, base = df[df.checkpoint == k].sort_values("eps"), ref[ref.checkpoint == k].sort_values("eps")
        width, wide = cell["mean_width_steer"].tolist(), base["mean_width_steer"].tolist()
        assert width[0] == 0.0 and width[0] < width[1] < width[2] and width[1] < wide[1] and width[2] < wide[2], (width, wide)
        assert (cell["rows"].values == base["rows"].values).all() and (cell["certified"].values >= base["certified"].values).all()
