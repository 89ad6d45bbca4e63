"""Iterated adversarial LiDAR on the GPU (copo_pgd_obs_seats_f32, copo_amd/eval/pgd.py).  The kernel cases are
those of tests/pgd_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, adversary_cases' 48 rows and lists, one level
table, `max_iters` = 4 -- and tests/test_pgd_cpu.py measures on the model alone what the comparisons here rely on.  Every case launches
the kernel a handful of times; its outputs and the references are computed once and shared by the tests."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adversary_cases as ac
import bank_cases as bc
import crossplay_numpy as cn
import pgd_cases as pc
import pgd_numpy as pn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
CASES = [(h, k) for h in pc.HIDDENS for k in pc.IN_DIMS]
N_OUT = pc.E * pc.N


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


def _buffers(c, group, level_of, words):
    pb = SimpleNamespace(K=pc.K, G=pc.G, N=pc.N, E=pc.E, cap=pc.CAP, n_out=N_OUT, rows=_dev(c["rows"]), counts=_dev(c["counts"]), group=_dev(group))
    gb = SimpleNamespace(K=pc.K, G=pc.G, L=len(words), level_of=_dev(level_of), levels=_dev(words), max_iters=pc.MAX_ITERS)
    return pb, gb


def _launch(bank, pb, gb, obs, in_dim, tick, max_iters=pc.MAX_ITERS, with_trace=True):
    seen = _poison(N_OUT, in_dim)
    trace = _poison(max_iters, N_OUT, in_dim) if with_trace else None
    bank.pgd_seats(pb, gb, obs, seen, pc.COL_LO, pc.COL_HI, pc.SEED, tick, trace, max_iters)
    torch.cuda.synchronize()
    return seen.cpu().numpy(), None if trace is None else trace.cpu().numpy(), None if tick is None else tick.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    c = pc.inputs(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), c["members"])
    bank.sync_mirror()
    pb, gb = _buffers(c, pc.GROUP, pc.LEVEL_OF, pc.words())
    obs = _dev(c["obs"])
    zero = lambda: torch.zeros(N_OUT, dtype=torch.int32, device="cuda")  # noqa: E731
    out = dict(first=_launch(bank, pb, gb, obs, in_dim, zero()), second=_launch(bank, pb, gb, obs, in_dim, zero()),
               no_tick=_launch(bank, pb, gb, obs, in_dim, None, with_trace=False), cut=_launch(bank, pb, gb, obs, in_dim, zero(), max_iters=1))
    tick = _dev(out["first"][2])
    out["next"] = _launch(bank, pb, gb, obs, in_dim, tick)
    # adversary_cases' table A through both entry points
    pa, ga = _buffers(c, ac.GROUP, ac.LEVEL_OF["A"], pc.fgsm_words())
    out["fgsm"] = _launch(bank, pa, ga, obs, in_dim, zero(), with_trace=False)
    one = _poison(N_OUT, in_dim)
    bank.perturb_seats(pa, SimpleNamespace(K=pc.K, G=pc.G, L=len(ac.LEVELS), level_of=ga.level_of, levels=_dev(ac.LEVELS)), obs, one, ac.COL_LO, ac.COL_HI)
    torch.cuda.synchronize()
    out["adv"] = one.cpu().numpy()
    assert _same(obs, _dev(c["obs"]))                              # the true observation is left alone
    return dict(inputs=c, out=out, replay=pc.model(hidden, in_dim, trace=out["first"][1]))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_replay_of_the_trace_gives_obs_seen(hidden, in_dim):
    """(a) Following the signs of the kernel's own trace, the numpy model gives obs_seen bit for bit on every listed row: the start, the
    step, the projection, the per-row iteration count and the rows frozen past it.  Rows that pass through equal obs in bits, rows in
    no list keep their poison, the trace is zero past a row's count, tick is 1 on listed rows and 0 elsewhere."""
    c = _case(hidden, in_dim)
    obs, (seen, trace, tick), m = c["inputs"]["obs"], c["out"]["first"], c["replay"]
    lo, hi = pc.COL_LO, pc.COL_HI
    for r in range(N_OUT):
        it = int(m["its"][r])
        if it < 0:
            assert (_u32(seen[r]) == POISON).all() and (_u32(trace[:, r]) == POISON).all() and tick[r] == 0, r
            continue
        assert tick[r] == 1, r
        assert np.array_equal(_u32(seen[r]), _u32(m["seen"][r])), (r, it)
        assert np.array_equal(_u32(seen[r][:lo]), _u32(obs[r][:lo])) and np.array_equal(_u32(seen[r][hi:]), _u32(obs[r][hi:])), r
        assert (_u32(trace[it:, r]) == 0).all(), (r, it)
        if it == 0:
            assert np.array_equal(_u32(seen[r]), _u32(obs[r])), r
        else:
            assert np.isfinite(trace[:it, r]).all() and all(np.abs(trace[i, r]).max() > 0.0 for i in range(it)), r
            assert not np.array_equal(_u32(seen[r]), _u32(obs[r])), r
    assert sorted(set(m["its"].tolist())) == [-1, 0, 1, 2, 3, 4]
    # max_iters = 1 cuts every level short
    seen1, trace1, _ = c["out"]["cut"]
    m1 = pc.model(hidden, in_dim, max_iters=1, trace=trace1)
    listed = m1["its"] >= 0
    assert np.array_equal(_u32(seen1[listed]), _u32(m1["seen"][listed])) and (_u32(seen1[~listed]) == POISON).all() and m1["its"].max() == 1


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_trace_against_float64(hidden, in_dim):
    """(b) Every trace[i] of an attacked row against the float64 gradient at the iterate that the replay reconstructs, as
    max_j |g - g64| / max_j |g64| per row and iteration.  The bound is measured per case, not fixed: `dev` = the same quantity for torch
    fp32 CPU autograd against float64 on the same iterate and objective, largest over the case; tau = 4 dev (`tanh_fast` and the MFMA
    order re-associate fp32 sums as torch does, only differently: the rule of test_gpu_adversary.py).  Every figure is printed before it
    is asserted."""
    c = _case(hidden, in_dim)
    trace, m, inp = c["out"]["first"][1], c["replay"], c["inputs"]
    worst = dev = 0.0
    n = 0
    for r, xs in m["iterates"].items():
        k, level = m["member"][r], m["level"][r]
        for i in range(int(m["its"][r])):
            g64 = pn.gradient(inp["nets"][k], xs[i], inp["obs"][r], level)
            top = np.abs(g64).max()
            g32 = pc.torch_gradient(inp["members"][k], xs[i], inp["obs"][r], level, torch.float32)
            dev = max(dev, float(np.abs(g32.astype(np.float64) - g64).max() / top))
            worst = max(worst, float(np.abs(trace[i, r].astype(np.float64) - g64).max() / top))
            n += 1
    tau = 4.0 * dev
    print("hidden %d in_dim %d: %d gradients, kernel %.3g, torch fp32 dev %.3g, tau %.3g, kernel / tau %.2f" % (hidden, in_dim, n, worst, dev, tau, worst / tau))
    assert n == 5 * 4 + 5 * 3 + 4 * 1 + 2 and 0.0 < tau < 1e-2
    assert worst <= tau, (worst, tau)


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_one_step_equals_the_fgsm_entry(hidden, in_dim):
    """(c) adversary_cases' table A with its levels as iters = 1, alpha = eps, flags = 0: obs_seen of both entry points, bit for bit."""
    c = _case(hidden, in_dim)
    assert np.array_equal(_u32(c["out"]["fgsm"][0]), _u32(c["out"]["adv"]))
    adv, obs = _u32(c["out"]["adv"]), _u32(c["inputs"]["obs"])
    assert int(((adv != obs).any(axis=1) & (adv[:, 0] != POISON)).sum()) == 11          # table A's eleven perturbed rows


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_determinism_and_the_tick(hidden, in_dim):
    """(d) Two launches from equal ticks: the same bits.  tick == NULL reads as 0.  A launch from the advanced tick differs on the rows
    with a random start and on no other row."""
    c = _case(hidden, in_dim)
    a, b, n, nxt = c["out"]["first"], c["out"]["second"], c["out"]["no_tick"], c["out"]["next"]
    assert np.array_equal(_u32(a[0]), _u32(b[0])) and np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(a[2], b[2])
    assert np.array_equal(_u32(a[0]), _u32(n[0]))
    m = c["replay"]
    random = np.array([r in m["level"] and bool(int(m["level"][r][5]) & pn.RANDOM_START) for r in range(N_OUT)])
    differs = (_u32(a[0]) != _u32(nxt[0])).any(axis=1)
    assert np.array_equal(differs, random) and random.sum() == 10
    assert np.array_equal(nxt[2], 2 * a[2]) and a[2].sum() == 18
    m2 = pc.model(hidden, in_dim, trace=nxt[1], tick=a[2])
    listed = m2["its"] >= 0
    assert np.array_equal(_u32(nxt[0][listed]), _u32(m2["seen"][listed]))


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_the_attack_raises_its_objective(hidden, in_dim):
    """(e) J64(obs_seen) > J64(o) on every targeted attacked row; |mu(obs_seen) - mu(o)| > 0 on every untargeted one."""
    c = _case(hidden, in_dim)
    seen, m, inp = c["out"]["first"][0], c["replay"], c["inputs"]
    gains, moves = [], []
    for r, level in m["level"].items():
        net, o = inp["nets"][m["member"][r]], inp["obs"][r]
        if int(level[5]) & pn.UNTARGETED:
            moves.append(float(np.abs(pn.mu(net, seen[r]) - pn.mu(net, o)).max()))
        else:
            gains.append(pn.objective(net, seen[r], o, level) - pn.objective(net, o, o, level))
    print("hidden %d in_dim %d: smallest gain %.3g of %d, smallest move %.3g of %d" % (hidden, in_dim, min(gains), len(gains), min(moves), len(moves)))
    assert len(gains) == 6 and len(moves) == 9 and min(gains) > 0.0 and min(moves) > 0.0


def test_refusals():
    """(f) What the Python layer and the entry refuse; nothing is written."""
    from copo_amd.eval.bank import PolicyBank
    c = pc.inputs(64, 91)
    bank = PolicyBank(_policy("ippo", 91, 64, False), c["members"])
    bank.sync_mirror()
    pb, gb = _buffers(c, pc.GROUP, pc.LEVEL_OF, pc.words())
    obs, seen = _dev(c["obs"]), _poison(N_OUT, 91)
    for bad in (dict(max_iters=0), dict(max_iters=17)):
        with pytest.raises(Exception):
            bank.pgd_seats(pb, gb, obs, seen, pc.COL_LO, pc.COL_HI, 0, None, None, **bad)
    with pytest.raises(Exception):
        bank.pgd_seats(pb, gb, obs, seen, pc.COL_LO, 92, 0, None, None)
    for bad in (dict(tick=torch.zeros(N_OUT, dtype=torch.int64, device="cuda")), dict(trace=torch.zeros(3, N_OUT, 91, device="cuda")),
                dict(tick=torch.zeros(N_OUT - 1, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            bank.pgd_seats(pb, gb, obs, seen, pc.COL_LO, pc.COL_HI, 0, **dict(dict(tick=None, trace=None), **bad))
    with pytest.raises(ValueError):
        bank.pgd_seats(pb, gb, obs[:, :90].contiguous(), seen, pc.COL_LO, pc.COL_HI)
    torch.cuda.synchronize()
    assert (_bits(seen) == POISON).all()


# ---- (g) the sampler ---------------------------------------------------------------------------------------------------------------------
E2E = (8, 8, 4)          # scenes, slots, T
ATTACK = [dict(), dict(eps=0.1, throttle=1.0, alpha=0.05, iters=3), dict(eps=0.05, alpha=0.02, iters=2, random_start=True, untargeted=True)]


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
    from copo_amd.eval.crossplay import SeatPlan
    from copo_amd.eval.pgd import PGDPlan
    plan = SeatPlan.pairs(2, 2, E2E[1], 0.5)
    assert plan.E == E2E[0] and plan.n_groups == 4
    return plan, PGDPlan(ATTACK, np.array([[1, 2], [0, 1], [2, -1], [1, 1]], np.int32))


def test_captured_fragment_equals_eager_and_the_tick_counts_steps(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.pgd import PGDSeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan, pgd = _plans()
    bank = PolicyBank(t.policy, ws)
    keys = ("obs_seen", "clipped", "flags", "tally", "obs", "tick", "dist_inputs")
    runs = {}
    for mode in (False, True):
        smp = PGDSeatSampler(t.env, t.policy, bank, plan, pgd, T, use_graph=mode, seed=11)
        smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
        runs[mode] = _fragments(smp, 2, keys)
        assert (smp._loop.graph is not None) == mode
    for f in range(2):
        for k in keys:
            assert _same(runs[False][f][k], runs[True][f][k]), (f, k)
    last = runs[True][1]
    lo, hi = smp.col_lo, smp.col_hi
    assert (lo, hi) == (19, 91) and not _same(last["obs_seen"], last["obs"][:T]) and last["tally"][:, :, 0].sum() > 0
    assert _same(last["obs_seen"][..., :lo], last["obs"][:T][..., :lo]) and _same(last["obs_seen"][..., hi:], last["obs"][:T][..., hi:])
    moved = (last["obs_seen"][..., lo:hi] - last["obs"][:T][..., lo:hi]).abs()
    assert float(moved.max()) <= 0.1 + 1e-6 and float(last["obs_seen"][..., lo:hi].min()) >= 0.0 and float(last["obs_seen"][..., lo:hi].max()) <= 1.0
    seat, group = torch.from_numpy(plan.seat).cuda(), torch.from_numpy(plan.group).cuda()[:, None]
    calm = ((group == 1) & (seat == 0)) | ((group == 2) & (seat == 1))
    assert _same(last["obs_seen"][:, calm], last["obs"][:T][:, calm]) and int(calm.sum()) == 2 * 2 * N // 2
    # tick = steps on seated rows (every seat of `pairs` is seated), 0 after reset
    assert (last["tick"] == 2 * T).all() and (runs[True][0]["tick"] == T).all()
    # the seat forward on obs_seen equals act_seats called by hand
    out = dict(action=_poison(E * N, 2), logp=_poison(E * N), dist_inputs=_poison(E * N, 4), clipped=_poison(E * N, 2))
    bank.act_seats(smp.seated.buffers, last["obs_seen"][T - 1].reshape(E * N, -1).contiguous(), smp.eps[T - 1].view(E * N, 2), **out)
    torch.cuda.synchronize()
    assert _same(out["dist_inputs"], last["dist_inputs"][T - 1].reshape(E * N, 4))
    smp.reset()
    assert int(smp.tick.abs().sum()) == 0


def test_identity_plan_is_the_plain_seat_sampler_and_set_pgd_keeps_the_graph(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatSampler
    from copo_amd.eval.pgd import PGDPlan, PGDSeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan, pgd = _plans()
    bank = PolicyBank(t.policy, ws)
    keys = ("obs", "clipped", "flags", "tally")
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, keys)
    calm = PGDPlan([dict(), dict(eps=0.1, alpha=0.1, iters=3), dict(throttle=1.0, alpha=0.1, iters=2)], pgd.level_of)      # identities, iters as `pgd`
    assert calm.max_iters == pgd.max_iters
    smp = PGDSeatSampler(t.env, t.policy, bank, plan, calm, T, use_graph=True)
    smp._loop.warmup = 0
    got = _fragments(smp, 2, keys + ("obs_seen",))
    for f in range(2):
        for k in keys:
            assert _same(plain[f][k], got[f][k]), (f, k)
        assert _same(got[f]["obs_seen"], got[f]["obs"][:T])
    assert plain[1]["tally"][:, :, 0].sum() > 0
    graph = smp._loop.graph
    smp.set_pgd(pgd)                                              # the same shapes: copied in, the graph stays
    assert smp._loop.graph is graph and graph is not None
    hot = _fragments(smp, 1, ("obs_seen", "obs"))
    assert not _same(hot[0]["obs_seen"], hot[0]["obs"][:T])
    smp.set_pgd(PGDPlan(ATTACK[:2], np.ones((4, 2), np.int32)))      # another L: the graph is dropped
    assert smp._loop.graph is None
    with pytest.raises(ValueError):
        smp.set_pgd(PGDPlan(ATTACK, np.zeros((5, 2), np.int32)))


def test_pgd_sweep_rows_frame(golden_dir):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SEAT_WORDS, SeatSampler
    from copo_amd.eval.evaluate import make_eval_trainer
    from copo_amd.eval.pgd import LEVEL_FIELDS, PGDLevel, PGDPlan, pgd_sweep_rows
    w = bc.golden_population(golden_dir, "copo_inter")
    levels = [PGDLevel(), PGDLevel(eps=0.1, throttle=1.0, alpha=0.05, iters=3)]
    N, steps, S = 8, 40, 2
    df = pgd_sweep_rows("copo", "inter", [w, dict(w)], levels, scenes_per_cell=S, num_agents=N, steps=steps, seed=0, labels=["a", "b"])
    rates = ["success", "crash_rate", "out_rate", "reward_per_step"]
    words = list(SEAT_WORDS)
    assert list(df.columns) == ["checkpoint", "label", "level", "role", "member", "share", "seats", "own_level"] + list(LEVEL_FIELDS) + words + rates
    assert [(r.checkpoint, r.level, r.role, r.member) for r in df.itertuples()] == [(0, 0, "impaired", 0), (0, 1, "impaired", 0),
                                                                                     (1, 0, "impaired", 1), (1, 1, "impaired", 1)]
    for r in df.itertuples():
        assert {k: getattr(r, k) for k in LEVEL_FIELDS} == levels[r.level].as_dict() and r.own_level == r.level
    assert (df["acted"] >= steps).all()
    seats, _ = PGDPlan.sweep(2, levels, S, N, 1.0)
    t = make_eval_trainer("copo", "inter", seats.E, N, 0)
    try:          # the identity rows hold what a plain SeatSampler tallies on the same plan, seeds and noise
        smp = SeatSampler(t.env, t.policy, PolicyBank(t.policy, [w, w]), seats, t.sampler.T, use_graph=t.config.get("use_hip_graphs", True))

        def cell_noise():          # the sweep's rule: the first cell's draw in every cell
            smp.eps.normal_()
            cells = smp.eps.view(smp.T, seats.n_groups, S, N, 2)
            cells[:, 1:].copy_(cells[:, :1])
        smp._draw_noise = cell_noise
        for _ in range(-(-steps // smp.T)):
            smp.sample()
        tally = smp.tally.cpu().numpy()
    finally:
        t.stop()
    for k in range(2):
        row = df[(df.checkpoint == k) & (df.level == 0)].iloc[0]
        assert [int(row[c]) for c in words] == tally[k * 2, k].tolist(), (k, row[words].tolist(), tally[k * 2, k].tolist())
    assert tally[:, :, 0].sum() > 0
