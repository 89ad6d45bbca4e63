"""Adversarial LiDAR on the GPU (copo_adv_obs_seats_f32, copo_amd/eval/adversary.py).  The kernel cases are those
of tests/adversary_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, three members with 0, 1 and 17 rows in lists of
32, 48 rows in 6 scenes of 8 slots, three scene groups, two level tables -- and tests/test_adversary_cpu.py measures on the float64
model alone what the comparisons here rely on.  Every case runs the kernel three times (with `grad`, again, without `grad`); its
outputs and the references are computed once and shared by the tests."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adversary_cases as ac
import adversary_numpy as an
import bank_cases as bc
import crossplay_numpy as cn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
CASES = [(h, k, t) for h in ac.HIDDENS for k in ac.IN_DIMS for t in ac.TABLES]


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


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim, table):
    from copo_amd.eval.bank import PolicyBank
    ref = ac.reference(hidden, in_dim, table)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), ref["members"])
    bank.sync_mirror()
    n_out = ac.E * ac.N
    pb = SimpleNamespace(K=ac.K, G=ac.G, N=ac.N, E=ac.E, cap=ac.CAP, n_out=n_out, rows=_dev(ref["rows"]), counts=_dev(ref["counts"]), group=_dev(ac.GROUP))
    ab = SimpleNamespace(K=ac.K, G=ac.G, L=len(ac.LEVELS), level_of=_dev(ac.LEVEL_OF[table]), levels=_dev(ac.LEVELS))
    obs = _dev(ref["obs"])
    out = {}
    for name, with_grad in (("first", True), ("second", True), ("no_grad", False)):
        seen, grad = _poison(n_out, in_dim), _poison(n_out, in_dim)
        bank.perturb_seats(pb, ab, obs, seen, ac.COL_LO, ac.COL_HI, grad=grad if with_grad else None)
        if name == "first":      # the seat forward right behind the launch, on the same stream, reads what it wrote
            eps = torch.randn(n_out, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(in_dim))
            fwd = [dict(action=_poison(n_out, 2), logp=_poison(n_out), dist_inputs=_poison(n_out, 4), clipped=_poison(n_out, 2)) for _ in range(2)]
            bank.act_seats(pb, seen, eps, **fwd[0])
            torch.cuda.synchronize()
            bank.act_seats(pb, seen.clone(), eps, **fwd[1])          # ... and called alone on a copy
        torch.cuda.synchronize()
        out[name] = (seen.cpu().numpy(), grad.cpu().numpy())
    assert _same(obs, _dev(ref["obs"]))                              # the true observation is left alone
    return dict(ref=ref, out=out, fwd=[{k: v.cpu().numpy() for k, v in f.items()} for f in fwd])


def _row_kinds(ref, table):
    """Per row: 'none' (in no list), 'copy' (no direction or no level), 'grad' (a direction at eps == 0), 'move' (perturbed)."""
    kinds = ["none"] * (ac.E * ac.N)
    for k in range(ac.K):
        for r in ref["rows"][k][:ref["counts"][k]]:
            lv = an.level_index(int(r), ac.N, k, ac.GROUP, ac.LEVEL_OF[table], len(ac.LEVELS))
            direction = lv >= 0 and (ac.LEVELS[lv][1] != 0.0 or ac.LEVELS[lv][2] != 0.0)
            kinds[int(r)] = "copy" if not direction else ("move" if ac.LEVELS[lv][0] != 0.0 else "grad")
    return kinds


def _eps_of_row(ref, table, r):
    for k in range(ac.K):
        if r in ref["rows"][k][:ref["counts"][k]].tolist():
            return ac.LEVELS[an.level_index(r, ac.N, k, ac.GROUP, ac.LEVEL_OF[table], len(ac.LEVELS))][0]
    raise AssertionError(r)


@pytest.mark.parametrize("hidden,in_dim,table", CASES)
def test_grad_against_float64(hidden, in_dim, table):
    """The bound is measured per case, not fixed: `dev` = the deviation of torch fp32 CPU autograd from the float64 model on the same
    rows, max_j |g32 - g64| / max_j |g64|, largest row; tau = 4 dev, measured where the test runs (torch's fp32 sums depend on the
    host's CPU).  Measured over the sixteen (hidden, width, table) cases on an MI355X host: dev 3.1e-7 .. 1.1e-6, tau 1.3e-6 .. 4.4e-6,
    the kernel's error against float64 in the same measure 3.8e-7 .. 1.1e-6, at most 0.44 of its case's tau (on a second host: dev
    2.3e-7 .. 7.4e-7, tau 9.1e-7 .. 3.0e-6, which the same kernel figures also meet).  Every figure is printed before it is asserted."""
    c = _case(hidden, in_dim, table)
    ref, (seen, grad) = c["ref"], c["out"]["first"]
    kinds = _row_kinds(ref, table)
    worst = 0.0
    for r, kind in enumerate(kinds):
        if kind == "none":
            assert (_u32(grad[r]) == POISON).all(), r
        elif kind == "copy":
            assert (_u32(grad[r]) == 0).all(), r
        else:
            g64 = ref["grad"][r]
            worst = max(worst, float(np.abs(grad[r].astype(np.float64) - g64).max() / np.abs(g64).max()))
    print("hidden %d in_dim %d table %s: kernel %.3g, torch fp32 %.3g, tau %.3g" % (hidden, in_dim, table, worst, ref["dev"], ref["tau"]))
    assert kinds.count("move") == (11 if table == "A" else 7) and kinds.count("grad") == (0 if table == "A" else 1)
    assert worst <= ref["tau"], (worst, ref["tau"])


@pytest.mark.parametrize("hidden,in_dim,table", CASES)
def test_obs_seen(hidden, in_dim, table):
    """(a) bit-equal to clamp(obs + eps sign(grad of the kernel), 0, 1) recomputed in numpy fp32 on the LiDAR columns and to obs
    elsewhere; (b) the signs are the float64 model's wherever |g| > tau max|g|, and at most 1 % of the elements are left out of that
    comparison; (c) pass-through rows and all-identity tiles are obs bit for bit, rows in no list keep their NaN."""
    c = _case(hidden, in_dim, table)
    ref, (seen, grad), obs = c["ref"], c["out"]["first"], c["ref"]["obs"]
    kinds = _row_kinds(ref, table)
    lo, hi = ac.COL_LO, ac.COL_HI
    compared = left_out = 0
    for r, kind in enumerate(kinds):
        if kind == "none":
            assert (_u32(seen[r]) == POISON).all(), r
        elif kind in ("copy", "grad"):
            assert np.array_equal(_u32(seen[r]), _u32(obs[r])), (r, kind)
        else:
            eps = np.float32(_eps_of_row(ref, table, r))
            want = obs[r].copy()
            want[lo:hi] = np.clip(obs[r][lo:hi] + eps * np.sign(grad[r][lo:hi]).astype(np.float32), np.float32(0.0), np.float32(1.0))
            assert want.dtype == np.float32 and np.array_equal(_u32(seen[r]), _u32(want)), r
            g64 = ref["grad"][r][lo:hi]
            big = np.abs(g64) > ref["tau"] * np.abs(ref["grad"][r]).max()
            compared, left_out = compared + int(big.sum()), left_out + int((~big).sum())
            assert np.array_equal(np.sign(grad[r][lo:hi])[big], np.sign(g64)[big]), r
            assert np.array_equal(seen[r][lo:hi][big], ref["seen"][r][lo:hi][big].astype(np.float32)), r
    assert compared > 0 and left_out <= 0.01 * (compared + left_out)
    assert any(not np.array_equal(_u32(seen[r]), _u32(obs[r])) for r, kind in enumerate(kinds) if kind == "move")
    if table == "A":          # member 2's second tile is row 42 alone, at level index -1: an all-identity tile
        assert kinds[42] == "copy" and kinds[41] == "copy" and kinds[0] == "move" and kinds[16] == "move"


@pytest.mark.parametrize("hidden,in_dim,table", CASES)
def test_no_interference_and_determinism(hidden, in_dim, table):
    c = _case(hidden, in_dim, table)
    a, b, n = c["out"]["first"], c["out"]["second"], c["out"]["no_grad"]
    assert np.array_equal(_u32(a[0]), _u32(b[0])) and np.array_equal(_u32(a[1]), _u32(b[1]))          # two launches: the same bits
    assert np.array_equal(_u32(a[0]), _u32(n[0])) and (_u32(n[1]) == POISON).all()                      # without `grad`: the same obs_seen
    for key in ("action", "logp", "dist_inputs", "clipped"):
        assert np.array_equal(_u32(c["fwd"][0][key]), _u32(c["fwd"][1][key])), key
    seated = np.array(_row_kinds(c["ref"], table)) != "none"
    assert not (_u32(c["fwd"][0]["logp"])[seated] == POISON).any() and (_u32(c["fwd"][0]["logp"])[~seated] == POISON).all()


def test_beam_saliency_is_the_gradient_and_perturbs_nothing():
    from copo_amd.eval.adversary import beam_saliency
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    hidden, in_dim = 64, 91
    ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
    seat = np.full((ac.E, ac.N), -1, np.int32)
    seat.reshape(-1)[[3, 20, 21]] = [0, 2, 2]
    bank = PolicyBank(_policy("ippo", in_dim, hidden, False), ws)
    g = beam_saliency(bank, PlanBuffers(SeatPlan(seat, n_members=3), "cuda"), _dev(obs), 1.0, 0.0).cpu().numpy()
    for r in range(ac.E * ac.N):
        k = int(seat.reshape(-1)[r])
        if k < 0:
            assert (g[r] == 0.0).all()
        else:
            g64 = an.input_gradient(ac.net_of(ws[k]), obs[r].astype(np.float64), 1.0, 0.0)
            assert np.abs(g[r] - g64).max() <= 1e-5 * np.abs(g64).max()          # (the measured bound is test_grad_against_float64's)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
E2E = (8, 8, 4)          # scenes, slots, T
ATTACK = [dict(), dict(eps=0.1, throttle=1.0), dict(eps=0.05, steer=1.0, throttle=-0.5)]


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
    from copo_amd.eval.adversary import AdversaryPlan
    from copo_amd.eval.crossplay import SeatPlan
    plan = SeatPlan.pairs(2, 2, E2E[1], 0.5)
    assert plan.E == E2E[0] and plan.n_groups == 4
    return plan, AdversaryPlan(ATTACK, np.array([[1, 2], [0, 1], [2, -1], [1, 1]], np.int32))


def test_captured_fragment_equals_eager(e2e):
    from copo_amd.eval.adversary import AdversarialSeatSampler
    from copo_amd.eval.bank import PolicyBank
    t, ws = e2e
    E, N, T = E2E
    plan, adv = _plans()
    bank = PolicyBank(t.policy, ws)
    keys = ("obs_seen", "clipped", "flags", "tally", "obs")
    runs = {}
    for mode in (False, True):
        smp = AdversarialSeatSampler(t.env, t.policy, bank, plan, adv, T, use_graph=mode)
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
    # group 1's focal seats (level 0) and group 2's partner seats (index -1) pass through
    seat, group = torch.from_numpy(plan.seat).cuda(), torch.from_numpy(plan.group).cuda()[:, None]
    calm = ((group == 1) & (seat == 0)) | ((group == 2) & (seat == 1))
    assert _same(last["obs_seen"][:, calm], last["obs"][:T][:, calm]) and int(calm.sum()) == 2 * 2 * N // 2


def test_identity_plan_is_the_plain_seat_sampler_and_set_adversary_keeps_the_graph(e2e):
    from copo_amd.eval.adversary import AdversarialSeatSampler, AdversaryPlan
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan, adv = _plans()
    bank = PolicyBank(t.policy, ws)
    keys = ("obs", "clipped", "flags", "tally")
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, keys)
    calm = AdversaryPlan([dict(), dict(eps=0.1), dict(steer=1.0)], adv.level_of)          # three identities, the shapes of `adv`
    smp = AdversarialSeatSampler(t.env, t.policy, bank, plan, calm, T, use_graph=True)
    smp._loop.warmup = 0
    got = _fragments(smp, 2, keys + ("obs_seen",))
    for f in range(2):
        for k in keys:
            assert _same(plain[f][k], got[f][k]), (f, k)
        assert _same(got[f]["obs_seen"], got[f]["obs"][:T])
    assert plain[1]["tally"][:, :, 0].sum() > 0
    graph = smp._loop.graph
    smp.set_adversary(adv)                                              # the same shapes: copied in, the graph stays
    assert smp._loop.graph is graph and graph is not None
    hot = _fragments(smp, 1, ("obs_seen", "obs"))
    assert not _same(hot[0]["obs_seen"], hot[0]["obs"][:T])
    smp.set_adversary(AdversaryPlan(ATTACK[:2], np.ones((4, 2), np.int32)))      # another L: the graph is dropped
    assert smp._loop.graph is None
    with pytest.raises(ValueError):
        smp.set_adversary(AdversaryPlan(ATTACK, np.zeros((5, 2), np.int32)))


def test_adversary_sweep_rows_frame(golden_dir):
    from copo_amd.eval.adversary import LEVEL_FIELDS, AdversarialSeatSampler, AdversaryLevel, AdversaryPlan, adversary_sweep_rows
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SEAT_WORDS, SeatSampler
    from copo_amd.eval.evaluate import make_eval_trainer
    w = bc.golden_population(golden_dir, "copo_inter")
    levels = [AdversaryLevel(), AdversaryLevel(eps=0.1, throttle=1.0)]
    N, steps, S = 8, 100, 2
    df = adversary_sweep_rows("copo", "inter", [w, dict(w)], levels, scenes_per_cell=S, num_agents=N, steps=steps, seed=0, labels=["a", "b"])
    rates = ["success", "crash_rate", "out_rate", "reward_per_step"]
    words = list(SEAT_WORDS)
    assert list(df.columns) == ["checkpoint", "label", "level", "role", "member", "share", "seats", "own_level"] + list(LEVEL_FIELDS) + words + rates
    assert [(r.checkpoint, r.level, r.role, r.member) for r in df.itertuples()] == [(0, 0, "impaired", 0), (0, 1, "impaired", 0),
                                                                                     (1, 0, "impaired", 1), (1, 1, "impaired", 1)]
    assert list(df["label"]) == ["a", "a", "b", "b"] and (df["share"] == 1.0).all() and (df["seats"] == N).all()
    for r in df.itertuples():
        assert {k: getattr(r, k) for k in LEVEL_FIELDS} == levels[r.level].as_dict() and r.own_level == r.level
        assert r.reward_per_step == r.reward_q16 / 65536.0 / r.acted
    assert (df["acted"] >= steps).all() and (df["done"] <= df["acted"]).all()
    seats, adv = AdversaryPlan.sweep(2, levels, S, N, 1.0)
    t = make_eval_trainer("copo", "inter", seats.E, N, 0)
    try:
        # the identity rows hold what a plain SeatSampler tallies on the same plan, seeds and noise
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
    # the attack moves the action the way it aims to: over the run the mean throttle of the agents that acted is strictly higher in the
    # attacked cells than in the identity cells (crash rates are not asserted: nobody has measured them)
    t = make_eval_trainer("copo", "inter", seats.E, N, 0)
    try:
        smp = AdversarialSeatSampler(t.env, t.policy, PolicyBank(t.policy, [w, w]), seats, adv, t.sampler.T, use_graph=t.config.get("use_hip_graphs", True))
        total, count = torch.zeros(seats.n_groups, dtype=torch.float64, device="cuda"), torch.zeros(seats.n_groups, dtype=torch.float64, device="cuda")
        for _ in range(-(-steps // smp.T)):
            smp.sample()
            acted = ((smp.flags & 1) > 0).view(smp.T, seats.n_groups, S * N).to(torch.float64)
            total += (smp.clipped[..., 1].view(smp.T, seats.n_groups, S * N).to(torch.float64) * acted).sum((0, 2))
            count += acted.sum((0, 2))
        again = smp.tally.cpu().numpy()
    finally:
        t.stop()
    mean = (total / count).cpu().numpy()
    print("mean throttle per cell (checkpoint x level):", mean.tolist())
    for r in df.itertuples():          # the same run again: the frame's words
        assert [int(getattr(r, c)) for c in words] == again[r.checkpoint * 2 + r.level, r.member].tolist()
    for k in range(2):
        assert mean[k * 2 + 1] > mean[k * 2], (k, mean.tolist())
