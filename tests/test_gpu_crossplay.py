"""Cross-play on the GPU (copo_mlp_forward_seats_f32, copo_seat_tally, copo_amd/eval/crossplay.py).  Every comparison is of bits or
integers.

Forward: an output row of the forward kernel is a fixed-order sum over its own inputs, and seat mode always runs the one-tile kernel,
so member k's rows must hold what `FusedLearner.act` (the one-tile single-member kernel at these sizes) writes for member k's weights
on its gathered rows; rows with seat -1 keep the poison they were filled with.  Tally: integers, against the python loops of
tests/crossplay_numpy.py.  End to end: the tally of a 60-step rollout of two populations against the device's trip log joined on
(scene, slot) -> seat; the captured sampler against the eager one; the (i, i) groups against a dense bank of member i."""
import ctypes as C

import numpy as np
import pytest
import torch

import bank_cases as bc
import crossplay_numpy as cn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import CANARY, _outputs, _policy  # noqa: E402

KEYS = ("dist_inputs", "action", "logp", "clipped")


def _bits(t):
    return t.view(torch.int32)


def _tables(E, N):
    """Two seat tables of K = 3.  (a): member 0 has no seat, member 1 one seat, member 2 seventeen rows (cap = 17), the rest nobody.
    (b): scattered over the slots, member 1 seventeen rows, member 0 nearly half of all rows (35 slots: 14, 200 slots: 97 = 6 x 16 + 1,
    seven workgroups), member 2 a sixteenth, the rest nobody."""
    n = E * N
    pick = np.random.RandomState(n).permutation(n)
    a = np.full(n, -1, np.int32)
    a[pick[0]] = 1
    a[pick[1:18]] = 2
    b = np.full(n, -1, np.int32)
    b[pick[:17]] = 1
    n0 = n // 2 - 3
    b[pick[17:17 + n0]] = 0
    b[pick[17 + n0:17 + n0 + n // 16]] = 2
    return a.reshape(E, N), b.reshape(E, N)


def _seats_against_single(golden_dir, name, odim, hidden, E, N, bf16):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.checkpoint_io import load_policy_weights
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    pol = _policy(name, odim, hidden, bf16)
    ws = bc.members(golden_dir, name + "_inter", odim, hidden, 3)
    g = torch.Generator(device="cuda").manual_seed(odim + E * N)
    obs = torch.rand(E * N, odim, device="cuda", generator=g) * 2 - 1
    eps = torch.randn(E * N, 2, device="cuda", generator=g)
    bank = PolicyBank(pol, ws)
    bank.sync_mirror()
    for seat in _tables(E, N):
        plan = SeatPlan(seat, n_members=3)
        assert plan.cap % 16 != 0 and 17 in plan.counts.tolist()
        want = _outputs(E * N)
        for k, w in enumerate(ws):
            n = int(plan.counts[k])
            if n == 0:
                continue
            load_policy_weights(pol.model, w)
            pol.fused.invalidate_mirror()
            pol.fused.sync_mirror()
            rows = torch.from_numpy(plan.rows[k, :n]).cuda()
            one = _outputs(n)
            pol.fused.act(obs[rows].contiguous(), eps[rows].contiguous(), one["action"], one["logp"], one["dist_inputs"], one["clipped"])
            for key in KEYS:
                assert not bool((_bits(one[key]) == CANARY).any()), key
                want[key][rows] = one[key]
        got = _outputs(E * N)
        bank.act_seats(PlanBuffers(plan, "cuda"), obs, eps, got["action"], got["logp"], got["dist_inputs"], got["clipped"])
        torch.cuda.synchronize()
        nobody = torch.from_numpy(seat.reshape(-1) < 0).cuda()
        assert bool(nobody.any())
        for key in KEYS:
            a, b = _bits(got[key]), _bits(want[key])
            assert bool((a[nobody] == CANARY).all()), "%s: a row with seat -1 was written" % key
            if not torch.equal(a, b):
                bad = torch.nonzero((a != b).reshape(E * N, -1).any(1)).reshape(-1)
                raise AssertionError("%s differs in %d rows, first row %d (member %d)" % (key, bad.numel(), int(bad[0]), int(seat.reshape(-1)[int(bad[0])])))
    return bank, obs, eps


@pytest.mark.parametrize("E,N", [(5, 7), (5, 40)])
@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("name,odim", [("copo", 92), ("ippo", 91)])
def test_seat_forward_equals_single_member_forward_on_gathered_rows(golden_dir, name, odim, hidden, E, N):
    _seats_against_single(golden_dir, name, odim, hidden, E, N, False)


def test_seat_forward_bf16_operands(golden_dir):
    _seats_against_single(golden_dir, "copo", 92, 64, 5, 7, True)


@pytest.mark.parametrize("hidden", [64, 256])
def test_uniform_plan_equals_the_dense_bank(golden_dir, hidden):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    K, per, N = 3, 2, 7
    pol = _policy("copo", 92, hidden, False)
    bank = PolicyBank(pol, bc.members(golden_dir, "copo_inter", 92, hidden, K))
    bank.sync_mirror()
    g = torch.Generator(device="cuda").manual_seed(hidden)
    obs = torch.rand(K * per * N, 92, device="cuda", generator=g) * 2 - 1
    eps = torch.randn(K * per * N, 2, device="cuda", generator=g)
    want, got = _outputs(K * per * N), _outputs(K * per * N)
    bank.act(obs, eps, want["action"], want["logp"], want["dist_inputs"], want["clipped"])
    plan = SeatPlan.uniform(np.arange(K * per) // per, N)
    bank.act_seats(PlanBuffers(plan, "cuda"), obs, eps, got["action"], got["logp"], got["dist_inputs"], got["clipped"])
    torch.cuda.synchronize()
    for key in KEYS:
        assert not bool((_bits(want[key]) == CANARY).any()) and torch.equal(_bits(got[key]), _bits(want[key])), key


def test_refusals_launch_nothing(golden_dir):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    pol = _policy("copo", 92, 64, False)
    bank = PolicyBank(pol, bc.members(golden_dir, "copo_inter", 92, 64, 3))
    bank.sync_mirror()
    plan = SeatPlan(_tables(5, 7)[1], n_members=3)
    pb = PlanBuffers(plan, "cuda")
    obs, eps = torch.zeros(35, 92, device="cuda"), torch.zeros(35, 2, device="cuda")
    out = _outputs(35)
    lib = bank._capi.lib

    def call(**kw):
        a = dict(cfg=C.byref(bank.cfg), theta=bank.theta.data_ptr(), theta_t=bank.theta_t.data_ptr(), stride=bank.stride, K=3,
                 rows=pb.rows.data_ptr(), counts=pb.counts.data_ptr(), cap=pb.cap, n_out=35, obs=obs.data_ptr(), dist=out["dist_inputs"].data_ptr(),
                 eps=eps.data_ptr(), action=out["action"].data_ptr(), logp=out["logp"].data_ptr(), clipped=out["clipped"].data_ptr(),
                 stream=bank._capi.current_stream())
        a.update(kw)
        return lib.copo_mlp_forward_seats_f32(*a.values())
    assert call(rows=None) == -1 and call(counts=None) == -1 and call(obs=None) == -1 and call(action=None) == -1
    assert call(cap=0) == -2 and call(n_out=0) == -2 and call(K=0) == -2 and call(K=65536) == -2
    assert call(stride=bank.stride - 4) == -2 and call(stride=bank.stride + 2) == -2
    with pytest.raises(ValueError, match="rows"):
        bank.act_seats(pb, obs[:34], eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])
    torch.cuda.synchronize()
    for key in KEYS:
        assert bool((_bits(out[key]) == CANARY).all()), key
    assert call() == 0                  # the same arguments, none replaced, do launch
    torch.cuda.synchronize()
    assert not bool((_bits(out["logp"])[torch.from_numpy(plan.seat.reshape(-1) >= 0).cuda()] == CANARY).any())


# ---- tally ---------------------------------------------------------------------------------------------------------------------------
def _tally_case(E, N, K, G, seed):
    rng = np.random.RandomState(seed)
    flags = np.resize(rng.permutation(256).astype(np.uint8), E * N)       # every bit combination once E * N >= 256, spread over the slots
    rng.shuffle(flags)
    rew = rng.normal(0.0, 2.0, E * N).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 2000.0, -2000.0, 0.5 / 65536, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, 1024.0, 0.0], np.float32)
    where = rng.permutation(E * N)[:min(E * N, 4 * len(special))]
    rew[where] = np.resize(special, len(where))
    seat = rng.randint(-1, K + 1, (E, N)).astype(np.int32)                 # -1 and K: nobody's
    group = rng.randint(-1, G + 1, E).astype(np.int32)                     # -1 and G: no group's
    if E == 1:
        group[:] = G - 1
    return flags.reshape(E, N), rew.reshape(E, N), seat, group


@pytest.mark.parametrize("E,N,K,G", [(1, 7, 1, 1), (3, 64, 3, 5), (3, 130, 64, 1), (1030, 7, 3, 5), (1030, 130, 64, 5), (1, 130, 3, 1)])
def test_tally_is_exact(E, N, K, G):
    from copo_amd import _capi
    flags, rew, seat, group = _tally_case(E, N, K, G, E + N + K)
    if E * N >= 256:
        assert len(np.unique(flags)) == 256
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d_flags, d_rew, d_seat, d_group = dev(flags), dev(rew), dev(seat), dev(group)
    out = torch.zeros(G + 1, K, 8, dtype=torch.int64, device="cuda")       # one group longer: the tail must stay 0
    call = lambda r: _capi.check(_capi.lib.copo_seat_tally(d_flags.data_ptr(), _capi.ptr(r), d_seat.data_ptr(), d_group.data_ptr(), E, N, K, G,  # noqa: E731
                                                           out.data_ptr(), _capi.current_stream()))
    call(d_rew)
    want = cn.tally(flags, rew, seat, group, K, G)
    got = out.cpu().numpy()
    assert np.array_equal(got[:G], want), np.argwhere(got[:G] != want)[:8].tolist()
    assert not got[G].any() and want[:, :, 0].sum() > 0
    # a second call without rewards accumulates the counts and leaves the reward word
    call(None)
    want2 = cn.tally(flags, None, seat, group, K, G, want.copy())
    got = out.cpu().numpy()
    assert np.array_equal(got[:G], want2) and not got[G].any()
    assert np.array_equal(want2[:, :, 6], want[:, :, 6]) and np.array_equal(want2[:, :, 0], 2 * want[:, :, 0])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(golden_dir):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    from copo_amd.eval.evaluate import make_eval_trainer
    plan = SeatPlan.pairs(*cn.E2E_PAIRS)
    t = make_eval_trainer("copo", "inter", plan.E, plan.N, cn.E2E_SEED)
    ws = cn.e2e_members(golden_dir)
    yield t, plan, ws, PolicyBank(t.policy, ws)
    t.stop()


def _fixed_noise(smp, noise, per):
    """Every group of `per` scenes gets noise[fragment] [T, per, N, 2]: what `BankSampler` does with its one draw per member."""
    state = dict(f=0)

    def draw():
        smp.eps.view(smp.T, smp.E // per, per, smp.N, 2).copy_(noise[state["f"]].unsqueeze(1))
        state["f"] += 1
    smp._draw_noise = draw


def _run(smp, n_frag):
    keep = []
    for _ in range(n_frag):
        b = smp.sample()
        torch.cuda.synchronize()
        keep.append({k: b[k].clone() for k in ("obs", "actions", "action_logp", "rewards", "flags")})
    return keep


def test_tally_equals_the_trip_log_joined_on_seats(e2e):
    from copo_amd import trips
    from copo_amd.eval.crossplay import SeatSampler
    t, plan, ws, bank = e2e
    smp = SeatSampler(t.env, t.policy, bank, plan, 1, use_graph=False)
    log = trips.TripLog(t.env.sim)
    try:
        smp.reset()
        log.record()
        for _ in range(cn.E2E_STEPS):
            smp.sample()
            log.record(smp.flags[0], smp.rew3[0, 0])
        log.flush()
        table = log.table()
        assert table.meta["dropped"] == 0
        joined = cn.trip_join(table.columns, plan.seat, plan.group, plan.K, plan.n_groups)
    finally:
        log.close()
    tally = smp.tally.cpu().numpy()
    print(tally[:, :, :6].tolist())
    assert np.array_equal(tally[:, :, :5], joined), (tally[:, :, :5].tolist(), joined.tolist())
    for g in range(plan.n_groups):           # the premise (tests/test_crossplay_cpu.py asserts it on the oracle): nothing compared is empty
        for k in {int(plan.focal[g]), int(plan.partner[g])}:
            assert tally[g, k, 1] >= 1 and tally[g, k, 0] >= cn.E2E_STEPS, (g, k, tally[g, k].tolist())
    assert not tally[0, 1].any() and not tally[3, 0].any()          # member 1 has no seat in group (0, 0), member 0 none in (1, 1)


def test_captured_fragment_equals_eager_and_the_diagonal_equals_a_dense_bank(e2e):
    from copo_amd.eval.bank import BankSampler, PolicyBank
    from copo_amd.eval.crossplay import SeatSampler
    t, plan, ws, bank = e2e
    K, per, N, _ = cn.E2E_PAIRS
    T, n_frag = cn.E2E_T, cn.E2E_STEPS // cn.E2E_T
    g = torch.Generator(device="cuda").manual_seed(7)
    noise = [torch.randn(T, per, N, 2, device="cuda", generator=g) for _ in range(n_frag)]
    runs = {}
    for mode in (False, True):
        smp = SeatSampler(t.env, t.policy, bank, plan, T, use_graph=mode)
        _fixed_noise(smp, noise, per)
        smp.reset()
        runs[mode] = (_run(smp, n_frag), smp.tally.cpu().numpy())
        if mode:
            assert smp._loop.graph is not None          # the third fragment was a replay
    (eager, tally_e), (graphed, tally_g) = runs[False], runs[True]
    for f in range(n_frag):
        for k in eager[f]:
            a, b = eager[f][k], graphed[f][k]
            assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), (f, k)
    assert np.array_equal(tally_e, tally_g) and tally_e[:, :, 1].sum() >= 8
    # scenes of group (i, i) against a dense bank whose member on those scenes is i: the same seeds, the same noise
    dense = BankSampler(t.env, t.policy, PolicyBank(t.policy, [ws[0], ws[0], ws[1], ws[1]]), T, use_graph=False)
    _fixed_noise(dense, noise, per)
    dense.reset()
    ref = _run(dense, n_frag)
    for i in range(K):
        grp = i * K + i
        s = slice(grp * per, (grp + 1) * per)
        tot = np.zeros((1, 1, 8), np.int64)
        for f in range(n_frag):
            for k in ("actions", "obs", "flags", "rewards"):
                a, b = eager[f][k][:, s], ref[f][k][:, s]
                assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b), (i, f, k)
            fl, rw = ref[f]["flags"][:, s].cpu().numpy(), ref[f]["rewards"][:, s].cpu().numpy()
            for step in range(T):
                cn.tally(fl[step], rw[step], np.zeros((per, N), np.int32), np.zeros(per, np.int32), 1, 1, tot)
        assert np.array_equal(tot[0, 0], tally_e[grp, i]), (i, tot.tolist(), tally_e[grp, i].tolist())
    assert not torch.equal(eager[-1]["actions"][:, :per], eager[-1]["actions"][:, -per:])          # the two members do differ


def test_pairs_plan_shares_its_scenes_between_the_pairs_and_not_its_noise(e2e):
    """A plan that declares `replica_scenes` is seeded one replica's seeds tiled; a `SeatSampler`'s noise stays every seat's own.  On the
    module's fixture, 4 pairs of 3 scenes x 40 slots, T = 4."""
    from copo_amd.eval.crossplay import SeatSampler
    t, plan, ws, bank = e2e
    K, per, N, _ = cn.E2E_PAIRS
    assert plan.replica_scenes == per
    smp = SeatSampler(t.env, t.policy, bank, plan, 4, use_graph=False)
    torch.manual_seed(3)
    smp.reset()
    obs0 = _bits(smp.obs[0]).view(K * K, per, N, smp.O).clone()
    assert torch.equal(obs0, obs0[:1].expand_as(obs0)) and bool(obs0.any())
    assert all(not torch.equal(obs0[0, a], obs0[0, b]) for a in range(per) for b in range(a))          # a replica's own scenes differ
    smp.obs[smp.T].copy_(smp.obs[0])          # (`sample()` after an explicit `reset()` starts from `obs[T]`)
    smp.sample()
    torch.cuda.synchronize()
    eps = smp.eps.view(smp.T, K * K, per, N, 2)
    assert all(not torch.equal(eps[:, r], eps[:, 0]) for r in range(1, K * K))


def test_cross_play_rows_frame(golden_dir):
    from copo_amd.eval.crossplay import SEAT_WORDS, cross_play_rows
    ws = cn.e2e_members(golden_dir)
    df = cross_play_rows("copo", "inter", ws, share=0.25, scenes_per_pair=2, num_agents=8, steps=40, seed=0, labels=["a", "b"])
    assert list(df.columns) == ["focal", "partner", "member", "label", "share"] + list(SEAT_WORDS) + ["success", "crash_rate", "out_rate", "reward_per_step"]
    assert [(r.focal, r.partner, r.member) for r in df.itertuples()] == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 1), (1, 0, 0), (1, 1, 1)]
    assert list(df["label"]) == ["a", "a", "b", "b", "a", "b"] and (df["share"] == 0.25).all()
    assert (df["acted"] >= 40).all() and (df["done"] <= df["acted"]).all()
    for r in df.itertuples():
        for rate, word in (("success", r.arrive), ("crash_rate", r.crash), ("out_rate", r.out)):
            v = getattr(r, rate)
            assert (np.isnan(v) and r.done == 0) or v == word / r.done
        assert r.reward_per_step == r.reward_q16 / 65536.0 / r.acted
