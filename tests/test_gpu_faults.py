"""Fault injection on the GPU (copo_fault_obs, copo_fault_act, copo_amd/eval/faults.py).  Every comparison is of bits or integers.

Kernels: against the python loops of tests/fault_numpy.py on the seeded cases of tests/fault_cases.py -- 15 rows and 200 rows of an odd
width with an odd first beam column, seats and groups outside their ranges, level indices outside theirs, ticks that differ per row,
three levels with the identity among them; fault_act three calls in a row over hand-made previous flags.  Sampler: identity levels
against the plain `SeatSampler`, the captured fragment against the eager one, healthy seats next to impaired ones, and the frame of
`fault_sweep_rows` with its level-0 rows against a plain `SeatSampler` on the same plan."""
import numpy as np
import pytest
import torch

import crossplay_numpy as cn
import fault_cases as fc
import fault_numpy as fn

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(E, N):
    seat, group, level_of, K, G = fc.tables(E, N, E * N)
    return seat, group, level_of, K, G, fc.level_words(), fc.ticks(E, N, E + N)


@pytest.mark.parametrize("E,N,O,col_lo,col_hi", fc.SHAPES)
def test_fault_obs_holds_the_models_bits(E, N, O, col_lo, col_hi):
    from copo_amd import _capi
    seat, group, level_of, K, G, levels, tick = _case(E, N)
    obs = fc.observations(E, N, O, O)
    want = fn.fault_obs(obs, col_lo, col_hi, seat, group, level_of, levels, tick, fc.SEED)
    d_obs, d_seat, d_group, d_lof, d_lv, d_tick = _dev(obs), _dev(seat), _dev(group), _dev(level_of), _dev(levels.view(np.int32)), _dev(tick)
    seen = torch.full((E * N + 1, O), POISON, dtype=torch.int32, device="cuda")          # one row longer: the tail must stay poison
    _capi.check(_capi.lib.copo_fault_obs(d_obs.data_ptr(), seen.data_ptr(), E, N, O, col_lo, col_hi, d_seat.data_ptr(), d_group.data_ptr(), K, G,
                                         d_lof.data_ptr(), d_lv.data_ptr(), len(levels), d_tick.data_ptr(), fc.SEED, _capi.current_stream()))
    got = seen.cpu().numpy().view(np.uint32)
    assert (got[E * N] == POISON).all()
    got, want_b = got[:E * N].reshape(E, N, O), _u32(want)
    assert np.array_equal(got, want_b), np.argwhere(got != want_b)[:8].tolist()
    assert np.array_equal(d_tick.cpu().numpy(), tick) and np.array_equal(_u32(d_obs.cpu().numpy()), _u32(obs))      # inputs untouched
    # what the case holds: rows that pass through for each reason and at the identity level, beams dropped, beams moved, both clamp ends
    lv = np.array([fn.level_of_row(r, N, seat, group, K, G, level_of, len(levels)) for r in range(E * N)]).reshape(E, N)
    assert {-1, 0, 1, 2} <= set(lv.reshape(-1).tolist())
    same = _u32(want) == _u32(obs)
    assert same[lv <= 0].all() and same[:, :, :col_lo].all() and same[:, :, col_hi:].all()
    beams, src = want[:, :, col_lo:col_hi], obs[:, :, col_lo:col_hi]
    assert (~same[lv == 1][:, col_lo:col_hi]).mean() > 0.5 and ((beams[lv == 2] == 1.0) & (src[lv == 2] != 1.0)).any()
    assert ((beams == 0.0) & (src != 0.0)).any() and ((beams == 1.0) & (src != 1.0)).any()
    assert -1 in seat and K in seat and -1 in group and (E <= 3 or G in group) and -1 in level_of and len(levels) in level_of


@pytest.mark.parametrize("E,N", [s[:2] for s in fc.SHAPES])
def test_fault_act_holds_the_models_bits_over_three_calls(E, N):
    from copo_amd import _capi
    seat, group, level_of, K, G, levels, tick = _case(E, N)
    prev = fc.actions(E, N, 99)
    d_seat, d_group, d_lof, d_lv = _dev(seat), _dev(group), _dev(level_of), _dev(levels.view(np.int32))
    d_prev, d_tick = _dev(prev), _dev(tick)
    lv = np.array([fn.level_of_row(r, N, seat, group, K, G, level_of, len(levels)) for r in range(E * N)]).reshape(E, N)
    stuck = np.zeros((E, N), bool)
    # call 0 without flags, calls 1 and 2 with hand-made previous flags: same occupant, DONE, SPAWNED, not ACTED, ENV_RESET
    for call, flags in enumerate((None, fc.previous_flags(E, N, 1), fc.previous_flags(E, N, 2))):
        act = fc.actions(E, N, call)
        w_act, w_prev, w_tick = fn.fault_act(act, prev, flags, seat, group, level_of, levels, tick, fc.SEED)
        d_act = _dev(act)
        d_flags = None if flags is None else _dev(flags)
        _capi.check(_capi.lib.copo_fault_act(d_act.data_ptr(), d_prev.data_ptr(), _capi.ptr(d_flags), E, N, d_seat.data_ptr(), d_group.data_ptr(), K, G,
                                             d_lof.data_ptr(), d_lv.data_ptr(), len(levels), d_tick.data_ptr(), fc.SEED, _capi.current_stream()))
        for name, got, want in (("act", d_act, w_act), ("prev", d_prev, w_prev)):
            g = _u32(got.cpu().numpy())
            assert np.array_equal(g, _u32(want)), (call, name, np.argwhere(g != _u32(want))[:8].tolist())
        assert np.array_equal(d_tick.cpu().numpy(), w_tick) and np.array_equal(w_tick, tick + 1)           # every row, pass-through rows too
        assert np.array_equal(_u32(w_act[lv <= 0]), _u32(act[lv <= 0])) and np.array_equal(_u32(w_prev), _u32(w_act))
        if flags is not None:
            same = ((flags & fn.ACTED) != 0) & ((flags & (fn.DONE | fn.SPAWNED | fn.ENV_RESET)) == 0)
            if E * N >= 100:          # (the 15 rows hold what their seed gives them; the 200 hold every case at the sticky level)
                for bit in (fn.DONE, fn.SPAWNED, fn.ENV_RESET):
                    assert (((flags & bit) != 0) & (lv == 2)).any()
            assert ((flags & fn.ACTED) == 0).any() and (same & (lv == 2)).any()
            # with act_sigma 0.5 on top a stuck action is not recognisable in `act`; count the draws that fired on eligible rows
            thr = int(levels[2][4])
            for r in np.nonzero((same & (lv == 2)).reshape(-1))[0]:
                stuck[r // N, r % N] |= (fn.hash_rng(fc.SEED, int(r), int(tick[r]), 0, fn.STICKY) >> 8) < thr
        prev, tick = w_prev, w_tick
    assert stuck.any()
    assert np.array_equal(tick, fc.ticks(E, N, E + N) + 3)


def test_sticky_alone_repeats_the_previous_action_of_the_same_occupant_only():
    """A level with nothing but sticky = 1: the device's `act` is `prev` exactly where the previous flags say "same occupant"."""
    from copo_amd import _capi
    E, N = 3, 5
    levels = np.stack([fn.words(), fn.words(sticky=1.0)])
    seat, group, level_of = np.zeros((E, N), np.int32), np.zeros(E, np.int32), np.array([[1]], np.int32)
    flags, act, prev = fc.previous_flags(E, N, 5), fc.actions(E, N, 6), fc.actions(E, N, 7)
    d_act, d_prev, d_tick = _dev(act), _dev(prev), torch.zeros(E * N, dtype=torch.int32, device="cuda")
    d_flags, d_seat, d_group, d_lof, d_lv = _dev(flags), _dev(seat), _dev(group), _dev(level_of), _dev(levels.view(np.int32))
    _capi.check(_capi.lib.copo_fault_act(d_act.data_ptr(), d_prev.data_ptr(), d_flags.data_ptr(), E, N, d_seat.data_ptr(), d_group.data_ptr(), 1, 1,
                                         d_lof.data_ptr(), d_lv.data_ptr(), 2, d_tick.data_ptr(), fc.SEED, _capi.current_stream()))
    same = ((flags & fn.ACTED) != 0) & ((flags & (fn.DONE | fn.SPAWNED | fn.ENV_RESET)) == 0)
    want = np.where(same[:, :, None], prev, act)
    assert same.any() and not same.all()
    assert np.array_equal(_u32(d_act.cpu().numpy()), _u32(want)) and np.array_equal(_u32(d_prev.cpu().numpy()), _u32(want))
    assert (d_tick.cpu().numpy() == 1).all()


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
E2E = (4, 8, 4)          # scenes, slots, T
HARSH = dict(lidar_sigma=0.1, lidar_dropout=0.1, dropout_value=1.0, act_sigma=0.2, sticky=0.25)


@pytest.fixture(scope="module")
def e2e(golden_dir):
    from copo_amd.eval.evaluate import make_eval_trainer
    t = make_eval_trainer("copo", "inter", E2E[0], E2E[1], 0)
    yield t, cn.e2e_members(golden_dir)
    t.stop()


def _fragments(smp, n_frag, keys, seed=3):
    """`n_frag` fragments after a reset under one torch seed (the action noise); clones of `keys` per fragment.  `sample()` after an
    explicit `reset()` starts from `obs[T]`, as between fragments, so the reset's observation is put there."""
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    keep = []
    for _ in range(n_frag):
        smp.sample()
        torch.cuda.synchronize()
        keep.append({k: getattr(smp, k).clone() for k in keys})
    return keep


def test_identity_levels_are_the_plain_seat_sampler(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    from copo_amd.eval.faults import FaultLevel, FaultPlan, FaultySeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(2, 1, N, 0.5)
    assert plan.E == E
    bank = PolicyBank(t.policy, ws)
    faults = FaultPlan([FaultLevel(), FaultLevel()], np.arange(plan.n_groups * 2).reshape(plan.n_groups, 2) % 2)
    keys = ("obs", "clipped", "flags", "tally")
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, keys)
    faulty = FaultySeatSampler(t.env, t.policy, bank, plan, faults, T, use_graph=False, fault_seed=fc.SEED)
    got = _fragments(faulty, 2, keys + ("obs_seen", "tick"))
    for f in range(2):
        for k in keys:
            assert _same(plain[f][k], got[f][k]), (f, k)
        assert _same(got[f]["obs_seen"], got[f]["obs"][:T]) and (got[f]["tick"] == (f + 1) * T).all()
    assert plain[1]["tally"][:, :, 0].sum() > 0 and not _same(plain[0]["obs"], plain[1]["obs"])


def test_captured_fragment_equals_eager(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    from copo_amd.eval.faults import FaultLevel, FaultPlan, FaultySeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(2, 1, N, 0.5)
    bank = PolicyBank(t.policy, ws)
    faults = FaultPlan([FaultLevel(**HARSH)], np.zeros((plan.n_groups, 2), np.int32))
    keys = ("obs_seen", "clipped", "tally", "tick", "obs", "flags")
    runs = {}
    for mode in (False, True):
        smp = FaultySeatSampler(t.env, t.policy, bank, plan, faults, T, use_graph=mode, fault_seed=fc.SEED)
        smp._loop.warmup = 0          # capture at the first fragment (the eager run before it has loaded every kernel): both fragments replay
        runs[mode] = _fragments(smp, 2, keys)
        assert (smp._loop.graph is not None) == mode
    for f in range(2):
        for k in keys:
            assert _same(runs[False][f][k], runs[True][f][k]), (f, k)
        # the capture itself runs nothing and every replay advances the device's counter
        assert (runs[True][f]["tick"] == (f + 1) * T).all()
    last = runs[True][1]
    assert not _same(last["obs_seen"], last["obs"][:T]) and last["tally"][:, :, 0].sum() > 0
    lo, hi = smp.col_lo, smp.col_hi
    assert _same(last["obs_seen"][..., :lo], last["obs"][:T][..., :lo]) and _same(last["obs_seen"][..., hi:], last["obs"][:T][..., hi:])
    beams = last["obs_seen"][..., lo:hi]
    assert beams.min() >= 0.0 and beams.max() <= 1.0


def test_reset_clears_the_fault_state_and_set_faults_keeps_the_graph(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    from copo_amd.eval.faults import FaultLevel, FaultPlan, FaultySeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(2, 1, N, 0.5)
    harsh = FaultPlan([FaultLevel(**HARSH)], np.zeros((plan.n_groups, 2), np.int32))
    smp = FaultySeatSampler(t.env, t.policy, PolicyBank(t.policy, ws), plan, harsh, T, use_graph=True, fault_seed=fc.SEED)
    smp._loop.warmup = 0
    first = _fragments(smp, 2, ("obs_seen", "clipped", "tick"))
    assert smp.prev.abs().sum() > 0 and smp.flags[T - 1].any()
    again = _fragments(smp, 2, ("obs_seen", "clipped", "tick"))          # reset: tick, prev and the previous flags start over
    for f in range(2):
        for k in first[f]:
            assert _same(first[f][k], again[f][k]), (f, k)
    graph = smp._loop.graph
    smp.set_faults(FaultPlan([FaultLevel()], np.zeros((plan.n_groups, 2), np.int32)))          # the same shapes: copied in, the graph stays
    assert smp._loop.graph is graph and graph is not None
    calm = _fragments(smp, 1, ("obs_seen", "obs"))
    assert _same(calm[0]["obs_seen"], calm[0]["obs"][:T])
    smp.set_faults(FaultPlan([FaultLevel(), FaultLevel(**HARSH)], np.ones((plan.n_groups, 2), np.int32)))      # another L: the graph is dropped
    assert smp._loop.graph is None
    smp._loop.warmup = 0
    back = _fragments(smp, 2, ("obs_seen", "clipped", "tick"))
    for f in range(2):
        for k in first[f]:
            assert _same(first[f][k], back[f][k]), (f, k)
    with pytest.raises(ValueError):
        smp.set_faults(FaultPlan([FaultLevel()], np.zeros((plan.n_groups + 1, 2), np.int32)))


def test_healthy_seats_next_to_impaired_ones_are_untouched(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.faults import FaultLevel, FaultPlan, FaultySeatSampler, sweep_members
    t, ws = e2e
    E, N, T = E2E
    seats, faults = FaultPlan.sweep(2, [FaultLevel(), FaultLevel(**HARSH)], 1, N, share=0.25)
    assert seats.E == E and faults.n_impaired == 2 and seats.K == 4
    smp = FaultySeatSampler(t.env, t.policy, PolicyBank(t.policy, sweep_members(ws, faults)), seats, faults, T, use_graph=False,
                            fault_seed=fc.SEED)
    forward_out = []
    act = smp.seated.act

    def recording_act(obs, eps, action, logp, dist_inputs, clipped=None):          # eager: what the forward wrote, before fault_act
        act(obs, eps, action, logp, dist_inputs, clipped)
        forward_out.append(clipped.clone())
    smp.seated.act = recording_act
    frags = _fragments(smp, 2, ("obs", "obs_seen", "clipped"))
    assert len(forward_out) == 2 * T
    healthy = torch.from_numpy(seats.seat < 2).cuda()                               # members 0, 1; members 2, 3 are the impaired copies
    harsh_cell = torch.from_numpy(np.repeat(faults.level == 1, faults.scenes_per_cell)).cuda()[:, None] & ~healthy
    assert int(healthy.sum()) == E * (N - 2) and int(harsh_cell.sum()) == 2 * 2
    moved_obs = moved_act = 0
    for f in range(2):
        obs, seen, clipped = frags[f]["obs"][:T], frags[f]["obs_seen"], frags[f]["clipped"]
        for s in range(T):
            fwd = forward_out[f * T + s]
            assert _same(seen[s][healthy], obs[s][healthy]) and _same(clipped[s][healthy], fwd[healthy]), (f, s)
            calm = ~healthy & ~harsh_cell                                           # the "impaired" seats of a level-0 cell
            assert _same(seen[s][calm], obs[s][calm]) and _same(clipped[s][calm], fwd[calm]), (f, s)
            moved_obs += int((_bits(seen[s][harsh_cell]) != _bits(obs[s][harsh_cell])).sum())
            moved_act += int((_bits(clipped[s][harsh_cell]) != _bits(fwd[harsh_cell])).sum())
    assert moved_obs > 0 and moved_act > 0


def test_sweep_plan_shares_scenes_and_noise_between_its_cells(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.faults import FaultLevel, FaultPlan, FaultySeatSampler, sweep_members
    t, ws = e2e
    E, N, T = E2E
    seats, faults = FaultPlan.sweep(1, [FaultLevel(), FaultLevel(**HARSH)], 2, N, share=1.0)          # two cells of two scenes
    assert seats.E == E and seats.replica_scenes == 2 == faults.scenes_per_cell
    smp = FaultySeatSampler(t.env, t.policy, PolicyBank(t.policy, sweep_members(ws[:1], faults)), seats, faults, T, use_graph=False,
                            fault_seed=fc.SEED)
    _fragments(smp, 1, ("eps",))
    smp.reset()
    obs0, eps = _bits(smp.obs[0]).view(2, 2, N, smp.O), _bits(smp.eps).view(T, 2, 2, N, 2)
    assert torch.equal(obs0[1], obs0[0]) and not torch.equal(obs0[0, 0], obs0[0, 1])
    assert torch.equal(eps[:, 1], eps[:, 0]) and not torch.equal(eps[:, 0, 0], eps[:, 0, 1]) and bool(eps.any())


def test_hand_built_plan_without_replica_scenes_gets_the_plain_samplers_seeds(e2e):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan(np.arange(E * N).reshape(E, N) % 2, n_members=2)
    assert plan.replica_scenes is None
    smp = SeatSampler(t.env, t.policy, PolicyBank(t.policy, ws), plan, T, use_graph=False)
    smp.reset()
    obs0 = _bits(smp.obs[0]).clone()
    assert all(not torch.equal(obs0[a], obs0[b]) for a in range(E) for b in range(a))          # every scene its own
    t.sampler.reset()
    assert _same(t.sampler.obs[0], smp.obs[0]) and torch.equal(_bits(smp.obs[0]), obs0)


def test_fault_sweep_rows_frame(golden_dir):
    import bank_cases as bc
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SEAT_WORDS, SeatSampler
    from copo_amd.eval.evaluate import make_eval_trainer
    from copo_amd.eval.faults import LEVEL_FIELDS, FaultLevel, FaultPlan, fault_sweep_rows
    w = bc.golden_population(golden_dir, "copo_inter")
    levels = [FaultLevel(), FaultLevel(**HARSH)]
    N, steps = 8, 40
    df = fault_sweep_rows("copo", "inter", [w, dict(w)], levels, scenes_per_cell=2, num_agents=N, steps=steps, seed=0, labels=["a", "b"])
    rates = ["success", "crash_rate", "out_rate", "reward_per_step"]
    assert list(df.columns) == ["checkpoint", "label", "level", "role", "member", "share", "seats", "own_level"] + list(LEVEL_FIELDS) + \
        list(SEAT_WORDS) + rates
    assert [(r.checkpoint, r.level, r.role, r.member) for r in df.itertuples()] == [(0, 0, "impaired", 0), (0, 1, "impaired", 0),
                                                                                     (1, 0, "impaired", 1), (1, 1, "impaired", 1)]
    assert list(df["label"]) == ["a", "a", "b", "b"] and (df["share"] == 1.0).all() and (df["seats"] == N).all()
    for r in df.itertuples():
        assert {k: getattr(r, k) for k in LEVEL_FIELDS} == levels[r.level].as_dict() and r.own_level == r.level
        for rate, word in (("success", r.arrive), ("crash_rate", r.crash), ("out_rate", r.out)):
            v = getattr(r, rate)
            assert (np.isnan(v) and r.done == 0) or v == word / r.done
        assert r.reward_per_step == r.reward_q16 / 65536.0 / r.acted
    assert (df["acted"] >= steps).all() and (df["done"] <= df["acted"]).all()
    # The two checkpoints are the same population, and every cell has the same scene seeds and the same action noise: their level-0 rows
    # are equal, word for word.  Their harsh rows are not compared: the kernels key every fault draw by the absolute row e N + n, which
    # differs between the two cells.  (No ordering of success between the levels is asserted: 40 steps prove nothing there.)
    words = list(SEAT_WORDS)
    same_cols = ["level", "role", "share", "seats", "own_level"] + list(LEVEL_FIELDS)
    by_k = [df[df.checkpoint == k].reset_index(drop=True) for k in range(2)]
    assert by_k[0][same_cols].equals(by_k[1][same_cols])
    assert by_k[0].loc[by_k[0].level == 0, words].values.tolist() == by_k[1].loc[by_k[1].level == 0, words].values.tolist()
    # level 0 is the identity: its rows hold what a plain SeatSampler tallies on the same plan, seeds and noise
    seats, faults = FaultPlan.sweep(2, levels, 2, N, 1.0)
    t = make_eval_trainer("copo", "inter", seats.E, N, 0)
    try:
        smp = SeatSampler(t.env, t.policy, PolicyBank(t.policy, [w, w]), seats, t.sampler.T, use_graph=t.config.get("use_hip_graphs", True))

        def cell_noise():          # the sweep's rule: the first cell's draw in every cell
            smp.eps.normal_()
            cells = smp.eps.view(smp.T, seats.n_groups, 2, N, 2)
            cells[:, 1:].copy_(cells[:, :1])
        smp._draw_noise = cell_noise
        for _ in range(-(-steps // smp.T)):
            smp.sample()
        tally = smp.tally.cpu().numpy()
    finally:
        t.stop()
    for k in range(2):
        g = k * 2
        row = df[(df.checkpoint == k) & (df.level == 0)].iloc[0]
        assert [int(row[c]) for c in words] == tally[g, k].tolist(), (k, row[words].tolist(), tally[g, k].tolist())
    assert tally[:, :, 0].sum() > 0
