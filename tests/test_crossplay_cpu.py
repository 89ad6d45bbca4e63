"""CPU: cross-play without a GPU -- `SeatPlan` against its restatement (tests/crossplay_numpy.py), the restated seat tally against a case
written out by hand, the launch plan of the seat forward (copo_debug_learner_plan with the SEATS fact), the refusals of the two new
entry points that come before any device call, and the premise of the GPU end-to-end test on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import crossplay_numpy as cn
from copo_amd.eval.crossplay import SEAT_WORDS, SeatPlan
from test_learner_plan_cpu import ALL, FORWARD, make_cfg, plan, query

SEATS = 16      # FACT_SEATS of csrc/learn_plan.inc


def _check_plan(p, seat, K):
    rows, counts, cap = cn.plan_lists(seat, K)
    assert p.K == K and p.cap == cap and p.rows.dtype == np.int64 and p.counts.dtype == np.int32
    assert np.array_equal(p.rows, rows) and np.array_equal(p.counts, counts) and p.rows.shape == (K, cap)
    seen = np.concatenate([p.rows[k, :p.counts[k]] for k in range(K)])
    seated = np.nonzero(np.asarray(seat).reshape(-1) >= 0)[0]
    assert len(seen) == len(set(seen.tolist())) and sorted(seen.tolist()) == seated.tolist()        # every seated row exactly once
    for k in range(K):
        mine = p.rows[k, :p.counts[k]]
        assert (np.diff(mine) > 0).all() and (np.asarray(seat).reshape(-1)[mine] == k).all() and (p.rows[k, p.counts[k]:] == 0).all()


def test_plan_of_a_free_table():
    rng = np.random.RandomState(0)
    seat = rng.randint(-1, 4, (5, 7)).astype(np.int32)
    seat[seat == 2] = -1                        # member 2 of 5 has no seat, member 4 none either
    p = SeatPlan(seat, n_members=5)
    _check_plan(p, seat, 5)
    assert p.counts[2] == 0 and p.counts[4] == 0 and p.n_groups == 1 and (p.group == 0).all()
    empty = SeatPlan(np.full((2, 3), -1), n_members=2)
    assert empty.cap == 1 and empty.counts.tolist() == [0, 0] and empty.rows.tolist() == [[0], [0]]
    with pytest.raises(ValueError):
        SeatPlan(seat, n_members=3)             # member 3 is seated
    with pytest.raises(ValueError):
        SeatPlan(np.full((2, 3), -2))
    with pytest.raises(ValueError):
        SeatPlan(np.zeros(4))


@pytest.mark.parametrize("K,S,N,share,n_focal", [(2, 3, 7, 0.5, 4), (3, 2, 40, 0.25, 10), (2, 1, 40, 1.0, 40), (1, 2, 7, 0.5, 4)])
def test_pair_builder(K, S, N, share, n_focal):
    p = SeatPlan.pairs(K, S, N, share)
    seat, group = cn.pair_seats(K, S, N, share)
    assert np.array_equal(p.seat, seat) and np.array_equal(p.group, group) and p.n_groups == K * K and p.E == K * K * S
    _check_plan(p, seat, K)
    assert p.n_focal == n_focal == int(round(share * N)) and p.share == share
    for g in range(K * K):
        i, j = g // K, g % K
        assert (p.focal[g], p.partner[g]) == (i, j)
        for e in range(g * S, (g + 1) * S):
            assert (p.seat[e, :n_focal] == i).all() and (p.seat[e, n_focal:] == j).all() and p.group[e] == g
    # member k: focal in K groups, partner in K groups
    assert p.counts.tolist() == [K * S * n_focal + K * S * (N - n_focal)] * K


def test_uniform_is_the_dense_bank():
    from copo_amd.eval.bank import members_of_scenes
    E, K, N = 12, 3, 7
    per = members_of_scenes(E, K)
    p = SeatPlan.uniform(np.arange(E) // per, N)
    assert p.K == K and p.cap == per * N and p.counts.tolist() == [per * N] * K
    for k in range(K):
        assert p.rows[k].tolist() == list(range(k * per * N, (k + 1) * per * N))       # rows [k R, (k + 1) R) of PolicyBank.act
    assert np.array_equal(p.group, np.arange(E) // per) and p.n_groups == K


def test_tally_restatement_on_a_case_written_out_by_hand():
    A, D, ARR, CR, OUT, MX, SP = cn.ACTED, cn.DONE, cn.ARRIVE, cn.CRASH, cn.OUT, cn.MAXSTEP, cn.SPAWNED
    nan, inf = float("nan"), float("inf")
    half = 0.5 / 65536.0
    #            slot 0            1                2            3         4              5            6
    flags = np.array([[A,          A | D | ARR | CR, SP,         A,        A | D | OUT,   A | SP,      D | ARR],           # scene 0, group 0
                      [A,          A,                A,          A,        A,             A | D | MX,  0],                 # scene 1, group 1
                      [A | D | CR, A,                A,          A,        A,             A,           A]], np.uint8)      # scene 2, group 7: out of range
    rew = np.array([[1.0,          -0.25,            5.0,        nan,      2000.0,        half,        9.0],
                    [inf,          -inf,             3 * half,   5 * half, -half,         0.125,       1.0],
                    [1.0] * 7], np.float32)
    seat = np.array([[0,           1,                1,          0,        1,             -1,          0],
                     [1,           1,                0,          0,        0,             2,           2],
                     [0] * 7], np.int32)
    group = np.array([0, 1, 7], np.int32)
    out = cn.tally(flags, rew, seat, group, 3, 2)
    q = 65536
    want = np.zeros((2, 3, 8), np.int64)
    # group 0, member 0: slots 0 and 3 acted (1.0 and NaN -> 0); slot 6 has DONE | ARRIVE without ACTED: nothing
    want[0, 0] = [2, 0, 0, 0, 0, 0, q, 0]
    # group 0, member 1: slot 1 DONE with ARRIVE and CRASH both counted, slot 2 SPAWNED only (word 7, its reward ignored), slot 4 OUT with
    # 2000 clamped to 1024; slot 5 has seat -1
    want[0, 1] = [2, 2, 1, 1, 1, 0, -q // 4 + 1024 * q, 1]
    # group 1, member 0: 3 / 2 -> 2, 5 / 2 -> 2, -1 / 2 -> -0 (half to even)
    want[1, 0] = [3, 0, 0, 0, 0, 0, 4, 0]
    # group 1, member 1: +inf and -inf clamp to +-1024 and cancel
    want[1, 1] = [2, 0, 0, 0, 0, 0, 0, 0]
    want[1, 2] = [1, 1, 0, 0, 0, 1, q // 8, 0]
    assert np.array_equal(out, want), np.argwhere(out != want).tolist()
    assert cn.reward_q16(half) == 0 and cn.reward_q16(3 * half) == 2 and cn.reward_q16(-3 * half) == -2 and cn.reward_q16(nan) == 0
    # NULL rew adds nothing; a second call accumulates
    twice = cn.tally(flags, None, seat, group, 3, 2, out.copy())
    want2 = 2 * want
    want2[:, :, 6] = want[:, :, 6]
    assert np.array_equal(twice, want2)
    assert len(SEAT_WORDS) == cn.WORDS


@pytest.mark.parametrize("hidden,bf16", [(64, False), (128, True), (256, False), (256, True), (512, False)])
def test_seat_forward_plan_names_the_one_tile_bank_kernels(hidden, bf16):
    c = make_cfg(hidden=hidden, bf16=bf16)
    for cap in (1, 17, 1000, 16384, 40000):
        (name, grid, block, lds), = plan(c, FORWARD, n=cap, n_members=5, facts=ALL | SEATS)
        dense, = plan(c, FORWARD, n=min(cap, 1000), n_members=5)                  # below the two-tile threshold
        assert name == dense[0] and name.endswith("1, true>") and (block, lds) == dense[2:]
        assert grid == (-(-cap // 16), 5, 1)
    if hidden == 256:      # the dense bank does take the two-tile kernel there
        assert plan(c, FORWARD, n=16384, n_members=5)[0][0].endswith("2, true>")
    assert query(c, FORWARD, n=100, n_members=0, facts=ALL | SEATS)[0] == -2      # seat mode is a mode of the bank
    assert query(make_cfg(hidden=96), FORWARD, n=100, n_members=2, facts=ALL | SEATS)[0] == -2


def test_refusals_before_any_device_call():
    from copo_amd import _capi
    assert {"copo_mlp_forward_seats_f32", "copo_seat_tally"} <= set(_capi.EXPORTED_SYMBOLS) and _capi.lib.copo_version() == 8
    c = make_cfg(hidden=64)
    one = 16       # any non-NULL address: every refusal below comes before the first use

    def fwd(**kw):
        a = dict(cfg=C.byref(c), theta=one, theta_t=one, stride=c.n_params, K=2, rows=one, counts=one, cap=4, n_out=8, obs=one, dist=one,
                 eps=None, action=None, logp=None, clipped=None, stream=None)      # (in the order of the C signature)
        a.update(kw)
        return _capi.lib.copo_mlp_forward_seats_f32(*a.values())

    def tally(**kw):
        a = dict(flags=one, rew=None, seat=one, group=one, E=1, N=7, K=2, G=1, out=one, stream=None)
        a.update(kw)
        return _capi.lib.copo_seat_tally(*a.values())
    assert fwd(rows=None) == -1 and fwd(counts=None) == -1 and fwd(theta=None) == -1 and fwd(obs=None) == -1
    assert fwd(cap=0) == -2 and fwd(n_out=0) == -2 and fwd(K=0) == -2 and fwd(K=65536) == -2
    assert fwd(stride=c.n_params - 4) == -2 and fwd(stride=c.n_params + 1) == -2
    assert fwd(eps=one) == -1                                                      # sampling without action / logp
    assert fwd(theta_t=one + 4) == -2                                              # mirror not 16-byte aligned
    for name in ("flags", "seat", "group", "out"):
        assert tally(**{name: None}) == -1 and b"copo_seat_tally" in _capi.lib.copo_last_error()
    assert tally(N=0) == -2 and tally(N=257) == -2 and tally(K=0) == -2 and tally(K=65536) == -2 and tally(G=0) == -2 and tally(E=-1) == -2
    assert tally(E=0) == 0                                                          # nothing to do: no launch


# ---- the premise of the GPU end-to-end test ------------------------------------------------------------------------------------------
def test_sixty_steps_finish_an_agent_of_each_member_in_every_group(golden_dir):
    """tests/test_gpu_crossplay.py compares per-(group, member) DONE counts of a 60-step rollout of pairs(2, 3, 40, 0.5): they must not
    be zero.  Here on the CPU oracle with the same two populations (the Gaussian means, no noise)."""
    import oracle_lib as ol
    from copo_amd.eval.get_policy_function import _gaussian_head, layer_arrays, population_layout
    p = SeatPlan.pairs(*cn.E2E_PAIRS)
    layout, sfx = population_layout("copo_inter")
    heads = [layer_arrays(w, layout, "default", sfx) for w in cn.e2e_members(golden_dir)]
    import trip_numpy as tn
    from copo_amd import trips
    o = ol.OracleSim(cn.e2e_config())
    log = tn.TripLog(p.E, p.N)
    try:
        out = o.reset(cn.e2e_seeds())
        log.record(*o.get_state())
        tot = np.zeros((p.n_groups, p.K, 8), np.int64)
        for _ in range(cn.E2E_STEPS):
            obs = out["obs"].reshape(p.E * p.N, -1).astype(np.float32)
            act = np.zeros((p.E * p.N, 2), np.float32)
            for k in range(p.K):
                mine = p.rows[k, :p.counts[k]]
                act[mine] = _gaussian_head(heads[k], obs[mine], True)
            out = o.step(np.clip(act, -1.0, 1.0).reshape(p.E, p.N, 2))
            cn.tally(out["flags"], out["rew"], p.seat, p.group, p.K, p.n_groups, tot)
            log.record(*o.get_state(), flags=out["flags"], rew=out["rew"])
    finally:
        o.close()
    # the join the GPU test makes between the device's trip log and the device's tally, here between the two restatements
    log.flush()
    assert log.dropped == 0
    joined = cn.trip_join(trips.decode(log.rows(), 0.1), p.seat, p.group, p.K, p.n_groups)
    assert np.array_equal(joined, tot[:, :, :5]), (joined.tolist(), tot[:, :, :5].tolist())
    print(tot[:, :, :6].tolist())
    for g in range(p.n_groups):
        for k in {int(p.focal[g]), int(p.partner[g])}:
            assert tot[g, k, 1] >= 1 and tot[g, k, 0] >= 60, (g, k, tot[g, k].tolist())
    assert tot[:, :, 2].sum() + tot[:, :, 3].sum() + tot[:, :, 4].sum() >= tot[:, :, 1].sum() >= 8
