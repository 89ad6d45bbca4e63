"""CPU: fault injection without a GPU -- `FaultLevel` / `FaultPlan` validation and packing against the restatement's word table, the
`sweep` tables, the numpy model's own distributions (tests/fault_numpy.py is what the GPU is compared with, so its `z` and its Bernoulli
draw are held to their sampling bounds here), and the refusals of the two entry points that come before any device call."""
import math

import numpy as np
import pytest

import fault_cases as fc
import fault_numpy as fn
from copo_amd.eval.faults import LEVEL_FIELDS, FaultLevel, FaultPlan, lidar_columns, sweep_members


def test_level_validation_and_words():
    assert FaultLevel().is_identity and not FaultLevel().words().any() and FaultLevel().words().dtype == np.uint32
    assert tuple(FaultLevel().as_dict()) == LEVEL_FIELDS == ("lidar_sigma", "lidar_dropout", "dropout_value", "act_sigma", "sticky")
    assert FaultLevel(dropout_value=1.0).is_identity            # a value nothing ever reads
    for lv in fc.LEVELS:
        w = FaultLevel(**lv).words()
        assert w.shape == (8,) and np.array_equal(w, fn.words(**lv)) and not w[5:].any()
    w = FaultLevel(lidar_sigma=0.5, lidar_dropout=1.0, dropout_value=-2.0, act_sigma=0.25, sticky=0.1).words()
    assert w[[0, 2, 3]].view(np.float32).tolist() == [0.5, -2.0, 0.25] and w[1] == 1 << 24 and w[4] == int(np.rint(0.1 * 2 ** 24)) == 1677722
    assert FaultLevel(lidar_dropout=2.0 ** -25).words()[1] == 0 and FaultLevel(lidar_dropout=3 * 2.0 ** -25).words()[1] == 2      # half to even
    for bad in (dict(lidar_sigma=-0.1), dict(act_sigma=-1e-9), dict(lidar_dropout=1.5), dict(lidar_dropout=-0.1), dict(sticky=1.0001),
                dict(sticky=float("nan")), dict(lidar_sigma=float("inf")), dict(dropout_value=float("nan")), dict(act_sigma="0.1"),
                dict(sticky=True)):
        with pytest.raises(ValueError):
            FaultLevel(**bad)
    with pytest.raises(TypeError):
        FaultLevel(noise=1.0)


def test_plan_validation_and_packing():
    from copo_amd.eval.crossplay import SeatPlan
    levels = [FaultLevel(**lv) for lv in fc.LEVELS]
    seat, group, level_of, K, G = fc.tables(5, 40, 1)
    p = FaultPlan(levels, level_of)
    assert (p.L, p.G, p.K) == (3, G, K) and p.level_of.dtype == np.int32 and np.array_equal(p.level_of, level_of)
    assert p.words.dtype == np.uint32 and p.words.shape == (3, 8) and np.array_equal(p.words, fc.level_words())
    assert FaultPlan(list(fc.LEVELS), level_of).levels == levels                 # dicts of the fields are taken too
    seats = SeatPlan(np.where(seat >= K, -1, seat), n_members=K, group=np.clip(group, 0, G - 1), n_groups=G)
    assert p.check(seats) is p
    with pytest.raises(ValueError):
        p.check(SeatPlan(np.zeros((5, 40), np.int32), n_members=K + 1, n_groups=G))
    with pytest.raises(ValueError):
        p.check(SeatPlan(np.zeros((5, 40), np.int32), n_members=K, n_groups=G + 1))
    with pytest.raises(ValueError):
        FaultPlan([], level_of)
    with pytest.raises(ValueError):
        FaultPlan(levels, np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        FaultPlan([dict(sticky=2.0)], level_of)


@pytest.mark.parametrize("share,n_imp", [(1.0, 40), (0.25, 10), (0.0, 0)])
def test_sweep_tables(share, n_imp):
    K, S, N = 3, 2, 40
    levels = [FaultLevel(**lv) for lv in fc.LEVELS]
    L = len(levels)
    seats, faults = FaultPlan.sweep(K, levels, S, N, share)
    doubled = share < 1.0
    KB = 2 * K if doubled else K
    assert faults.check(seats) is faults and faults.doubled == doubled and faults.n_impaired == n_imp == int(round(share * N))
    assert (seats.E, seats.N, seats.K, seats.n_groups) == (K * L * S, N, KB, K * L) and seats.replica_scenes == S
    assert faults.level_of.shape == (K * L, KB) and faults.share == share and faults.n_checkpoints == K
    for g in range(K * L):
        k, lv = g // L, g % L
        assert (faults.checkpoint[g], faults.level[g]) == (k, lv)
        for e in range(g * S, (g + 1) * S):
            assert seats.group[e] == g
            assert (seats.seat[e, :n_imp] == (K + k if doubled else k)).all() and (seats.seat[e, n_imp:] == k).all()
        # the impaired member drives at the cell's level; every healthy member (and every member without a seat) at level 0
        assert faults.level_of[g, K + k if doubled else k] == lv
        if doubled:
            assert (faults.level_of[g, :K] == 0).all()
        assert np.count_nonzero(faults.level_of[g]) == (1 if lv else 0)
    assert levels[0].is_identity
    # seat counts: member k is healthy in L cells of S scenes, member K + k impaired in as many
    if doubled:
        assert seats.counts.tolist() == [L * S * (N - n_imp)] * K + [L * S * n_imp] * K
    else:
        assert seats.counts.tolist() == [L * S * N] * K
    ws = [dict(a=np.zeros(1)), dict(a=np.ones(1)), dict(a=np.full(1, 2.0))]
    bank = sweep_members(ws, faults)
    assert len(bank) == KB and all(bank[m] is ws[m % K] for m in range(KB))      # members k and K + k: the same weights


def test_sweep_refusals():
    harsh = FaultLevel(sticky=0.5)
    with pytest.raises(ValueError):
        FaultPlan.sweep(2, [harsh, FaultLevel()], 2, 8, 0.25)        # the healthy seats need the identity at level 0
    seats, faults = FaultPlan.sweep(2, [harsh, FaultLevel()], 2, 8, 1.0)         # nobody is healthy: any levels
    assert seats.K == 2 and faults.level_of.tolist() == [[0, 0], [1, 0], [0, 0], [0, 1]]
    for bad in (dict(K=0), dict(scenes_per_cell=0), dict(N=0), dict(share=1.5), dict(share=-0.1), dict(levels=[])):
        a = dict(K=2, levels=[FaultLevel()], scenes_per_cell=1, N=4, share=1.0)
        a.update(bad)
        with pytest.raises(ValueError):
            FaultPlan.sweep(**a)


def test_lidar_columns_of_a_config():
    from copo_amd.sim import SimConfig
    c = SimConfig(map="intersection", num_envs=1, num_agents=4, enable_lcf=False)
    lo, hi = lidar_columns(c)
    assert (lo, hi) == (19, 91) == (c.ego_dim + c.navi_dim, c.obs_dim)          # an odd first column, beams to the end of an odd row
    c = SimConfig(map="intersection", num_envs=1, num_agents=4)
    assert lidar_columns(c) == (19, 91) and c.lcf_col == 91 and c.obs_dim == 92       # the LCF entry behind the beams is not touched


# ---- the numpy model itself ------------------------------------------------------------------------------------------------------------
N_DRAWS = 1 << 16


@pytest.fixture(scope="module")
def draws():
    """2^16 draws of each kind under a fixed seed, over rows, ticks and beams as the kernels index them."""
    h = np.empty((3, N_DRAWS), np.uint32)
    for i in range(N_DRAWS):
        row, tick, beam = i & 255, (i >> 8) & 15, i >> 12
        h[0, i] = fn.hash_rng(fc.SEED, row, tick, beam, fn.LIDAR_A)
        h[1, i] = fn.hash_rng(fc.SEED, row, tick, beam, fn.LIDAR_B)
        h[2, i] = fn.hash_rng(fc.SEED, row, tick, beam, fn.DROP)
    return h


def test_model_hash_is_the_simulators():
    """`hash_rng` against values of the chain worked out by hand from `mix32` (murmur3's finaliser), and `mix32` against murmur3's
    published fixed points."""
    assert fn.mix32(0) == 0 and fn.mix32(1) == 0x514E28B7 and fn.mix32(0xFFFFFFFF) == 0x81F16F39
    h = fn.mix32(0x9E3779B9 + 5)
    for v in (0, 1, 2, 3, 4):
        h = fn.mix32(h ^ v)
    assert fn.hash_rng(5, 1, 2, 3, 4) == h
    assert fn.hash_rng(5 + (7 << 32), 1, 2, 3, 4) != h and fn.hash_rng(5, 1, 2, 3, 33) != fn.hash_rng(5, 1, 2, 3, 34)
    assert len({fn.DROP, fn.LIDAR_A, fn.LIDAR_B, fn.STICKY, fn.ACT_A, fn.ACT_B} | {1, 2, 3, 4, 16}) == 11       # none is the simulator's


def test_model_z_moments_and_tails(draws):
    z = np.array([fn.z_of(int(a), int(b)) for a, b in zip(draws[0], draws[1])], np.float32)
    assert z.dtype == np.float32
    n = float(N_DRAWS)
    mean, var = float(z.astype(np.float64).mean()), float(z.astype(np.float64).var())
    print("z over 2^16 draws: mean %.5f variance %.5f min %.4f max %.4f" % (mean, var, z.min(), z.max()))
    # the mean of n draws of variance 1: standard error 1 / sqrt(n); the sample variance of n normal draws: sqrt(2 / n) (the sum of four
    # uniforms has a fourth moment of 2.7, not 3, so the normal figure is the wider one).  Five standard errors each.
    assert abs(mean) <= 5.0 / math.sqrt(n) and abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert np.abs(z).max() <= 3.47 and np.abs(z).max() <= fn.Z_MAX * (1 + 2.0 ** -23)
    # the ends of the range and its centre
    top = fn.z_of(0xFFFFFFFF, 0xFFFFFFFF)
    assert top == -fn.z_of(0, 0) and abs(float(top) - fn.Z_MAX) <= fn.Z_MAX * 2.0 ** -23 and fn.z_of(0xFFFF0000, 0x0000FFFF) == 0.0
    assert 3.46 < fn.Z_MAX < 3.47 and fn.Z_SCALE.view(np.uint32) == 0x37DDB3D7


def test_model_dropout_frequency(draws):
    p = 0.1
    thr = int(fn.words(lidar_dropout=p)[1])
    assert thr == int(np.rint(p * 2 ** 24))
    freq = float(((draws[2] >> 8) < thr).mean())
    se = math.sqrt(p * (1.0 - p) / N_DRAWS)                  # binomial
    print("dropout at p = 0.1 over 2^16 draws: %.5f (standard error %.5f)" % (freq, se))
    assert abs(freq - p) <= 5.0 * se
    assert not ((draws[2] >> 8) < 0).any() and ((draws[2] >> 8) < (1 << 24)).all()          # p = 0 never fires, p = 1 always


def test_model_rules_on_a_case_written_out_by_hand():
    """One scene, four slots: the sticky rule's cases and the pass-through rows, with a level whose sticky draw always fires."""
    levels = np.stack([fn.words(), fn.words(sticky=1.0)])
    seat = np.array([[0, 0, 0, -1]], np.int32)
    group, level_of = np.array([0], np.int32), np.array([[1]], np.int32)
    act = np.array([[[0.1, 0.2], [0.3, 0.4], [0.5, 0.6], [0.7, 0.8]]], np.float32)
    prev = -act
    flags = np.array([[fn.ACTED, fn.ACTED | fn.DONE, fn.ACTED | fn.SPAWNED, fn.ACTED]], np.uint8)
    a, p, t = fn.fault_act(act, prev, flags, seat, group, level_of, levels, np.array([0, 5, 6, 7], np.int32), fc.SEED)
    assert np.array_equal(a[0, 0], prev[0, 0]) and np.array_equal(a[0, 1:], act[0, 1:])      # only the same occupant sticks; seat -1 never
    assert np.array_equal(p, a) and t.tolist() == [1, 6, 7, 8]                               # prev and tick move in every row
    a, p, t = fn.fault_act(act, prev, None, seat, group, level_of, levels, np.zeros(4, np.int32), fc.SEED)
    assert np.array_equal(a, act) and np.array_equal(p, act) and t.tolist() == [1, 1, 1, 1]  # no flags: nothing sticks
    flags[0, 0] = fn.ACTED | fn.ENV_RESET
    assert np.array_equal(fn.fault_act(act, prev, flags, seat, group, level_of, levels, np.zeros(4, np.int32), fc.SEED)[0], act)
    # observations: dropout of probability 1 replaces exactly the beams of the seated rows
    levels = np.stack([fn.words(), fn.words(lidar_dropout=1.0, dropout_value=0.25)])
    obs = fc.observations(1, 4, 7, 3)
    seen = fn.fault_obs(obs, 2, 6, seat, group, level_of, levels, np.zeros(4, np.int32), fc.SEED)
    assert (seen[0, :3, 2:6] == 0.25).all() and np.array_equal(seen[0, 3], obs[0, 3])
    assert np.array_equal(seen[0, :, :2], obs[0, :, :2]) and np.array_equal(seen[0, :, 6:], obs[0, :, 6:])
    # noise moves every beam of a seated row by at most 3.47 sigma and keeps it in [0, 1]
    levels = np.stack([fn.words(), fn.words(lidar_sigma=0.01)])
    seen = fn.fault_obs(obs, 2, 6, seat, group, level_of, levels, np.zeros(4, np.int32), fc.SEED)
    d = np.abs(seen[0, :3, 2:6].astype(np.float64) - obs[0, :3, 2:6])
    assert d.max() <= 0.0347 and (d > 0).sum() >= 6 and seen[0, :3, 2:6].min() >= 0.0 and seen[0, :3, 2:6].max() <= 1.0


# ---- the entry points, before any device call ------------------------------------------------------------------------------------------
def test_symbols_abi_and_refusals():
    from copo_amd import _capi
    assert {"copo_fault_obs", "copo_fault_act"} <= set(_capi.EXPORTED_SYMBOLS) and _capi.lib.copo_version() == 8
    a16, b16 = 16, 32      # any two non-NULL addresses: every refusal below comes before the first use

    def obs(**kw):
        a = dict(obs=a16, obs_seen=b16, E=1, N=5, O=13, col_lo=3, col_hi=13, seat=a16, group=a16, K=2, G=1, level_of=a16, levels=a16, L=3,
                 tick=a16, seed=fc.SEED, stream=None)      # (in the order of the C signature)
        a.update(kw)
        return _capi.lib.copo_fault_obs(*a.values())

    def act(**kw):
        a = dict(act=a16, prev=b16, flags_prev=None, E=1, N=5, seat=a16, group=a16, K=2, G=1, level_of=a16, levels=a16, L=3, tick=a16,
                 seed=fc.SEED, stream=None)
        a.update(kw)
        return _capi.lib.copo_fault_act(*a.values())
    for call, name, ptrs in ((obs, b"copo_fault_obs", ("obs", "obs_seen", "seat", "group", "level_of", "levels", "tick")),
                             (act, b"copo_fault_act", ("act", "prev", "seat", "group", "level_of", "levels", "tick"))):
        for p in ptrs:
            assert call(**{p: None}) == -1 and name in _capi.lib.copo_last_error(), p
        for bad in (dict(E=-1), dict(N=0), dict(K=0), dict(K=65536), dict(G=0), dict(L=0), dict(E=1 << 20, N=1 << 11)):
            assert call(**bad) == -1 and name in _capi.lib.copo_last_error(), bad
        assert call(E=0) == 0                                                       # nothing to do: no launch
    for bad in (dict(O=0), dict(col_lo=-1), dict(col_lo=14, col_hi=13), dict(col_hi=14), dict(col_lo=5, col_hi=4)):
        assert obs(**bad) == -1 and b"copo_fault_obs" in _capi.lib.copo_last_error(), bad
    assert obs(obs_seen=a16) == -1 and b"copo_fault_obs" in _capi.lib.copo_last_error() and b"obs == obs_seen" in _capi.lib.copo_last_error()
