"""The policy jury on the GPU (copo_jury_obs_seats_f32, copo_jury_tally, copo_amd/eval/jury.py).  The kernel cases
are those of tests/jury_cases.py -- hidden 64 / 128 / 256 / 512, observation widths 91 and 92, adversary_cases' 48 rows, two judge
tables -- and tests/test_jury_cpu.py checks their premise on the float64 model alone.  The verdicts are compared in BITS with the seat
forward; the fold's integer words exactly with tests/jury_numpy.py, its two float64 divergence words within one unit per counted pair.
Outputs and references are computed once per case and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bank_cases as bc
import crossplay_numpy as cn
import jury_cases as jc
import jury_numpy as jn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = jc.POISON
CASES = [(h, k) for h in jc.HIDDENS for k in jc.IN_DIMS]
N_OUT = jc.E * jc.N
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


def _lists(rows, counts, n_out=N_OUT, K=jc.K):
    """What `jury_seats` and `act_seats` read of a plan's buffers."""
    return SimpleNamespace(K=K, cap=rows.shape[1], n_out=n_out, rows=_dev(rows), counts=_dev(counts))


def _jury(bank, table, obs, verdict=None):
    rows, counts, _ = jn.jury_lists(jc.SEAT, jc.GROUP, jc.JUDGES[table])
    verdict = _poison(N_OUT, jc.K, 4) if verdict is None else verdict
    bank.jury_seats(_lists(rows, counts), obs, verdict)
    torch.cuda.synchronize()
    return verdict.cpu().numpy()


def _seat_forward(bank, rows, counts, obs):
    """dist_inputs [n_out][4] of the unchanged seat forward under these lists; rows in no list keep the poison."""
    out = dict(action=_poison(N_OUT, 2), logp=_poison(N_OUT), dist_inputs=_poison(N_OUT, 4))
    bank.act_seats(_lists(rows, counts), obs, torch.zeros(N_OUT, 2, device="cuda"), **out)
    torch.cuda.synchronize()
    return out["dist_inputs"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    ref = jc.reference(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), ref["members"])
    bank.sync_mirror()
    obs = _dev(ref["obs"])
    out = {t: _jury(bank, t, obs) for t in jc.TABLES}
    out["again"] = _jury(bank, "A", obs)
    alone = {}          # per table and judge: the seat forward with member j ALONE seated, on its jury list
    for t in jc.TABLES:
        rows, counts, _ = jn.jury_lists(jc.SEAT, jc.GROUP, jc.JUDGES[t])
        for j in range(jc.K):
            only = np.zeros_like(counts)
            only[j] = counts[j]
            alone[t, j] = _seat_forward(bank, rows, only, obs)
    # the drive: every member on the rows it is seated on
    from copo_amd.eval.crossplay import SeatPlan
    seats = SeatPlan(jc.SEAT, jc.K, jc.GROUP, jc.G)
    drive = _seat_forward(bank, seats.rows, seats.counts, obs)
    assert _same(obs, _dev(ref["obs"]))                              # the observation is left alone
    return dict(ref=ref, bank=bank, obs=obs, out=out, alone=alone, drive=drive, seats=seats)


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_verdicts_are_the_seat_forwards_bits(hidden, in_dim):
    """(1) verdict[r][j] == dist_inputs[r] of a seat-forward launch with member j alone on its jury list, as uint32; entries outside
    every list keep the poison; two launches agree in bits; and the numbers are the float64 model's up to fp32."""
    c = _case(hidden, in_dim)
    for t in jc.TABLES:
        got = _u32(c["out"][t])
        rows, counts, _ = jn.jury_lists(jc.SEAT, jc.GROUP, jc.JUDGES[t])
        assert tuple(counts) == jc.COUNTS[t]
        for j in range(jc.K):
            listed = np.zeros(N_OUT, bool)
            listed[rows[j, :counts[j]]] = True
            want = _u32(c["alone"][t, j])
            assert (want[listed] != POISON).all() and (want[~listed] == POISON).all()
            assert np.array_equal(got[listed, j], want[listed]), (t, j)
            assert (got[~listed, j] == POISON).all(), (t, j)
        assert (got[40:] == POISON).all()                            # scene 5: its group is out of range
    assert np.array_equal(_u32(c["out"]["A"]), _u32(c["out"]["again"]))
    v64 = c["ref"]["verdict64"]
    written = _u32(c["out"]["A"])[..., 0] != POISON
    worst = float(np.abs(c["out"]["A"].astype(np.float64) - v64)[written].max())
    print("hidden %d in_dim %d: max |verdict - float64 model| = %.3g" % (hidden, in_dim, worst))
    assert worst < 1e-3          # (a sanity bound on top of the bit-equality: fp32 sums of at most 512 terms of magnitude <= 1)


@pytest.mark.parametrize("hidden", (64, 256))
def test_jury_verdicts_is_the_everyone_launch_and_the_dense_bank(hidden):
    """(2) `jury_verdicts` on a plain array == the launch with every member judging every row == K dense `bank.act` calls, in bits."""
    from copo_amd.eval.jury import jury_verdicts
    c = _case(hidden, 92)
    got = jury_verdicts(c["bank"], c["obs"])
    every = _poison(N_OUT, jc.K, 4)
    c["bank"].jury_seats(_lists(np.tile(np.arange(N_OUT, dtype=np.int64), (jc.K, 1)), np.full(jc.K, N_OUT, np.int32)), c["obs"], every)
    dense = dict(action=_poison(jc.K * N_OUT, 2), logp=_poison(jc.K * N_OUT), dist_inputs=_poison(jc.K * N_OUT, 4))
    c["bank"].act(c["obs"].repeat(jc.K, 1), torch.zeros(jc.K * N_OUT, 2, device="cuda"), **dense)
    torch.cuda.synchronize()
    assert got.shape == (N_OUT, jc.K, 4) and _same(got, every)
    assert _same(got, dense["dist_inputs"].view(jc.K, N_OUT, 4).transpose(0, 1))
    listed = _u32(c["out"]["A"]) != POISON
    assert np.array_equal(_u32(got.cpu().numpy())[listed], _u32(c["out"]["A"])[listed])          # whichever rows share the tile


def test_refusals():
    """(3) What the Python layer and the entries refuse; nothing is launched: the poison is intact."""
    from copo_amd import _capi
    c = _case(64, 91)
    bank, obs = c["bank"], c["obs"]
    rows, counts, _ = jn.jury_lists(jc.SEAT, jc.GROUP, jc.JUDGES["A"])
    jb, verdict = _lists(rows, counts), _poison(N_OUT, jc.K, 4)
    for bad in (dict(obs=obs[:, :90].contiguous()), dict(verdict=_poison(N_OUT, jc.K, 3)), dict(verdict=_poison(N_OUT, 2, 4)),
                dict(verdict=torch.zeros(N_OUT, jc.K, 4, dtype=torch.float64, device="cuda")), dict(verdict=_poison(N_OUT, 4, jc.K).transpose(1, 2))):
        with pytest.raises(ValueError):
            bank.jury_seats(jb, **dict(dict(obs=obs, verdict=verdict), **bad))
    with pytest.raises(ValueError):
        bank.jury_seats(_lists(rows[:2], counts[:2], K=2), obs, verdict)
    import ctypes as C
    good = dict(cfg=C.byref(bank.cfg), theta=bank.theta.data_ptr(), theta_t=bank.theta_t.data_ptr(), member_stride=bank.stride, n_members=jc.K,
                rows=jb.rows.data_ptr(), counts=jb.counts.data_ptr(), cap=jb.cap, n_out=N_OUT, obs_src=obs.data_ptr(), verdict=verdict.data_ptr(),
                stream=_capi.current_stream())
    call = lambda **kw: _capi.lib.copo_jury_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("rows", "counts", "verdict", "obs_src", "theta", "theta_t"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(cap=0), dict(n_out=0), dict(n_members=0), dict(n_members=65536), dict(member_stride=bank.stride - 4), dict(member_stride=bank.stride + 2)):
        assert call(**bad) == -2, bad
    fold = torch.zeros(jc.G, jc.K, jc.K, 8, dtype=torch.int64, device="cuda")
    tgood = dict(flags=_dev(jc.flags()).data_ptr(), dist=verdict.data_ptr(), verdict=verdict.data_ptr(), seat=_dev(jc.SEAT).data_ptr(),
                 group=_dev(jc.GROUP).data_ptr(), judges=_dev(jc.JUDGES["A"]).data_ptr(), E=jc.E, N=jc.N, K=jc.K, G=jc.G, ds=0.1, dt=0.1,
                 out=fold.data_ptr(), stream=_capi.current_stream())
    tally = lambda **kw: _capi.lib.copo_jury_tally(*dict(tgood, **kw).values())  # noqa: E731
    for name in ("flags", "dist", "verdict", "seat", "group", "judges", "out"):
        assert tally(**{name: None}) == -1, name
    for bad in (dict(E=-1), dict(N=0), dict(N=257), dict(K=0), dict(K=65536), dict(G=0)):
        assert tally(**bad) == -2, bad
    torch.cuda.synchronize()
    assert (_bits(verdict) == POISON).all() and int(fold.abs().sum()) == 0


# ---- the fold ----------------------------------------------------------------------------------------------------------------------------
def _fold_gpu(flags, dist, verdict, seat, group, judges, deltas, times=2):
    from copo_amd.eval.jury import jury_tally
    E, N = seat.shape
    G, K = judges.shape
    pb = SimpleNamespace(K=K, G=G, N=N, E=E, n_out=E * N, seat=_dev(seat), group=_dev(group))
    jb = SimpleNamespace(K=K, G=G, n_out=E * N, judges=_dev(judges))
    out = torch.zeros(G, K, K, 8, dtype=torch.int64, device="cuda")
    d_flags, d_dist, d_verdict = _dev(flags), _dev(np.asarray(dist, F)), _dev(np.asarray(verdict, F))
    for _ in range(times):          # it accumulates
        jury_tally(d_flags, d_dist, d_verdict, pb, jb, deltas, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_fold(got_twice, want, where):
    """Folded twice against the model folded once: words 0-4 doubled exactly, word 7 kept exactly, words 5 and 6 within one unit per
    counted pair and fold (each pair is quantised once to 2^-16; a last-ulp difference of exp moves it across a rounding boundary by one
    unit at the most)."""
    assert np.array_equal(got_twice[..., :5], 2 * want[..., :5]), where
    assert np.array_equal(got_twice[..., 7], want[..., 7]), where
    off = np.abs(got_twice[..., 5:7] - 2 * want[..., 5:7])
    print("%s: KL words off by at most %d units (bound: %d), %d pairs" % (where, int(off.max()), int(2 * want[..., 0].max()), int(want[..., 0].sum())))
    assert (off <= 2 * want[..., 0][..., None]).all(), where
    assert (got_twice[..., 5:7] % 2 == 0).all(), where          # the second fold adds what the first added: no dependence on the order


@pytest.mark.parametrize("hidden,in_dim", [(64, 91), (256, 92)])
def test_fold_on_the_kernels_own_verdicts(hidden, in_dim):
    """(4) Against jury_numpy on the kernel's verdicts and the seat forward's dist_inputs; the diagonal is zero in words 1-7."""
    c = _case(hidden, in_dim)
    flags = jc.flags()
    dist = c["drive"].copy()
    dist[_u32(dist) == POISON] = 0.0          # rows nobody drives: what the sampler's zero-initialised buffer holds
    for t in jc.TABLES:
        verdict = c["out"][t].copy()
        verdict[_u32(verdict) == POISON] = 0.0
        want = jn.jury_fold(flags, dist, verdict, jc.SEAT, jc.GROUP, jc.JUDGES[t], jc.DELTAS)
        got = _fold_gpu(flags, dist, verdict, jc.SEAT, jc.GROUP, jc.JUDGES[t], jc.DELTAS)
        _check_fold(got, want, "table %s hidden %d" % (t, hidden))
        once = _fold_gpu(flags, dist, verdict, jc.SEAT, jc.GROUP, jc.JUDGES[t], jc.DELTAS, times=1)
        assert np.array_equal(2 * once[..., :7], got[..., :7]) and np.array_equal(once[..., 7], got[..., 7])
        assert want[..., 0].sum() > 0 and 0 < want[..., 1].sum() < want[..., 0].sum() and want[..., 5].sum() > 0
        for g in range(jc.G):
            for k in range(jc.K):
                if jc.JUDGES[t][g, k]:
                    assert not got[g, k, k, 1:].any(), (t, g, k)          # the bit-equality of test 1, seen through the fold
        assert not got[..., 0][np.repeat(jc.JUDGES[t][:, None, :], jc.K, 1) == 0].any()


def test_fold_on_a_hand_made_case_and_at_scale():
    """(5)"""
    from test_jury_cpu import hand_case
    h = hand_case()
    got = _fold_gpu(h["flags"], h["dist"], h["verdict"], h["seat"], h["group"], h["judges"], h["deltas"])
    _check_fold(got, h["want"], "hand-made")
    E, N, K, G = 256, 40, 16, 5
    rng = np.random.RandomState(11)
    seat = rng.randint(-1, K, (E, N)).astype(np.int32)
    seat[rng.rand(E, N) < 0.2] = -1
    seat[7, :] = 5          # a whole scene of one member
    flags = rng.choice(np.array([0, 1, 1 | 2, 64], np.uint8), (E, N), p=[0.2, 0.6, 0.1, 0.1])
    group = rng.randint(-1, G + 1, E).astype(np.int32)
    judges = (rng.rand(G, K) < 0.6).astype(np.int32)
    judges[1], judges[2] = 0, 1
    dist = np.concatenate([rng.randn(E, N, 2) * 0.3, rng.randn(E, N, 2) * 0.2 - 0.5], axis=-1).astype(F)
    verdict = (dist.reshape(E * N, 1, 4) + np.concatenate([rng.randn(E * N, K, 2) * 0.1, rng.randn(E * N, K, 2) * 0.05], axis=-1)).astype(F)
    own = rng.rand(E * N, K) < 0.1
    verdict[own] = np.repeat(dist.reshape(E * N, 1, 4), K, 1)[own]          # equal bits: zero in every word but the count
    verdict[rng.rand(E * N, K) < 0.01, 0] = np.nan
    verdict[rng.rand(E * N, K) < 0.01, 3] = np.nan
    dist[rng.rand(E, N) < 0.01, 1] = np.nan
    group[0], seat[0, 5:7], flags[0, 5:7] = 2, (2, 4), 1                      # two counted rows under every judge
    dist[0, 5:7] = (0.1, -0.1, -0.5, -0.5)
    verdict[5, 3] = (3000.0, -3000.0, -0.5, -0.5)                             # beyond the clamp of q
    verdict[6, 2] = (0.1, -0.1, 80.0, -0.5)                                   # a KL that overflows the clamp
    deltas = (0.08, 0.11)
    want = jn.jury_fold(flags, dist, verdict, seat, group, judges, deltas)
    got = _fold_gpu(flags, dist, verdict, seat, group, judges, deltas)
    _check_fold(got, want, "at scale")
    assert want[..., 0].sum() > 30000 and 0 < want[..., 1].sum() < want[..., 0].sum() and not want[1].any() and want[..., 7].max() == 1024 * 65536


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------
E2E = (9, 8, 4)          # scenes (3 x 3 pairs, one scene each), slots, T


@pytest.fixture(scope="module")
def e2e(golden_dir):
    from copo_amd.eval.evaluate import make_eval_trainer
    t = make_eval_trainer("copo", "inter", E2E[0], E2E[1], 0)
    ws = cn.e2e_members(golden_dir)
    yield t, ws + [bc.perturbed(ws[0], 2, 0.05)]
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


def test_captured_fragment_equals_eager_and_the_drive_is_untouched(e2e):
    """(6)"""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    from copo_amd.eval.jury import JuryPlan, JurySeatSampler, jury_verdicts
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(3, 1, N, 0.5)
    assert plan.E == E and plan.n_groups == 9
    jury = JuryPlan.seated(plan)
    bank = PolicyBank(t.policy, ws)
    keys = ("verdict", "jury_tally", "tally", "actions", "clipped", "flags", "obs", "dist_inputs", "logp")
    runs = {}
    for mode in (False, True):
        smp = JurySeatSampler(t.env, t.policy, bank, plan, jury, T, use_graph=mode, deltas=jc.DELTAS)
        smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
        runs[mode] = _fragments(smp, 2, keys)
        assert (smp._loop.graph is not None) == mode
    for f in range(2):
        for k in keys:
            assert _same(runs[False][f][k], runs[True][f][k]), (f, k)
    plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, ("tally", "actions", "clipped", "flags", "obs", "dist_inputs", "logp"))
    for f in range(2):
        for k in plain[f]:
            assert _same(plain[f][k], runs[True][f][k]), (f, k)          # the jury does not touch the drive
    assert smp.sample()["verdict"] is smp.verdict
    # the jury tally of the two fragments == jury_numpy folded over their recorded obs / dist_inputs / flags, verdicts from jury_verdicts
    want = np.zeros((9, 3, 3, 8), np.int64)
    for f in range(2):
        frag = runs[True][f]
        for step in range(T):
            v = jury_verdicts(bank, frag["obs"][step].reshape(E * N, -1).contiguous())
            judged = torch.from_numpy(np.repeat(jury.judges[plan.group], N, 0) != 0).cuda() & torch.from_numpy(plan.seat.reshape(-1, 1) >= 0).cuda()
            assert _same(frag["verdict"][step].reshape(E * N, 3, 4)[judged], v[judged])
            assert (frag["verdict"][step].reshape(E * N, 3, 4)[~judged] == 0).all()
            jn.jury_fold(frag["flags"][step].cpu().numpy(), frag["dist_inputs"][step].cpu().numpy(), v.cpu().numpy(), plan.seat, plan.group,
                         jury.judges, jc.DELTAS, want)
        got = frag["jury_tally"].cpu().numpy()
        assert np.array_equal(got[..., :5], want[..., :5]) and np.array_equal(got[..., 7], want[..., 7]), f
        assert (np.abs(got[..., 5:7] - want[..., 5:7]) <= want[..., 0][..., None]).all(), f
    st = runs[True][1]["tally"].cpu().numpy()
    for g in range(9):
        i, j = g // 3, g % 3
        for k in {i, j}:
            for m in {i, j}:
                assert got[g, k, m, 0] == st[g, k, 0] > 0          # every acted seat-step, once per judge
            assert not got[g, k, k, 1:].any()
        assert got[g][np.ix_([k for k in range(3) if k not in (i, j)], range(3))].sum() == 0
    assert got[1, 0, 1, 5] > 0 and got[1, 0, 1, 7] > 0
    smp.clear_tally()
    assert int(smp.jury_tally.abs().sum()) == 0 and int(smp.tally.abs().sum()) == 0
    graph = smp._loop.graph
    smp.set_jury(JuryPlan.panel(plan, [0, 2]))          # other list capacities: the graph is dropped
    assert graph is not None and smp._loop.graph is None
    with pytest.raises(ValueError):
        smp.set_jury(JuryPlan.everyone(SeatPlan.pairs(3, 2, N, 0.5)))


def test_jury_rows_frame(golden_dir):
    """(7)"""
    from copo_amd.eval.jury import JURY_WORDS, jury_matrix, jury_rows
    w = bc.golden_population(golden_dir, "copo_inter")
    df = jury_rows("copo", "inter", [w, dict(w)], plan="seated", share=0.5, deltas=(0.05, 0.05), scenes_per_pair=2, num_agents=8, steps=8, seed=0,
                   labels=["a", "b"])
    assert list(df.columns) == ["group", "focal", "partner", "driver", "judge", "driver_label", "judge_label", "delta_steer", "delta_throttle",
                                *JURY_WORDS, "disagree_rate", "d_steer", "d_throttle", "d_logstd", "kl_driver_judge", "kl_judge_driver", "sym_kl",
                                "max_dev"]
    keys = [(r.focal, r.partner, r.driver, r.judge) for r in df.itertuples()]
    assert keys == [(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1), (0, 1, 1, 0), (0, 1, 1, 1), (1, 0, 0, 0), (1, 0, 0, 1), (1, 0, 1, 0), (1, 0, 1, 1),
                    (1, 1, 1, 1)]
    assert (df["pairs"] > 0).all()
    # two identical members: no disagreement and no divergence, off the diagonal too
    for col in ("disagree", "d_steer_q16", "d_throttle_q16", "d_logstd_q16", "kl_driver_judge_q16", "kl_judge_driver_q16", "max_dev_q16"):
        assert (df[col] == 0).all(), col
    assert (df["disagree_rate"] == 0.0).all() and (df["sym_kl"] == 0.0).all() and (df["max_dev"] == 0.0).all()
    assert (jury_matrix(df, 2).to_numpy() == 0.0).all()
    every = jury_rows("copo", "inter", [w, bc.perturbed(w, 1, 0.05)], plan="everyone", scenes_per_pair=1, num_agents=8, steps=4, seed=0)
    assert len(every) == 2 + 4 + 4 + 2 and (every["pairs"] > 0).all()
    off = every[every.driver != every.judge]
    assert (off["sym_kl"] > 0).all() and (every[every.driver == every.judge]["sym_kl"] == 0.0).all()
    m = jury_matrix(every).to_numpy()
    assert m[0, 1] == m[1, 0] > 0 and m[0, 0] == m[1, 1] == 0.0
