"""Representation similarity on the GPU (copo_hidden_obs_seats_f32, copo_cka_accumulate, copo_cka_finish, copo_amd/eval/similarity.py,
DESIGN.md section 8w).  The cases are those of tests/similarity_cases.py; tests/test_similarity_cpu.py checks their premises on the
float64 model alone.  Tolerances follow test_gpu_certify.py's rule: tau = 4 dev, dev what torch fp32 on the CPU loses on the same
quantity against float64; each is printed before it is asserted.  The Gram kernel on grid inputs is compared in BITS.  Outputs and
references are computed once per case and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bank_cases as bc
import crossplay_numpy as cn
import jury_numpy as jn
import similarity_cases as sc
import similarity_numpy as sn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = sc.POISON
CASES = [(h, k) for h in sc.HIDDENS for k in sc.IN_DIMS]
N_OUT = sc.E * sc.N
CAP = 24          # the lists' capacity in the launch tests: six positions behind the 18 listed rows
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lists(counts, cap=CAP):
    """Every member's list is the common one, cut to its count (0: an empty judge); the tail holds row 0."""
    rows = np.zeros((sc.K, cap), np.int64)
    for j, c in enumerate(counts):
        rows[j, :c] = sc.rows()[:c]
    return SimpleNamespace(K=sc.K, cap=cap, n_out=N_OUT, rows=_dev(rows), counts=_dev(np.asarray(counts, np.int32)))


def _accumulators(M, H, R):
    from copo_amd.eval.similarity import SimilarityAccumulators
    return SimilarityAccumulators(M, H, R, "cuda")


def _accumulate(hidden, panel, rows, count, flags, seat, rows_of, acc):
    from copo_amd.eval.similarity import cka_accumulate
    cka_accumulate(hidden, _dev(np.asarray(panel, np.int32)), _dev(rows), _dev(np.array([count], np.int32)), _dev(flags).view(-1), _dev(seat).view(-1),
                   -1 if rows_of is None else rows_of, acc.S, acc.s, acc.n)


@functools.lru_cache(maxsize=None)
def _case(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    ref = sc.reference(hidden, in_dim)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), ref["members"])
    bank.sync_mirror()
    obs = _dev(ref["obs"])
    out = {}
    for name, counts in (("all", (sc.COUNT,) * 3), ("again", (sc.COUNT,) * 3), ("empty", (sc.COUNT, 0, 17))):
        hid = _poison(sc.K, CAP, 2, hidden)
        bank.hidden_seats(_lists(counts), obs, hid)
        out[name] = hid
    verdict = _poison(N_OUT, sc.K, 4)
    bank.jury_seats(_lists((sc.COUNT,) * 3), obs, verdict)
    torch.cuda.synchronize()
    assert torch.equal(obs, _dev(ref["obs"]))          # the observation is left alone
    return dict(ref=ref, bank=bank, obs=obs, hidden={k: v.cpu().numpy() for k, v in out.items()}, hidden_dev=out["all"], verdict=verdict.cpu().numpy())


@pytest.mark.parametrize("hidden,in_dim", CASES)
def test_the_hidden_launch_equals_the_jury(hidden, in_dim):
    """(1) W3 / b3 in float64 on the stored h2 against the jury kernel's verdict, within 4 x what torch fp32 loses on that head sum; h1 /
    h2 within tau of the float64 model; two launches agree in bits; positions past the count and an empty judge's plane keep the poison."""
    c = _case(hidden, in_dim)
    ref, hid, rows = c["ref"], c["hidden"]["all"], sc.rows()
    assert (_u32(hid[:, sc.COUNT:]) == POISON).all() and (_u32(hid[:, :sc.COUNT]) != POISON).all()
    assert np.array_equal(_u32(hid), _u32(c["hidden"]["again"]))
    e = c["hidden"]["empty"]
    assert (_u32(e[1]) == POISON).all() and (_u32(e[2, 17:]) == POISON).all()
    assert np.array_equal(_u32(e[0]), _u32(hid[0])) and np.array_equal(_u32(e[2, :17]), _u32(hid[2, :17]))          # whichever rows share the tile
    worst = dev = 0.0
    for j, w in enumerate(ref["members"]):
        net = sc.ac.net_of(w)
        h2 = hid[j, :sc.COUNT, 1]
        want = sn.heads64(net, h2)
        got = c["verdict"][rows, j].astype(np.float64)
        W3, b3 = (torch.from_numpy(np.asarray(a, F)) for a in net[4:])
        dev = max(dev, float(np.abs((torch.from_numpy(h2) @ W3.T + b3).numpy().astype(np.float64) - want).max()))
        worst = max(worst, float(np.abs(got - want).max()))
    print("hidden %d in_dim %d: max |verdict - W3 h2 + b3 in float64| = %.3g, torch fp32's own %.3g, tau = %.3g" % (hidden, in_dim, worst, dev, 4 * dev))
    assert (_u32(c["verdict"][rows]) != POISON).all() and dev > 0.0
    assert worst <= 4.0 * dev
    off = float(np.abs(hid[:, :sc.COUNT].astype(np.float64) - ref["hidden64"][:, rows]).max())
    print("hidden %d in_dim %d: max |h - float64 model| = %.3g, torch fp32's own %.3g, tau = %.3g" % (hidden, in_dim, off, ref["dev_hidden"], ref["tau_hidden"]))
    assert off <= ref["tau_hidden"]


@pytest.mark.parametrize("H", sc.HIDDENS)
def test_the_gram_kernel_is_exact_on_grid_inputs(H):
    """(2) Hand-made workspaces with values in {-1, -0.5, 0, 0.5, 1}, NaN at every position that is not counted, random flags, three
    launches that accumulate: S, s and n equal the float64 model bit for bit, with one plane and with two.  320 rows cross the
    promotion interval (128 rows) and the row split."""
    for count in sc.GRID_COUNTS:
        for rows_of in sc.ROWS_OF:
            g = sc.grid_case(H, count, rows_of)
            for R in sc.GRID_PLANES:
                acc = _accumulators(sc.GRID_K, H, R)
                for ws, flags, _ in g["steps"]:
                    _accumulate(_dev(ws), range(sc.GRID_K), g["rows"], count, flags, g["seat"], rows_of, acc)
                torch.cuda.synchronize()
                S, s, n = acc.S.cpu().numpy(), acc.s.cpu().numpy(), acc.n.cpu().numpy()
                where = (H, count, rows_of, R)
                assert int(n.sum()) == g["acc"]["n"], where
                assert np.array_equal(S.sum(axis=0), g["acc"]["S"]), where          # (every value is a multiple of 1/4 far below 2^53: the sums are exact)
                assert np.array_equal(s.sum(axis=0), g["acc"]["s"]), where
                if R == 2 and count > sc.CHUNK:
                    assert n[0] > 0 and n[1] > 0 and np.abs(S[1]).max() > 0, where          # both planes took their chunks
                if R == 2 and count <= sc.CHUNK:
                    assert not S[1].any() and not s[1].any() and n[1] == 0, where
    assert sc.grid_case(H, 320, None)["acc"]["n"] > 2 * sc.PROMOTE_ROWS


@functools.lru_cache(maxsize=None)
def _gram(hidden, in_dim, rows_of):
    """The Gram kernel on the hidden launch's own output, the step accumulated three times, twice over."""
    c = _case(hidden, in_dim)
    runs = []
    for _ in range(2):
        acc = _accumulators(sc.K, hidden, 1)
        for _ in range(3):
            _accumulate(c["hidden_dev"], range(sc.K), np.concatenate([sc.rows(), np.zeros(CAP - sc.COUNT, np.int64)]), sc.COUNT, sc.jc.flags(), sc.SEAT,
                        rows_of, acc)
        runs.append((acc, acc.finish()))
    return runs


@pytest.mark.parametrize("hidden,in_dim", [(64, 91), (256, 92), (512, 91)])
def test_the_gram_kernel_on_real_activations(hidden, in_dim):
    """(3) S within tau of the float64 model of the same fp32 activations; two runs of the sequence give the same bits."""
    c = _case(hidden, in_dim)
    for rows_of in sc.ROWS_OF:
        (a0, _), (a1, _) = _gram(hidden, in_dim, rows_of)
        for name in ("S", "s", "n"):
            assert torch.equal(getattr(a0, name), getattr(a1, name)), name
        m = sc.model(c["hidden"]["all"][:, :sc.COUNT], rows_of)
        want = 3.0 * m["acc"]["S"]
        dev = 3.0 * float(np.abs(sc.torch_gram32(c["hidden"]["all"][:, :sc.COUNT], range(sc.K), m["mask"]).astype(np.float64) - m["acc"]["S"]).max())
        off = float(np.abs(a0.S.cpu().numpy()[0] - want).max())
        print("hidden %d rows_of %s: max |S - float64 model| = %.3g, torch fp32's own %.3g, tau = %.3g, n = %d" % (hidden, rows_of, off, dev, 4 * dev, m["acc"]["n"]))
        assert int(a0.n.cpu()[0]) == 3 * m["acc"]["n"] and dev > 0.0
        assert off <= 4.0 * dev
        # s: an fp32 sum of n values of magnitude <= 1 per launch loses n (n - 1) half-ulps of n at the most, whatever the order
        assert np.abs(a0.s.cpu().numpy()[0] - 3.0 * m["acc"]["s"]).max() <= 3.0 * m["acc"]["n"] ** 2 * 2.0 ** -24


@pytest.mark.parametrize("hidden,in_dim", [(64, 91), (256, 92)])
def test_finish_and_cka(hidden, in_dim):
    """(4) cka within 1e-5 of the model applied to the kernel's own accumulators (finish is float64: summation order only), cka(a, a) ==
    1 within 1e-12, the unit statistics, and n == 0 gives NaN in the frame."""
    from copo_amd.eval.similarity import SimilarityPlan, similarity_frame, unit_frame
    from copo_amd.eval.crossplay import SeatPlan
    plan = SimilarityPlan(SeatPlan(sc.SEAT, sc.K, sc.GROUP, sc.G))
    for rows_of in sc.ROWS_OF:
        acc, got = _gram(hidden, in_dim, rows_of)[0]
        own = dict(S=acc.S.cpu().numpy()[0], s=acc.s.cpu().numpy()[0], n=int(acc.n.cpu()[0]))
        hs = sn.hsic(own, sc.K)
        want = sn.cka(hs, own["n"])
        assert got["n"] == own["n"] >= 2
        print("hidden %d rows_of %s: max |cka - model| = %.3g" % (hidden, rows_of, float(np.abs(got["cka"] - want).max())))
        assert np.abs(got["cka"] - want).max() < 1e-5 and np.allclose(got["hsic"], hs, rtol=1e-9, atol=0)
        for layer in range(2):
            assert np.abs(np.diag(got["cka"][:, :, layer]) - 1.0).max() < 1e-12
        assert np.array_equal(got["hsic"], got["hsic"].transpose(1, 0, 2))
        mean, var = sn.unit_stats(own, sc.K)
        assert np.allclose(got["mean"], mean, rtol=0, atol=1e-14) and np.allclose(got["var"], var, rtol=0, atol=1e-12)
        u = unit_frame(got["mean"], got["var"], got["n"], plan)
        assert len(u) == sc.K * 2 and [(r.dead_units, r.saturated_units) for r in u.itertuples()] == [sn.census(mean[a, l], var[a, l])[:2] for a in range(sc.K) for l in range(2)]
    empty = _accumulators(sc.K, hidden, 2).finish()
    assert empty["n"] == 0 and np.isnan(empty["cka"]).all() and not empty["hsic"].any() and not empty["var"].any()
    assert np.isnan(similarity_frame(empty["hsic"], empty["n"], plan)["cka"]).all()


@pytest.mark.parametrize("hidden,in_dim", [(64, 91), (256, 92)])
def test_the_permuted_twin(hidden, in_dim):
    """(4, the twin) cka(0, 0') within 4 x |1 - cka| of the torch-fp32 CPU pipeline, while the jury sees the same policy (symmetric KL
    ~ 0) and the weight distance is large."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.jury import jury_verdicts
    from copo_amd.eval.similarity import cka_of, hidden_activations
    ref = sc.reference(hidden, in_dim)
    w0 = ref["members"][0]
    pair = [w0, sc.twin_of(w0)]
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), pair)
    obs = _dev(ref["obs"])
    got = cka_of(bank, obs)
    h32 = sc.torch_hidden32(pair, ref["obs"])
    every = np.ones(N_OUT, bool)
    acc32 = dict(S=sc.torch_gram32(h32, (0, 1), every).astype(np.float64), s=h32.sum(axis=1, dtype=np.float32).astype(np.float64), n=N_OUT)
    dev = float(np.abs(1.0 - sn.cka(sn.hsic(acc32, 2), N_OUT)[0, 1]).max())
    off = float(np.abs(1.0 - got["cka"][0, 1]).max())
    print("hidden %d: |1 - cka(0, 0')| = %.3g, the torch fp32 pipeline's %.3g, tau = %.3g" % (hidden, off, dev, 4 * dev))
    assert got["n"] == N_OUT and dev > 0.0
    assert off <= 4.0 * dev
    v = jury_verdicts(bank, obs).cpu().numpy()
    sym = max(0.5 * (jn.kl(v[r, 0], v[r, 1]) + jn.kl(v[r, 1], v[r, 0])) for r in range(N_OUT))
    print("hidden %d: largest symmetric KL of the pair %.3g, weight distance %.3g" % (hidden, sym, sc.weight_distance(*pair)))
    assert sym < 1e-9 and sc.weight_distance(*pair) > 1.0
    hid = hidden_activations(bank, obs)
    assert tuple(hid.shape) == (2, N_OUT, 2, hidden)
    assert np.abs(hid.cpu().numpy().astype(np.float64) - sc.hidden_of(pair, ref["obs"])).max() <= ref["tau_hidden"]


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
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    keep = []
    for _ in range(n_frag):
        smp.sample()
        torch.cuda.synchronize()
        keep.append({k: (getattr(smp.acc, k[4:]) if k.startswith("acc.") else getattr(smp, k)).clone() for k in keys})
    return keep


def test_captured_fragment_equals_eager_and_the_drive_is_untouched(e2e):
    """(5)"""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    from copo_amd.eval.similarity import SimilarityPlan, SimilaritySeatSampler, hidden_activations
    t, ws = e2e
    E, N, T = E2E
    plan = SeatPlan.pairs(3, 1, N, 0.5)
    bank = PolicyBank(t.policy, ws)
    drive = ("tally", "actions", "clipped", "flags", "obs", "dist_inputs", "logp")
    keys = ("acc.S", "acc.s", "acc.n", "hidden") + drive
    for rows_of in sc.ROWS_OF:
        similarity = SimilarityPlan(plan, rows_of=rows_of)
        runs = {}
        for mode in (False, True):
            smp = SimilaritySeatSampler(t.env, t.policy, bank, plan, similarity, T, use_graph=mode)
            smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
            runs[mode] = _fragments(smp, 2, keys)
            assert (smp._loop.graph is not None) == mode
        for f in range(2):
            for k in keys:
                assert torch.equal(runs[False][f][k], runs[True][f][k]), (f, k)
        plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 2, drive)
        for f in range(2):
            for k in drive:
                assert torch.equal(plain[f][k], runs[True][f][k]), (f, k)          # the study does not touch the drive
        # the accumulators of the two fragments == the float64 model over their recorded obs / flags, activations from hidden_activations
        want = None
        for f in range(2):
            for step in range(T):
                full = hidden_activations(bank, runs[True][f]["obs"][step].reshape(E * N, -1).contiguous()).cpu().numpy()
                mask = sn.counted(similarity.rows, similarity.count, runs[True][f]["flags"][step].cpu().numpy(), plan.seat, similarity.rows_of)
                want = sn.accumulate(full[:, similarity.rows], range(3), mask, want)
        got = runs[True][1]
        R = smp.acc.R
        assert int(got["acc.n"].sum()) == want["n"] > 2 and R == similarity.planes(256)
        scale = float(np.abs(want["S"]).max())
        assert np.abs(got["acc.S"].sum(dim=0).cpu().numpy() - want["S"]).max() < 1e-5 * scale
        st = got["tally"].cpu().numpy()
        assert want["n"] == (st[:, 1, 0].sum() if rows_of == 1 else st[..., 0].sum())          # every acted seat-step, once
        frame, units = smp.frame(labels=["a", "b", "c"]), smp.units()
        assert len(frame) == 3 * 3 * 2 and (frame["n"] == want["n"]).all() and len(units) == 3 * 2
        assert (frame[frame.member_a == frame.member_b]["cka"] - 1.0).abs().max() < 1e-12
        off = frame[frame.member_a != frame.member_b]["cka"]
        assert ((off > 0) & (off < 1)).all()
        smp.clear_tally()
        assert int(smp.acc.n.sum()) == 0 and not smp.acc.S.any() and int(smp.tally.abs().sum()) == 0


def test_refusals_and_similarity_rows(golden_dir):
    """(6) What the Python layer and the entries refuse (nothing is launched), and the frame of `similarity_rows`."""
    import ctypes as C
    from copo_amd import _capi
    from copo_amd.eval.similarity import cka_accumulate, cka_finish, similarity_matrix, similarity_rows
    c = _case(64, 91)
    bank, obs = c["bank"], c["obs"]
    jb, hid = _lists((sc.COUNT,) * 3), _poison(sc.K, CAP, 2, 64)
    for bad in (dict(obs=obs[:, :90].contiguous()), dict(hidden=_poison(sc.K, CAP, 2, 128)), dict(hidden=_poison(sc.K, CAP + 1, 2, 64)),
                dict(hidden=torch.zeros(sc.K, CAP, 2, 64, dtype=torch.float64, device="cuda")), dict(hidden=_poison(sc.K, 2, CAP, 64).transpose(1, 2))):
        with pytest.raises(ValueError):
            bank.hidden_seats(jb, **dict(dict(obs=obs, hidden=hid), **bad))
    good = dict(cfg=C.byref(bank.cfg), theta=bank.theta.data_ptr(), theta_t=bank.theta_t.data_ptr(), member_stride=bank.stride, n_members=sc.K,
                rows=jb.rows.data_ptr(), counts=jb.counts.data_ptr(), cap=jb.cap, n_out=N_OUT, obs_src=obs.data_ptr(), hidden=hid.data_ptr(),
                stream=_capi.current_stream())
    call = lambda **kw: _capi.lib.copo_hidden_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("rows", "counts", "hidden", "obs_src", "theta", "theta_t"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(cap=0), dict(n_out=0), dict(n_members=0), dict(n_members=65536), dict(member_stride=bank.stride - 4), dict(hidden=hid.data_ptr() + 4)):
        assert call(**bad) == -2, bad
    acc = _accumulators(sc.K, 64, 1)
    panel, rows, count = _dev(np.arange(sc.K, dtype=np.int32)), _dev(np.zeros(CAP, np.int64)), _dev(np.array([sc.COUNT], np.int32))
    flags, seat = _dev(sc.jc.flags()).view(-1), _dev(sc.SEAT).view(-1)
    args = dict(hidden=hid, panel=panel, rows=rows, count=count, flags=flags, seat=seat, rows_of=-1, S=acc.S, s=acc.s, n=acc.n)
    for bad in (dict(hidden=hid[:, :, :1]), dict(panel=panel.long()), dict(rows=rows[:5]), dict(count=count.long()), dict(flags=flags[:9]),
                dict(seat=seat.long()), dict(S=acc.S.float()), dict(s=acc.s[:, :2]), dict(n=acc.n.int()), dict(S=acc.S[:, :5])):
        with pytest.raises(ValueError):
            cka_accumulate(**dict(args, **bad))
    with pytest.raises(_capi.CopoError):
        cka_accumulate(**dict(args, rows_of=3))
    with pytest.raises(ValueError):
        cka_finish(acc.S, acc.s, acc.n, acc.hsic[:2], acc.n_out, acc.mean, acc.var)
    low = dict(hidden=hid.data_ptr(), n_members=sc.K, cap=CAP, H=64, panel=panel.data_ptr(), n_panel=sc.K, rows=rows.data_ptr(), count=count.data_ptr(),
               flags=flags.data_ptr(), seat=seat.data_ptr(), n_out=N_OUT, rows_of=-1, n_planes=1, S=acc.S.data_ptr(), s=acc.s.data_ptr(), n=acc.n.data_ptr(),
               stream=_capi.current_stream())
    raw = lambda **kw: _capi.lib.copo_cka_accumulate(*dict(low, **kw).values())  # noqa: E731
    for name in ("hidden", "panel", "rows", "count", "flags", "seat", "S", "s", "n"):
        assert raw(**{name: None}) == -1, name
    for bad in (dict(H=96), dict(H=1024), dict(H=0), dict(n_panel=0), dict(n_panel=256), dict(n_planes=0), dict(n_planes=9), dict(cap=0), dict(n_out=0),
                dict(n_members=0), dict(rows_of=3), dict(hidden=hid.data_ptr() + 4)):
        assert raw(**bad) == -2, bad
    fin = dict(S=acc.S.data_ptr(), s=acc.s.data_ptr(), n=acc.n.data_ptr(), n_panel=sc.K, H=64, n_planes=1, hsic=acc.hsic.data_ptr(), n_out=acc.n_out.data_ptr(),
               mean=acc.mean.data_ptr(), var=acc.var.data_ptr(), stream=_capi.current_stream())
    rawf = lambda **kw: _capi.lib.copo_cka_finish(*dict(fin, **kw).values())  # noqa: E731
    for name in ("S", "s", "n", "hsic", "n_out", "mean", "var"):
        assert rawf(**{name: None}) == -1, name
    for bad in (dict(H=32), dict(n_panel=0), dict(n_planes=9)):
        assert rawf(**bad) == -2, bad
    torch.cuda.synchronize()
    assert (hid.view(torch.int32) == POISON).all() and not acc.S.any() and not acc.s.any() and not acc.n.any()
    # ---- similarity_rows ----
    w = bc.golden_population(golden_dir, "copo_inter")
    df = similarity_rows("copo", "inter", [w, dict(w), bc.perturbed(w, 1, 0.05)], scenes_per_pair=1, num_agents=8, steps=8, seed=0, labels=["a", "b", "c"])
    assert list(df.columns) == ["member_a", "member_b", "label_a", "label_b", "layer", "rows_of", "n", "hsic", "cka"]
    assert [(r.member_a, r.member_b, r.layer) for r in df.itertuples()] == [(a, b, l) for a in range(3) for b in range(3) for l in ("h1", "h2")]
    assert (df["n"] > 2).all() and (df["rows_of"] == -1).all()
    same = df[(df.member_a == 0) & (df.member_b == 1)]
    assert (same["cka"] - 1.0).abs().max() < 1e-12          # two identical members: equal bits in, equal sums out
    other = df[(df.member_a == 0) & (df.member_b == 2)]["cka"]
    assert ((other > 0.5) & (other < 1.0)).all()
    m = similarity_matrix(df, "h2").to_numpy()
    assert m.shape == (3, 3) and np.array_equal(m, m.T)
    one = similarity_rows("copo", "inter", [w, bc.perturbed(w, 1, 0.05)], rows_of=1, scenes_per_pair=1, num_agents=8, steps=4, seed=0)
    assert len(one) == 2 * 2 * 2 and (one["rows_of"] == 1).all() and 0 < one["n"].iloc[0] < df["n"].iloc[0]
    with pytest.raises(ValueError):
        similarity_rows("copo", "inter", [w], steps=4)
    with pytest.raises(ValueError):
        similarity_rows("copo", "inter", [w, w], rows_of=2, steps=4)
