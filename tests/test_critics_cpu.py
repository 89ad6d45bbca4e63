"""CPU: the critic audit (copo_amd/eval/critics.py, copo_value_obs_seats_f32, copo_audit_*) -- the forward form of
the audit against the backward recursion on the crafted streams, the frame arithmetic and its two fixed points, the plans, the loader
that keeps value nets, the bank's refusals, and what is exported and refused without touching a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_numpy as cn


def test_the_streams_cover_what_they_claim():
    s = cc.stream()
    lengths, both, trunc, open_ = cc.covered(s)
    assert {1, 2, 17} <= lengths and both >= 10 and trunc >= 3 and open_ >= 5
    assert (s["seat"] == -1).sum() == 2 and set(s["group"]) == {0, 1, 2} and (s["flags"] & cn.F_ENV_RESET).any()
    v = s["values"][(s["flags"] & cn.F_ACTED) != 0]
    assert (v < -2.0).any() and (v > 2.0).any() and set(cc.GAMMAS) == {1.0, 0.99, 0.9}
    assert {b for b, _ in cc.CONFIGS} >= {1, 16} and {c for _, c in cc.CONFIGS} == {False, True}


@pytest.mark.parametrize("bins,count_truncated", cc.CONFIGS)
def test_forward_form_is_the_backward_recursion(bins, count_truncated):
    """The identity: the carried sums give sum G_t, sum V_t G_t, sum G_t^2 and the per-bin sums of G_t, to 1e-10 relative."""
    s = cc.stream()
    fs, fw = cn.forward_fold(s, cc.GAMMAS, cc.RANGES, bins, count_truncated, cc.K, cc.G)
    bs, bw = cn.backward_fold(s, cc.GAMMAS, cc.RANGES, bins, count_truncated, cc.K, cc.G)
    assert fs[..., cn.AGENTS].sum() >= 30 and (fs[..., cn.SUM_GG] > 0).any()
    for w in cn.COUNT_WORDS:
        assert np.array_equal(fs[..., w], bs[..., w]) and np.array_equal(fw[..., w], bw[..., w]), w
    scale = np.maximum(np.abs(bs).max(axis=(0, 1), keepdims=True), 1.0)          # per (head, word): the sums cancel, the terms do not
    assert (np.abs(fs - bs) / scale).max() <= 1e-10
    assert np.abs(fw - bw).max() <= fs[..., cn.AGENTS].max()          # one rounding per agent
    assert not fs[..., cn.BIN_COUNT + bins:cn.BIN_VALUE].any() and np.array_equal(fs[..., cn.BIN_COUNT:cn.BIN_VALUE].sum(-1), fs[..., cn.STEPS])
    assert np.allclose(fs[..., cn.BIN_RETURN:].sum(-1), fs[..., cn.SUM_G], rtol=0, atol=1e-9)
    trunc = fs[..., cn.TRUNCATED].sum()
    assert trunc > 0
    if not count_truncated:          # the truncated agents are in no other word
        other, _ = cn.forward_fold(s, cc.GAMMAS, cc.RANGES, bins, True, cc.K, cc.G)
        assert other[..., cn.AGENTS].sum() == fs[..., cn.AGENTS].sum() + trunc


def test_permuted_scenes_give_the_same_model_words():
    s = cc.stream()
    a = cn.forward_fold(s, cc.GAMMAS, cc.RANGES, 16, False, cc.K, cc.G)[1]
    b = cn.forward_fold(cc.permuted(s), cc.GAMMAS, cc.RANGES, 16, False, cc.K, cc.G)[1]
    assert np.array_equal(a, b) and a.any()


def _words_of(V, Gt, audit, head=0):
    from copo_amd.eval import critics as cr
    w = np.zeros(cr.N_WORDS, np.int64)
    q = lambda x: int(np.rint(float(x) * cr.Q16))  # noqa: E731
    w[:8] = [1, len(V), 0, q(V.sum()), q((V * V).sum()), q(Gt.sum()), q((V * Gt).sum()), q((Gt * Gt).sum())]
    lo, hi = audit.value_range[head]
    for v, g in zip(V, Gt):
        b = cn.bin_of(v, lo, hi, audit.bins)
        w[cr.BIN_COUNT + b] += 1
        w[cr.BIN_VALUE + b] += q(v)
        w[cr.BIN_RETURN + b] += q(g)
    return w


def test_frame_arithmetic_and_fixed_points():
    from copo_amd.eval import critics as cr
    from copo_amd.eval.crossplay import SeatPlan
    audit = cr.CriticAudit([0.99], (-4.0, 4.0), bins=4)
    Gt = np.array([0.5, -1.0, 2.0, 3.5, -2.5, 1.25])          # multiples of 2^-16: every word is exact
    perfect = cr.critic_stats(_words_of(Gt, Gt, audit))
    assert perfect["explained_variance"] == 1.0 and perfect["bias"] == 0.0 and perfect["rmse"] == 0.0 and abs(perfect["corr"] - 1.0) < 1e-12
    const = cr.critic_stats(_words_of(np.full(6, 0.75), Gt, audit))
    assert const["explained_variance"] == 0.0 and np.isnan(const["corr"]) and const["bias"] == 0.75 - Gt.mean()
    V = np.array([1.0, -0.5, 1.5, 3.0, -3.0, 0.0])
    got = cr.critic_stats(_words_of(V, Gt, audit))
    assert np.isclose(got["explained_variance"], 1.0 - np.var(Gt - V) / np.var(Gt)) and np.isclose(got["bias"], (V - Gt).mean())
    assert np.isclose(got["rmse"], np.sqrt(((V - Gt) ** 2).mean())) and np.isclose(got["corr"], np.corrcoef(V, Gt)[0, 1])
    assert np.isclose(got["mean_return"], Gt.mean()) and np.isclose(got["mean_value"], V.mean())
    assert all(np.isnan(v) for v in cr.critic_stats(np.zeros(cr.N_WORDS, np.int64)).values())
    plan = SeatPlan.pairs(2, 1, 4, 0.5)
    words = np.zeros((4, 2, 1, cr.N_WORDS), np.int64)
    words[:, :, 0] = _words_of(V, Gt, audit)
    df = cr.critic_frame(words, plan, audit, ["a", "b"])
    assert len(df) == 6 and list(df["label"]) == ["a", "a", "b", "a", "b", "b"] and {"focal", "partner", "head_name", "explained_variance"} <= set(df.columns)
    assert (df["steps"] == 6).all() and np.allclose(df["bias"], (V - Gt).mean())
    cal = cr.calibration_frame(words, plan, audit, ["a", "b"])
    assert len(cal) == 6 * 4 and cal["count"].sum() == 6 * 6
    one = cal[(cal["group"] == 0) & (cal["bin"] == 3)].iloc[0]          # [2, 4): V = 3.0 alone
    assert (one["count"], one["mean_value"], one["mean_return"], one["value_lo"], one["value_hi"]) == (1, 3.0, 3.5, 2.0, 4.0)
    assert np.isnan(cr.calibration_frame(np.zeros_like(words), plan, audit)["mean_value"]).all()
    with pytest.raises(ValueError, match="critic words"):
        cr.critic_frame(words[:, :1], plan, audit)


def test_plan_and_range_refusals():
    from copo_amd.eval import critics as cr
    for bad in (dict(gammas=[]), dict(gammas=[0.9] * 4), dict(gammas=[1.5]), dict(gammas=[-0.1]), dict(bins=0), dict(bins=17), dict(bins=2.5),
                dict(value_range=(1.0, 1.0)), dict(value_range=(2.0, -2.0)), dict(value_range=(0.0, np.inf)), dict(value_range=((0, 1), (0, 1))),
                dict(value_range=(0.0, 1.0, 2.0))):
        with pytest.raises(ValueError, match="CriticAudit"):
            cr.CriticAudit(**dict(dict(gammas=[0.99]), **bad))
    a = cr.CriticAudit([0.99, 0.99, 1.0], ((-1, 1), (-2, 2), (0, 4)), bins=16, count_truncated=True)
    assert a.heads == 3 and a.value_range[2] == (0.0, 4.0) and np.array_equal(a.bin_edges(2), np.linspace(0, 4, 17)) and a.count_truncated
    assert cr.CriticAudit([0.9, 0.9], (-3, 3)).value_range == ((-3.0, 3.0),) * 2
    uni = cr.audit_plan(3, 2, 4)
    assert (uni.E, uni.K, uni.n_groups, uni.replica_scenes) == (6, 3, 3, 2) and list(uni.group) == [0, 0, 1, 1, 2, 2] and (uni.seat[2:4] == 1).all()
    pairs = cr.audit_plan(2, 3, 4, pairs=True, share=0.25)
    assert (pairs.E, pairs.n_groups, pairs.n_focal) == (12, 4, 1) and cr.audit_plan(2, 1, 4, pairs=True).n_focal == 2
    with pytest.raises(ValueError, match="audit_plan"):
        cr.audit_plan(0, 1, 4)
    with pytest.raises(ValueError, match="goes with pairs"):          # whole scenes per member have no share: not ignored, refused
        cr.audit_plan(2, 1, 4, share=0.25)
    for kw in (dict(bins=0), dict(value_range=(1, 0)), dict(gammas=[2.0])):          # refused before any device is touched
        with pytest.raises(ValueError, match="CriticAudit"):
            cr.critic_audit_rows("ippo", "inter", [{}], **kw)
    with pytest.raises(ValueError, match="no members"):
        cr.critic_audit_rows("ippo", "inter", [])

    class FakeBank:
        has_values, K = False, 1
    with pytest.raises(ValueError, match="no value nets"):
        cr.check_critic_input("x", None, FakeBank(), 91)


def _state(seed=0, in_dim=7, hidden=8, copo=True):
    rng = np.random.RandomState(seed)
    sd = {}
    nets = [("_hidden_layers.0._model.0", hidden, in_dim), ("_hidden_layers.1._model.0", hidden, hidden), ("_logits._model.0", 4, hidden),
            ("_value_branch_separate.0._model.0", hidden, in_dim), ("_value_branch_separate.1._model.0", hidden, hidden), ("_value_branch._model.0", 1, hidden)]
    if copo:
        for name in ("nei_value_network", "global_value_network"):
            nets += [(name + ".0._model.0", hidden, in_dim), (name + ".1._model.0", hidden, hidden), (name + ".2._model.0", 1, hidden)]
    for name, o, i in nets:
        sd[name + ".weight"], sd[name + ".bias"] = rng.randn(o, i).astype(np.float32), rng.randn(o).astype(np.float32)
    return sd


def test_loader_keeps_value_keys_only_on_request(tmp_path):
    from copo_amd.eval import checkpoint_io as io

    class Model:
        def __init__(self, sd):
            self.sd = sd

        def state_dict(self):
            return {k: torch.from_numpy(v) for k, v in self.sd.items()}
    sd = _state()
    ckpt, npz, pol_npz = str(tmp_path / "checkpoint-1"), str(tmp_path / "full.npz"), str(tmp_path / "policy.npz")
    io.save_tune_style_checkpoint(Model(dict(sd, lcf_parameters=np.zeros(2))), ckpt)
    np.savez(npz, **sd)
    io.export_policy_npz(Model(sd), pol_npz)
    plain, = io.load_members([ckpt])
    again = io.checkpoint_policy_weights(ckpt)
    assert list(plain) == list(again) and all(np.array_equal(plain[k], again[k]) for k in plain)
    assert sorted(plain) == sorted([k for k in sd if "value" not in k] + ["lcf_parameters"])          # today's dict: no value entry
    full, from_npz, pol = io.load_members([ckpt, npz, pol_npz], values=True)
    assert sorted(full) == sorted(list(sd) + ["lcf_parameters"]) and sorted(from_npz) == sorted(sd)
    for k in sd:
        assert np.array_equal(full[k], sd[k]) and np.array_equal(from_npz[k], sd[k]), k
    vsd = io.value_state_dict(full)
    assert sorted(vsd) == sorted(k for k in sd if "value" in k) and len(vsd) == 18 and all(v.dtype == torch.float32 for v in vsd.values())
    assert torch.equal(vsd["nei_value_network.2._model.0.weight"], torch.from_numpy(sd["nei_value_network.2._model.0.weight"]))
    assert io.value_state_dict(pol) == {} and not any(io.is_value_key(k) for k in pol)
    assert io.is_value_key("_value_branch._model.0.bias") and not io.is_value_key("_logits._model.0.bias") and not io.is_value_key("lcf_parameters")


def test_bank_refuses_members_without_or_with_other_value_nets():
    """The checks run on the host before any member is loaded: a model stub with a fused learner's face is enough."""
    from copo_amd.eval.bank import PolicyBank
    sd = _state()

    class Model:
        def state_dict(self):
            return {k: torch.from_numpy(v) for k, v in sd.items()}

    class Fused:
        can_forward = True

    class Policy:
        fused, model = Fused(), Model()
    policy_only = {k: v for k, v in sd.items() if "value" not in k}
    with pytest.raises(ValueError, match=r"member 1: no value entry _value_branch_separate\.0\._model\.0\.weight"):
        PolicyBank(Policy(), [sd, policy_only], values=True)
    lacks_one = {k: v for k, v in sd.items() if k != "global_value_network.2._model.0.bias"}
    with pytest.raises(ValueError, match=r"member 0: no value entry global_value_network\.2\._model\.0\.bias"):
        PolicyBank(Policy(), [lacks_one], values=True)
    other = dict(sd)
    other["nei_value_network.0._model.0.weight"] = np.zeros((8, 9), np.float32)
    with pytest.raises(ValueError, match=r"member 2: nei_value_network\.0\._model\.0\.weight has shape \(8, 9\), the model's is \(8, 7\)"):
        PolicyBank(Policy(), [sd, sd, other], values=True)


def test_exports_and_refusals():
    """The new entry points, their ctypes signatures, and what they refuse without touching a device."""
    from copo_amd import _abi, _capi
    names = {"copo_value_obs_seats_f32", "copo_audit_create", "copo_audit_record", "copo_audit_read", "copo_audit_reset", "copo_audit_destroy"}
    assert names <= set(_capi.EXPORTED_SYMBOLS) and _capi.lib.copo_version() == 8 == _abi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), "..", "include", "copo_hip.h")).read()
    assert all("int %s(" % n in header for n in names)
    assert _capi.lib.copo_value_obs_seats_f32.argtypes == [C.POINTER(_capi.PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                                          C.c_int64, C.c_int64] + [C.c_void_p] * 4
    assert (_abi.AUDIT_WORDS, _abi.AUDIT_MAX_BINS, _abi.AUDIT_BIN_COUNT, _abi.AUDIT_BIN_VALUE, _abi.AUDIT_BIN_RETURN) == (56, 16, 8, 24, 40)
    assert C.sizeof(_abi.AuditCfg) == 8 * 4 + 9 * 8
    from copo_amd.eval import critics as cr
    assert (cr.N_WORDS, cr.MAX_BINS, cr.BIN_COUNT, cr.BIN_VALUE, cr.BIN_RETURN) == (cn.WORDS, cn.MAX_BINS, cn.BIN_COUNT, cn.BIN_VALUE, cn.BIN_RETURN) == (56, 16, 8, 24, 40)
    cfg = _capi.PpoCfg()
    H, K1 = 64, 92
    net = K1 * H + H + H * H + H + H + 4          # (a value net; offsets below are multiples of 4)
    cfg.mb, cfg.hidden, cfg.act_dim, cfg.n_value_heads, cfg.n_params = 64, H, 2, 3, 4 * 12000
    for h in range(3):
        v, base = cfg.val[h], 12000 * (h + 1)
        v.in_dim, v.out_dim, v.w1, v.b1, v.w2, v.b2, v.w3, v.b3 = K1, 1, base, base + K1 * H, base + K1 * H + H, base + K1 * H + H + H * H, base + net - H - 4, base + net - 4
    fake = 4096          # an aligned non-NULL address: every call below is refused before anything is launched
    good = dict(cfg=C.byref(cfg), theta=fake, theta_t=fake, member_stride=cfg.n_params, n_members=2, rows=fake, counts=fake, cap=4, n_out=8, obs_src=fake,
                cc_src=None, values=fake, stream=None)
    call = lambda **kw: _capi.lib.copo_value_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for bad in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "values"):
        assert call(**{bad: None}) == -1 and b"copo_value_obs_seats_f32" in _capi.lib.copo_last_error(), bad
    for bad in (dict(cap=0), dict(n_out=0), dict(n_members=0), dict(n_members=65536), dict(member_stride=cfg.n_params - 4), dict(member_stride=cfg.n_params + 2),
                dict(theta_t=fake + 4)):
        assert call(**bad) == -2 and b"copo_value_obs_seats_f32" in _capi.lib.copo_last_error(), bad
    for field, value in (("hidden", 96), ("hidden", 32), ("n_value_heads", 0), ("n_value_heads", 4), ("operand_dtype", 1)):
        keep = getattr(cfg, field)
        setattr(cfg, field, value)
        assert call() == -2, (field, value)
        setattr(cfg, field, keep)
    cfg.val[1].in_dim = K1 + 4          # heads of different widths cannot share one source
    assert call() == -2
    cfg.val[1].in_dim = K1
    cfg.val[2].w2 += 2
    assert call() == -2
    cfg.val[2].w2 -= 2
    # the audit handle: NULL and DIM before the device is touched
    out = C.c_void_p()
    a = _abi.AuditCfg(E=2, N=3, K=2, G=1, heads=1, bins=4)
    a.gamma[0], a.lo[0], a.hi[0] = 0.99, -1.0, 1.0
    assert _capi.lib.copo_audit_create(None, C.byref(out)) == -1 and _capi.lib.copo_audit_create(C.byref(a), None) == -1
    for field, value in (("E", 0), ("N", 0), ("K", 0), ("K", 65536), ("G", 0), ("heads", 0), ("heads", 4), ("bins", 0), ("bins", 17)):
        keep = getattr(a, field)
        setattr(a, field, value)
        assert _capi.lib.copo_audit_create(C.byref(a), C.byref(out)) == -2 and b"copo_audit_create" in _capi.lib.copo_last_error() and not out.value, (field, value)
        setattr(a, field, keep)
    for gamma, lo, hi in ((1.5, -1.0, 1.0), (-0.1, -1.0, 1.0), (0.9, 1.0, 1.0), (0.9, 0.0, float("inf")), (float("nan"), 0.0, 1.0)):
        a.gamma[0], a.lo[0], a.hi[0] = gamma, lo, hi
        assert _capi.lib.copo_audit_create(C.byref(a), C.byref(out)) == -5 and not out.value, (gamma, lo, hi)
    assert _capi.lib.copo_audit_record(None, fake, fake, fake, fake, fake, fake, fake, None) == -1
    assert _capi.lib.copo_audit_read(None, fake, None) == -1 and _capi.lib.copo_audit_reset(None, None) == -1 and _capi.lib.copo_audit_destroy(None) == -1


def test_cli_registers_the_audit_next_to_the_study_table(tmp_path, monkeypatch):
    """`--critic-audit` runs through `run_study` with the checkpoints' value nets kept; its options are refused without it."""
    from copo_amd.eval import checkpoint_io, critics, evaluate
    study, = evaluate.CRITIC_STUDIES
    assert (study.option, study.module, study.rows, study.members) == ("critic_audit", "critics", "critic_audit_rows", dict(values=True))
    assert study.option not in [s.option for s in evaluate.STUDIES] and sorted(evaluate.CRITIC_GOES_WITH) == ["critic_bins", "critic_range", "cross_play_pairs"]
    called = []

    def fake_rows(algo, env, weights_list, **kw):
        called.append((algo, env, list(weights_list), kw))
        audit = critics.CriticAudit([0.99], kw["value_range"], kw["bins"])
        plan = critics.audit_plan(2, 1, 4, kw["pairs"], kw.get("share"))
        words = np.ones((plan.n_groups, 2, 1, critics.N_WORDS), np.int64)
        df = critics.critic_frame(words, plan, audit, kw["labels"])
        df.attrs["calibration"] = critics.calibration_frame(words, plan, audit, kw["labels"])
        return df
    monkeypatch.setattr(critics, "critic_audit_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths, values=False: ["w:%s:%s" % (p, values) for p in paths])
    table = str(tmp_path / "t.csv")
    evaluate.main(["--algo", "ippo", "--critic-audit", "a", "b", "--table", table, "--steps", "16", "--scenes-per-pair", "3", "--num-agents", "4"])
    assert called.pop() == ("ippo", "inter", ["w:a:True", "w:b:True"], dict(bins=8, value_range=critics.DEFAULT_RANGE, pairs=False, num_agents=4,
                                                                             steps=16, labels=["a", "b"], scenes_per_pair=3))
    assert os.path.getsize(table) > 0
    evaluate.main(["--critic-audit", "a", "b", "--table", table, "--critic-bins", "16", "--critic-range", "-1", "3", "--cross-play-pairs", "--share", "0.25"])
    kw = called.pop()[3]
    assert (kw["bins"], kw["value_range"], kw["pairs"], kw["share"]) == (16, (-1.0, 3.0), True, 0.25)
    for argv in (["--critic-bins", "4"], ["--critic-range", "0", "1"], ["--cross-play-pairs"], ["--cross-play", "a", "b", "--table", table, "--critic-bins", "4"],
                 ["--critic-audit", "a", "--table", table, "--critic-bins", "0"], ["--critic-audit", "a", "--table", table, "--critic-range", "1", "0"],
                 ["--critic-audit", "a"], ["--critic-audit", "a", "--jury", "b", "--table", table], ["--jury", "b", "--critic-audit", "a", "--table", table],
                 ["--critic-audit", "a", "--table", table, "--share", "0.25"], ["--critic-audit", "a", "--table", table, "--jury-plan", "seated"],
                 ["--critic-audit", "a", "--table", table, "--probe-ridge", "0.1"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        assert e.value.code == 2, argv
    assert not called
