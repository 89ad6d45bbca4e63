"""The critic audit on the GPU (copo_value_obs_seats_f32, copo_audit_*, copo_amd/eval/critics.py).  The value pass is
compared in BITS with copo_mlp_forward_rows_f32 per member (FusedLearner.values(rows=...)) and with the float64 model of
tests/forward_numpy.py under the bound tests/forward_cases.py states for value heads; the audit record runs the crafted streams of
tests/critic_cases.py against tests/critic_numpy.py; the sampler against a plain SeatSampler and against the model fed with its own
recorded values, rewards and flags."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_numpy as cn
import forward_cases as fc

pytestmark = pytest.mark.gpu

from test_gpu_forward_float64 import _load, _policy, _ratio  # noqa: E402

POISON = 0x7fc0beef
N_OUT, CAP = 96, 33
COUNTS = ((0, 1, 15), (16, 17, CAP))
# (algorithm, hidden, observation width): heads 1 and 3, hidden 64 and 256, a width that is a multiple of 4 and one that is not
BIT_CASES = (("copo", 64, 91), ("copo", 256, 92), ("ippo", 64, 92), ("ippo", 256, 91))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _u32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _lists(rows, counts, n_out, K):
    return SimpleNamespace(K=K, cap=rows.shape[1], n_out=n_out, rows=_dev(rows), counts=_dev(np.asarray(counts, np.int32)))


def _state_of(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _members(model, K, sigma=0.1):
    """K full state dicts of the model's shapes: its own, then perturbed copies (every float32 entry, the value nets included)."""
    base = _state_of(model)
    out = [base]
    for k in range(1, K):
        rng = np.random.RandomState(900 + k)
        out.append({n: (v + sigma * rng.standard_normal(v.shape)).astype(np.float32) if v.dtype == np.float32 else v for n, v in base.items()})
    return out


def _single(pol, member, obs, rows):
    """[heads][n_out] of copo_mlp_forward_rows_f32 with `member` loaded into the policy alone; zeros off the list."""
    from copo_amd.eval.checkpoint_io import load_policy_state_dict
    load_policy_state_dict(pol.model, {k: torch.from_numpy(v) for k, v in member.items() if v.dtype == np.float32})
    pol.fused.invalidate_mirror()
    pol.fused.sync_mirror()
    got = pol.fused.values(obs, None, rows=_dev(np.asarray(rows, np.int64)))
    torch.cuda.synchronize()
    return got.clone()


def _bits_case(algo, hidden, width, which):
    from copo_amd.eval.bank import PolicyBank
    pol = _policy(algo, "none", width, hidden)
    keep = _state_of(pol.model)
    members = _members(pol.model, 3)
    bank = PolicyBank(pol, members, values=True)
    bank.sync_mirror()
    nv = int(bank.cfg.n_value_heads)
    rng = np.random.RandomState(hidden + width + which)
    obs = _dev(rng.uniform(-1.0, 1.0, (N_OUT, width)).astype(np.float32))
    counts = COUNTS[which]
    perm = rng.permutation(N_OUT)
    rows = np.zeros((3, CAP), np.int64)
    at = 0
    for k, c in enumerate(counts):
        rows[k, :c] = perm[at:at + c]          # unsorted, no row twice
        at += c
    listed = [list(rows[k, :c]) for k, c in enumerate(counts)]
    bad = None
    if which == 1:          # one index outside [0, n_out) in the middle of a list: skipped, its neighbours are not
        bad = (2, 7, rows[2, 7])
        rows[2, 7] = N_OUT + 5
        listed[2].remove(bad[2])
    out = _poison(N_OUT + 4, nv)
    pb = _lists(rows, counts, N_OUT, 3)
    bank.value_seats(pb, obs, out[:N_OUT])
    torch.cuda.synchronize()
    again = _poison(N_OUT + 4, nv)
    bank.value_seats(pb, obs, again[:N_OUT])
    torch.cuda.synchronize()
    alone = [_single(pol, members[k], obs, listed[k]) if listed[k] else None for k in range(3)]
    from copo_amd.eval.checkpoint_io import load_policy_state_dict
    load_policy_state_dict(pol.model, {k: torch.from_numpy(v) for k, v in keep.items() if v.dtype == np.float32})
    return dict(nv=nv, out=out, again=again, alone=alone, listed=listed, bad=bad, members=members, obs=obs)


@pytest.mark.parametrize("which", [0, 1], ids=["counts_0_1_15", "counts_16_17_cap"])
@pytest.mark.parametrize("algo,hidden,width", BIT_CASES)
def test_value_pass_holds_the_single_member_bits(algo, hidden, width, which):
    c = _bits_case(algo, hidden, width, which)
    assert c["nv"] == (3 if algo == "copo" else 1)
    got = _u32(c["out"])
    seen = np.zeros(N_OUT, bool)
    for k, rows in enumerate(c["listed"]):
        if not rows:
            continue
        want = _u32(c["alone"][k])          # [heads][n_out]
        for h in range(c["nv"]):
            assert np.array_equal(got[rows, h], want[h, rows]), (k, h)
        seen[rows] = True
    assert seen.sum() == sum(len(r) for r in c["listed"]) and not (got[:N_OUT][seen] == POISON).any()
    assert (got[:N_OUT][~seen] == POISON).all() and (got[N_OUT:] == POISON).all()          # rows in no list, and past the array
    if c["bad"] is not None:
        assert not seen[c["bad"][2]]          # the row the bad index replaced is in no list now
    assert np.array_equal(got, _u32(c["again"]))
    if c["nv"] > 1 and c["listed"][1]:          # the members and the heads do differ
        r = c["listed"][1][0]
        assert len({int(v) for v in got[r]}) == c["nv"]


@pytest.mark.parametrize("name", ["copo_92", "copo_260"])
def test_value_pass_against_float64(name):
    """forward_cases' CoPO critic cases (hidden 256 at width 92, hidden 64 at width 260): the case's value nets in both members of a bank,
    its 49 rows dealt over the two lists; within the case's own tau for value heads."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.critics import critic_values
    c = fc.critic_case(name)
    v = c["variants"]["plain"]
    pol = _policy(c["pclass"], c["fuse"], c["width"], c["hidden"])
    _load(pol, v["nets"])
    sd = _state_of(pol.model)
    bank = PolicyBank(pol, [sd, sd], values=True)
    bank.sync_mirror()
    obs = _dev(c["obs"])
    rows = np.zeros((2, 32), np.int64)
    rows[0, :17], rows[1, :32] = np.arange(17), np.arange(17, fc.ROWS)
    out = _poison(fc.ROWS, 3)
    bank.value_seats(_lists(rows, (17, 32), fc.ROWS, 2), obs, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().T          # [heads][rows]
    ratio = _ratio(got, v["x64"]["values"], v["tau"]["values"])
    print("%s: value pass err / tau %.3f (tau %.3g)" % (name, ratio, v["tau"]["values"]))
    assert np.isfinite(got).all() and v["tau"]["values"] <= 4.0 * fc.DEV_CAP["values"] and ratio <= 1.0
    one = critic_values(bank, obs, 1)
    assert np.array_equal(_u32(one), _u32(out))


def _run_stream(s, bins, count_truncated):
    from copo_amd.eval.critics import AuditFold, CriticAudit
    audit = CriticAudit(cc.GAMMAS, cc.RANGES, bins, count_truncated)
    fold = AuditFold(cc.E, cc.N, cc.K, cc.G, audit, "cuda")
    try:
        dev = {k: _dev(v) for k, v in s.items()}
        for t in range(cc.T):
            fold.record(dev["flags"][t], dev["values"][t], dev["rew"][t], dev["nei_rew"][t], dev["glob_rew"][t], dev["seat"], dev["group"])
        first = fold.words().cpu().numpy()
        fold.reset()
        assert not fold.words().cpu().numpy().any()
        return first
    finally:
        fold.close()


def _check_words(got, want_sums, want_words):
    """Count words exact; every quantised word within `agents` quanta of the model's cell: one rounding per finished agent."""
    assert got.shape == want_words.shape
    for w in cn.COUNT_WORDS:
        assert np.array_equal(got[..., w], want_words[..., w]), w
    slack = want_words[..., cn.AGENTS][..., None]
    assert (np.abs(got - want_words) <= slack).all(), np.abs(got - want_words).max()
    assert (np.abs(got / cn.Q - want_sums) <= (slack + 1) / cn.Q)[..., cn.SUM_V:cn.BIN_COUNT].all()


@pytest.mark.parametrize("bins,count_truncated", cc.CONFIGS)
def test_audit_record_on_the_crafted_streams(bins, count_truncated):
    s = cc.stream()
    got = _run_stream(s, bins, count_truncated)
    sums, words = cn.forward_fold(s, cc.GAMMAS, cc.RANGES, bins, count_truncated, cc.K, cc.G)
    assert words[..., cn.AGENTS].sum() >= 30 and words[..., cn.TRUNCATED].sum() >= 3
    _check_words(got, sums, words)
    print("bins %d count_truncated %s: largest |word - model| %d quanta over %d agents" % (bins, count_truncated, np.abs(got - words).max(),
                                                                                           words[..., cn.AGENTS].sum() // len(cc.GAMMAS)))
    assert np.array_equal(_run_stream(cc.permuted(s), bins, count_truncated), got)          # another slot order: identical accumulators


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
SMP_T, SMP_FRAGMENTS, SMP_HORIZON = 20, 2, 12


@pytest.fixture(scope="module")
def session():
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    from copo_amd.eval.evaluate import make_eval_trainer
    plan = SeatPlan.pairs(2, 1, 8, 0.5)          # 4 scenes x 8 slots
    t = make_eval_trainer("copo", "inter", plan.E, plan.N, 0, env_config=dict(horizon=SMP_HORIZON))
    members = _members(t.policy.model, 2, 0.05)
    yield t, plan, members, PolicyBank(t.policy, members, values=True)
    t.stop()


def _fixed_noise(smp, noise):
    state = dict(f=0)

    def draw():
        smp.eps.copy_(noise[state["f"]])
        state["f"] += 1
    smp._draw_noise = draw


def _drive(smp, noise, keys):
    _fixed_noise(smp, noise)
    smp.reset()
    keep = []
    for _ in range(len(noise)):
        b = smp.sample()
        torch.cuda.synchronize()
        keep.append({k: b[k].clone() for k in keys})
    return keep


def test_sampler_drives_as_a_plain_one_and_folds_what_the_model_folds(session):
    from copo_amd.eval.critics import CriticAudit, CriticSeatSampler
    from copo_amd.eval.crossplay import SeatSampler
    t, plan, members, bank = session
    audit = CriticAudit(t.policy.gae_gammas(), (-1.0, 1.0), bins=4, count_truncated=True)
    assert audit.gammas == (0.99, 0.99, 1.0)
    g = torch.Generator(device="cuda").manual_seed(11)
    noise = [torch.randn(SMP_T, plan.E, plan.N, 2, device="cuda", generator=g) for _ in range(SMP_FRAGMENTS)]
    drive = ("actions", "flags", "rewards", "obs")
    plain = SeatSampler(t.env, t.policy, bank, plan, SMP_T, use_graph=False)
    ref = _drive(plain, noise, drive)
    eager = CriticSeatSampler(t.env, t.policy, bank, plan, audit, SMP_T, use_graph=False)
    got = _drive(eager, noise, drive + ("critic_values", "nei_rewards", "global_rewards"))
    for f in range(SMP_FRAGMENTS):
        for k in drive:
            a, b = ref[f][k], got[f][k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (f, k)
    assert torch.equal(plain.tally, eager.tally) and int(eager.tally[..., 1].sum()) >= 8
    words = eager.audit_words().cpu().numpy()
    # the numpy model fed with the sampler's own record
    cat = lambda k: np.concatenate([got[f][k].cpu().numpy() for f in range(SMP_FRAGMENTS)])  # noqa: E731
    s = dict(flags=cat("flags"), values=cat("critic_values"), rew=cat("rewards"), nei_rew=cat("nei_rewards"), glob_rew=cat("global_rewards")[:, :, 0],
             seat=plan.seat, group=plan.group)
    sums, want = cn.forward_fold(s, audit.gammas, audit.value_range, audit.bins, True, plan.K, plan.n_groups)
    assert want[..., cn.AGENTS].sum() >= 3 * 8 and want[..., cn.TRUNCATED].sum() >= 3
    _check_words(words, sums, want)
    assert not words[0, 1].any() and not words[3, 0].any()          # member 1 has no seat in group (0, 0), member 0 none in (1, 1)
    # one captured graph: the eager run has warmed every launch, so the first fragment is captured and both are replays
    graphed = CriticSeatSampler(t.env, t.policy, bank, plan, audit, SMP_T, use_graph=True)
    graphed._loop.warmup = 0
    again = _drive(graphed, noise, ("actions", "flags", "critic_values"))
    assert graphed._loop.graph is not None
    for f in range(SMP_FRAGMENTS):
        for k in ("actions", "flags", "critic_values"):
            a, b = got[f][k], again[f][k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (f, k)
    assert np.array_equal(graphed.audit_words().cpu().numpy(), words) and torch.equal(graphed.tally, eager.tally)
    eager.clear_tally()
    assert not eager.audit_words().cpu().numpy().any()
    for smp in (eager, graphed):
        smp.fold.close()


def test_refusals_on_the_device(session):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.critics import CriticAudit, CriticSeatSampler
    t, plan, members, bank = session
    with pytest.raises(ValueError, match="no value nets"):
        CriticSeatSampler(t.env, t.policy, PolicyBank(t.policy, members), plan, CriticAudit([0.99, 0.99, 1.0]), 4, use_graph=False)
    with pytest.raises(ValueError, match="3 value heads"):
        CriticSeatSampler(t.env, t.policy, bank, plan, CriticAudit([0.99]), 4, use_graph=False)
    with pytest.raises(ValueError, match="without value nets"):
        PolicyBank(t.policy, members).value_seats(None, None, None)
    mf = _policy("ccppo", "mf", 91, 64)
    with pytest.raises(ValueError, match="centralised critic"):
        CriticSeatSampler(SimpleNamespace(sim=SimpleNamespace(O=91)), mf, PolicyBank(mf, [_state_of(mf.model)], values=True), plan, CriticAudit([0.99]), 4)


def test_a_shifted_critic_shows_in_the_table(session):
    """Member 1 is member 0 with the last bias of its ego value net shifted by +1, on the same scenes under the same noise: the two drive
    alike, so `bias` of the ego head is 1 higher to 1e-3 and `rmse` rises with it (its square by 2 bias + 1).  `explained_variance` = 1 - Var(G - V) / Var(G) does
    not see a constant shift (a variance does not), so there the two agree to rounding: the table tells them apart by `bias`."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.critics import CriticAudit, CriticSeatSampler, audit_plan, critic_frame
    from copo_amd.eval.evaluate import make_eval_trainer
    t0, _plan, members, _bank = session
    shifted = dict(members[0])
    shifted["_value_branch._model.0.bias"] = members[0]["_value_branch._model.0.bias"] + np.float32(1.0)
    plan = audit_plan(2, 2, 8)
    assert plan.E == 4 and plan.replica_scenes == 2
    audit = CriticAudit(t0.policy.gae_gammas(), (-2.0, 3.0), bins=5, count_truncated=True)
    g = torch.Generator(device="cuda").manual_seed(12)
    noise = []
    for _ in range(SMP_FRAGMENTS):
        half = torch.randn(SMP_T, 2, plan.N, 2, device="cuda", generator=g)
        noise.append(torch.cat([half, half], dim=1))          # both members' scenes under one draw
    smp = CriticSeatSampler(t0.env, t0.policy, PolicyBank(t0.policy, [members[0], shifted], values=True), plan, audit, SMP_T, use_graph=False)
    _drive(smp, noise, ("flags",))
    words = smp.audit_words().cpu().numpy()
    smp.fold.close()
    df = critic_frame(words, plan, audit, ["base", "shifted"])
    ego = df[df["head"] == 0].set_index("label")
    print(ego[["agents", "steps", "bias", "rmse", "explained_variance", "mean_value", "mean_return"]].to_string())
    assert ego.loc["base", "steps"] == ego.loc["shifted", "steps"] >= 100 and ego.loc["base", "sum_g_q16"] == ego.loc["shifted", "sum_g_q16"]
    assert abs(ego.loc["shifted", "bias"] - ego.loc["base", "bias"] - 1.0) <= 1e-3
    assert abs(ego.loc["shifted", "explained_variance"] - ego.loc["base", "explained_variance"]) <= 1e-3 * max(1.0, abs(ego.loc["base", "explained_variance"]))
    # with d = V - G of the base critic, rmse^2 = Var(d) + bias^2: the shift moves the bias from b to b + 1, so the squared rmse moves by
    # exactly 2 b + 1 (quantisation: 2^-16 per agent, far below the 1e-3 allowed here)
    b = ego.loc["base", "bias"]
    assert abs(ego.loc["shifted", "rmse"] ** 2 - ego.loc["base", "rmse"] ** 2 - (2.0 * b + 1.0)) <= 1e-3
    assert ego.loc["shifted", "rmse"] > ego.loc["base", "rmse"] + 0.5          # (holds while the base critic's bias is above -0.25 or so: printed)
    other = df[df["head"] == 1].set_index("label")          # the heads that were not touched agree in every word
    assert other.loc["base", "sum_v_q16"] == other.loc["shifted", "sum_v_q16"]
