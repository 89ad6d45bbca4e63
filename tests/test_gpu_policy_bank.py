"""A bank of K policies in one batch (copo_mlp_forward_bank_f32, copo_sim_set_lcf_table, copo_amd/eval/bank.py, evaluate_bank_rows).

Every comparison here is of bits.  Forward: an output row of the forward kernel is a fixed-order sum over its own inputs and does not
depend on the rows that share its tile, so member k's rows of a bank launch must equal what `FusedLearner.act` writes for member k's
weights on that slice alone.  The two-tile variant (hidden 256, at least 16 384 rows) does NOT round every row as the one-tile variant
does -- with the variant chosen from K x R rows, K = 3 and R = 5512 gave 1 differing row of 16 536 -- so the bank launcher picks the
variant the single launcher picks for R rows: the cases at R = 5512 (K x R above the threshold, R below) and R = 16 392 (both above)
hold it to that.  Simulator: scene e with row e of a table
must equal scene e of a plain simulator given that row through set_lcf_dist; the plain simulator is pinned to the CPU oracle by
test_gpu_sim_parity.py.  End to end: every member of a bank sees the seeds and the noise of a bank of one."""
import numpy as np
import pytest
import torch

import bank_cases as bc

pytestmark = pytest.mark.gpu

from test_gpu_fused_learner import _make  # noqa: E402

CANARY = 0x7FC0BEEF                   # a quiet NaN with a payload: nothing the kernel computes
_POLICIES = {}


def _policy(name, odim, hidden, bf16):
    # (a bfloat16 CoPO policy has no fused learner -- the LCF meta pass has no bfloat16 mode -- so the bfloat16 cases take the policy
    # net of the 92-wide population through an IPPO policy of that width: the policy nets have one shape)
    name = "ippo" if bf16 else name
    key = (name, odim, hidden, bf16)
    if key not in _POLICIES:
        over = dict(policy_dtype="bfloat16") if bf16 else {}
        _POLICIES[key] = _make(name, "none", odim, fused=True, hiddens=(hidden, hidden), **over)
        assert _POLICIES[key].fused is not None
    return _POLICIES[key]


def _outputs(rows):
    f = lambda *s: torch.full(s, CANARY, dtype=torch.int32, device="cuda").view(torch.float32)  # noqa: E731
    return dict(action=f(rows, 2), logp=f(rows), dist_inputs=f(rows, 4), clipped=f(rows, 2))


def _bank_against_single(golden_dir, name, odim, hidden, K, R, bf16):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.checkpoint_io import load_policy_weights
    pol = _policy(name, odim, hidden, bf16)
    ws = bc.members(golden_dir, name + "_inter", odim, hidden, K)
    g = torch.Generator(device="cuda").manual_seed(odim + R)
    obs = torch.rand(K * R, odim, device="cuda", generator=g) * 2 - 1
    eps = torch.randn(K * R, 2, device="cuda", generator=g)
    want = _outputs(K * R)
    for k, w in enumerate(ws):
        load_policy_weights(pol.model, w)
        pol.fused.invalidate_mirror()
        pol.fused.sync_mirror()
        s = slice(k * R, (k + 1) * R)
        pol.fused.act(obs[s], eps[s], want["action"][s], want["logp"][s], want["dist_inputs"][s], want["clipped"][s])
    bank = PolicyBank(pol, ws)
    bank.sync_mirror()
    got = _outputs((K + 1) * R)           # one member longer: the tail must keep the canary
    bank.act(obs, eps, got["action"], got["logp"], got["dist_inputs"], got["clipped"])
    torch.cuda.synchronize()
    for key in want:
        a, b = got[key].view(torch.int32), want[key].view(torch.int32)
        assert not bool((b == CANARY).any()), key
        assert bool((a[K * R:] == CANARY).all()), "%s: written past the last member" % key
        if not torch.equal(a[:K * R], b):
            bad = torch.nonzero((a[:K * R] != b).reshape(K * R, -1).any(1)).reshape(-1)
            raise AssertionError("%s differs in %d rows, first row %d (member %d, row %d of it)" % (
                key, bad.numel(), int(bad[0]), int(bad[0]) // R, int(bad[0]) % R))
    if K > 1:
        assert not torch.equal(want["dist_inputs"][:R], want["dist_inputs"][R:2 * R])       # members really differ


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [40, 200])
@pytest.mark.parametrize("hidden", [256, 64])
@pytest.mark.parametrize("name,odim", [("copo", 92), ("ippo", 91)])
@pytest.mark.parametrize("K", [1, 3])
def test_bank_forward_equals_single_member_forward(golden_dir, K, name, odim, hidden, R, bf16):
    """R = 40 leaves a masked tail in the 16-row tile (and in the 32-row one), and member boundaries at rows 40 and 80 fall inside what
    a flat launch would make one tile; 92 inputs take the 128-bit load path, 91 the scalar one."""
    _bank_against_single(golden_dir, name, odim, hidden, K, R, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,R", [(3, 5512), (2, 16392)])
def test_bank_forward_around_the_two_tile_threshold(golden_dir, K, R, bf16):
    """3 x 5512 rows: 16 536 rows in the launch, but each member has fewer than the 16 384 of the two-tile variant, which a launch of
    one member would not take.  2 x 16 392 rows: both take it; 16 392 = 512 x 32 + 8 leaves a masked tail in every member's last tile."""
    _bank_against_single(golden_dir, "copo", 92, 256, K, R, bf16)


def test_bank_refuses_what_it_cannot_hold(golden_dir):
    from copo_amd.eval.bank import PolicyBank
    pol = _policy("copo", 92, 256, False)
    w = bc.golden_population(golden_dir, "copo_inter")
    before = pol.fused.flat.flat.clone()
    with pytest.raises(ValueError, match="member 1"):
        PolicyBank(pol, [w, bc.golden_population(golden_dir, "ippo_inter")])
    with pytest.raises(ValueError, match="no members"):
        PolicyBank(pol, [])
    assert torch.equal(pol.fused.flat.flat, before)
    bank = PolicyBank(pol, [w, bc.perturbed(w, 1)])
    assert torch.equal(pol.fused.flat.flat, before)              # the model's own weights are put back
    with pytest.raises(ValueError, match="rows"):
        bank.act(torch.zeros(41, 92, device="cuda"), None, None, None, None)


# ---- per-scene LCF distribution ----------------------------------------------------------------------------------------------------
OUT_KEYS = ("obs", "rew", "nei_rew", "glob_rew", "flags", "lcf", "nbr_idx", "nbr_cnt", "mf_cnt", "nbr_dist", "info", "agent_id")


def _snap(out):
    return {k: out[k].clone() for k in OUT_KEYS}


def _same_scene(tag, got, e, want):
    for k in OUT_KEYS:
        a, b = got[k][e], want[k][e]
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), "%s: %s of scene %d differs" % (tag, k, e)


def _sims(block):
    from copo_amd.sim import VecSim
    sims = [VecSim(bc.lcf_config()) for _ in range(4)]
    for s in sims:
        s.set_block(block)
    return sims[0], sims[1:]


def _compare_all(tag, banked_out, plain_outs):
    per = bc.LCF_E // len(plain_outs)
    for e in range(bc.LCF_E):
        _same_scene(tag, banked_out, e, plain_outs[e // per])


@pytest.mark.parametrize("block", [64, 256, -2], ids=["one_wave_per_scene", "several_waves_per_scene", "packed"])
def test_scene_lcf_table_equals_plain_simulators(block):
    """Phase 1: a table of three distributions against three plain simulators of one distribution each.  Phase 2: the table lifted and
    another single distribution set mid-rollout, the same call on the plain ones.  Phase 3: the table back with a forced LCF over
    it, against the forced LCF alone.  Every phase must see spawns in every scene, or it proves nothing.  With several waves per scene
    the draws of a respawn are made ahead of time by another wave than the one that spawns: the third path that reads the table."""
    banked, plain = _sims(block)
    act = torch.from_numpy(bc.lcf_actions()).cuda()
    banked.set_lcf_table(bc.lcf_table())
    for s, (mean, std) in zip(plain, bc.LCF_TABLE_ROWS):
        s.set_lcf_dist(mean, std)
    _compare_all("reset", _snap(banked.reset(bc.lcf_seeds())), [_snap(s.reset(bc.lcf_seeds())) for s in plain])
    spawned = torch.zeros(3, bc.LCF_E, dtype=torch.int64, device="cuda")
    lcf_seen = [[], [], []]
    for t in range(bc.LCF_STEPS + 2 * bc.LCF_PHASE):
        phase = 0 if t < bc.LCF_STEPS else (1 if t < bc.LCF_STEPS + bc.LCF_PHASE else 2)
        if t == bc.LCF_STEPS:
            banked.set_lcf_table(None)
            for s in [banked] + plain:
                s.set_lcf_dist(*bc.LCF_SECOND_DIST)
        if t == bc.LCF_STEPS + bc.LCF_PHASE:
            banked.set_lcf_table(bc.lcf_table())
            for s in [banked] + plain:
                s.set_force_lcf(bc.LCF_FORCED)
        got = _snap(banked.step(act))
        _compare_all("step %d (block %d)" % (t, block), got, [_snap(s.step(act)) for s in plain])
        new = (got["flags"] & 64) != 0
        spawned[phase] += new.sum(-1)
        if phase == 0:
            for grp in range(3):
                lcf_seen[grp].append(got["lcf"][2 * grp:2 * grp + 2][new[2 * grp:2 * grp + 2]])
    spawned = spawned.cpu().numpy()
    assert (spawned[0] >= 20).all() and (spawned[1:] >= 8).all(), spawned
    means = [float(torch.cat(v).mean()) for v in lcf_seen]             # the table was in force: the groups' draws sit around their means
    for m, (mean, std) in zip(means, bc.LCF_TABLE_ROWS):
        assert abs(m - mean) < 4 * std / np.sqrt(40), (means, bc.LCF_TABLE_ROWS)
    for s in [banked] + plain:
        s.close()


def test_captured_step_sees_a_table_set_after_the_capture():
    """The step is captured with no table; a table set later and pushed by `flush` is what the replays draw from."""
    banked, plain = _sims(64)
    act = torch.from_numpy(bc.lcf_actions()).cuda()
    banked.reset(bc.lcf_seeds())
    for s in plain:
        s.reset(bc.lcf_seeds())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(3):
            _compare_all("warm-up %d" % t, _snap(banked.step(act)), [_snap(s.step(act)) for s in plain])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        banked.step(act)
    banked.set_lcf_table(bc.lcf_table())
    banked.flush()
    for s, (mean, std) in zip(plain, bc.LCF_TABLE_ROWS):
        s.set_lcf_dist(mean, std)
    spawned = torch.zeros(bc.LCF_E, dtype=torch.int64, device="cuda")
    for t in range(bc.LCF_STEPS):
        graph.replay()
        got = _snap(banked.out)
        _compare_all("replay %d" % t, got, [_snap(s.step(act)) for s in plain])
        spawned += ((got["flags"] & 64) != 0).sum(-1)
    assert (spawned.cpu().numpy() >= 15).all(), spawned
    assert not torch.equal(got["lcf"][0], got["lcf"][2]) or not torch.equal(got["obs"][0], got["obs"][2])
    for s in [banked] + plain:
        s.close()


def test_table_is_validated_like_the_single_distribution():
    from copo_amd._capi import CopoError
    from copo_amd.sim import VecSim
    sim = VecSim(bc.lcf_config())
    bad = bc.lcf_table()
    bad[3, 1] = 0.0
    with pytest.raises(ValueError, match="scene 3"):
        sim.set_lcf_table(bad)
    rc = sim._capi.lib.copo_sim_set_lcf_table(sim._h, bad.ctypes.data)          # the library's own check
    assert rc == -5 and b"scene 3" in sim._capi.lib.copo_last_error()
    with pytest.raises(CopoError):
        sim._capi.check(rc)
    with pytest.raises(ValueError, match="shape"):
        sim.set_lcf_table(bc.lcf_table()[:4])
    sim.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_bank_rows_equal_the_rows_of_banks_of_one(golden_dir):
    """Three members on 12 scenes against each member alone on 4: the same seeds, the same noise, so the same rows -- all columns but
    `member` / `label`, with `scene` counted within the member."""
    from copo_amd.eval.evaluate import evaluate_bank_rows
    w0 = bc.golden_population(golden_dir, "copo_inter")
    ws = [w0, bc.perturbed(w0, 1, 0.05), bc.perturbed(w0, 2, 0.05)]
    lcfs = [(0.368, 0.088), (0.0, 0.1), (-0.3, 0.05)]
    kw = dict(num_agents=8, scene_episodes=1, seed=3, env_config=dict(horizon=60, delay_done=5))
    df = evaluate_bank_rows("copo", "inter", ws, lcfs=lcfs, num_envs=12, labels=["a", "b", "c"], **kw)
    assert len(df) == 3 * 4 * 1 and list(df["scene"]) == list(range(12))
    assert list(df["member"]) == [s // 4 for s in range(12)] and list(df["label"]) == [("a", "b", "c")[s // 4] for s in range(12)]
    rewards = []
    for k in range(3):
        one = evaluate_bank_rows("copo", "inter", [ws[k]], lcfs=[lcfs[k]], num_envs=4, **kw)
        mine = df[df["member"] == k].drop(columns=["member", "label"]).reset_index(drop=True)
        mine["scene"] -= 4 * k
        one = one.drop(columns=["member", "label"])
        assert list(mine.columns) == list(one.columns)
        for col in one.columns:
            a, b = mine[col].to_numpy(), one[col].to_numpy()
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                         b.view(np.uint64) if b.dtype == np.float64 else b), (k, col, a, b)
        rewards.append(one["episode_reward_mean"].to_numpy())
    assert not np.array_equal(rewards[0], rewards[1]) and not np.array_equal(rewards[0], rewards[2])
