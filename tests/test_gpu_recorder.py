"""Device evaluation recorder on the GPU (copo_recorder_*, copo_amd/eval/device_recorder.py) against the restatement of its rules
(tests/recorder_numpy.py), against the reference's own numbers (tests/golden/recorder.npz) and, end to end, against `VecRecorder`.

Bounds.  The restatement sums over slots in the device's order, both divide in IEEE float64, so counts, `env_episode_steps`, scene,
episode index and every minimum / maximum of inputs and of step means are compared exactly.  The summed and derived columns are held
to rtol = atol = 1e-9 (float64 re-association over at most 70 slots x 200 steps of magnitudes at most 1e3 is below 1e-10).  The minimum
and maximum of the SVO estimate select exactly but are values of atan2, which the device's and numpy's maths libraries each round within
2 units in the last place, and of one more product: they are held to 8 units in the last place (exact where the clamp to [0, 90] acts)."""
import numpy as np
import pytest

import recorder_cases as rc
import recorder_numpy as rn

pytestmark = pytest.mark.gpu

ULP_COLUMNS = ("svo_estimate_deg_min", "svo_estimate_deg_max")


def _device(fragments, E, N, **kwargs):
    """(rows float64 [n, NCOL], (stored, dropped), episodes int64 [E]) of a DeviceRecorder that has consumed the fragments"""
    from copo_amd.eval.device_recorder import DeviceRecorder
    rec = DeviceRecorder(E, N, "cuda:0", **kwargs)
    try:
        for b in fragments:
            _add(rec, b)
        return rec.rows().cpu().numpy(), rec.count(), rec.episodes().cpu().numpy()
    finally:
        rec.close()


def _add(rec, b):
    import torch
    rec.add({k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()})


def _compare(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, -2:], want[:, -2:]), (got[:, -2:], want[:, -2:])
    for k, col in enumerate(rn.COLUMNS):
        if col in ULP_COLUMNS:
            assert (np.abs(got[:, k] - want[:, k]) <= 8 * np.spacing(np.abs(want[:, k]))).all(), (col, got[:, k], want[:, k])
        elif col in rn.EXACT:
            assert np.array_equal(got[:, k], want[:, k]), (col, got[:, k], want[:, k])
        else:
            np.testing.assert_allclose(got[:, k], want[:, k], rtol=1e-9, atol=1e-9, err_msg=col)


def _both(fragments, E, N, **kwargs):
    got, count, episodes = _device(fragments, E, N, **kwargs)
    ref = rc.restate(fragments, E, N, **kwargs)
    _compare(got, ref.rows)
    assert count == (len(ref.rows), ref.dropped) and np.array_equal(episodes, ref.episodes)
    return got, ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return rc.golden_cases(golden_dir)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_golden_episodes(golden, c):
    """E = 1, N = 6 / 9 / 12: the reference's scripted episodes as they are, against the restatement and against the reference's values."""
    stream, ref = golden[c]
    T, _, N = stream["flags"].shape
    assert N == (6, 9, 12)[c]
    got, _ = _both([stream], 1, N)
    row = dict(zip(rn.COLUMNS, got[0]))
    assert len(got) == 1 and row["env_episode_steps"] == T
    for col in rn.COLUMNS[:24] + rc.SVO:
        np.testing.assert_allclose(row[col], ref[col], rtol=2e-6, atol=2e-6, err_msg=col)


# five scenes: two episodes inside one fragment of 8 (scene 1), an episode that ends at step 0 with nobody terminated (scene 2), scenes
# that finish at different steps, one that never finishes (scene 4)
RESETS = {0: [13, 30], 1: [17, 22], 2: [0, 26], 3: [39]}


@pytest.fixture(scope="module")
def stream():
    return rc.scripted(5, 40, 40, RESETS, seed=1, lonely=((3, 7),))


def test_fragments_do_not_change_the_rows(stream):
    """E = 5, N = 40, T = 40 as one fragment and as five of 8: bit-identical rows, in the order of their fragments.  The stream holds
    every kind of row."""
    f = stream["flags"]
    reset_step = ((f & rn.F_ENV_RESET) > 0).any(-1, keepdims=True)
    assert ((f & (rn.F_DONE | rn.F_SPAWNED)) == (rn.F_DONE | rn.F_SPAWNED)).any()                    # a row with F_DONE | F_SPAWNED
    assert (((f & (rn.F_ACTED | rn.F_SPAWNED)) == rn.F_SPAWNED) & reset_step).any()                 # spawned-only, resetting step
    assert (((f & (rn.F_ACTED | rn.F_SPAWNED)) == rn.F_SPAWNED) & ~reset_step).any()                # spawned-only, ordinary step
    whole, ref = _both([stream], 5, 40)
    parts, _ = _both(rc.cut(stream, 8), 5, 40)
    assert parts[:, -2].tolist() == [0, 1, 1, 0, 2, 3]                       # (fragment, scene, step) order
    assert whole.tobytes() == parts[np.lexsort((parts[:, -1], parts[:, -2]))].tobytes()
    assert whole[:, -2].tolist() == [0, 0, 1, 1, 2, 3] and whole[:, -1].tolist() == [0, 1, 0, 1, 1, 0]
    assert ref.episodes.tolist() == [2, 2, 2, 1, 0]


@pytest.mark.parametrize("N", [70, 130])
def test_more_slots_than_lanes(N):
    """Lanes stride over the slots: two and three slots per lane (the kernel's instances for N <= 128 and above)."""
    s = rc.scripted(3, N, 24, {0: [11], 1: [5, 23], 2: [16]}, seed=N)
    _both(rc.cut(s, 12), 3, N)


def test_an_agent_without_neighbours_has_an_svo_of_45_degrees():
    """nbr_cnt = 0 throughout: the neighbourhood reward falls back to the agent's own, positive here, so atan2 sees equal arguments."""
    s = rc.scripted(1, 3, 30, {0: [29]}, seed=5, lonely=((0, 0), (0, 1), (0, 2)))
    assert (s["nbr_cnt"] == 0).all() and (s["nei_rewards"] == 0).all()
    got, _ = _both([s], 1, 3)
    row = dict(zip(rn.COLUMNS, got[0]))
    assert row["num_agents_total"] >= 3
    for col in rc.SVO[:3]:
        assert abs(row[col] - 45.0) < 1e-12, (col, row[col])
    assert row["svo_reward"] > 0


def test_limit_ignores_the_steps_after_a_scenes_last_episode(stream):
    got, ref = _both(rc.cut(stream, 8), 5, 40, limit=1)
    assert got[:, -2].tolist() == [0, 1, 3] and ref.episodes.tolist() == [1, 1, 1, 1, 0]      # scene 2: its first episode left no row
    assert got[:, 24].tolist() == [14, 18, 40]


def test_overflow_drops_the_later_rows_in_fragment_scene_step_order(stream):
    """max_rows = 2, five episodes with a row in three scenes: what is stored depends on the fragments, by (fragment, scene, step)."""
    s = {k: v[:, :3] for k, v in stream.items()}
    whole, ref = _both([s], 3, 40, max_rows=2)
    assert ref.dropped == 3 and list(zip(whole[:, -2], whole[:, -1])) == [(0, 0), (0, 1)]
    parts, ref = _both(rc.cut(s, 8), 3, 40, max_rows=2)
    assert ref.dropped == 3 and list(zip(parts[:, -2], parts[:, -1])) == [(0, 0), (1, 0)]


def test_clear_keeps_the_open_state_and_reset_forgets_it(stream):
    from copo_amd.eval.device_recorder import DeviceRecorder
    frags = rc.cut(stream, 8)
    rec, ref = DeviceRecorder(5, 40, "cuda:0", max_rows=16), rn.RecorderNumpy(5, 40, max_rows=16)
    try:
        for b in frags[:3]:
            _add(rec, b)
            ref.add(*(b[k] for k in rc.KEYS))
        assert rec.count() == (len(ref.rows), 0) and len(ref.rows) == 3
        rec.clear()
        ref.clear()
        assert rec.count() == (0, 0) and np.array_equal(rec.episodes().cpu().numpy(), ref.episodes)
        for b in frags[3:]:
            _add(rec, b)
            ref.add(*(b[k] for k in rc.KEYS))
        _compare(rec.rows().cpu().numpy(), ref.rows)             # (the episodes that were open over the clear, with their first steps)
        assert len(ref.rows) == 3
        _add(rec, frags[0])                                      # something open again
        rec.reset()
        assert rec.count() == (0, 0) and not rec.episodes().any()
        for b in frags:
            _add(rec, b)
        _compare(rec.rows().cpu().numpy(), rc.restate(frags, 5, 40).rows)
        means = rec.means()
        frame = rec.frame()
        assert list(frame.columns) == list(rn.COLUMNS) + ["scene"] and frame["scene"].tolist() == [0, 1, 1, 0, 2, 3]
        assert means["num_agents_total"] == pytest.approx(frame["num_agents_total"].mean())
    finally:
        rec.close()


def test_add_rejects_what_it_cannot_read(stream):
    import torch
    from copo_amd._capi import CopoError
    from copo_amd.eval.device_recorder import DeviceRecorder
    with pytest.raises(CopoError, match="max_rows=0"):
        DeviceRecorder(5, 40, "cuda:0", max_rows=0)
    rec = DeviceRecorder(5, 40, "cuda:0")
    try:
        b = {k: torch.from_numpy(v).cuda() for k, v in rc.cut(stream, 8)[0].items()}
        with pytest.raises(ValueError, match="nbr_cnt"):
            rec.add(dict(b, nbr_cnt=b["nbr_cnt"].to(torch.int64)))
        with pytest.raises(ValueError, match="infos"):
            rec.add(dict(b, infos=b["infos"][..., :4]))
        with pytest.raises(ValueError, match="flags"):
            rec.add(dict(b, flags=b["flags"].cpu()))
        assert rec.count() == (0, 0)
    finally:
        rec.close()
    rec.close()


def test_end_to_end_next_to_the_vectorised_recorder():
    """Intersection, 4 scenes x 8 agents, a short horizon: every sampled fragment goes to a `VecRecorder` and to a `DeviceRecorder`
    until every scene has finished one episode."""
    import torch
    from copo_amd.eval.device_recorder import DeviceRecorder
    from copo_amd.eval.evaluate import make_eval_trainer
    from copo_amd.eval.vec_recorder import COLUMNS, F_ENV_RESET, VecRecorder
    t = make_eval_trainer("ippo", "inter", num_envs=4, num_agents=8, env_config=dict(horizon=40, neighbours_distance=20.0))
    smp = t.sampler
    vec, dev = VecRecorder(smp.E, smp.device), DeviceRecorder(smp.E, smp.N, smp.device, max_rows=8, limit=1)
    try:
        ep = torch.zeros(smp.E, dtype=torch.int64, device=smp.device)
        n_frag = 0
        while bool((ep < 1).any()) and n_frag * smp.T <= 12 * 40:
            b = smp.sample()
            ended = ((b["flags"] & F_ENV_RESET) > 0).any(-1).to(torch.int64)
            vec.add(b, keep=(ep[None] + torch.cumsum(ended, 0) - ended) < 1)
            dev.add(b)
            ep = ep + ended.sum(0)
            n_frag += 1
            assert torch.equal(dev.episodes(), ep.clamp(max=1))
        assert bool((ep >= 1).all()), "no scene episode ended in %d fragments of %d steps" % (n_frag, smp.T)
        rows = dev.rows().cpu().numpy()
        assert dev.count() == (len(vec.rows), 0) and len(vec.rows) == smp.E
        for r in vec.rows:
            mine = rows[rows[:, -2] == r["scene"]]
            assert len(mine) == 1 and mine[0, -1] == 0
            np.testing.assert_allclose(mine[0, :25], [r[c] for c in COLUMNS], rtol=1e-9, atol=1e-9)
        mean, lo, hi, reward = rows[:, 25], rows[:, 26], rows[:, 27], rows[:, 28]
        assert np.isfinite(rows).all() and (lo >= 0).all() and (hi <= 90).all() and (lo <= mean).all() and (mean <= hi).all()
        assert np.isfinite(reward).all()
    finally:
        dev.close()
        t.stop()
