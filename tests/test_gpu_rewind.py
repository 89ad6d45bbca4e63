"""Scene rewind on the GPU (copo_rewind_*, copo_amd/rewind.py) against the numpy restatement of its rules (tests/rewind_numpy.py): the ring
and the fork on hand-set states across two ring wraps, branches that resume their source bit for bit, the LCF override, the tally, no
effect on the source, and the dict env with the clip recorder and the rewind buffer side by side.

Every comparison is exact on raw bits: the feature is copies, integer logic and one fp32 clamp."""
import ctypes as C
import os

import numpy as np
import pytest

import clip_numpy as cn
import rewind_numpy as rn
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _hand_state(E, N, r):
    """distinct bit patterns per (field, scene, slot, record): float fields hold NaN payloads, infinities and negative zero among them"""
    w = (np.arange(16 * E * N, dtype=np.uint32).reshape(16, E, N) * np.uint32(2654435761) + np.uint32(0x01000193 * (r + 1))).astype(np.uint32)
    w[0, :, 0] = 0x7FC00000 + r + 1                      # quiet NaN with a payload
    w[1, :, 0] = 0xFFA00001 + r                          # negative signalling-NaN pattern
    w[2, :, 0] = 0x80000000                              # -0.0
    w[10, :, N - 1] = 0x80000000
    status = (np.arange(E)[:, None] + np.arange(N)[None, :] + r) % 3
    w[13] = (w[13] & np.uint32(0xFFFFFF00)) | status.astype(np.uint32)
    env = np.stack([np.full(E, r), np.full(E, r // 4), np.full(E, 1000 + r), np.ones(E, np.int64)], 1).astype(np.int32)
    return w.view(np.float32), env


@pytest.mark.parametrize("N", [7, 64])
def test_ring_and_fork_against_the_restatement(N):
    """E = 5 (the second workgroup of the record launch is ragged), depth 3, stride 2, 11 records: the ring wraps twice.  After every
    record every (scene, rec in -1..12) is forked into scenes 2.. of a target of 8."""
    import torch
    from copo_amd.rewind import RewindBuffer
    from copo_amd.sim import VecSim
    E, TE, FIRST = 5, 8, 2
    kw = dict(map="intersection", map_kwargs=dict(exit_length=80.0)) if N > 30 else dict(map="intersection")
    src, tgt = VecSim(SimConfig(num_envs=E, num_agents=N, **kw)), VecSim(SimConfig(num_envs=TE, num_agents=N, **kw))
    buf = RewindBuffer(src, depth=3, stride=2)
    ring = rn.RewindRing(E, N, 3, 2)
    try:
        src.reset()
        tgt.reset()
        assert buf.span() is None and buf.n_records == 0
        recs = list(range(-1, 13))
        for r in range(11):
            st, env = _hand_state(E, N, r)
            _set_state(src, st, env)
            buf.record()
            ring.record(st, env)
            assert buf.n_records == r + 1 and buf.span() == ring.span()
            for e in range(E):
                base_st, base_env = _hand_state(TE, N, 100 + r * E + e)      # what the target holds before the fork
                _set_state(tgt, base_st, base_env)
                for lo in range(0, len(recs), TE - FIRST):
                    part = recs[lo:lo + TE - FIRST]
                    watch = [(e + k + r) % (N + 2) - 1 for k in range(len(part))]      # -1 and N among them
                    status, aid = buf.fork(tgt, [e] * len(part), part, watch_slots=watch, first=FIRST)
                    want_st, want_env = base_st.copy(), base_env.copy()
                    want_status, want_aid = ring.fork(want_st, want_env, FIRST, [e] * len(part), part, watch_slots=watch)
                    got_st, got_env = _np_state(tgt)
                    assert np.array_equal(status.cpu().numpy(), want_status) and np.array_equal(aid.cpu().numpy(), want_aid), (r, e, part)
                    assert np.array_equal(got_st.view(np.uint32), want_st.view(np.uint32)), (r, e, part)
                    assert np.array_equal(got_env, want_env), (r, e, part)
                    base_st, base_env = want_st, want_env
            st_after, env_after = _np_state(src)                           # the source is only read
            assert np.array_equal(st_after.view(np.uint32), st.view(np.uint32)) and np.array_equal(env_after, env)
        assert ring.span() == (6, 10)
        # a scene index outside the source is refused on the device; copies fill consecutive scenes
        status = buf.fork(tgt, [E, -1, 2], [10, 10, 9], copies=2, first=1)
        assert status.cpu().numpy().tolist() == [-1, -1, -1, -1, 8, 8]
        got_st, got_env = _np_state(tgt)
        assert np.array_equal(got_st.view(np.uint32)[:, 5], _hand_state(E, N, 8)[0].view(np.uint32)[:, 2])
        assert np.array_equal(got_st.view(np.uint32)[:, 6], got_st.view(np.uint32)[:, 5]) and got_env[1].tolist() == [0, 0, 0, 1]
        buf.reset()
        assert buf.span() is None and buf.fork(tgt, [0], [0]).cpu().numpy().tolist() == [-1]
    finally:
        buf.close()
        src.close()
        tgt.close()


RESUME_CASES = dict(intersection=dict(map="intersection", num_envs=3, num_agents=8, horizon=30, delay_done=3),
                    tollgate=dict(map="tollgate", num_envs=2, num_agents=10, horizon=30, delay_done=3),
                    intersection_packed=dict(map="intersection", num_envs=3, num_agents=8, horizon=30, delay_done=3))
KEYS = ("obs", "rew", "nei_rew", "glob_rew", "flags", "nbr_idx", "nbr_cnt", "mf_cnt", "lcf", "agent_id")


def _same_outputs(got, want, scene_got, scene_want, tag):
    """one scene of two step outputs, masked as the simulator writes them: obs / lcf rows where ACTED or SPAWNED, neighbour rows
    where ACTED"""
    f = want["flags"][scene_want]
    assert np.array_equal(got["flags"][scene_got], f), tag
    present = (f & 0x41) != 0
    before = ((f & 0x01) != 0) | (((f & 0x40) != 0) & ((f & 0x80) == 0))      # the lists are those of the scene before a horizon reset
    for k in KEYS:
        g, w = _bits(got[k])[scene_got], _bits(want[k])[scene_want]
        if k in ("obs", "lcf", "agent_id"):
            g, w = g[present], w[present]
        elif k == "nbr_idx":
            g, w = g[before], w[before]
        assert np.array_equal(g, w), (tag, k)


@pytest.mark.parametrize("name", sorted(RESUME_CASES))
def test_a_branch_resumes_the_source_bit_for_bit(name):
    """stride 3, depth 4, 110 steps of random actions.  After step 60 (the ring holds records 51 .. 60) every scene is forked at an old
    record (52 -> stored record 51, the oldest) and at a recent one (60) into a `Branches` of another size, 2 E scenes x 2 copies + 1
    spare; the source goes on, then the branches replay the recorded actions and must give the source's outputs of the steps from their
    record on.  The two copies of a fork give the same outputs under that mask and hold the same state, every bit of it, after every
    step.  `_packed`: the source runs in the packed launch shape, the target in the default one."""
    import torch
    from copo_amd.rewind import Branches, RewindBuffer
    from copo_amd.sim import VecSim
    cfg = SimConfig(**RESUME_CASES[name])
    E, N = cfg.num_envs, cfg.num_agents
    src = VecSim(cfg)
    if name.endswith("_packed"):
        src.set_block(-4)
    buf = RewindBuffer(src, depth=4, stride=3)
    br = Branches(buf, 4 * E + 1)
    rng = np.random.RandomState(23)
    FORK_AT, STEPS, OLD = 60, 110, 51
    acts = [rn.random_actions(rng, E, N) for _ in range(STEPS)]
    outs = {}
    try:
        src.reset()
        buf.record()
        for t in range(STEPS):                                             # step t leads from record t to record t + 1
            out = src.step(torch.from_numpy(acts[t]).cuda())
            buf.record()
            if t >= OLD:
                outs[t] = {k: out[k].cpu().numpy() for k in KEYS}
            if t + 1 == FORK_AT:
                assert buf.span() == (OLD, FORK_AT)
                spare = [x.clone() for x in br.sim.get_state()]
                status = br.fork(list(range(E)) * 2, [OLD + 1] * E + [FORK_AT] * E, copies=2)
                assert status.cpu().numpy().tolist() == [OLD] * (2 * E) + [FORK_AT] * (2 * E)
                for x, y in zip(spare, br.sim.get_state()):                # the spare scene (the last) is untouched
                    assert torch.equal(x[..., -1, :].view(torch.int32), y[..., -1, :].view(torch.int32))
        seen = {OLD: 0, FORK_AT: 0}
        respawn = {OLD: False, FORK_AT: False}
        for k in range(STEPS - OLD):
            act = np.zeros((br.B, N, 2), np.float32)
            for j in range(2 * E):                                         # branches 0 .. 2E-1 start at record 51, 2E .. 4E-1 at record 60
                act[j] = acts[OLD + k][j // 2]
                if FORK_AT + k < STEPS:
                    act[2 * E + j] = acts[FORK_AT + k][j // 2]
            got = br.step(torch.from_numpy(act).cuda())
            got = {key: got[key].cpu().numpy() for key in KEYS}
            for start, base in ((OLD, 0), (FORK_AT, 2 * E)):
                if start + k >= STEPS:
                    continue
                want = outs[start + k]
                for j in range(2 * E):
                    _same_outputs(got, want, base + j, j // 2, (name, start, k, j))
                seen[start] |= int(np.bitwise_or.reduce(want["flags"].reshape(-1)))
                respawn[start] |= bool((((want["flags"] & 0x40) != 0) & ((want["flags"] & 0x80) == 0)).any())
                for j in range(0, 2 * E, 2):                               # the two copies equal each other: the outputs under the
                    _same_outputs(got, got, base + j + 1, base + j, (name, start, k, j, "copies"))      # same mask (the other rows
            st, env = _np_state(br.sim)                                    # are left from the target's own reset), the state whole
            for j in range(0, 4 * E, 2):
                assert np.array_equal(st.view(np.uint32)[:, j], st.view(np.uint32)[:, j + 1]) and np.array_equal(env[j], env[j + 1]), (name, k, j)
        print(name, "flags seen", {k: hex(v) for k, v in seen.items()}, "respawn inside an episode", respawn)
        assert all(v & 0x80 for v in seen.values()) and all(respawn.values())      # both windows span a scene reset and a respawn
        assert (br.outcomes()["steps"] == STEPS - OLD).all()
    finally:
        br.close()
        buf.close()
        src.close()


def test_lcf_override():
    import torch
    from copo_amd.rewind import Branches, RewindBuffer
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="intersection", num_envs=2, num_agents=10, horizon=40, delay_done=3, respawn_cooldown=8)
    src = VecSim(cfg)
    buf = RewindBuffer(src, depth=2, stride=1)
    br = Branches(buf, 8)
    rng = np.random.RandomState(5)
    try:
        src.reset()
        for t in range(23):                                                # (after 23 steps slots of every status exist, asserted below)
            src.step(torch.from_numpy(rn.random_actions(rng, 2, 10)).cuda())
        buf.record()
        st, env = _np_state(src)
        status_byte = st.view(np.uint32)[13] & 0xFF
        assert {0, 1, 2} <= set(status_byte.reshape(-1).tolist()), "the state must hold EMPTY, ALIVE and WRECK slots"
        lcf = [np.nan, 3.0, -0.25, -7.0]
        br.fork([0, 1], [0, 0], copies=4, lcf=lcf * 2)
        got, got_env = _np_state(br.sim)
        want, want_env = got.copy(), got_env.copy()
        ring = rn.RewindRing(2, 10, 2, 1)
        ring.record(st, env)
        ring.fork(want, want_env, 0, [0, 1], [0, 0], copies=4, lcf=lcf * 2)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_env, want_env)
        for j, (e, v) in enumerate([(0, x) for x in lcf] + [(1, x) for x in lcf]):
            alive = status_byte[e] == rn.ST_ALIVE
            same = np.ones(16, bool)
            same[10] = False
            assert np.array_equal(got.view(np.uint32)[same][:, j], st.view(np.uint32)[same][:, e])
            assert np.array_equal(got.view(np.uint32)[10, j][~alive], st.view(np.uint32)[10, e][~alive])       # EMPTY / WRECK: bit-unchanged
            if np.isnan(v):
                assert np.array_equal(got.view(np.uint32)[10, j], st.view(np.uint32)[10, e])
            else:
                assert (got[10, j][alive] == np.float32(min(max(v, -1.0), 1.0))).all() and alive.any()
        # the lcf observation column of the agents that go on driving follows
        act = torch.zeros(8, 10, 2, device="cuda")
        out = br.step(act)
        flags, obs = out["flags"].cpu().numpy(), out["obs"].cpu().numpy()
        col = cfg.lcf_col
        checked = 0
        for j, (e, v) in enumerate([(0, x) for x in lcf] + [(1, x) for x in lcf]):
            goes_on = (status_byte[e] == rn.ST_ALIVE) & ((flags[j] & 0x01) != 0) & ((flags[j] & 0x02) == 0)
            src_lcf = st[10, e]
            want_col = ((src_lcf if np.isnan(v) else np.float32(min(max(v, -1.0), 1.0))) + np.float32(1.0)) * np.float32(0.5)
            assert np.array_equal(obs[j, goes_on, col], np.broadcast_to(want_col, (10,))[goes_on].astype(np.float32)), (j, v)
            checked += int(goes_on.sum())
        assert checked >= 8
    finally:
        br.close()
        buf.close()
        src.close()


def test_tally_on_the_device():
    import torch
    from copo_amd import rewind
    from copo_amd.sim import VecSim
    steps, watch, want = rn.hand_tally_case()
    rows = torch.from_numpy(rn.tally_init(3)).cuda()
    for f in steps:
        rewind.tally(torch.from_numpy(f).cuda(), torch.from_numpy(watch).cuda(), rows)
    assert np.array_equal(rows.cpu().numpy(), want), rows.cpu().numpy().tolist()
    rows = torch.from_numpy(rn.tally_init(3)).cuda()
    for f in steps:
        rewind.tally(torch.from_numpy(f).cuda(), None, rows)
    assert np.array_equal(rows.cpu().numpy()[:, :6], want[:, :6]) and rows.cpu().numpy()[:, 6:].tolist() == [[0, -1]] * 3
    # a 60-step branch rollout: 6 scenes x 64 slots (a full wave; two workgroups, the second ragged), watched slots of every kind
    cfg = SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=2, num_agents=64, horizon=25, delay_done=2)
    src = VecSim(cfg)
    buf = rewind.RewindBuffer(src, depth=1, stride=1)
    br = rewind.Branches(buf, 6)
    rng = np.random.RandomState(9)
    try:
        src.reset()
        buf.record()
        watch = [0, 63, 17, -1, 64, 5]
        status, aid = br.fork([0, 1], [0, 0], copies=3, watch_slots=watch)
        assert status.cpu().numpy().tolist() == [0] * 6 and br.watch_slots.cpu().numpy().tolist() == watch
        want = rn.tally_init(6)
        for t in range(60):
            out = br.step(torch.from_numpy(rn.random_actions(rng, 6, 64)).cuda())
            rn.tally(out["flags"].cpu().numpy(), watch, want)
        got = br.tally.cpu().numpy()
        print(got.tolist())
        assert np.array_equal(got, want)
        assert (want[:, rn.T_CRASH] > 0).any() and (want[:, rn.T_MAXSTEP] > 0).any() and (want[[0, 1, 2, 5], rn.T_WATCH_STEP] >= 0).all()
        o = br.outcomes()
        assert list(o) == list(rewind.TALLY_KEYS) and np.array_equal(o["crash"], want[:, rn.T_CRASH]) and o["watch_step"][3] == -1
        br.fork([0], [0], first=2)                                          # the rows of the written scenes start over, the others stay
        got2 = br.tally.cpu().numpy()
        assert got2[2].tolist() == list(rn.TALLY_INIT) and np.array_equal(np.delete(got2, 2, 0), np.delete(want, 2, 0))
        assert br.watch_slots.cpu().numpy().tolist() == [0, 63, -1, -1, 64, 5]
    finally:
        br.close()
        buf.close()
        src.close()


def _throttles(obs):
    """straight ahead, a throttle of its own per agent: followers run into slower leaders"""
    return {k: np.array([0.0, 0.3 + 0.07 * ((int(k[5:]) * 7) % 10)]) for k in obs}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    return a == b or (a != a and b != b)


def test_nothing_touches_the_source_and_refusals_launch_nothing():
    import torch
    from copo_amd import _capi
    from copo_amd.rewind import Branches, RewindBuffer
    from copo_amd.sim import VecSim
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    lib, st = _capi.lib, _capi.current_stream()
    # the env key changes nothing
    base = dict(num_agents=10, horizon=30, delay_done=2)
    off = MultiAgentIntersectionEnv(base)
    on = MultiAgentIntersectionEnv(dict(base, rewind=dict(depth=3, stride=2), event_clips=dict(pre=3, post=1, max_clips=8)))
    try:
        with pytest.raises(AssertionError):
            off.rewind_buffer()
        oa, ob = off.reset(), on.reset()
        for t in range(40):
            ra, rb = off.step(_throttles(oa)), on.step(_throttles(ob))
            assert _same(ra, rb), t
            oa, ob = ra[0], rb[0]
        buf = on.rewind_buffer()
        assert buf.n_records == 41 and buf.span() == (36, 40)
        ob = on.reset()                                                     # by hand: the count goes on, the old records cannot be forked
        assert buf.n_records == 42 and buf.span() is None
        br = Branches(buf, 2)
        assert br.fork([0, 0], [41, 42]).cpu().numpy().tolist() == [-1, -1]
        on.step(_throttles(ob))
        assert buf.span() == (42, 42) and br.fork([0, 0], [41, 43]).cpu().numpy().tolist() == [-1, 42]
        br.close()
    finally:
        off.close()
        on.close()
    sim = VecSim(SimConfig(map="intersection", num_envs=4, num_agents=5))
    other_n = VecSim(SimConfig(map="intersection", num_envs=2, num_agents=6))
    other_map = VecSim(SimConfig(map="parkinglot", num_envs=2, num_agents=5))      # 48 routes, 11 spawn places: not the Intersection's 16 / 48
    tgt = VecSim(SimConfig(map="intersection", num_envs=3, num_agents=5))
    h = C.c_void_p()
    try:
        for s in (sim, other_n, other_map, tgt):
            s.reset()
        for bad, code in (((0, 1), -2), ((65, 1), -2), ((4, 0), -2), ((4, -3), -2)):
            assert lib.copo_rewind_create(sim._h, C.byref(_capi.RewindCfg(*bad)), C.byref(h)) == code and not h.value, bad
        good = _capi.RewindCfg(4, 1)
        assert lib.copo_rewind_create(sim._h, None, C.byref(h)) == -1 and lib.copo_rewind_create(sim._h, C.byref(good), None) == -1
        with pytest.raises(_capi.CopoError):
            RewindBuffer(sim, depth=100)
        buf = RewindBuffer(sim, depth=4, stride=1)
        before = [x.clone() for x in sim.get_state()]
        buf.record()
        i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")     # noqa: E731
        sc, rc, status = i32(0, 1), i32(0, 0), i32(7, 7)
        args = (sc.data_ptr(), rc.data_ptr(), None, None, None, status.data_ptr(), None, st)
        states = {s: [x.clone() for x in s.get_state()] for s in (sim, other_n, other_map, tgt)}
        assert lib.copo_rewind_fork(buf._h, sim._h, 0, 2, *args) == -5                            # the target is the source
        assert lib.copo_rewind_fork(buf._h, other_n._h, 0, 2, *args) == -2                        # 6 slots
        assert lib.copo_rewind_fork(buf._h, other_map._h, 0, 2, *args) == -2                      # another map: other routes / spawns
        for first, S in ((0, 0), (2, 2), (-1, 2), (0, 4)):
            assert lib.copo_rewind_fork(buf._h, tgt._h, first, S, *args) == -2, (first, S)
        for k in (0, 1, 5):
            assert lib.copo_rewind_fork(buf._h, tgt._h, 0, 2, *(None if j == k else a for j, a in enumerate(args))) == -1
        assert lib.copo_rewind_fork(None, tgt._h, 0, 2, *args) == -1 and lib.copo_rewind_fork(buf._h, None, 0, 2, *args) == -1
        flags, rows = torch.zeros(2, 5, dtype=torch.uint8, device="cuda"), torch.from_numpy(rn.tally_init(2)).cuda()
        assert lib.copo_rewind_tally(None, None, rows.data_ptr(), 2, 5, st) == -1 and lib.copo_rewind_tally(flags.data_ptr(), None, None, 2, 5, st) == -1
        assert lib.copo_rewind_tally(flags.data_ptr(), None, rows.data_ptr(), 2, 65, st) == -2
        assert lib.copo_rewind_tally(flags.data_ptr(), None, rows.data_ptr(), -1, 5, st) == -2
        for s, was in states.items():                                       # nothing was launched
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(was, s.get_state()))
        assert status.cpu().numpy().tolist() == [7, 7] and rows.cpu().numpy().tolist() == [list(rn.TALLY_INIT)] * 2
        assert lib.copo_rewind_fork(buf._h, tgt._h, 1, 2, *args) == 0 and status.cpu().numpy().tolist() == [0, 0]
        for x, y in zip(before, sim.get_state()):                           # record and fork only read the source
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        act = torch.zeros(3, 5, 2, device="cuda")
        act[..., 1] = 0.5
        assert torch.isfinite(tgt.step(act)["rew"]).all()
        buf.close()
        buf.close()                                                         # closing twice is harmless
    finally:
        for s in (sim, other_n, other_map, tgt):
            s.close()


def _float64_policy(golden_dir):
    """obs [..., O] -> actions [..., 2]: the Gaussian head's mean of the reference's CoPO Intersection population, evaluated in float64
    and rounded once, so that the rows do not depend on how many rows one call holds"""
    from copo_amd.eval.get_policy_function import layer_arrays, population_layout
    with np.load(os.path.join(golden_dir, "eval_policy_function.npz")) as f:
        pre = "copo_inter/w/"
        w = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    layout, sfx = population_layout("copo_inter")
    layers = [(a.astype(np.float64), b.astype(np.float64)) for a, b in layer_arrays(w, layout, "default", sfx)]

    def act(obs):
        x = obs.reshape(-1, obs.shape[-1]).astype(np.float64)
        for d, (a, b) in enumerate(layers):
            x = x @ a + b
            if d < len(layers) - 1:
                x = np.tanh(x)
        return np.ascontiguousarray(x[:, :2].astype(np.float32).reshape(obs.shape[:-1] + (2,)))
    return act


def test_end_to_end_a_crash_is_driven_again(golden_dir):
    """The env (two scenes of the reference's CoPO Intersection population, deterministic actions) with `event_clips` (crash, pre 6, post
    2) and `rewind` (depth 4, stride 1).  With 4 records in the ring a committed clip's first record is still there only when the clip
    is short: seeds 6008 / 6009 and 50 steps were picked on the CPU oracle -- scene 1 has a clip that ends at record 44 and the next
    crash at record 46, whose clip is records 45..48.  Forked at record 45, the branch with the LCF unchanged crashes again: the
    watched slot ends with the CRASH bit in the branch's step that leads from record 45 to record 46."""
    import torch
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    from copo_amd.rewind import Branches
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv, get_lcf_env
    mean, std = meta_svo_lookup_table["copo_inter"]
    env = get_lcf_env(MultiAgentIntersectionEnv)(dict(
        num_envs=2, num_agents=30, delay_done=5, start_seed=6008, lcf_mean=float(mean), lcf_std=float(std), lcf_normal_std=float(std),
        event_clips=dict(pre=6, post=2, max_clips=16, flags=("crash",)), rewind=dict(depth=4, stride=1, keep_obs=True)))
    policy = _float64_policy(golden_dir)
    tr, ring = cn.ClipTracker(2, 30, 6, 2, 16, flag_mask=0x08), rn.RewindRing(2, 30, 4, 1)
    br = None
    driven = 0
    try:
        buf = env.rewind_buffer()
        br = Branches(buf, 3)
        out = env.vec_reset()
        st, e4 = _np_state(env.sim)
        tr.record(st, e4, None)
        ring.record(st, e4)
        for t in range(50):
            out = env.vec_step(torch.from_numpy(policy(out["obs"].cpu().numpy())).cuda())
            st, e4 = _np_state(env.sim)
            n0 = tr.n_clips
            tr.record(st, e4, out["flags"].cpu().numpy())
            ring.record(st, e4)
            assert buf.span() == ring.span()
            for c in range(n0, tr.n_clips):
                h = dict(zip(("scene", "first_rec", "length", "trig_rec", "trig_slot", "kind", "trig_aid", "n_events"), tr.header[c].tolist()))
                if h["first_rec"] < ring.span()[0]:
                    continue
                status, aid = br.fork([h["scene"]], [h["first_rec"]], copies=2, lcf=[np.nan, 1.0], watch_slots=h["trig_slot"], first=1)
                scratch_st, scratch_env = np.zeros((16, 3, 30), np.float32), np.zeros((3, 4), np.int32)
                want_status, want_aid = ring.fork(scratch_st, scratch_env, 1, [h["scene"]], [h["first_rec"]], copies=2, watch_slots=[h["trig_slot"]] * 2)
                assert np.array_equal(status.cpu().numpy(), want_status) and np.array_equal(aid.cpu().numpy(), want_aid)
                print("clip", h, "status", want_status.tolist(), "watch_aid", want_aid.tolist())
                if want_aid[0] != h["trig_aid"]:
                    continue
                # the branch step that takes record r to r + 1 is tally step r - (record forked); the crash shows in the flags that
                # lead to trig_rec
                want_step = (h["trig_rec"] - 1) - int(want_status[0])
                br.rollout(lambda obs: torch.from_numpy(policy(obs.cpu().numpy())).cuda(), h["trig_rec"] - h["first_rec"] + 2)
                o = br.outcomes()
                print("outcomes", {k: v.tolist() for k, v in o.items()})
                assert o["watch_flags"][1] & 0x08 and o["watch_flags"][1] & 0x02 and o["watch_step"][1] == want_step, (h, o)
                driven += 1
        cs = env.event_clips(flush=True)
        tr.flush()
        assert np.array_equal(cs.header, tr.header[:tr.n_clips])
        assert driven >= 1, "no crash clip was still inside the ring"
    finally:
        if br is not None:
            br.close()
        env.close()
