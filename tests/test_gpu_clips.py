"""Event clips on the GPU (copo_clip_*, copo_amd/clips.py) against the numpy restatement of their rules (tests/clip_numpy.py): hand-set
states across a ring wrap, synthetic streams at the sizes where the ordered commit can go wrong, a rollout of the reference's CoPO
population with scene resets; exact replay of the renderer and of the interaction meter from a played-back clip; repeatability, no
effect on the simulation, the dict env and `vis --replay` surface, and the C entry points' argument checks.

Every comparison is bit for bit: the feature is copies, integer logic and fp32 `<`.

The rollout case (interact_cases.rollout_config: Intersection, 3 scenes x 10 slots, 120 steps) has ONE crash, so `flags=("crash",)` gives
one clip.  The trigger flags used here are ("crash", "out", "maxstep"): the crash, the one agent that leaves the road and the agents
that reach the 55-step horizon -- the last of a draining scene, so those clips span the scene's reset.  ("out" and "arrive" do not
suffice: nobody arrives within 55 steps.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_numpy as cn
import interact_cases as ic
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUT_FLAGS = ("crash", "out", "maxstep")
ROLLOUT_MASK = 0x08 | 0x10 | 0x20
PRE, POST = 12, 4
FILM = (96, 64)                      # width, height of the replay frames


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _pool(rec):
    """the WHOLE pool of a recorder (max_clips entries, stored or not) and its counters"""
    import torch
    from copo_amd import _capi
    M, N = rec.max_clips, rec.sim.N
    header = torch.full((M, 8), -1, dtype=torch.int32, device="cuda")
    snaps = torch.full((M, rec.cap, 6, N), -1, dtype=torch.int32, device="cuda")
    envw = torch.full((M, rec.cap, 2), -1, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib.copo_clip_read(rec._h, 0, M, header.data_ptr(), snaps.data_ptr(), envw.data_ptr(), _capi.current_stream()))
    return header.cpu().numpy(), snaps.cpu().numpy().view(np.uint32), envw.cpu().numpy(), rec.count()


def _same_pool(rec, tr, tag=""):
    header, snaps, envw, (n, dropped) = _pool(rec)
    print(tag, "clips", n, "dropped", dropped, "restatement", tr.n_clips, tr.dropped)
    assert (n, dropped) == (tr.n_clips, tr.dropped), tag
    assert np.array_equal(header, tr.header), (tag, np.argwhere(header != tr.header)[:5].tolist())
    assert np.array_equal(snaps, tr.snaps), (tag, np.argwhere(snaps != tr.snaps)[:5].tolist())
    assert np.array_equal(envw, tr.envw), (tag, np.argwhere(envw != tr.envw)[:5].tolist())
    cs = rec.clips()
    assert len(cs) == n and np.array_equal(cs.header, tr.header[:n]) and np.array_equal(cs.snaps, tr.snaps[:n]) and np.array_equal(cs.envw, tr.envw[:n])
    return cs


def test_hand_set_states_across_a_ring_wrap():
    """E = 2, N = 5, pre = 3, post = 1 (a ring of 5), 11 records of distinct states: scene 0 fires at record 1 (a clip of the 3 records
    there are), scene 1 at record 7 (records 4..8, the ring has wrapped: record 8 lies in ring slot 3)."""
    import torch
    from copo_amd.clips import ClipRecorder
    from copo_amd.sim import VecSim
    sim = VecSim(SimConfig(map="intersection", num_envs=2, num_agents=5))
    rec = ClipRecorder(sim, pre=3, post=1, max_clips=4, flags=("crash",))
    tr = cn.ClipTracker(2, 5, 3, 1, 4, flag_mask=0x08)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        states = []
        for r in range(11):
            st = ic.random_state(st0, 100 + r)
            st.view(np.int32)[13] |= (r + 1) << 8                   # bits above the status byte: not part of a snapshot
            env = env0.copy()
            env[:, 0], env[:, 1] = r, r // 4
            flags = np.zeros((2, 5), np.uint8)
            flags[:, 0] = 0x01 | 0x40                               # flags outside the mask never fire
            if r == 1:
                flags[0, 3] = flags[0, 4] = 0x08 | 0x02
            if r == 7:
                flags[1, 2] = 0x08
            states.append((st, env))
            _set_state(sim, st, env)
            rec.record(flags=torch.from_numpy(flags).cuda())
            tr.record(st, env, flags)
        cs = _same_pool(rec, tr, "hand-set")
        assert len(cs) == 2 and cs.header[0].tolist() == [0, 0, 3, 1, 3, 1, int(states[1][0].view(np.int32)[14, 0, 3]), 1]
        assert cs.header[1].tolist() == [1, 4, 5, 7, 2, 1, int(states[7][0].view(np.int32)[14, 1, 2]), 1]
        for c, (scene, records) in enumerate(((0, [0, 1, 2]), (1, [4, 5, 6, 7, 8]))):
            for k, r in enumerate(records):                          # word for word the states that were set
                su = states[r][0].view(np.uint32)
                for w, f in enumerate((0, 1, 2, 3)):
                    assert np.array_equal(cs.snaps[c, k, w], su[f, scene]), (c, k, w)
                assert np.array_equal(cs.snaps[c, k, 4], su[13, scene] & 0xFF) and np.array_equal(cs.snaps[c, k, 5], su[14, scene])
                assert cs.envw[c, k].tolist() == [r, r // 4]
        assert not cs.snaps[0, 3:].any()
        # the recorder only reads the simulator: the last state that was set is still there
        st, env = _np_state(sim)
        assert np.array_equal(st.view(np.int32), states[-1][0].view(np.int32)) and np.array_equal(env, states[-1][1])
    finally:
        rec.close()
        sim.close()


def _stream(base, env0, p_flag, records=40):
    """records of a synthetic stream: (state, env, flags, ttc or None, gap or None), the triggers at random"""
    rng = np.random.RandomState(5)
    _, E, N = base[0].shape
    for r in range(records):
        st = base[r % len(base)].copy()
        st[0] += np.float32(r)                                   # a state of its own per record
        env = env0.copy()
        env[:, 0], env[:, 1] = r, rng.randint(0, 3, E)
        flags = (rng.randint(0, 256, (E, N)) & 0xE7).astype(np.uint8)      # every bit outside the mask at random
        flags |= (0x08 * (rng.rand(E, N) < p_flag) + 0x10 * (rng.rand(E, N) < p_flag)).astype(np.uint8)
        ttc = rng.uniform(0.0, 10.0, (E, N)).astype(np.float32)            # below 0.05: 0.5 % of the slots
        gap = rng.uniform(0.0, 10.0, (E, N)).astype(np.float32)            # below 0.02: 0.2 %
        ttc[rng.rand(E, N) < 0.2], gap[rng.rand(E, N) < 0.2] = np.inf, np.inf
        ttc[rng.rand(E, N) < 0.05], gap[rng.rand(E, N) < 0.05] = np.nan, np.nan
        yield st, env, flags, (ttc if r % 7 != 3 else None), (gap if r % 5 != 2 else None)      # a NULL array now and then


@pytest.mark.parametrize("shape", ["1x64", "300x3"])
def test_synthetic_stream(shape):
    """1 x 64: a full wave of slots.  300 x 3: more scenes than a wave and than a 256-thread workgroup, 40 records, a pool of 64 that
    overflows, with records whose ready scenes lie on both sides of scene 64 and of scene 256."""
    import torch
    from copo_amd.clips import ClipRecorder
    from copo_amd.sim import VecSim
    if shape == "1x64":
        cfg, p_flag, max_clips = SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=1, num_agents=64), 0.002, 16
    else:
        cfg, p_flag, max_clips = SimConfig(map="intersection", num_envs=300, num_agents=3), 0.02, 64
    E, N = cfg.num_envs, cfg.num_agents
    sim = VecSim(cfg)
    rec = ClipRecorder(sim, pre=3, post=2, max_clips=max_clips, flags=("crash", "out"), ttc_below=0.05, gap_below=0.02)
    tr = cn.ClipTracker(E, N, 3, 2, max_clips, flag_mask=0x18, ttc_below=0.05, gap_below=0.02)
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        base = [ic.random_state(st0, 40 + k) for k in range(4)]
        for st, env, flags, ttc, gap in _stream(base, env0, p_flag):
            _set_state(sim, st, env)
            rec.record(flags=torch.from_numpy(flags).cuda(), ttc=None if ttc is None else torch.from_numpy(ttc).cuda(),
                       gap=None if gap is None else torch.from_numpy(gap).cuda())
            tr.record(st, env, flags, ttc, gap)
        _same_pool(rec, tr, shape)
        kinds = set(tr.header[:tr.n_clips, cn.H_KIND].tolist())
        print(shape, "kinds", sorted(kinds), "ready per record", [len(x) for x in tr.ready_log])
        assert tr.n_clips >= 3 and len(kinds) >= 2
        if shape == "300x3":
            assert tr.n_clips == max_clips and tr.dropped > 0                                       # the pool overflowed
            assert any(x and min(x) < 64 <= max(x) for x in tr.ready_log)                            # ready scenes on both sides of 64
            assert any(x and min(x) < 256 <= max(x) for x in tr.ready_log)                           # and of 256
            assert np.bitwise_or.reduce(tr.header[:tr.n_clips, cn.H_KIND]) == cn.KIND_FLAG | cn.KIND_TTC | cn.KIND_GAP
        rec.flush()
        tr.flush()
        _same_pool(rec, tr, shape + " flushed")
        rec.reset()                                                  # an empty recorder again, records from 0
        tr.reset()
        for r in range(4):
            flags = np.full((E, N), 0x08 if r == 1 else 0, np.uint8)
            _set_state(sim, base[r], env0)
            rec.record(flags=torch.from_numpy(flags).cuda())
            tr.record(base[r], env0, flags)
        _same_pool(rec, tr, shape + " after reset")
        assert tr.n_clips == min(E, max_clips) and tr.header[0].tolist()[:4] == [0, 0, 4, 1]
    finally:
        rec.close()
        sim.close()


def _rollout(golden_dir, live=False, tracker=None):
    """120 steps of the rollout case with a recorder on ROLLOUT_FLAGS; `live`: also a live renderer (trail ring of 5) and meter whose
    per-record outputs are kept.  Returns dict(pool=(header, snaps, envw, counts), clips=ClipSet, frames0, frames5, gap, ttc)."""
    import torch
    from copo_amd.clips import ClipRecorder
    from copo_amd.interact import InteractionMeter
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import VecSim
    cfg = ic.rollout_config()
    sim = VecSim(cfg)
    rec = ClipRecorder(sim, pre=PRE, post=POST, max_clips=32, flags=ROLLOUT_FLAGS)
    ren = TopDownRenderer(sim, FILM[0], FILM[1], trail=5) if live else None
    meter = InteractionMeter(sim) if live else None
    act = ic.rollout_policy(golden_dir)
    res = dict(frames0=[], frames5=[], gap=[], ttc=[])

    def after(flags):
        rec.record(flags=flags)
        if tracker is not None:
            st, env = _np_state(sim)
            tracker.record(st, env, None if flags is None else flags.cpu().numpy())
        if live:
            ren.record()
            res["frames0"].append(ren.frames(trail=0).cpu().numpy())
            res["frames5"].append(ren.frames(trail=5).cpu().numpy())
            gap, ttc = meter.record()
            res["gap"].append(gap.cpu().numpy())
            res["ttc"].append(ttc.cpu().numpy())
    try:
        out = sim.reset()
        after(None)
        for t in range(ic.ROLLOUT_STEPS):
            out = sim.step(torch.from_numpy(act(out["obs"].cpu().numpy())).cuda())
            after(out["flags"])
        res["pool"] = _pool(rec)
        res["clips"] = rec.clips()
        if tracker is not None:
            _same_pool(rec, tracker, "rollout")
        return res
    finally:
        for x in (rec, ren, meter):
            if x is not None:
                x.close()
        sim.close()


@pytest.fixture(scope="module")
def rollout(golden_dir):
    tr = cn.ClipTracker(3, 10, PRE, POST, 32, flag_mask=ROLLOUT_MASK)
    res = _rollout(golden_dir, live=True, tracker=tr)
    res["tracker"] = tr
    return res


@pytest.fixture(scope="module")
def player(rollout):
    from copo_amd.clips import ClipPlayer
    p = ClipPlayer(rollout["clips"])
    yield p
    p.close()


def test_rollout_against_the_restatement(rollout):
    tr, cs = rollout["tracker"], rollout["clips"]            # (the pool was compared with the restatement's inside the rollout)
    print(cs.header.tolist())
    assert len(cs) >= 3 and tr.dropped == 0
    assert (cs.column("first_rec") > 0).any()
    spans = [c for c in range(len(cs)) if len(set(cs.envw[c, :cs.info(c)["length"], 1].tolist())) > 1]
    assert spans, "no clip spans a scene reset"
    assert (cs.column("kind") == cn.KIND_FLAG).all() and (cs.column("length") <= PRE + POST + 1).all()


def test_exact_replay_of_the_renderer(rollout, player):
    cs = rollout["clips"]
    for c in range(len(cs)):
        i = cs.info(c)
        records = range(i["first_rec"], i["first_rec"] + i["length"])
        live0 = np.stack([rollout["frames0"][r][i["scene"]] for r in records])
        live5 = np.stack([rollout["frames5"][r][i["scene"]] for r in records])
        got0 = player.render(c, trail=0, film_size=FILM)
        assert got0.shape == (i["length"], FILM[1], FILM[0], 4) and got0.dtype == np.uint8
        assert np.array_equal(got0, live0), (c, np.argwhere(got0 != live0)[:3].tolist())
        got5 = player.render(c, trail=5, film_size=FILM)
        assert np.array_equal(got5[5:], live5[5:]), (c, np.argwhere(got5[5:] != live5[5:])[:3].tolist())
        assert i["length"] > 5
    assert any((rollout["frames5"][r] != rollout["frames0"][r]).any() for r in range(len(rollout["frames0"])))      # trails are drawn


def test_exact_replay_of_the_meter(rollout, player):
    cs = rollout["clips"]
    finite = 0
    for c in range(len(cs)):
        i = cs.info(c)
        records = range(i["first_rec"], i["first_rec"] + i["length"])
        m = player.interaction(c)
        for key in ("gap", "ttc"):
            live = np.stack([rollout[key][r][i["scene"]] for r in records])
            assert m[key].shape == live.shape == (i["length"], 10)
            assert np.array_equal(m[key].view(np.uint32), live.view(np.uint32)), (c, key)
            finite += int(np.isfinite(live).sum())
    assert finite > 0


def test_two_identical_runs_give_identical_clips(rollout, golden_dir):
    again = _rollout(golden_dir)
    for a, b in zip(rollout["pool"][:3], again["pool"][:3]):
        assert np.array_equal(a, b)
    assert rollout["pool"][3] == again["pool"][3] and rollout["pool"][3][0] >= 3


def test_recording_does_not_perturb_the_simulation():
    import torch
    from copo_amd.clips import ClipRecorder
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="roundabout", num_envs=8)
    a, b = VecSim(cfg), VecSim(cfg)
    rec = ClipRecorder(a, pre=5, post=2, max_clips=8, flags=("crash", "out", "done"))
    rng = np.random.RandomState(3)
    keys = ("obs", "rew", "nei_rew", "flags", "nbr_idx", "lcf")

    def bits(t):
        t = t.cpu()
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    try:
        a.reset()
        b.reset()
        rec.record()
        for t in range(60):
            act = np.zeros((8, a.N, 2), np.float32)
            act[..., 0], act[..., 1] = rng.uniform(-1.0, 1.0, (8, a.N)), rng.uniform(-0.3, 1.0, (8, a.N))
            act = torch.from_numpy(act).cuda()
            oa = a.step(act)
            rec.record(flags=oa["flags"])
            if t == 30:
                rec.flush()
                rec.clips()
            ob = b.step(act)
            for k in keys:
                assert torch.equal(bits(oa[k]), bits(ob[k])), (t, k)
        for x, y in zip(a.get_state(), b.get_state()):
            assert torch.equal(bits(x), bits(y))
        n, dropped = rec.count()
        assert n == 8 and dropped > 0
    finally:
        rec.close()
        a.close()
        b.close()


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


def test_dict_env():
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    base = dict(num_agents=10, horizon=30, delay_done=2)
    with pytest.raises(ValueError):
        MultiAgentIntersectionEnv(dict(base, event_clips=dict(ttc_below=1.0)))
    off = MultiAgentIntersectionEnv(base)
    on = MultiAgentIntersectionEnv(dict(base, event_clips=dict(pre=6, post=2, max_clips=16, flags=("crash",))))
    try:
        with pytest.raises(AssertionError):
            off.event_clips()
        oa, ob = off.reset(), on.reset()
        assert _same(oa, ob)
        crashed = {}                                       # record -> the agents the env reported crashed in that step
        for t in range(45):
            ra, rb = off.step(_throttles(oa)), on.step(_throttles(ob))
            assert _same(ra, rb), t                        # obs, rewards, dones, info: the key changes nothing
            assert not any("clip" in k for v in rb[3].values() for k in v)
            oa, ob = ra[0], rb[0]
            crashed[t + 1] = {a for a, v in rb[3].items() if v.get("crash")}
            assert not rb[2]["__all__"]
        cs = on.event_clips(flush=True)
        print(cs.header.tolist(), {k: v for k, v in crashed.items() if v})
        assert len(cs) >= 1 and any(crashed.values())
        for c in range(len(cs)):
            i = cs.info(c)
            assert i["kind"] == cn.KIND_FLAG and i["scene"] == 0
            assert "agent%d" % i["trig_aid"] in crashed[i["trig_rec"]], i
        assert cs.meta["pre"] == 6 and cs.meta["sim_config"]["map"] == "intersection" and cs.N == 10
        ob = on.reset()                                    # clips survive a reset; the env goes on
        on.step(_throttles(ob))
        assert len(on.event_clips()) >= len(cs)
    finally:
        off.close()
        on.close()
        on.close()


def test_vis_replay_writes_the_clips(rollout, player, tmp_path):
    from copo_amd.render import read_ppm
    cs = rollout["clips"].select(scene=[0])
    cs = type(cs)(cs.header[:2], cs.snaps[:2], cs.envw[:2], cs.meta)
    assert len(cs) == 2
    path, out = str(tmp_path / "clips.npz"), tmp_path / "replay"
    cs.save(path)
    cmd = [sys.executable, "-m", "copo_amd.vis", "--replay", path, "--out", str(out), "--size", str(FILM[0]), str(FILM[1])]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["clip_000", "clip_001"]
    ids = [c for c in range(len(rollout["clips"])) if rollout["clips"].info(c)["scene"] == 0][:2]
    for k, c in enumerate(ids):
        want = player.render(c, film_size=FILM)          # the CLI's defaults: whole map, trail 25
        files = sorted(os.listdir(out / ("clip_%03d" % k)))
        assert files == ["frame_%05d.ppm" % f for f in range(cs.info(k)["length"])], files
        for f, name in enumerate(files):
            assert np.array_equal(read_ppm(str(out / ("clip_%03d" % k) / name)), want[f, :, :, :3]), (k, f)


def test_argument_errors_leave_everything_usable():
    import torch
    from copo_amd import _capi
    from copo_amd.clips import ClipPlayer, ClipRecorder
    from copo_amd.interact import InteractionMeter
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import VecSim
    lib = _capi.lib
    sim = VecSim(SimConfig(map="intersection", num_envs=4, num_agents=5))
    other = VecSim(SimConfig(map="intersection", num_envs=2, num_agents=6))
    act = torch.zeros(4, 5, 2, device="cuda")
    act[..., 1] = 0.5
    h = C.c_void_p()
    st = _capi.current_stream()
    try:
        sim.reset()
        other.reset()
        for bad, code in (((-1, 1, 8, 8, 0.0, 0.0), -2), ((1, -1, 8, 8, 0.0, 0.0), -2), ((200, 56, 8, 8, 0.0, 0.0), -2), ((3, 1, 0, 8, 0.0, 0.0), -2),
                          ((3, 1, 8, 8, -1.0, 0.0), -5), ((3, 1, 8, 8, 0.0, float("nan")), -5), ((3, 1, 8, 0x100, 0.0, 0.0), -5),
                          ((200, 55, 2 ** 31 - 1, 8, 0.0, 0.0), -3)):               # the last: a pool of 66 TB, which the device refuses
            assert lib.copo_clip_create(sim._h, C.byref(_capi.ClipCfg(*bad)), C.byref(h)) == code, bad
            assert lib.copo_last_error() and not h.value
        good = _capi.ClipCfg(3, 1, 8, 8, 0.0, 0.0)
        assert lib.copo_clip_create(sim._h, None, C.byref(h)) == -1 and lib.copo_clip_create(sim._h, C.byref(good), None) == -1
        with pytest.raises(_capi.CopoError):
            ClipRecorder(sim, pre=300)
        with pytest.raises(ValueError):
            ClipRecorder(sim, flags=("bump",))
        rec, ren, meter = ClipRecorder(sim, pre=3, post=0, max_clips=8, flags=("acted",)), TopDownRenderer(sim, 64, 64, trail=4), InteractionMeter(sim)
        out = sim.step(act)
        rec.record(flags=out["flags"])
        n, d = C.c_int32(), C.c_int32()
        assert lib.copo_clip_count(rec._h, None, C.byref(d), st) == -1 and lib.copo_clip_count(rec._h, C.byref(n), None, st) == -1
        buf = torch.zeros(8 * 4 * 6 * 5, dtype=torch.int32, device="cuda")
        assert lib.copo_clip_read(rec._h, -1, 1, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), st) == -2
        assert lib.copo_clip_read(rec._h, 4, 5, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), st) == -2
        assert lib.copo_clip_read(rec._h, 0, 1, None, buf.data_ptr(), buf.data_ptr(), st) == -1
        with pytest.raises(ValueError):
            rec.record(flags=out["flags"].to(torch.int32))
        with pytest.raises(ValueError):
            rec.record(ttc=torch.zeros(4, 4, device="cuda"))
        cs = rec.clips()                                   # every scene fired (post = 0): 4 clips of 1 record, in scene order
        assert rec.count() == (4, 0) and cs.column("scene").tolist() == [0, 1, 2, 3] and cs.column("length").tolist() == [1] * 4
        # scatter: NULL pointers, a cap outside 1..256, another N, S > E, S < 1
        snaps, envw = torch.from_numpy(cs.snaps.view(np.int32)).cuda(), torch.from_numpy(cs.envw).cuda()
        ci, fi = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        args = (snaps.data_ptr(), envw.data_ptr(), cs.cap, 5, ci.data_ptr(), fi.data_ptr(), 4, st)
        before = [x.clone() for x in sim.get_state()]
        for k in (0, 1, 4, 5):
            assert lib.copo_clip_scatter(sim._h, *(None if j == k else a for j, a in enumerate(args))) == -1
        assert lib.copo_clip_scatter(None, *args) == -1
        assert lib.copo_clip_scatter(sim._h, *args[:2], 0, *args[3:]) == -2 and lib.copo_clip_scatter(sim._h, *args[:2], 257, *args[3:]) == -2
        assert lib.copo_clip_scatter(other._h, *args) == -2                        # 6 slots there
        assert lib.copo_clip_scatter(sim._h, *args[:6], 5, st) == -2 and lib.copo_clip_scatter(sim._h, *args[:6], 0, st) == -2
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, sim.get_state()))      # nothing was launched
        # scenes >= S are left alone; -1 is an all-EMPTY scene
        fi[1] = -1
        assert lib.copo_clip_scatter(sim._h, *args[:6], 2, st) == 0
        after = [x.cpu().numpy() for x in sim.get_state()]
        b4 = [x.cpu().numpy() for x in before]
        assert np.array_equal(after[0].view(np.int32)[:, 2:], b4[0].view(np.int32)[:, 2:]) and np.array_equal(after[1][2:], b4[1][2:])
        assert not after[0].view(np.int32)[:, 1].any() and after[1][1].tolist() == [0, 0, 0, 1]
        assert np.array_equal(after[0].view(np.uint32)[[0, 1, 2, 3, 14], 0], cs.snaps[0, 0, [0, 1, 2, 3, 5]])
        assert np.array_equal(after[0].view(np.uint32)[13, 0], cs.snaps[0, 0, 4]) and not after[0].view(np.int32)[4:13, 0].any()
        assert after[1][0].tolist() == [int(cs.envw[0, 0, 0]), int(cs.envw[0, 0, 1]), 0, 1]
        player = ClipPlayer(cs)
        for bad in (([0], 1), ([4], 0), ([0, 1], 0), ([0], -2)):
            with pytest.raises(ValueError):
                player.seek(*bad)
        player.seek([3], 0)
        player.close()
        # everything still works, and reset / close in either order with the renderer and the meter
        sim.reset()
        out = sim.step(act)
        rec.record(flags=out["flags"])
        ren.record()
        meter.record()
        assert rec.count() == (8, 0) and ren.frames(scenes=[0]).shape == (1, 64, 64, 4) and meter.summary(flush_open=True)["steps"] > 0
        rec.reset()
        ren.clear()
        meter.reset()
        rec.record(flags=out["flags"])
        assert rec.count() == (4, 0)
        ren.close()
        rec.record(flags=out["flags"])
        rec.close()
        rec.close()                                        # closing twice is harmless
        meter.record()
        meter.close()
        rec2, ren2 = ClipRecorder(sim, pre=1, post=1), TopDownRenderer(sim, 64, 64)
        rec2.reset()
        ren2.close()
        rec2.record(flags=out["flags"])
        rec2.flush()
        rec2.close()
        assert torch.isfinite(sim.step(act)["rew"]).all()
    finally:
        sim.close()
        other.close()
