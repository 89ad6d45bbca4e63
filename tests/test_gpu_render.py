"""Top-down renderer on the GPU (copo_render_*, copo_amd/render.py): pixel parity with the numpy restatement of the render rules
(tests/render_numpy.py) on every map family, the trail ring across episode resets and slot reuse, status colours read from the
simulator's state, no effect on the simulation, the dict env's render() and the vis CLI, and the C entry points' argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import render_numpy as rn
from copo_amd.sim import SimConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [dict(map="intersection"), dict(map="roundabout"), dict(map="tollgate", toll_buildings=1), dict(map="tollgate", toll_buildings=2),
        dict(map="bottleneck"), dict(map="parkinglot"), dict(map="pgmap", map_kwargs=dict(sequence="SXCOS", seed=3))]


def _act(rng, E, N, A=2):
    a = np.zeros((E, N, A), np.float32)
    a[..., 0] = rng.uniform(-1.0, 1.0, (E, N))
    a[..., 1] = rng.uniform(-0.3, 1.0, (E, N))
    return a


def _step(sim, rng):
    import torch
    return sim.step(torch.from_numpy(_act(rng, sim.E, sim.N, sim.A)).cuda())


def _state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _compare(tag, gpu, ref, amb):
    """every unambiguous pixel exact, ambiguous pixels under 0.1 % of each image"""
    g = gpu.cpu().numpy()
    assert (g[..., 3] == 255).all(), tag
    bad = (g[..., :3] != ref).any(-1) & ~amb
    n_amb = amb.sum(axis=(1, 2))
    print(tag, "ambiguous pixels per image:", n_amb.tolist())
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g[bad][:5, :3].tolist(), ref[bad][:5].tolist())
    assert (n_amb < 1e-3 * amb.shape[1] * amb.shape[2]).all(), (tag, n_amb.tolist())


# Sub-pixel shifts of a view centre, as fractions of a pixel.  With the line half width max(0.1 m, m / 2) a lane line whose centre sits
# on a pixel row (0.1 m/px) or between two rows (the map views) has BOTH its edges within a millimetre of a row of pixel centres; on
# the axis-aligned maps that happens to a few percent of the lines of any view.  Each view of the parity tests takes the first shift
# under which the restatement finds fewer than 0.05 % of its pixels ambiguous (the pass rule allows 0.1 %).
SHIFTS = [(0.0, 0.0), (0.3141, 0.2718), (0.1618, 0.4142), (0.0577, 0.3606), (0.4339, 0.1127), (0.2236, 0.6931), (0.7071, 0.5772)]


def _views_and_reference(mp, st, env, scenes, views, W, H, **trail):
    out_v, refs, ambs = [], [], []
    for e, v in zip(scenes, views):
        best = None
        for fx, fy in SHIFTS:
            vv = np.array([v[0] + fx * v[2], v[1] + fy * v[2], v[2]], np.float32)
            ref, amb = rn.render_frame(mp, st, env, int(e), vv, W, H, **trail)
            if best is None or amb.sum() < best[2].sum():
                best = (vv, ref, amb)
            if amb.sum() < 5e-4 * W * H:
                break
        out_v.append(best[0])
        refs.append(best[1])
        ambs.append(best[2])
    return np.stack(out_v), np.stack(refs), np.stack(ambs)


def _first_alive(st):
    status = st.view(np.int32)[13] & 0xFF
    return np.array([int(np.argmax(status[e] == rn.ST_ALIVE)) for e in range(st.shape[1])])


@pytest.mark.parametrize("kw", MAPS, ids=lambda kw: kw["map"] + str(kw.get("toll_buildings", "")))
def test_frames_match_the_numpy_restatement(kw):
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import VecSim
    cfg = SimConfig(num_envs=8, **kw)
    sim = VecSim(cfg)
    r512, r320 = TopDownRenderer(sim, 512, 512), TopDownRenderer(sim, 320, 200)
    mp = rn.Map(cfg)
    rng = np.random.RandomState(1)
    try:
        sim.reset()
        for phase in ("reset", "30 steps"):
            if phase != "reset":
                for _ in range(30):
                    _step(sim, rng)
            st, env = _state(sim)
            all8 = np.arange(8)
            follow = _first_alive(st)
            cases = [("map 512x512", r512, all8, dict(view="map")),
                     ("follow 0.1 m/px", r512, all8, dict(view="follow", m_per_px=0.1, follow_slot=follow)),
                     ("map 320x200", r320, all8, dict(view="map")),
                     ("subset [5, 0, 3]", r512, np.array([5, 0, 3]), dict(view="map"))]
            for name, r, scenes, kv in cases:
                slots = kv["follow_slot"][scenes] if "follow_slot" in kv else 0
                views, ref, amb = _views_and_reference(mp, st, env, scenes, r.views(scenes, kv["view"], kv.get("m_per_px"), slots),
                                                       r.W, r.H)
                gpu = r.frames(scenes=scenes, views=views)
                assert tuple(gpu.shape) == (len(scenes), r.H, r.W, 4)
                _compare("%s %s %s" % (cfg.map, phase, name), gpu, ref, amb)
    finally:
        r512.close()
        r320.close()
        sim.close()


def test_trail_across_episode_resets_and_slot_reuse():
    """K = 5 over the last 12 of 30 steps of 30-step episodes: scenes reset inside the window (their pre-reset snapshots are not drawn)
    and slots are taken over by new agents (each drawn in its own colour)."""
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="intersection", num_envs=8, horizon=30, delay_done=0)
    sim = VecSim(cfg)
    r = TopDownRenderer(sim, 512, 512, trail=5)
    mp = rn.Map(cfg)
    rng = np.random.RandomState(0)
    try:
        sim.reset()
        for _ in range(18):
            _step(sim, rng)
        r.record()
        snaps = [_state(sim)]
        for _ in range(12):
            _step(sim, rng)
            r.record()
            snaps.append(_state(sim))
        st, env = snaps[-1]
        window = snaps[-5:]
        reset_in_window = [e for e in range(8) if any(s[1][e, 1] != env[e, 1] for s in window)]
        assert reset_in_window, "no scene reset inside the trail window"
        reused = 0
        for e in range(8):
            cur = [s for s in window if s[1][e, 1] == env[e, 1]]
            for n in range(sim.N):
                alive = [(s[0].view(np.int32)[14, e, n]) for s in cur if (s[0].view(np.int32)[13, e, n] & 0xFF) == rn.ST_ALIVE]
                reused += len(set(alive)) > 1
        assert reused > 0, "no slot changed agents inside the window"
        print("scenes reset inside the window:", reset_in_window, "slots reused:", reused)
        for K in (5, 3):
            views, ref, amb = _views_and_reference(mp, st, env, range(8), r.views(np.arange(8), "map"), 512, 512,
                                                   trail_snaps=snaps[-K:], K=K)
            gpu = r.frames(views=views, trail=K)
            _compare("trail K=%d" % K, gpu, ref, amb)
        plain = r.frames(views=views, trail=0)
        assert (r.frames(views=views, trail=5).cpu() != plain.cpu()).any()
        r.clear()
        assert (r.frames(views=views, trail=5).cpu() == plain.cpu()).all()      # an empty ring draws no trail
    finally:
        r.close()
        sim.close()


def test_status_pixels():
    from copo_amd.render import PALETTE, WRECK, TopDownRenderer
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="intersection", num_envs=8)
    sim = VecSim(cfg)
    r = TopDownRenderer(sim, 512, 512)
    mp = rn.Map(cfg)
    rng = np.random.RandomState(2)
    try:
        sim.reset()
        for _ in range(40):
            _step(sim, rng)
        st, env = _state(sim)
        views = r.views(np.arange(8), "map")
        img = r.frames(views=views).cpu().numpy()[..., :3]
        si = st.view(np.int32)
        counts = {rn.ST_ALIVE: 0, rn.ST_WRECK: 0}
        lower = {rn.BACKGROUND, rn.ROAD, rn.LINE, tuple(int(c) for c in mp.box_rgb)}
        empty_checked = 0
        for e in range(8):
            cx, cy, m = (float(v) for v in views[e])
            status = si[13, e] & 0xFF
            for n in range(sim.N):
                x, y = float(st[0, e, n]), float(st[1, e, n])
                # a higher slot's body drawn over this centre hides it
                if any(status[k] in (rn.ST_ALIVE, rn.ST_WRECK) and
                       rn.obb_test(np.array([x]), np.array([y]), float(st[0, e, k]), float(st[1, e, k]), np.cos(st[2, e, k]),
                                   np.sin(st[2, e, k]), mp.hl + 0.5, mp.hw + 0.5)[0][2][0] for k in range(n + 1, sim.N)):
                    continue
                j = int(np.floor((x - cx) / m + 256.0))
                i = int(np.floor((cy - y) / m + 256.0))
                if not (0 <= i < 512 and 0 <= j < 512):
                    continue
                px = tuple(int(c) for c in img[e, i, j])
                if status[n] == rn.ST_WRECK:
                    assert px == WRECK, (e, n, px)
                elif status[n] == rn.ST_ALIVE:
                    assert px == tuple(int(c) for c in PALETTE[si[14, e, n] % 12]), (e, n, px)
                if status[n] in counts:
                    counts[status[n]] += 1
        assert counts[rn.ST_ALIVE] >= 20 and counts[rn.ST_WRECK] >= 1, counts
        # an EMPTY slot leaves the layers below untouched: empty a driving slot with no other body within 3 m, render again
        st_t, env_t = sim.get_state()
        e = 0
        live = [k for k in range(sim.N) if (si[13, e, k] & 0xFF) in (rn.ST_ALIVE, rn.ST_WRECK)]
        alone = [n for n in live if (si[13, e, n] & 0xFF) == rn.ST_ALIVE and
                 not any(k != n and abs(st[0, e, k] - st[0, e, n]) < 3 and abs(st[1, e, k] - st[1, e, n]) < 3 for k in live)]
        assert alone, "no isolated driving slot in scene 0"
        n = alone[-1]
        st2 = st.copy()
        st2.view(np.int32)[13, e, n] = 0
        import torch
        sim.set_state(torch.from_numpy(st2).cuda(), env_t)
        v1, ref, amb = _views_and_reference(mp, st2, env, [e], views[:1], 512, 512)
        gpu = r.frames(scenes=[e], views=v1)
        _compare("slot %d emptied" % n, gpu, ref, amb)
        x, y = float(st[0, e, n]), float(st[1, e, n])
        j, i = int(np.floor((x - v1[0, 0]) / v1[0, 2] + 256.0)), int(np.floor((v1[0, 1] - y) / v1[0, 2] + 256.0))
        px = tuple(int(c) for c in gpu.cpu().numpy()[0, i, j, :3])
        assert px in lower, px
        empty_checked += 1
        print("checked", counts, "empty slot centre:", px, empty_checked)
    finally:
        r.close()
        sim.close()


def test_rendering_does_not_perturb_the_simulation():
    import torch
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import VecSim
    cfg = SimConfig(map="roundabout", num_envs=8)
    a, b = VecSim(cfg), VecSim(cfg)
    r = TopDownRenderer(a, 256, 256, trail=8)
    rng = np.random.RandomState(3)
    keys = ("obs", "rew", "nei_rew", "flags", "nbr_idx", "lcf")

    def bits(t):
        t = t.cpu()
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    try:
        a.reset()
        b.reset()
        for t in range(50):
            act = torch.from_numpy(_act(rng, 8, a.N)).cuda()
            oa = a.step(act)
            r.record()
            r.frames(view="map", trail=8)
            ob = b.step(act)
            for k in keys:
                assert torch.equal(bits(oa[k]), bits(ob[k])), (t, k)
        for x, y in zip(a.get_state(), b.get_state()):
            assert torch.equal(bits(x), bits(y))
    finally:
        r.close()
        a.close()
        b.close()


def test_dict_env_render():
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    env = MultiAgentIntersectionEnv(dict(num_agents=20))
    rng = np.random.RandomState(4)
    try:
        o = env.reset()
        f0 = env.render(mode="top_down", num_stack=25)
        assert f0.shape == (512, 512, 3) and f0.dtype == np.uint8
        snaps = [_state(env.sim)]            # the renderer recorded the pose at creation, then one per step
        for _ in range(12):
            o, r, d, i = env.step({k: rng.uniform(-0.2, 1.0, 2) for k in o})
            snaps.append(_state(env.sim))
        f1 = env.render(mode="top_down", num_stack=25)
        assert (f1 != f0).any()
        one = env.render(mode="top_down", num_stack=1)
        diff = (one != f1).any(-1)
        assert diff.any()
        # pixels that differ lie on the bodies of the 24 snapshots drawn as the trail
        mp = rn.Map(env.sim_config)
        from copo_amd.render import map_view
        view = map_view(env.sim.tables, 512, 512)
        cx, cy, m = (float(v) for v in np.asarray(view, np.float32))
        X = cx + ((np.arange(512) + 0.5) - 256.0) * m
        Y = cy - ((np.arange(512) + 0.5) - 256.0) * m
        xx, yy = np.meshgrid(X, Y)
        trail = np.zeros((512, 512), bool)
        for st, _ in snaps[-24:]:
            for n in range(env.sim.N):
                if (st.view(np.int32)[13, 0, n] & 0xFF) in (1, 2):
                    trail |= rn.obb_test(xx, yy, float(st[0, 0, n]), float(st[1, 0, n]), np.cos(st[2, 0, n]), np.sin(st[2, 0, n]),
                                         mp.hl, mp.hw)[0][2]
        assert not (diff & ~trail).any(), int((diff & ~trail).sum())
        ids = [a for a in env._slot_ids if a is not None]
        assert env.render(mode="top_down", track_agent=ids[0]).shape == (512, 512, 3)
        assert env.render(mode="top_down", film_size=(320, 200)).shape == (200, 320, 3)
    finally:
        env.close()


def test_evaluation_envs_render_into_frames():
    from copo_amd.eval.evaluate_population import get_make_env
    env = get_make_env("inter", render=True)()
    try:
        o, d = env.reset(), {"__all__": False}
        for _ in range(3):
            o, r, d, i = env.step({k: np.array([0.0, 0.5]) for k in o})
        assert len(env.frames) == 3 and env.frames[0].shape == (512, 512, 3)
    finally:
        env.close()


def test_vis_cli_writes_frames(tmp_path, golden_dir):
    out = tmp_path / "vis"
    cmd = [sys.executable, "-m", "copo_amd.vis", "--env", "inter", "--algo", "copo", "--weights",
           os.path.join(golden_dir, "eval_policy_function.npz"), "--key", "copo_inter", "--steps", "15", "--out", str(out),
           "--follow", "0"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    files = sorted(os.listdir(out))
    assert files == ["frame_%05d.ppm" % k for k in range(15)], files
    from copo_amd.render import read_ppm
    assert read_ppm(str(out / files[-1])).shape == (512, 512, 3)


def test_argument_errors_leave_the_handle_usable():
    import torch
    from copo_amd import _capi
    from copo_amd.render import PALETTE, TopDownRenderer
    from copo_amd.sim import VecSim
    lib = _capi.lib
    sim = VecSim(SimConfig(map="intersection", num_envs=4))
    sim.reset()
    pal = np.ascontiguousarray(PALETTE)
    h = C.c_void_p()
    for w, hh, k in ((0, 64, 0), (4097, 64, 0), (64, 0, 0), (64, 4097, 0), (64, 64, -1), (64, 64, 33)):
        assert lib.copo_render_create(sim._h, w, hh, k, pal.ctypes.data, C.byref(h)) == -2, (w, hh, k)
    assert lib.copo_render_create(sim._h, 64, 64, 0, None, C.byref(h)) == -1
    assert lib.copo_render_create(sim._h, 64, 64, 0, pal.ctypes.data, None) == -1
    r = TopDownRenderer(sim, 64, 48, trail=4)
    try:
        r.record()
        ref = r.frames(view="map").cpu()
        sc = torch.arange(4, dtype=torch.int32).cuda()
        views = torch.from_numpy(r.views(np.arange(4))).cuda()
        out = torch.zeros(4, 48, 64, dtype=torch.int32).cuda()
        st = _capi.current_stream()
        f = lib.copo_render_frames
        assert f(r._h, sc.data_ptr(), 0, views.data_ptr(), 0, out.data_ptr(), st) == -2
        assert f(r._h, sc.data_ptr(), 5, views.data_ptr(), 0, out.data_ptr(), st) == -2
        assert f(r._h, sc.data_ptr(), 4, views.data_ptr(), 5, out.data_ptr(), st) == -2        # above the capacity
        assert f(r._h, sc.data_ptr(), 4, views.data_ptr(), -1, out.data_ptr(), st) == -2
        assert f(r._h, None, 4, views.data_ptr(), 0, out.data_ptr(), st) == -1
        assert f(r._h, sc.data_ptr(), 4, None, 0, out.data_ptr(), st) == -1
        assert f(r._h, sc.data_ptr(), 4, views.data_ptr(), 0, None, st) == -1
        torch.cuda.synchronize()
        assert (out.cpu() == 0).all()                       # nothing was launched
        with pytest.raises(ValueError):
            r.frames(scenes=[4])                            # scene indices are checked on the host
        assert torch.equal(r.frames(view="map").cpu(), ref)
        assert f(r._h, sc.data_ptr(), 4, views.data_ptr(), 4, out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.uint8).view(4, 48, 64, 4), r.frames(view="map", trail=4).cpu())
    finally:
        r.close()
        sim.close()
