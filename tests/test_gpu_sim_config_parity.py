"""HIP simulator vs the CPU oracle, bit for bit, where test_gpu_sim_parity.py does not reach: LiDAR against buildings it sees
(toll_buildings=1) in every launch shape, the SimConfig knobs whose kernel branches the default configurations never take, and the
step as training runs it -- replayed from a captured graph, with the LCF setters and flush() between replays.  Every comparison is
raw-bit equality of all outputs; test_sim_config_premises_cpu.py shows on the oracle alone that the cases enter those branches."""
import ctypes as C
import weakref

import numpy as np
import pytest

import sim_config_cases as sc
from test_gpu_sim_parity import OUT_KEYS, _compare

pytestmark = pytest.mark.gpu


def _pair(cfg, block, chunk=0):
    import oracle_lib as ol
    from copo_amd.sim import VecSim
    g, o = VecSim(cfg), ol.OracleSim(cfg)
    g.set_block(block)
    if chunk:
        g.set_chunk(chunk)
    return g, o


def _rollout(tag, cfg, block, steps, sigma=0.12, calls=None, chunk=0):
    """Reset + `steps` steps on both simulators with the case's seeds, actions and setter calls; returns the oracle's last outputs."""
    import torch
    g, o = _pair(cfg, block, chunk)
    E, N = g.E, g.N
    sc.apply_calls(calls, -1, g, o)
    _compare(tag + " reset", g.reset(sc.seeds(E)), o.reset(sc.seeds(E)))
    rng = np.random.RandomState(3)
    for t in range(steps):
        sc.apply_calls(calls, t, g, o)
        a = sc.actions(rng, E, N, t, sigma)
        _compare("%s step %d" % (tag, t), g.step(torch.from_numpy(a).cuda()), o.step(a))
    gs, ge = g.get_state()
    os_, oe = o.get_state()
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), os_.view(np.uint32))
    assert np.array_equal(ge.cpu().numpy()[:, :3], oe[:, :3])
    g.close()
    o.close()


@pytest.mark.parametrize("block,E,N,lasers,chunk", [c[1:] for c in sc.VISIBLE_SHAPES], ids=[c[0] for c in sc.VISIBLE_SHAPES])
def test_visible_buildings_rollout_bit_exact(block, E, N, lasers, chunk):
    """A1: the Tollgate with buildings the LiDAR sees, in every shape that has box code or an LDS layout of its own."""
    _rollout("buildings block %d" % block, sc.visible_config(E, N, lasers), block, sc.STEPS_A, chunk=chunk)


@pytest.mark.parametrize("block", [64, 512, -4])
def test_crafted_building_scenes_bit_exact(block):
    """A2: poses the rollouts do not produce (sim_config_cases.crafted_building_scenes): on the cull radius of the box test and one
    fp32 step either side, a face one fp32 step inside / outside the LiDAR's range, headings along and across a building's long
    axis (rays parallel to its faces), a vehicle between a vehicle and a building and one behind a building (the minimum of the two
    returns in both orders), a body that touches a building by a centimetre and one that misses it, vehicles far from everything.
    On the oracle: the poses named for it have beams shortened by a building against a run with hidden buildings on the same state.
    (On the cull radius itself no beam can reach: the nearest face is range + the smaller half extent away.)"""
    import torch
    import oracle_lib as ol
    cfg = sc.visible_config(sc.CRAFT_E, sc.CRAFT_N, 72)
    g, o = _pair(cfg, block)
    h = ol.OracleSim(sc.visible_config(sc.CRAFT_E, sc.CRAFT_N, 72, buildings=2))
    seeds = sc.seeds(sc.CRAFT_E)
    _compare("reset", g.reset(seeds), o.reset(seeds))
    h.reset(seeds)
    st, env = o.get_state()
    st = st.copy()
    named = sc.crafted_building_scenes(cfg, st)
    o.set_state(st, env)
    h.set_state(st, env)
    g.set_state(torch.from_numpy(st).cuda(), torch.from_numpy(env).cuda())
    a = sc.crafted_actions()
    cols = sc.lidar_cols(cfg)
    for t in range(sc.CRAFT_STEPS):
        go, oo = g.step(torch.from_numpy(a).cuda()), o.step(a)
        _compare("crafted step %d (block %d)" % (t, block), go, oo)
        if t == 0:
            vis, hid = oo["obs"][..., cols].copy(), h.step(a)["obs"][..., cols].copy()
            for k in ("reach_in_long", "reach_in_short", "parallel_along", "parallel_across", "parallel_end_face", "behind_vehicle",
                      "before_building"):
                assert (vis[named[k]] < hid[named[k]]).any(), k
            assert oo["flags"][named["touching"]] & 8 and not oo["flags"][named["clear"]] & 8
    for s in (g, o, h):
        s.close()


def test_box_table_error_codes():
    """A3: more static boxes than COPO_MAX_BOXES, or boxes without a table, are COPO_ERR_CONFIG (-5 in include/copo_hip.h; -2 is
    COPO_ERR_DIM) with a message that names the field -- never a simulator that reads past the table."""
    from copo_amd import _capi
    from copo_amd.sim import fill_cfg_struct
    max_boxes = 16                                     # COPO_MAX_BOXES
    cfg = sc.visible_config(2, 8, 72)
    struct, keep = fill_cfg_struct(cfg, _capi.SimCfg)
    assert 0 < struct.n_boxes <= max_boxes
    n, table = struct.n_boxes, struct.boxes
    h = C.c_void_p()
    big = np.zeros((max_boxes + 1, 6), np.float32)     # (the table really holds that many: the count alone is refused)
    big[:, 2], big[:, 4:] = 1.0, 1.0
    struct.n_boxes, struct.boxes = max_boxes + 1, big.ctypes.data
    rc = _capi.lib.copo_sim_create(C.byref(struct), 0, C.byref(h))
    assert rc == -5 and _capi.ERR_NAMES[rc] == "COPO_ERR_CONFIG" and b"n_boxes" in _capi.lib.copo_last_error()
    struct.n_boxes, struct.boxes = n, None
    rc = _capi.lib.copo_sim_create(C.byref(struct), 0, C.byref(h))
    assert rc == -5 and b"n_boxes" in _capi.lib.copo_last_error()
    struct.n_boxes, struct.boxes = -1, table
    assert _capi.lib.copo_sim_create(C.byref(struct), 0, C.byref(h)) == -5
    struct.n_boxes = n
    assert _capi.lib.copo_sim_create(C.byref(struct), 0, C.byref(h)) == 0        # ... and the table as filled is accepted
    assert _capi.lib.copo_sim_destroy(h) == 0


_KNOBS = sc.knob_cases()


@pytest.mark.parametrize("block", sc.KNOB_BLOCKS)
@pytest.mark.parametrize("name,map_name,N,kw,sigma", _KNOBS, ids=[c[0] for c in _KNOBS])
def test_config_knob_rollout_bit_exact(name, map_name, N, kw, sigma, block):
    """B: friction limit in the substep loop, respawn cooldown, other substep counts, counter-clockwise beams, other body margins,
    other mean-field / neighbour radii, rounds 2-5's Tollgate scene, and the forced LCF through copo_sim_set_force_lcf (set before
    the reset, changed, lifted, then another distribution) -- `lcf` and the LCF observation column are among the compared outputs."""
    assert "lcf" in OUT_KEYS and "obs" in OUT_KEYS
    cfg = sc.sim_config(map_name, sc.KNOB_E, N, **kw)
    _rollout("%s block %d" % (name, block), cfg, block, sc.STEPS_B, sigma, sc.KNOB_CALLS.get(name))


def test_force_lcf_out_of_range_is_refused():
    from copo_amd import _capi
    from copo_amd.sim import VecSim
    g = VecSim(sc.sim_config("intersection", 2, 12))
    with pytest.raises(_capi.CopoError) as ei:
        g.set_force_lcf(1.5)
    assert ei.value.code == -5
    g.set_force_lcf(-100.0)
    g.close()


@pytest.mark.parametrize("block", [64, -4])
def test_captured_step_bit_exact(block):
    """C: one step captured into a graph on a single stream and replayed 120 (+ 20: sim_config_cases) times with fresh actions in the static buffer.  The LCF
    mean / forced LCF / std / capacity live in device memory: a setter followed by flush() must reach the replayed launches, which
    were captured before it (capi.hip: flush_lcf)."""
    import torch
    cfg = sc.sim_config("intersection", sc.GRAPH_E, sc.GRAPH_N, horizon=sc.GRAPH_HORIZON)
    g, o = _pair(cfg, block)
    E, N = g.E, g.N
    seeds = sc.seeds(E)
    _compare("reset", g.reset(seeds), o.reset(seeds))
    rng = np.random.RandomState(3)
    static_act = torch.zeros(E, N, 2, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    t = 0
    with torch.cuda.stream(side):
        for _ in range(3):                             # eager warm-up on a side stream
            a = sc.actions(rng, E, N, t)
            static_act.copy_(torch.from_numpy(a))
            _compare("warm-up step %d" % t, g.step(static_act), o.step(a))
            t += 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(static_act)                             # (captured, not run: the simulator's state does not advance here)
    spawned_after = {40: 0, 60: 0, 80: 0}
    for r in range(sc.GRAPH_STEPS + sc.GRAPH_EXTRA):
        if r in sc.GRAPH_CALLS:
            sc.apply_calls(sc.GRAPH_CALLS, r, g, o)
            g.flush()
        a = sc.actions(rng, E, N, t)
        static_act.copy_(torch.from_numpy(a))
        graph.replay()
        oo = o.step(a)
        _compare("replay %d (block %d)" % (r, block), g.out, oo)
        for k in spawned_after:
            if r >= k:
                spawned_after[k] += int(((oo["flags"] & 64) != 0).sum())
        if r >= 80:
            assert not (oo["flags"][:, 20:] & 64).any()          # capacity 20: nobody spawns beyond it
        t += 1
    assert all(v > 0 for v in spawned_after.values()), spawned_after      # every setting was drawn from by somebody
    del graph
    g.close()
    o.close()


def test_shape_setters_call_the_weak_callbacks():
    """A holder of a captured rollout registers a weak callback in VecSim.on_shape_change: set_block and set_chunk must call it (a
    graph captured with the old shape is stale), and a holder that is gone must be dropped, not kept alive."""
    from copo_amd.sim import VecSim

    class Holder:
        calls = 0

        def reset(self):
            self.calls += 1

    g = VecSim(sc.sim_config("intersection", 2, 12))
    keep, gone = Holder(), Holder()
    g.on_shape_change.append(weakref.WeakMethod(keep.reset))
    g.on_shape_change.append(weakref.WeakMethod(gone.reset))
    g.set_block(128)
    assert (keep.calls, gone.calls) == (1, 1)
    del gone
    g.set_chunk(2)
    assert keep.calls == 2 and len(g.on_shape_change) == 1
    g.set_block(-2)
    assert keep.calls == 3
    g.close()
