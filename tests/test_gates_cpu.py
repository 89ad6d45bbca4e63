"""CPU: the restatement of the traffic gates (tests/gate_numpy.py) on cases worked out by hand, `for_map` on four maps, a rollout of the
reference's CoPO Intersection population on the CPU oracle with the premises the GPU comparison rests on, the `.npz` round trip, the
overlay, and the library surface of `copo_gate_*` (exports, ctypes binding, NULL-argument codes)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gate_cases as gc
import gate_numpy as gn
import interact_cases as ic
from copo_amd import gates
from copo_amd.sim import SimConfig

G0 = gc.HAND_GATES[0]


def test_side_rules_one_by_one():
    c = gn.crossing
    assert c(G0, 99, 45, 101, 45) == 1 and c(G0, 101, 45, 99, 45) == -1
    assert c(G0, 99, 45, 100, 45) == 1                      # cur exactly on the line counts forward
    assert c(G0, 100, 45, 99, 45) == -1                     # prev exactly on the line, moving right of A -> B: backward
    assert c(G0, 100, 45, 101, 45) == 0                     # ... moving left: nothing
    assert c(G0, 99, 50, 101, 50) == 1 and c(G0, 99, 40, 101, 40) == 1        # through the endpoints
    assert c(G0, 99, gc.Y_PAST_A, 101, gc.Y_PAST_A) == 0    # one fp32 step beyond A
    assert c(G0, 99, float(np.nextafter(np.float32(40.0), np.float32(0.0))), 101, float(np.nextafter(np.float32(40.0), np.float32(0.0)))) == 0
    assert c(G0, 100, 41, 100, 49) == 0 and c(G0, 100, 45, 100, 45) == 0 and c(G0, 99, 45, 99, 45) == 0      # along the gate, no motion
    assert c(G0, 99, 30, 101, 62) == 1 and c(G0, 99, 30, 101, 72) == 0        # oblique: y at x = 100 is 46, then 51
    nan = float("nan")
    assert c(G0, nan, 45, 101, 45) == 0 and c(G0, 99, 45, nan, 45) == 0 and c(G0, 99, nan, 101, 45) == 0
    assert [gn.speed_q(v) for v in (0.0, -3.0, 300.0, 10.001953125, 10.005859375, nan)] == [0, 0, 65280, 2560, 2562, 0]


def _hand_run(N, gates_, sections, kw, upto=gc.HAND_RECORDS):
    ref = gn.Recorder(gates_, sections, gc.HAND_E, N, **kw)
    st0, env0 = np.zeros((16, gc.HAND_E, N), np.float32), np.zeros((gc.HAND_E, 4), np.int32)
    for r in range(upto):
        ref.set_groups(gc.hand_groups(kw["groups"], r))
        ref.record(*gc.hand_record(st0, env0, r))
    return ref


def test_hand_sequence_gives_the_counts_worked_out_by_hand():
    """agent-id change, episode change, ALIVE -> WRECK -> ALIVE, NaN, two and three slots crossing one gate in one record (headway 0),
    headway and travel-time clipping, tt = 0 when gate_in = gate_out, a group out of range whose memory is kept"""
    ref = _hand_run(7, gc.HAND_GATES, gc.HAND_SECTIONS, gc.HAND_KW)
    for k in gn.RAW:
        assert np.array_equal(getattr(ref, k), gc.HAND_EXPECTED[k]), (k, getattr(ref, k).tolist(), gc.HAND_EXPECTED[k].tolist())
    assert ref.max_crossings_of_a_gate_in_a_scene_record == 3
    # G = 1 with scene 3 out of range throughout: the sum over the three groups less what scene 3 added to group 2
    one = _hand_run(7, gc.HAND_GATES, gc.HAND_SECTIONS, dict(gc.HAND_KW, groups=1))
    gc.check_invariants(one)                                 # (they hold per group while no scene changes its group)
    assert one.count.tolist() == [[[4 * 2 + 2 + 0, 2 * 2 + 1 + 1], [3 * 2, 0]]] and one.scene_records.tolist() == [24] and one.alive.tolist() == [42 * 2 + 34 + 12]


def test_forget_and_reset():
    ref = _hand_run(7, gc.HAND_GATES, gc.HAND_SECTIONS, gc.HAND_KW, upto=1)
    ref.forget()                                             # record 1 would count three forward crossings of gate 0 in scene 0
    st0, env0 = np.zeros((16, gc.HAND_E, 7), np.float32), np.zeros((gc.HAND_E, 4), np.int32)
    ref.record(*gc.hand_record(st0, env0, 1))
    assert ref.count.sum() == 0 and ref.scene_records.tolist() == [4, 2, 2] and ref.r == 2
    ref.record(*gc.hand_record(st0, env0, 2))                # followed again: slot 6 of scene B and slot 0 of scene C go back
    assert ref.count.sum() == 2 and ref.count[1:, 0, 1].tolist() == [1, 1]
    ref.reset()
    assert ref.r == 0 and all(getattr(ref, k).sum() == 0 for k in gn.RAW) and ref.group.tolist() == [0, 1, 2, 3, 0]


def test_padded_tables_cross_a_lot():
    """the launch-limit cases of the GPU test are not empty: 32 gates, 64 sections, 64 slots"""
    ref = _hand_run(64, gc.padded_gates(32), gc.padded_sections(64, 32), gc.HAND_KW)
    gc.check_invariants(ref)
    assert (ref.count.sum((0, 2)) > 0).all() and ref.sec_count.sum() > 20 and ref.count[:, :, 1].sum() > 20
    assert ref.max_crossings_of_a_gate_in_a_scene_record >= 3 and ref.headway[:, :, 1:].sum() > 0


@pytest.mark.parametrize("name", ["intersection", "roundabout", "bottleneck", "tollgate"])
def test_for_map_gates(name):
    from copo_amd import maps
    t = SimConfig(map=name).tables()
    g, sections, route_section = gates.gates_for_map(t, inset=10.0)
    assert g.dtype == np.float32 and np.isfinite(g).all() and 1 <= len(g) <= 32 and len(sections) <= 64
    assert len(route_section) == t.n_routes and all(0 <= s < len(sections) for s in route_section)      # every route owns exactly one section
    assert len(set(sections)) == len(sections) and set(route_section) == set(range(len(sections)))
    for i in range(len(g)):                                  # merged: no two gates agree to 1 cm
        for j in range(i):
            assert np.abs(g[i].astype(np.float64) - g[j]).max() > 0.01, (i, j)
    w = t.lane_width
    for r in range(t.n_routes):
        total = float(t.route_meta[r, 0])
        gi, go = sections[route_section[r]]
        pts = maps.route_points(t, r, step=0.5)
        for gate, s in ((g[gi], 10.0), (g[go], total - 10.0)):
            (x, y, th), lanes = gates.route_pose(t, r, s)
            d = gate[2:].astype(np.float64) - gate[:2]
            # perpendicular to the route: the gate runs along the route's right-hand normal
            off = np.arctan2(d[1], d[0]) - (th - np.pi / 2)
            assert abs((off + np.pi) % (2 * np.pi) - np.pi) < 1e-4, (r, s, off)
            assert abs(np.hypot(*d) - (lanes * w + 1.0)) < 1e-3
            # forward along the route: route points just before the gate have side < 0, those after it side >= 0
            ahead = (pts[:, 0] - x) * np.cos(th) + (pts[:, 1] - y) * np.sin(th)
            near = np.hypot(pts[:, 0] - x, pts[:, 1] - y) < 4.0
            before, after = pts[near & (ahead < -0.2)], pts[near & (ahead > 0.2)]
            assert len(before) and len(after) and (gates.side(gate, before) < 0).all() and (gates.side(gate, after) >= 0).all(), (r, s)
            assert gn.crossing(gate, before[-1][0], before[-1][1], after[0][0], after[0][1]) == 1
    if name == "intersection":
        assert len(g) == 8 and len(sections) == 16
    with pytest.raises(ValueError):
        gates.gates_for_map(t, inset=0.5 * float(t.route_meta[:, 0].min()))


def test_for_map_refuses_more_than_the_limits():
    t = SimConfig(map="parkinglot").tables()
    try:
        g, s, _ = gates.gates_for_map(t, inset=2.0)
        assert len(g) <= 32 and len(s) <= 64
    except ValueError as err:
        assert "by hand" in str(err)


@pytest.fixture(scope="module")
def oracle_rollout(golden_dir):
    import oracle_lib as ol
    cfg = gc.rollout_config()
    o = ol.OracleSim(cfg)
    try:
        g, sections, _ = gc.rollout_gates(cfg)
        ref = gn.Recorder(g, sections, o.E, o.N, **gc.ROLLOUT_KW)
        ref.set_groups(gc.ROLLOUT_GROUPS)
        out, act = o.reset(), ic.rollout_policy(golden_dir)
        ref.record(*o.get_state())
        for t in range(gc.ROLLOUT_STEPS):
            out = o.step(act(out["obs"]))
            ref.record(*o.get_state())
        return ref
    finally:
        o.close()


def test_rollout_invariants_and_premises(oracle_rollout):
    ref = oracle_rollout
    gc.check_invariants(ref)
    gc.check_premises(ref)
    print("forward %s backward %s; sections %s; headway bins %s; first crossings %d; most crossings of a gate in a scene-record %d"
          % (ref.count[:, :, 0].sum(0).tolist(), ref.count[:, :, 1].sum(0).tolist(), ref.sec_count.sum(0).tolist(), ref.headway.sum((0, 1)).tolist(),
             ref.first_crossings, ref.max_crossings_of_a_gate_in_a_scene_record))
    assert ref.scene_records.tolist() == [3 * (gc.ROLLOUT_STEPS + 1), 2 * (gc.ROLLOUT_STEPS + 1)] and (ref.count[:, :, 0].sum(1) > 0).all()
    d = gates.derive(ref.raw(), 0.1)
    assert np.nanmax(d["mean_speed"]) > 1.0 and np.nanmin(d["mean_travel_s"]) > 5.0 and (d["density"] > 5).all()


def test_derive_and_npz_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    G, L, S, T, HB, TB = 2, 3, 2, 4, 5, 6
    raw = {k: rng.randint(0, 50, shp).astype(np.int64) for k, shp in gates.shapes(G, L, S, T, HB, TB).items()}
    raw["scene_records"][:] = (40, 0)
    raw["count"][0, 0, 0], raw["count"][0, 1, 0], raw["sec_count"][0, 1], raw["sec_count"][0, 0] = 0, 7, 0, 3
    block = np.concatenate([raw[k].reshape(-1) for k in gates.RAW])
    assert gates.RAW == gn.RAW and all(np.array_equal(v, raw[k]) for k, v in gates.split(block, G, L, S, T, HB, TB).items())
    d = gates.derive(raw, 0.1)
    assert set(d) == set(gates.RAW) | set(gates.DERIVED)
    assert d["flow_per_hour"][0, 1, 1] == raw["count"][0, 1, 1] / (40 * 0.1) * 3600.0 and np.isnan(d["flow_per_hour"][1]).all()
    assert np.isnan(d["mean_speed"][0, 0, 0]) and d["mean_speed"][0, 1, 0] == raw["speed_q"][0, 1, 0] / 256.0 / raw["count"][0, 1, 0]
    assert np.isnan(d["mean_travel_s"][0, 1]) and d["mean_travel_s"][0, 0] == raw["sec_sum"][0, 0] / raw["sec_count"][0, 0] * 0.1
    assert np.allclose(d["headway_s"], np.arange(HB) * 0.1) and d["density"][0] == raw["alive"][0] / 40.0 and np.isnan(d["density"][1])
    d["meta"] = dict(gates=[[0.0, 1.0, 2.0, 3.5]] * L, sections=[[0, 1], [2, 2]], groups=G, bins=[T, 7], headway_bins=HB, tt_bins=[TB, 10],
                     route_section=None, n_records=9, dt=0.1, num_agents=30, sim_config=dataclasses.asdict(SimConfig(map="roundabout", num_envs=2)))
    path = gates.save(str(tmp_path / "gates.npz"), d)
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(gates.RAW + ("meta",))
    back = gates.load(path)
    assert back["meta"] == d["meta"] and SimConfig(**back["meta"]["sim_config"]).map == "roundabout"
    for k in gates.RAW + gates.DERIVED:
        assert np.array_equal(back[k], d[k], equal_nan=True), k


def test_gate_overlay_draws_the_line_and_the_forward_tick():
    """16 x 16 frame at 0.5 m per pixel centred on (4, 4): x = 4 is the border of columns 7 | 8 (column 8 holds it), y = 1 .. 7 are rows
    14 .. 2.  The gate (4, 7) -> (4, 1) runs down: forward is +x, the tick runs from (4, 4) to (6, 4): row 8 (y = 4 is the border 7 | 8,
    row 8 holds it), columns 8 .. 12."""
    frame = np.full((16, 16, 4), 100, np.uint8)
    out = gates.gate_overlay(frame, (4.0, 4.0, 0.5), [(4.0, 7.0, 4.0, 1.0)])
    assert out.shape == (16, 16, 3) and out.dtype == np.uint8 and (frame == 100).all()
    line = (out == gates.GATE_COLOUR).all(-1)
    tick = (out == gates.TICK_COLOUR).all(-1)
    assert line[:, 8].sum() >= 12 and line.sum() == line[:, 8].sum() and line[2, 8] and line[13, 8]
    assert tick[8, 9:13].all() and tick.sum() == tick[8].sum() and not tick[8, :8].any()
    assert ((out != 100).any(-1) == (line | tick)).all()
    # a gate outside the frame leaves it alone
    assert (gates.gate_overlay(frame, (4.0, 4.0, 0.5), [(100.0, 7.0, 100.0, 1.0)]) == 100).all()


def test_library_exports_and_binds_the_gate_entries():
    from copo_amd import _capi
    names = ["copo_gate_create", "copo_gate_set_groups", "copo_gate_record", "copo_gate_read", "copo_gate_forget", "copo_gate_reset",
             "copo_gate_destroy", "copo_gate_words"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    assert C.sizeof(_capi.GateCfg) == 32 and [f[0] for f in _capi.GateCfg._fields_] == ["L", "S", "G", "T", "bin_records", "HB", "TB", "tt_bin"]
    assert (_capi.GATE_MAX_GATES, _capi.GATE_MAX_SECTIONS, _capi.GATE_MAX_GROUPS, _capi.GATE_MAX_BINS, _capi.GATE_MAX_HIST) == \
        (gates.MAX_GATES, gates.MAX_SECTIONS, gates.MAX_GROUPS, gates.MAX_BINS, gates.MAX_HIST)
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    cfg = _capi.GateCfg(2, 3, 3, 2, 3, 3, 2, 2)
    assert _capi.lib.copo_gate_words(C.byref(cfg)) == sum(int(np.prod(s)) for s in gates.shapes(3, 2, 3, 2, 3, 2).values())
    assert _capi.lib.copo_gate_words(None) == 0
    # NULL arguments are refused before any device call
    h, g = C.c_void_p(), np.zeros((2, 4), np.float32)
    assert _capi.lib.copo_gate_create(None, C.byref(cfg), g.ctypes.data, None, C.byref(h)) == -1 and b"copo_gate_create" in _capi.lib.copo_last_error()
    for fn, args in (("copo_gate_set_groups", (None, None, None)), ("copo_gate_record", (None, None)), ("copo_gate_read", (None, None, None, None)),
                     ("copo_gate_forget", (None, None)), ("copo_gate_reset", (None, None)), ("copo_gate_destroy", (None,))):
        assert getattr(_capi.lib, fn)(*args) == -1 and fn.encode() in _capi.lib.copo_last_error(), fn
