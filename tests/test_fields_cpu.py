"""CPU: the restatement of the traffic field maps (tests/field_numpy.py) on cases worked out by hand, the last-seen rule on a hand-made
flag sequence, stride and group routing, `heat_overlay`, the `.npz` round trip, the library surface of `copo_field_*` (exports, ctypes
binding, NULL-argument codes), and the share of ambiguous footprint pairs of the GPU test's cases, measured on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import field_cases as fc
import field_numpy as fn
import interact_cases as ic
from copo_amd import fields

ALIVE, WRECK, EMPTY = fc.ALIVE, fc.WRECK, fc.EMPTY
DONE, ARRIVE, CRASH, OUT = fn.F_DONE, fn.F_ARRIVE, fn.F_CRASH, fn.F_OUT


def _state(E, N, rows):
    """State block [16][E][N] from {(e, n): (x, y, heading, speed, status)}"""
    st = np.zeros((16, E, N), np.float32)
    for (e, n), body in rows.items():
        ic.put(st, e, n, body, 10 * e + n)
    return st


@pytest.mark.parametrize("case", sorted(fc.HAND_CASES))
def test_hand_cases(case):
    grid = fn.Grid(**fc.HAND_GRID)
    bodies = fc.HAND_CASES[case][0]
    ref = fn.Recorder(grid, 1, len(bodies), fc.HL, fc.HW)
    ref.record(_state(1, len(bodies), {(0, n): b for n, b in enumerate(bodies)}))
    want = fc.expected_maps(case, grid)
    assert ref.ambiguous_pairs == 0
    assert np.array_equal(ref.lo[0], want), {fn.LAYERS[k]: np.argwhere(ref.lo[0, k] != want[k]).tolist() for k in range(10)}
    assert np.array_equal(ref.hi[0], want[:2]) and ref.scene_records.tolist() == [1]
    assert ref.sure_pairs == want[0].sum() + want[1].sum()


def test_quantisation_rounds_half_to_even_in_float32():
    v = np.array([0.0, -3.0, 300.0, 10.001953125, 10.005859375, 255.0, 1e-4], np.float32)
    assert fn.speed_q(v).tolist() == [0, 0, 65280, 2560, 2562, 65280, 0]
    vx, vy = fn.velocity_q(np.array([-3.0, 300.0, -300.0, 4.0]), np.array([0.0, 0.0, 0.0, np.pi / 2]))
    assert vx.tolist() == [-768, 65280, -65280, 0] and vy.tolist() == [0, 0, 0, 1024]
    # a centre on a cell border belongs to the cell above it (all of these are exact in float32)
    g = fn.Grid(-63.375, 0.0, 8, 8, 0.5)
    ix, iy, inside = fn.centre_cells(np.array([-63.375, -62.875, -63.38, -59.375], np.float32), np.array([0.0, 3.999, -0.0, 4.0], np.float32), g)
    assert inside.tolist() == [True, True, False, False] and ix[:2].tolist() == [0, 1] and iy[:2].tolist() == [0, 7]
    assert float(g.inv) == 2.0 and float(fn.Grid(0, 0, 1, 1, 0.3).inv) == float(np.float32(1.0 / np.float64(np.float32(0.3))))


def test_last_seen_rule_through_slot_reuse_and_scene_reset():
    """One scene, two slots; slot 1 drives along undisturbed.  Slot 0: seen at cell (10, 10); crashes, and the step kernel has already put
    a new agent into the slot at (110.5, 45.5): the crash belongs to (10, 10).  That agent moves to (21, 15) and ends with OUT and ARRIVE
    set: one count each, there.  A DONE of a slot that was EMPTY in the record before counts nowhere; the record after a scene reset has
    no flags; after `forget()` a DONE counts nowhere either."""
    grid = fn.Grid(**fc.HAND_GRID)
    ref = fn.Recorder(grid, 1, 2, fc.HL, fc.HW, stride=2)
    other = (95.5, 33.5, 0.0, 1.0, ALIVE)

    def rec(body0, f0):
        flags = None if f0 is None else np.array([[f0, 1]], np.uint8)
        ref.record(_state(1, 2, {(0, 0): body0, (0, 1): other}), flags)
    rec((100.5, 40.5, 0.0, 5.0, ALIVE), None)                   # record 0 (accumulates)
    rec((110.5, 45.5, 0.0, 5.0, ALIVE), 1 | DONE | CRASH)       # 1: the successor is already in the slot
    rec((111.5, 45.5, 0.0, 5.0, ALIVE), 1)                      # 2 (accumulates)
    rec((111.5, 45.5, 0.0, 0.0, EMPTY), 1 | DONE | OUT | ARRIVE)  # 3
    rec((111.5, 45.5, 0.0, 0.0, EMPTY), DONE | CRASH)           # 4 (accumulates): the slot was EMPTY in record 3
    rec((92.5, 47.5, 0.0, 5.0, ALIVE), None)                    # 5: after a scene reset
    ref.forget()
    rec((93.5, 47.5, 0.0, 5.0, ALIVE), 1 | DONE | CRASH)        # 6 (accumulates)
    crash, out, arrive, visits = (ref.lo[0, fn.L[k]] for k in ("crash", "out", "arrive", "visits"))
    assert crash.sum() == 1 and crash[10, 10] == 1
    assert out.sum() == 1 and out[15, 21] == 1 and arrive.sum() == 1 and arrive[15, 21] == 1
    # stride 2: records 0, 2, 4, 6 accumulate; slot 0 is ALIVE in 0, 2, 6, slot 1 in all four -- events counted in the odd records too
    assert ref.scene_records.tolist() == [4] and visits.sum() == 7
    assert visits[10, 10] == 1 and visits[15, 21] == 1 and visits[17, 3] == 1 and visits[3, 5] == 4


def test_stride_and_group_routing():
    """Three scenes with the same body; groups (1, -1, 0) of G = 2, then (0, 2, 0): a group outside 0..G-1 adds nothing, not even an
    event, but its slots are still remembered -- the event fires once the scene is routed again."""
    grid = fn.Grid(**fc.HAND_GRID)
    ref = fn.Recorder(grid, 3, 1, fc.HL, fc.HW, groups=2, stride=3)
    st = _state(3, 1, {(e, 0): (100.5, 40.5, 0.0, 2.0, ALIVE) for e in range(3)})
    crash = np.full((3, 1), 1 | DONE | CRASH, np.uint8)
    ref.set_groups([1, -1, 0])
    ref.record(st)
    for _ in range(3):
        ref.record(st, crash)
    assert ref.scene_records.tolist() == [2, 2]                              # records 0 and 3, one scene each
    assert [int(ref.lo[g, fn.L["visits"], 10, 10]) for g in (0, 1)] == [2, 2]
    assert [int(ref.lo[g, fn.L["crash"], 10, 10]) for g in (0, 1)] == [3, 3]   # every record with flags, whatever the stride
    assert ref.lo[:, fn.L["occupancy"]].sum() == 4 * 5
    ref.set_groups([0, 2, 0])
    ref.record(st, crash)                                                    # record 4: no accumulation
    assert [int(ref.lo[g, fn.L["crash"], 10, 10]) for g in (0, 1)] == [5, 3] and ref.scene_records.tolist() == [2, 2]
    ref.set_groups([0, 1, 0])
    ref.record(st, crash)                                                    # scene 1 was remembered while it was switched off
    assert [int(ref.lo[g, fn.L["crash"], 10, 10]) for g in (0, 1)] == [7, 4]


def test_heat_overlay_on_a_4x4_map():
    """4 x 4 cells of 2 m from (10, 20) under a 16 x 16 frame at 0.5 m per pixel centred on the grid's middle (14, 24): a cell is 4 x 4
    pixels, pixel row 0 is the TOP (y = 27.75: cell row 3).  lo = 1, hi = 4 by default: value 1 -> t = 0 -> (40, 60, 200); 4 -> t = 1 ->
    (220, 40, 40); 2.5 -> t = 0.5 -> half way between stops 1 and 2: (140, 210, 120).  On grey 100 with alpha 160:
    (100 x 96 + c x 160) >> 8."""
    lay = np.zeros((4, 4))
    lay[0, 0], lay[3, 3], lay[1, 2], lay[2, 0] = 1.0, 4.0, 2.5, np.nan
    frame = np.full((16, 16, 4), 100, np.uint8)
    out = fields.heat_overlay(frame, lay, (14.0, 24.0, 0.5), grid=(10.0, 20.0, 2.0))
    assert out.shape == (16, 16, 3) and out.dtype == np.uint8 and (frame == 100).all()

    def mix(c):
        return [(100 * 96 + v * 160) >> 8 for v in c]
    assert out[15, 0].tolist() == mix((40, 60, 200)) and out[12, 3].tolist() == mix((40, 60, 200))           # cell (0, 0): bottom left
    assert out[0, 15].tolist() == mix((220, 40, 40)) and out[3, 12].tolist() == mix((220, 40, 40))           # cell (3, 3): top right
    assert out[8, 8].tolist() == mix((140, 210, 120)) and out[11, 11].tolist() == mix((140, 210, 120))       # cell (2, 1)
    painted = (out != 100).any(-1)
    assert painted.sum() == 3 * 16                                                                       # zeros and NaN untouched
    # a frame larger than the grid: pixels outside stay; fixed bounds clip
    big = fields.heat_overlay(np.full((32, 32, 3), 100, np.uint8), lay, (14.0, 24.0, 0.5), lo=2.0, hi=3.0, grid=(10.0, 20.0, 2.0))
    assert (big != 100).any(-1).sum() == 3 * 16 and big[8 + 15, 8].tolist() == mix((40, 60, 200)) and big[8, 8 + 15].tolist() == mix((220, 40, 40))
    with pytest.raises(ValueError):
        fields.heat_overlay(frame, lay, (14.0, 24.0, 0.5))


def test_npz_round_trip_and_derived_arrays(tmp_path):
    rng = np.random.RandomState(0)
    maps = rng.randint(0, 50, (2, 10, 3, 4)).astype(np.int64)
    maps[:, 4:6] -= 25
    maps[0, 2, 0, 0], maps[1, 2, 2, 3] = 0, 5
    rec = np.array([7, 0], np.int64)
    d = fields.derive(maps, rec, 0.1)
    assert set(d) == set(fields.LAYERS) | set(fields.DERIVED) | {"scene_records"} and fields.LAYERS == fn.LAYERS
    assert np.isnan(d["mean_speed"][0, 0, 0]) and np.isnan(d["flow"][0, :, 0, 0]).all()
    assert d["mean_speed"][1, 2, 3] == maps[1, 3, 2, 3] / 256.0 / maps[1, 2, 2, 3] and d["flow"].shape == (2, 2, 3, 4)
    assert d["flow"][1, 1, 2, 3] == maps[1, 5, 2, 3] / 256.0 / maps[1, 2, 2, 3]
    assert np.allclose(d["occupancy_s"], maps[:, 0] * 0.1) and np.allclose(d["occupancy_frac"][0], maps[0, 0] / 7.0)
    assert np.isnan(d["occupancy_frac"][1]).all()
    from copo_amd.sim import SimConfig
    import dataclasses
    d["meta"] = dict(x0=-63.37, y0=1.5, cell=0.5, W=4, H=3, groups=2, ttc_below=1.5, stride=3, n_records=9, dt=0.1, num_agents=30,
                     sim_config=dataclasses.asdict(SimConfig(map="roundabout", num_envs=2)))
    path = fields.save(str(tmp_path / "maps.npz"), d)
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["maps", "meta", "scene_records"]
    back = fields.load(path)
    assert back["meta"] == d["meta"] and SimConfig(**back["meta"]["sim_config"]).map == "roundabout"
    for k in fields.LAYERS + fields.DERIVED + ("scene_records",):
        assert np.array_equal(back[k], d[k], equal_nan=True), k


def test_grid_for_map_covers_the_road_tables():
    from copo_amd import maps
    from copo_amd.sim import SimConfig
    t = SimConfig(map="intersection").tables()
    xa, xb, ya, yb = maps.bounding_box(t)
    for cell in (1.0, 0.5):
        x0, y0, W, H = fields.grid_for_map(t, cell=cell, margin=5.0)
        assert x0 == xa - 5.0 and y0 == ya - 5.0 and x0 + W * cell >= xb + 5.0 > x0 + (W - 1) * cell and y0 + H * cell >= yb + 5.0
    with pytest.raises(ValueError):
        fields.grid_for_map(t, cell=0.05)


def test_library_exports_and_binds_the_field_entries():
    from copo_amd import _capi
    names = ["copo_field_create", "copo_field_set_groups", "copo_field_record", "copo_field_read", "copo_field_forget", "copo_field_reset",
             "copo_field_destroy"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS and getattr(_capi.lib, name).restype is C.c_int
    assert C.sizeof(_capi.FieldCfg) == 28 and [f[0] for f in _capi.FieldCfg._fields_] == ["x0", "y0", "cell", "W", "H", "G", "ttc_below"]
    assert (_capi.FIELD_LAYERS, _capi.FIELD_MAX_SIDE, _capi.FIELD_MAX_GROUPS) == (len(fields.LAYERS), fields.MAX_SIDE, fields.MAX_GROUPS)
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    # NULL arguments are refused before any device call
    h, cfg = C.c_void_p(), _capi.FieldCfg(0.0, 0.0, 1.0, 8, 8, 1, 0.0)
    assert _capi.lib.copo_field_create(None, C.byref(cfg), C.byref(h)) == -1
    assert b"copo_field_create" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_set_groups(None, None, None) == -1 and b"copo_field_set_groups" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_record(None, None, None, 1, None) == -1 and b"copo_field_record" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_read(None, None, None, None) == -1 and b"copo_field_read" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_forget(None, None) == -1 and b"copo_field_forget" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_reset(None, None) == -1 and b"copo_field_reset" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_field_destroy(None) == -1 and b"copo_field_destroy" in _capi.lib.copo_last_error()


def test_chosen_cases_stay_under_the_ambiguity_cap(golden_dir):
    """The cases of the GPU comparison (tests/test_gpu_fields.py), by the restatement alone: ambiguous (body, cell) pairs are at most 1 %
    of the sure pairs of every case -- a condition on the cases, not a tolerance; geometry predicts about 0.3 % at 1 m cells -- and the
    rollout (here on the CPU oracle, which the HIP simulator matches bit for bit) has what it is meant to have: crashes, wrecks, slots
    taken over inside an episode and scene resets."""
    import oracle_lib as ol
    share = {}
    for N, seeds in ((64, ic.RANDOM_SEEDS_64), (7, ic.RANDOM_SEEDS_7)):
        for seed, aligned in seeds:
            st = ic.random_state(np.zeros((16, 5, N), np.float32), seed, aligned)
            for k, gk in enumerate(fc.RANDOM_GRIDS[N]):
                ref = fn.Recorder(fn.Grid(**gk), 5, N, fc.HL, fc.HW, groups=3)
                ref.set_groups(fc.RANDOM_GROUPS)
                ref.record(st)
                assert ref.sure_pairs >= 40 and ref.ambiguous_pairs <= 0.01 * ref.sure_pairs, (N, seed, aligned, k, ref.sure_pairs, ref.ambiguous_pairs)
                assert ref.lo[:, fn.L["visits"]].sum() > 0 and ref.lo[:, fn.L["wreck"]].sum() > 0
                share["%d/%d%s/%d" % (N, seed, "a" if aligned else "", k)] = (ref.ambiguous_pairs, ref.sure_pairs)
    cfg = fc.rollout_config()
    o = ol.OracleSim(cfg)
    try:
        recs = []
        for gk, groups, stride in fc.rollout_grids(cfg):
            r = fn.Recorder(fn.Grid(**gk), o.E, o.N, cfg.veh_half_len, cfg.veh_half_wid, groups=groups, stride=stride)
            r.set_groups(fc.ROLLOUT_GROUPS if groups > 1 else np.zeros(o.E))
            recs.append(r)
        out, act = o.reset(), ic.rollout_policy(golden_dir)
        for r in recs:
            r.record(o.get_state()[0])
        agents_of, episodes = {}, set()
        for t in range(fc.ROLLOUT_STEPS):
            out = o.step(act(out["obs"]))
            st, env = o.get_state()
            for r in recs:
                r.record(st, out["flags"])
            si = st.view(np.int32)
            for e, n in zip(*np.nonzero((si[13] & 0xFF) == ALIVE)):
                agents_of.setdefault((e, int(env[e, 1]), n), set()).add(int(si[14, e, n]))
            episodes |= {(e, int(env[e, 1])) for e in range(o.E)}
        for r in recs:
            assert r.ambiguous_pairs <= 0.01 * r.sure_pairs, (r.ambiguous_pairs, r.sure_pairs)
            share["rollout %.1f m" % float(r.grid.cell)] = (r.ambiguous_pairs, r.sure_pairs)
            for k in ("crash", "wreck", "visits"):
                assert r.lo[:, fn.L[k]].sum() > 0, k
        print({k: "%d / %d = %.2f %%" % (a, s, 100.0 * a / s) for k, (a, s) in share.items()})
        assert sum(len(v) > 1 for v in agents_of.values()) >= 1, "no slot was taken over inside an episode"
        assert len(episodes) >= 2 * o.E, "not every scene was reset"
    finally:
        o.close()
