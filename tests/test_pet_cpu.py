"""CPU: the restatement of the encroachment log (tests/pet_numpy.py) on the sequences worked out by hand, its fp32 footprint against the
float64 one of tests/field_numpy.py, the type thresholds, two rollouts on the CPU oracle with the premises the GPU comparison rests on,
the overflow rule, `decode` / `summary` / `join` / `of` by hand, the `.npz` round trips, the cell-width check and the library surface of
`copo_pet_*` (exports, ctypes binding, NULL / DIM / CONFIG codes)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import field_numpy as fn
import pet_cases as pc
import pet_numpy as pn
from copo_amd import encroach, trips
from copo_amd.sim import SimConfig


def _hand(N, **kwargs):
    ref = pc.hand_log(N, **kwargs)
    pc.run_hand(N, lambda r, st, env: ref.record(st, env), ref.forget)
    return ref


@pytest.mark.parametrize("N", [7, 64])
def test_hand_sequence_gives_the_rows_written_out_by_hand(N):
    """a perpendicular crossing with PET 3; a follower entering its leader's stamps; a second touch of the same partner; two new partners
    in one record; the earlier agent gone before the second comes; a slot turnover that clears the bit in its own and in another slot's
    mask; an episode change that voids the stamps; r - q == window and window + 1; two bodies over one cell centre in one record; bodies
    half outside the grid; `forget()`; N = 64 adds lanes 62 and 63 and a low lane with a partner in lane 63"""
    ref = _hand(N)
    got, want = ref.rows(), pc.hand_expected(N)
    assert (ref.n_rows, ref.dropped) == (len(want), 0) and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want).tolist()
    assert ref.r == pc.HAND_RECORDS and ref.second_touches == 5 and ref.turnovers_in_window == 1
    pc.check_invariants(ref)
    if N == 7:
        assert ref.hist[0].tolist() == pc.HAND_HIST
        assert {(int(x), int(y)): int(ref.critical[0, y, x]) for y, x in np.argwhere(ref.critical[0])} == pc.HAND_CRITICAL_MAP
    # the stamp kept where two bodies cover one cell centre in one record is the larger word: agent 26 in slot 6, heading up
    assert int(ref.stamps[1, 25 * 32 + 14]) == pn.stamp(pc.HAND_RECORDS - 1, 26, 64, 6) > pn.stamp(pc.HAND_RECORDS - 1, 25, 0, 5)
    # a body half outside the grid stamps the cells that exist: rows 29 .. 31 of column 4 in scene 0, columns 0 .. 1 of row 5 in scene 1 (the
    # follower went on over them)
    assert [int(w) & 0xFF for w in ref.stamps[0, [29 * 32 + 4, 30 * 32 + 4, 31 * 32 + 4]]] == [5, 5, 5] and int(ref.stamps[0, 28 * 32 + 4]) >> 32 == 1
    assert [int(w) >> 32 for w in ref.stamps[1, [5 * 32, 5 * 32 + 1]]] == [3, 3]
    # `forget` set every epoch to 10 and cleared the masks; scene 2's episode change had set its epoch to 8
    assert ref.epoch.tolist()[:3] == [10, 10, 10] and int(ref.met[1, 5]) == 1 << 6 and int(ref.met[2, 4]) == 0
    d = encroach.decode(got, 0.1, (0.0, 0.0, 1.0, 32))
    assert d["pet_s"][d["rec"] == 3][0] == pytest.approx(0.3) and set(d["type"]) == {"following", "crossing"}


def test_episode_change_alone_voids_and_forget_alone_voids():
    ref = pc.hand_log(7)
    pc.run_hand(7, lambda r, st, env: ref.record(st, env), ref.forget, upto=9)
    assert ref.epoch.tolist() == [0, 0, 8] and ref.rows()[-1].tolist()[:2] == [1, 5 | (6 << 6)]      # record 8: (8, 28) of scene 2 gave no row
    other = _hand(7)
    assert other.n_rows == ref.n_rows + 2


def test_fp32_footprint_agrees_with_the_float64_one_and_fm_is_exact():
    """every sure cell of tests/field_numpy.py is in C(n), nothing outside its ambiguous band is; `fm` against exact rational arithmetic"""
    from fractions import Fraction
    rng = np.random.RandomState(5)
    g = fn.Grid(-3.0, 2.0, 40, 36, 1.0)
    for _ in range(300):
        x, y, th = np.float32(rng.uniform(-8, 44)), np.float32(rng.uniform(-4, 42)), np.float32(rng.uniform(-3.2, 3.2))
        sure, amb = fn.footprint(x, y, th, g, pc.HL, pc.HW)
        c = set(pn.cells(x, y, th, g, pc.HL, pc.HW).tolist())
        lo, hi = set((sure[0] * g.W + sure[1]).tolist()), set((amb[0] * g.W + amb[1]).tolist())
        assert lo <= c <= lo | hi
    for _ in range(2000):
        a, b, c = (np.float32(v) for v in rng.standard_normal(3) * 10.0 ** rng.randint(-3, 4, 3))
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        got = float(pn.fm(a, b, c))
        lo, hi = float(np.nextafter(np.float32(got), np.float32(-np.inf))), float(np.nextafter(np.float32(got), np.float32(np.inf)))
        assert abs(exact - Fraction(got)) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi)))
    s, c = pn.sincos_det(np.float32(0.0))
    assert (float(s), float(c)) == (0.0, 1.0) and float(pn.sincos_det(np.float32(np.pi / 2))[0]) == 1.0
    for th in rng.uniform(-7, 7, 200):
        s, c = pn.sincos_det(np.float32(th))
        assert abs(float(s) - np.sin(np.float64(np.float32(th)))) < 3e-7 and abs(float(c) - np.cos(np.float64(np.float32(th)))) < 3e-7


def test_type_thresholds_and_heading_quantisation():
    for d, want in ((0, 0), (21, 0), (22, 1), (64, 1), (106, 1), (107, 2), (128, 2)):
        for hq_a in (0, 5, 200, 255):
            for sign in (1, -1):
                hq_b = (hq_a + sign * d) & 255
                assert pn.type_index(hq_a, hq_b) == want == int(encroach.type_index(hq_a, hq_b)), (d, hq_a, sign)
    assert (encroach.FOLLOW_Q, encroach.OPPOSE_Q) == (pn.FOLLOW_Q, pn.OPPOSE_Q) == (21, 107)      # 30 deg = 21.3 steps, 150 deg = 106.7
    assert [pn.heading_q(v) for v in (0.0, np.pi / 2, np.pi, -np.pi / 2, -np.pi, 2 * np.pi, 0.012, 0.0123)] == [0, 64, 128, 192, 128, 0, 0, 1]
    assert pn.stamp(0, 0, 0, 0) == 1 << 32 and pn.stamp(6, 0x12345, 200, 63) == (7 << 32) | (0x2345 << 16) | (200 << 8) | 63


def _table():
    cfg = SimConfig(map="intersection", num_envs=3, num_agents=7)
    meta = encroach.pet_meta(cfg, 7, (0.0, 0.0, 1.0, 32, 32), pc.HAND_WINDOW, pc.HAND_CRITICAL, 1, 100, dropped=3, n_records=12)
    return encroach.EncroachmentTable(pc.hand_expected(7), meta)


def test_decode_summary_of_join_and_npz_round_trip(tmp_path):
    t = _table()
    assert len(t) == 13 and len(encroach.ROW_KEYS) == encroach.WORDS == 16
    assert t.slot_b.tolist()[:4] == [4, 4, 1, 1] and t.slot_a.tolist()[:4] == [5, 6, 0, 0] and t.aid_b.tolist()[:4] == [14, 14, 21, 31]
    assert t.pet.tolist() == [2, 2, 2, 2, 3, 2, 4, 2, 4, 2, 1, 1, 1] and np.allclose(t.pet_s, t.pet * 0.1) and t.episode.tolist()[-2] == 6
    assert t.cell_xy[0].tolist() == [4.5, 26.5] and t.cell_xy[4].tolist() == [10.5, 10.5] and t.n_cells.tolist()[2] == 2 and t.n_cells.tolist()[8] == 3
    assert t.type.tolist() == ["crossing", "crossing", "following", "crossing", "crossing", "crossing", "crossing", "crossing", "following", "crossing",
                               "crossing", "crossing", "crossing"]
    assert t.second[2].tolist() == [1, 21, 0] and t.first[2].tolist() == [1, 20, 0]
    # speeds: 1 + slot + rec / 4 of the record of the encounter, both parties; the pose is b's
    assert t.speed_b[4] == 1 + 1 + 0.75 and t.speed_a[4] == 1 + 0 + 0.75 and t.pose_b[4].tolist() == [10.5, 8.5, float(np.float32(np.pi / 2)), 2.75]
    s = t.summary()
    assert [(r["type"], r["band"], r["count"]) for r in s] == [("following", (0.0, 0.5), 2), ("crossing", (0.0, 0.5), 11)]
    assert s[0]["pet_s"] == pytest.approx(0.3) and s[1]["share"] == 11 / 13 and "crossing" in t.text()
    assert t.of(2, 30, 5).tolist() == [3, 7, 8] and t.of(2, 32, 5).tolist() == [7, 9] and t.of(2, 34, 6).tolist() == [11] and t.of(2, 34, 5).tolist() == []
    # join with a hand-made trip table: (scene, aid, episode) -> its row
    who = [(0, 14, 0), (1, 20, 0), (2, 35, 6), (2, 30, 5), (2, 30, 6), (0, 30, 5)]
    raw = np.zeros((len(who), 16), np.uint32)
    for k, (scene, aid, ep) in enumerate(who):
        raw[k, :4] = scene, k, aid, ep
    j = t.join(trips.TripTable(raw, dict(dt=0.1)))
    assert j["second"].tolist() == [0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 2, -1] and j["first"].tolist() == [-1, -1, 1, 3, -1, -1, -1, 3, 3, -1, -1, -1, -1]
    assert j["missing"] == 26 - 7
    path = t.save(str(tmp_path / "pet.npz"))
    back = encroach.EncroachmentTable.load(path)
    assert np.array_equal(back.raw, t.raw) and back.meta == t.meta and back.meta["dropped"] == 3 and back.meta["window"] == 4
    assert back.meta["sim_config"] == dataclasses.asdict(SimConfig(map="intersection", num_envs=3, num_agents=7))
    for k in t.columns:
        assert np.array_equal(back[k], t[k]), k
    f = t.frame()
    assert len(f) == 13 and list(f.columns) == list(encroach.RAW + ("type",) + encroach.DERIVED)
    assert len(encroach.EncroachmentTable(np.zeros((0, 16), np.uint32), t.meta).summary()) == 0


def test_aggregates_dict_and_its_npz_round_trip(tmp_path):
    ref = _hand(7)
    meta = _table().meta
    a = encroach.aggregates_dict(ref.hist, ref.critical, meta)
    assert a["pet_s"].tolist() == pytest.approx([0.1, 0.2, 0.3, 0.4]) and a["count"].tolist() == [[2, 11, 0]]
    assert a["critical_frac"][0, 0] == 0.5 and a["critical_frac"][0, 1] == 9 / 11 and np.isnan(a["critical_frac"][0, 2])
    path = encroach.save(str(tmp_path / "agg.npz"), a)
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["critical", "hist", "meta"] and f["hist"].dtype == np.int64
    b = encroach.load(path)
    assert np.array_equal(b["hist"], a["hist"]) and np.array_equal(b["critical"], a["critical"]) and b["meta"] == a["meta"]
    assert np.array_equal(b["critical_frac"], a["critical_frac"], equal_nan=True)
    # the overlay goes through the field maps' blend: a critical cell is painted, the rest of the frame is not
    frame = np.zeros((32, 32, 3), np.uint8)
    over = encroach.fields.heat_overlay(frame, a["critical"][0], (16.0, 16.0, 1.0), grid=(0.0, 0.0, 1.0))
    assert over[31 - 25, 14].any() and not over[0, 0].any()


def test_overflow_and_groups_in_the_restatement():
    full, small = _hand(7), _hand(7, max_rows=9)
    assert small.n_rows == 9 and small.dropped == 4 and np.array_equal(small.rows(), full.rows()[:9])
    assert np.array_equal(small.hist, full.hist) and np.array_equal(small.critical, full.critical) and small.total_closed == full.total_closed
    ref = pc.hand_log(7, groups=2)
    ref.set_groups([1, 0, 7])
    pc.run_hand(7, lambda r, st, env: ref.record(st, env), ref.forget)
    per_scene = [int((full.rows()[:, 0] == e).sum()) for e in range(3)]
    assert ref.n_rows == full.n_rows and ref.hist[1].sum() == per_scene[0] and ref.hist[0].sum() == per_scene[1] and ref.hist.sum() == 13 - per_scene[2]


def test_cell_width_check():
    hw = SimConfig().veh_half_wid
    assert encroach.max_cell(hw) == pytest.approx(1.3096, abs=1e-4) and encroach.max_cell(0.9256) == pytest.approx(1.309, abs=1e-3)
    pn.EncroachmentLog(1, 4, fn.Grid(0.0, 0.0, 8, 8, 1.3), pc.HL, hw)
    with pytest.raises(ValueError):
        pn.EncroachmentLog(1, 4, fn.Grid(0.0, 0.0, 8, 8, 1.31), pc.HL, hw)
    assert encroach.state_bytes(1, 40, 100, 100, 50, 1, 1) == 80000 + 800 + 16 + 8 * 10150 + 64 + 16
    assert encroach.state_bytes(16384, 40, 165, 175, 50, 1, 65536) > 3.7e9


# observed on the CPU oracle: rows, following, crossing, pet <= critical_records, slot turnovers inside a live window
ROLLOUT_FOUND = {"intersection": (246, 220, 26, 15, 24), "roundabout": (302, 293, 9, 23, 10)}


@pytest.mark.parametrize("name", ["intersection", "roundabout"])
def test_rollout_premises_on_the_cpu_oracle(golden_dir, name):
    """6 x 40, 100 steps of the reference's Intersection population on the CPU oracle: the premises without which the GPU comparison
    could pass vacuously, with the counts found as lower bounds"""
    import oracle_lib as ol
    cfg = pc.rollout_config(name)
    g = pc.rollout_grid(cfg)
    ref = pn.EncroachmentLog(cfg.num_envs, 40, g, pc.HL, pc.HW, window=pc.ROLLOUT_WINDOW, critical_records=pc.ROLLOUT_CRITICAL)
    o = ol.OracleSim(cfg)
    try:
        act = pc.rollout_policy(golden_dir, name)
        out = o.reset()
        ref.record(*o.get_state())
        for _ in range(pc.ROLLOUTS[name]["steps"]):
            out = o.step(act(out["obs"]))
            ref.record(*o.get_state())
    finally:
        o.close()
    pc.check_invariants(ref)
    d = encroach.decode(ref.rows(), cfg.dt, (g.x0, g.y0, g.cell, g.W))
    found = (ref.n_rows, int((d["type"] == "following").sum()), int((d["type"] == "crossing").sum()), int((d["pet"] <= pc.ROLLOUT_CRITICAL).sum()),
             ref.turnovers_in_window)
    print(name, "rows, following, crossing, critical, turnovers in a live window:", found, "second touches", ref.second_touches)
    assert all(f >= w >= 1 for f, w in zip(found, ROLLOUT_FOUND[name])), (found, ROLLOUT_FOUND[name])
    assert ref.dropped == 0 and ref.hist.sum() == ref.n_rows and ref.critical.sum() == found[3]


def test_library_exports_and_binds_the_pet_entries():
    from copo_amd import _capi
    names = ["copo_pet_create", "copo_pet_set_groups", "copo_pet_record", "copo_pet_forget", "copo_pet_count", "copo_pet_read", "copo_pet_aggregates",
             "copo_pet_memory", "copo_pet_clear", "copo_pet_reset", "copo_pet_destroy"]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libcopo_hip.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    assert C.sizeof(_capi.PetCfg) == 36 and [f[0] for f in _capi.PetCfg._fields_] == ["x0", "y0", "cell", "W", "H", "G", "window", "critical_records", "max_rows"]
    assert (_capi.PET_WORDS, _capi.PET_MAX_WINDOW, _capi.PET_TYPES) == (pn.WORDS, 4096, 3)
    assert _capi.lib.copo_version() == 8                                  # additive: the ABI number stays
    # NULL arguments are refused before any device call
    lib, h, cfg = _capi.lib, C.c_void_p(), _capi.PetCfg(0.0, 0.0, 1.0, 32, 32, 1, 50, 10, 16)
    assert lib.copo_pet_create(None, C.byref(cfg), C.byref(h)) == -1 and b"copo_pet_create" in lib.copo_last_error()
    out = (C.c_int64 * 2)()
    for fn_name, args in (("copo_pet_set_groups", (None,) * 3), ("copo_pet_record", (None, None)), ("copo_pet_forget", (None, None)),
                          ("copo_pet_count", (None, out, None)), ("copo_pet_read", (None, 0, 0, None, None)), ("copo_pet_aggregates", (None,) * 4),
                          ("copo_pet_memory", (None,) * 4), ("copo_pet_clear", (None, None)), ("copo_pet_reset", (None, None)), ("copo_pet_destroy", (None,))):
        assert getattr(lib, fn_name)(*args) == -1 and fn_name.encode() in lib.copo_last_error(), fn_name
    # the configuration is checked before any device call as well: a handle that is not NULL is enough to get there (its body is all
    # zeros: half width 0, so every cell is too wide and what passes the DIM checks ends as CONFIG)
    fake = C.create_string_buffer(1 << 16)
    for bad, code in pc.refused_configs(_capi):
        assert lib.copo_pet_create(C.cast(fake, C.c_void_p), C.byref(bad), C.byref(h)) == code and b"copo_pet_create" in lib.copo_last_error(), \
            [getattr(bad, f[0]) for f in bad._fields_]
        assert not h.value
    assert lib.copo_pet_create(C.cast(fake, C.c_void_p), C.byref(cfg), C.byref(h)) == -5 and b"wider" in lib.copo_last_error()
    assert lib.copo_pet_create(C.cast(fake, C.c_void_p), None, C.byref(h)) == -1
