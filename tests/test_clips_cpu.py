"""CPU: the event-clip rules as tests/clip_numpy.py restates them (hand sequences of the per-scene state machine and of the ordered
commit), the numpy side of copo_amd/clips.py (ClipSet save / load / select, flag names, the CLI's event list) and the library's
copo_clip_* exports.  Every comparison is exact: the feature is copies, integer logic and float32 `<`."""
import ctypes as C

import numpy as np
import pytest

import clip_numpy as cn

E, N = 3, 4


def state(r, E=E, N=N):
    """A state block [16][E][N] of distinct words for record r, the status byte with other bits set above it, and its env block"""
    st = (np.arange(16 * E * N, dtype=np.int64).reshape(16, E, N) + 100000 * (r + 1)).astype(np.int32)
    st[13] = ((r + 7) << 8) | ((st[13] + r) % 3)
    env = np.stack([np.full(E, r), np.full(E, r // 5), np.full(E, 99), np.ones(E, np.int64)], 1).astype(np.int32)
    return st, env


def flags_at(*hits):
    f = np.zeros((E, N), np.uint8)
    for e, n in hits:
        f[e, n] = 0x08
    return f


def run(tr, n_records, hits=None, ttc=None, gap=None, flags_on=True):
    """n_records records; hits: {record: [(scene, slot), ...]} crash flags"""
    for r in range(n_records):
        st, env = state(r, tr.E, tr.N)
        f = flags_at(*(hits or {}).get(r, [])) if flags_on else None
        tr.record(st, env, f, None if ttc is None else ttc.get(r), None if gap is None else gap.get(r))


def expect_frames(tr, c, scene, records):
    for k, r in enumerate(records):
        w, v = cn.snapshot(*state(r, tr.E, tr.N))
        assert np.array_equal(tr.snaps[c, k], w[scene]) and np.array_equal(tr.envw[c, k], v[scene]), (c, k, r)
    assert not tr.snaps[c, len(records):].any() and not tr.envw[c, len(records):].any()


def test_snapshot_takes_the_six_words_and_the_status_byte_only():
    st, env = state(4)
    w, v = cn.snapshot(st, env)
    assert w.shape == (E, 6, N) and v.shape == (E, 2)
    for k, f in enumerate((0, 1, 2, 3)):
        assert np.array_equal(w[:, k], st[f].view(np.uint32))
    assert np.array_equal(w[:, 4], st[13].view(np.uint32) & 0xFF) and (st[13] >> 8 != 0).all()
    assert np.array_equal(w[:, 5], st[14].view(np.uint32)) and np.array_equal(v, env[:, :2])


def test_trigger_at_record_0():
    tr = cn.ClipTracker(E, N, 3, 1, 8, flag_mask=0x08)
    run(tr, 4, {0: [(1, 2), (1, 3)]})
    assert tr.n_clips == 1 and tr.dropped == 0
    assert tr.header[0].tolist() == [1, 0, 2, 0, 2, cn.KIND_FLAG, int(state(0)[0][14, 1, 2]), 1]
    expect_frames(tr, 0, 1, [0, 1])
    assert tr.ready_log == [[], [1], [], []]


def test_trigger_before_pre_records_exist_gives_a_short_clip():
    tr = cn.ClipTracker(E, N, 5, 2, 8, flag_mask=0x08)
    run(tr, 6, {2: [(0, 0)]})
    assert tr.header[0].tolist()[:5] == [0, 0, 5, 2, 0]
    expect_frames(tr, 0, 0, [0, 1, 2, 3, 4])


def test_trigger_during_a_countdown_is_counted_and_makes_no_second_clip():
    tr = cn.ClipTracker(E, N, 2, 3, 8, flag_mask=0x08)
    run(tr, 12, {4: [(2, 1)], 5: [(2, 0)], 7: [(2, 3)]})
    assert tr.n_clips == 1
    assert tr.header[0].tolist() == [2, 2, 6, 4, 1, cn.KIND_FLAG, int(state(4)[0][14, 2, 1]), 3]
    expect_frames(tr, 0, 2, [2, 3, 4, 5, 6, 7])


def test_back_to_back_clips_of_a_scene_share_no_record():
    tr = cn.ClipTracker(E, N, 4, 1, 8, flag_mask=0x08)
    run(tr, 12, {3: [(0, 1)], 5: [(0, 2)], 6: [(0, 2)]})
    assert tr.n_clips == 2
    assert tr.header[0].tolist()[:4] == [0, 0, 5, 3] and tr.header[1].tolist()[:4] == [0, 5, 2, 5]      # lo = 5 after the first
    assert tr.header[1, cn.H_N_EVENTS] == 2
    expect_frames(tr, 0, 0, [0, 1, 2, 3, 4])
    expect_frames(tr, 1, 0, [5, 6])


def test_a_ring_that_wrapped_several_times():
    tr = cn.ClipTracker(E, N, 3, 1, 8, flag_mask=0x08)
    run(tr, 30, {23: [(1, 0)]})
    assert tr.header[0].tolist()[:4] == [1, 20, 5, 23]
    expect_frames(tr, 0, 1, [20, 21, 22, 23, 24])


def test_post_0_commits_in_the_record_that_armed():
    tr = cn.ClipTracker(E, N, 2, 0, 8, flag_mask=0x08)
    run(tr, 6, {3: [(0, 3)], 4: [(0, 3)]})
    assert tr.ready_log[3] == [0] and tr.ready_log[4] == [0] and tr.n_clips == 2
    assert tr.header[0].tolist()[:4] == [0, 1, 3, 3] and tr.header[1].tolist()[:4] == [0, 4, 1, 4]
    expect_frames(tr, 1, 0, [4])


def test_overflow_keeps_the_lowest_scenes_of_the_record():
    tr = cn.ClipTracker(E, N, 1, 0, 2, flag_mask=0x08)
    run(tr, 4, {1: [(2, 0)], 2: [(0, 0), (1, 1), (2, 2)]})
    assert tr.n_clips == 2 and tr.dropped == 2
    assert tr.header[:, cn.H_SCENE].tolist() == [2, 0] and tr.header[1].tolist()[:4] == [0, 1, 2, 2]
    # the dropped scenes are idle again and lose the records of the dropped clip
    assert tr.armed == [None] * 3 and tr.lo == [3, 3, 3]


def test_flush_commits_the_armed_scenes_with_what_they_have():
    tr = cn.ClipTracker(E, N, 2, 5, 8, flag_mask=0x08)
    run(tr, 7, {4: [(2, 0)], 6: [(0, 1)]})
    assert tr.n_clips == 0
    tr.flush()
    assert tr.n_clips == 2 and tr.header[0].tolist()[:4] == [0, 4, 3, 6] and tr.header[1].tolist()[:4] == [2, 2, 5, 4]
    expect_frames(tr, 1, 2, [2, 3, 4, 5, 6])
    tr.flush()                                  # nothing is armed any more
    assert tr.n_clips == 2 and tr.lo == [7, 0, 7]
    st, env = state(7)
    tr.record(st, env, flags_at((0, 0)))
    tr.flush()
    assert tr.header[2].tolist()[:4] == [0, 7, 1, 7]


def test_nan_and_inf_never_fire_and_kinds_are_ored():
    ttc = np.full((E, N), np.inf, np.float32)
    ttc[0, 1], ttc[1, 2], ttc[2, 0] = np.nan, 1.0, np.float32(0.99999994)
    gap = np.full((E, N), np.inf, np.float32)
    gap[2, 3], gap[1, 0] = 0.25, 0.5
    tr = cn.ClipTracker(E, N, 1, 0, 8, flag_mask=0x08, ttc_below=1.0, gap_below=0.5)
    run(tr, 3, {1: [(2, 2)]}, ttc={1: ttc}, gap={1: gap})
    assert tr.n_clips == 1                                       # scene 0: NaN; scene 1: ttc == 1.0 and gap == 0.5 are not below
    assert tr.header[0].tolist()[:6] == [2, 0, 2, 1, 0, cn.KIND_FLAG | cn.KIND_TTC | cn.KIND_GAP]       # lowest firing slot: the ttc one
    off = cn.ClipTracker(E, N, 1, 0, 8, flag_mask=0, ttc_below=0.0, gap_below=0.0)      # a mask / threshold of 0 is off
    run(off, 3, {1: [(2, 2)]}, ttc={1: np.zeros((E, N), np.float32)}, gap={1: np.zeros((E, N), np.float32)})
    assert off.n_clips == 0


def test_a_null_array_turns_its_trigger_off():
    tr = cn.ClipTracker(E, N, 1, 0, 8, flag_mask=0x08, ttc_below=1.0)
    run(tr, 4, {1: [(0, 0)]}, flags_on=False)
    assert tr.n_clips == 0
    run(tr, 1, ttc={0: np.zeros((E, N), np.float32)}, flags_on=False)
    assert tr.n_clips == 3 and (tr.header[:3, cn.H_KIND] == cn.KIND_TTC).all()


def _clipset():
    from copo_amd.clips import ClipSet, clip_meta
    from copo_amd.sim import SimConfig
    tr = cn.ClipTracker(E, N, 2, 1, 8, flag_mask=0x08, gap_below=0.5)
    gap = np.full((E, N), np.inf, np.float32)
    gap[1, 1] = 0.1
    run(tr, 9, {2: [(0, 1)], 6: [(2, 3)]}, gap={4: gap})
    cfg = SimConfig(map="intersection", map_kwargs=dict(exit_length=80.0), num_envs=E, num_agents=N)
    return ClipSet(tr.header[:tr.n_clips], tr.snaps[:tr.n_clips], tr.envw[:tr.n_clips], clip_meta(cfg, N, 2, 1)), tr


def test_clipset_save_load_select(tmp_path):
    from copo_amd.clips import ClipSet
    cs, tr = _clipset()
    assert len(cs) == 3 and cs.column("scene").tolist() == [0, 1, 2] and cs.column("kind").tolist() == [1, 4, 1]
    path = str(tmp_path / "clips.npz")
    cs.save(path)
    with np.load(path, allow_pickle=False) as f:                # no pickled objects
        assert set(f.files) == {"header", "snaps", "envw", "meta"} and f["snaps"].dtype == np.uint32
    back = ClipSet.load(path)
    assert np.array_equal(back.header, cs.header) and np.array_equal(back.snaps, cs.snaps) and np.array_equal(back.envw, cs.envw)
    assert back.meta == cs.meta and back.meta["pre"] == 2 and back.meta["post"] == 1 and back.meta["dt"] == 0.1
    assert back.meta["hl"] == 2.2575 and back.meta["hw"] == 0.926
    cfg = back.sim_config(num_envs=2)
    assert (cfg.map, cfg.map_kwargs, cfg.num_envs, cfg.num_agents) == ("intersection", dict(exit_length=80.0), 2, N)
    # float views are the raw bits
    assert back.x.dtype == np.float32 and np.array_equal(back.x.view(np.uint32), back.snaps[:, :, 0])
    assert np.array_equal(back.speed.view(np.uint32), back.snaps[:, :, 3]) and np.array_equal(back.agent_id.view(np.uint32), back.snaps[:, :, 5])
    assert back.info(1) == dict(zip(("scene", "first_rec", "length", "trig_rec", "trig_slot", "kind", "trig_aid", "n_events"),
                                    (int(v) for v in tr.header[1])))
    assert back.select(kind="gap").column("scene").tolist() == [1]
    assert back.select(kind=("flag", "ttc")).column("scene").tolist() == [0, 2]
    assert back.select(scene=[2, 1]).column("scene").tolist() == [1, 2]
    assert len(back.select(kind="flag", scene=1)) == 0 and back.select(kind="flag", scene=1).snaps.shape == (0, 4, 6, N)


def test_flag_names_and_the_cli_event_list():
    from copo_amd import _capi
    from copo_amd.clips import FLAG_BITS, flag_mask
    from copo_amd.vis import parse_clip_on
    assert FLAG_BITS == dict(acted=_capi.F_ACTED, done=_capi.F_DONE, arrive=_capi.F_ARRIVE, crash=_capi.F_CRASH, out=_capi.F_OUT,
                             maxstep=_capi.F_MAXSTEP, spawned=_capi.F_SPAWNED, env_reset=_capi.F_ENV_RESET)
    assert flag_mask(("crash", "out")) == 0x18 and flag_mask(()) == 0 and flag_mask(0x04) == 4
    with pytest.raises(ValueError):
        flag_mask(("crashed",))
    with pytest.raises(ValueError):
        flag_mask(0x100)
    assert parse_clip_on("crash,out,ttc<1.0,gap<0.5") == dict(flags=("crash", "out"), ttc_below=1.0, gap_below=0.5)
    assert parse_clip_on("crash") == dict(flags=("crash",), ttc_below=0.0, gap_below=0.0)
    for bad in ("ttc", "crash<1", "gap<0", "bump"):
        with pytest.raises(ValueError):
            parse_clip_on(bad)


def test_library_exports_and_null_checks_without_a_gpu():
    from copo_amd import _capi
    names = ["copo_clip_create", "copo_clip_record", "copo_clip_flush", "copo_clip_count", "copo_clip_read", "copo_clip_reset",
             "copo_clip_destroy", "copo_clip_scatter"]
    lib = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS and getattr(_capi.lib, name).restype is C.c_int
    assert C.sizeof(_capi.ClipCfg) == 24 and (_capi.CLIP_MAX_CAP, _capi.CLIP_WORDS, _capi.CLIP_HEADER) == (256, cn.WORDS, cn.HEADER)
    cfg = _capi.ClipCfg(3, 1, 8, 0x08, 0.0, 0.0)
    h = C.c_void_p()
    assert _capi.lib.copo_clip_create(None, C.byref(cfg), C.byref(h)) == -1
    assert b"copo_clip_create" in _capi.lib.copo_last_error()
    n = C.c_int32()
    for rc in (_capi.lib.copo_clip_record(None, None, None, None, None), _capi.lib.copo_clip_flush(None, None),
               _capi.lib.copo_clip_count(None, C.byref(n), C.byref(n), None), _capi.lib.copo_clip_read(None, 0, 1, None, None, None, None),
               _capi.lib.copo_clip_reset(None, None), _capi.lib.copo_clip_destroy(None),
               _capi.lib.copo_clip_scatter(None, None, None, 4, 5, None, None, 1, None)):
        assert rc == -1
