"""CPU: the scene-rewind rules as tests/rewind_numpy.py restates them -- a scene forked from a stored snapshot resumes the CPU oracle bit
for bit (state words, env words and seed are the whole resumable state of a scene), the fork selection at its edges, the tally on hand
flags -- and the library's copo_rewind_* exports.  Every comparison is exact."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import oracle_lib as ol
import rewind_numpy as rn
from copo_amd.sim import SimConfig

DEPTH, STRIDE, STEPS, WINDOW = 4, 3, 260, 59
CHECKPOINTS = (11, 38, 131, 212)          # records after which every snapshot in the ring is forked: 4 stored records each
RESUME_CASES = dict(intersection=(3, 8, 30), parkinglot=(2, 6, 25), tollgate=(2, 10, 30))      # map: scenes, slots, horizon


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _resume(cfg1, ring, scene, rec, seed, acts, outs, reset_seed=777):
    """fork (scene, rec) into a one-scene oracle that was reset with another seed and drive it with the recorded actions; returns
    the number of mismatching words against the source's outputs"""
    o = ol.OracleSim(cfg1)
    try:
        o.reset(np.array([reset_seed], np.uint64))
        st, env = o.get_state()
        status, _ = ring.fork(st, env, 0, [scene], [rec])
        assert status[0] == rec
        o.set_state(st, env, seeds=np.array([seed], np.uint64))
        bad = 0
        for t in range(rec, min(rec + WINDOW, STEPS)):
            got = o.step(acts[t][scene:scene + 1])
            want = outs[t]
            bad += int((got["flags"][0] != want["flags"][scene]).sum())
            bad += int((_bits(got["rew"][0]) != _bits(want["rew"][scene])).sum())
            bad += int(_bits(got["glob_rew"])[0] != _bits(want["glob_rew"])[scene])
            rows = (want["flags"][scene] & 0x41) != 0
            bad += int((_bits(got["obs"][0])[rows] != _bits(want["obs"][scene])[rows]).sum())
        return bad
    finally:
        o.close()


@pytest.mark.parametrize("name", sorted(RESUME_CASES))
def test_a_fork_resumes_the_oracle_bit_for_bit(name):
    E, N, horizon = RESUME_CASES[name]
    cfg = SimConfig(map=name, num_envs=E, num_agents=N, horizon=horizon)
    cfg1 = dataclasses.replace(cfg, num_envs=1)
    seeds = np.arange(E, dtype=np.uint64) + np.uint64(cfg.start_seed)
    src = ol.OracleSim(cfg)
    ring = rn.RewindRing(E, N, DEPTH, STRIDE)
    rng = np.random.RandomState(17)                    # (with this seed every map has crashes, checked below)
    acts, outs, saved = [], [], {}
    try:
        src.reset(seeds)
        ring.record(*src.get_state())
        for t in range(STEPS):
            act = rn.random_actions(rng, E, N)
            out = src.step(act)
            acts.append(act)
            outs.append({k: out[k].copy() for k in ("flags", "rew", "glob_rew", "obs")})
            ring.record(*src.get_state())
            if t + 1 in CHECKPOINTS:
                saved[t + 1] = [list(r) for r in ring.rings]
    finally:
        src.close()
    seen = np.bitwise_or.reduce(np.stack([o["flags"] for o in outs]).reshape(-1))
    assert seen & rn.F_ENV_RESET and seen & rn.F_SPAWNED and seen & rn.F_CRASH, hex(seen)
    forks = 0
    for r_now, rings in saved.items():
        view = rn.RewindRing(E, N, DEPTH, STRIDE)
        view.r, view.rings = r_now + 1, rings
        assert [x[0] for x in rings[0]] == [r_now - r_now % STRIDE - STRIDE * k for k in (3, 2, 1, 0)]
        for e in range(E):
            for rec, _, _ in rings[e]:
                assert _resume(cfg1, view, e, rec, seeds[e], acts, outs) == 0, (name, e, rec)
                forks += 1
    assert forks == 16 * E
    # another seed: the same state, other draws -- the window must hold a draw (a respawn or a reset) and the fork must leave the source
    view = rn.RewindRing(E, N, DEPTH, STRIDE)
    view.r, view.rings = CHECKPOINTS[-1] + 1, saved[CHECKPOINTS[-1]]
    rec = saved[CHECKPOINTS[-1]][0][0][0]
    window = np.bitwise_or.reduce(np.stack([o["flags"][0] for o in outs[rec:rec + WINDOW]]).reshape(-1))
    assert window & (rn.F_SPAWNED | rn.F_ENV_RESET)
    assert _resume(cfg1, view, 0, rec, seeds[0] + np.uint64(1000), acts, outs) > 0


def _states(n, E=3, N=4):
    """record r -> (state block [16][E][N] of distinct words with ALIVE / WRECK / EMPTY status bytes below other bits, env block)"""
    out = []
    for r in range(n):
        st = (np.arange(16 * E * N, dtype=np.int64).reshape(16, E, N) + 100000 * (r + 1)).astype(np.int32)
        st[13] = ((r + 7) << 8) | ((np.arange(E)[:, None] + np.arange(N)[None, :] + r) % 3)      # status byte: (scene + slot + record) % 3
        st[10] = np.float32(0.25 + r).view(np.int32)
        env = np.stack([np.full(E, r), np.full(E, r // 5), np.full(E, 99 + r), np.ones(E, np.int64)], 1).astype(np.int32)
        out.append((st, env))
    return out


def _fork1(ring, scene, rec, **kw):
    t_st, t_env = np.full((16, 5, ring.N), -7, np.int32), np.full((5, 4), -7, np.int32)
    status, aid = ring.fork(t_st, t_env, 1, [scene], [rec], **kw)
    return status, aid, t_st, t_env


def test_selection_edge_cases():
    E, N = 3, 4
    ring = rn.RewindRing(E, N, 3, 2)
    states = _states(12, E, N)
    status, _, t_st, t_env = _fork1(ring, 0, 0)                        # nothing recorded
    assert status[0] == -1 and not t_st[:, 1].any() and t_env[1].tolist() == [0, 0, 0, 1] and (t_st[:, [0, 2, 3, 4]] == -7).all()
    assert ring.span() is None
    for r in range(9):
        ring.record(*states[r])                                        # records 0..8: stored 0 2 4 6 8, the ring holds 4 6 8
    assert ring.span() == (4, 8)
    for rec, want in ((5, 4), (4, 4), (7, 6), (8, 8), (9, 8), (1000, 8),      # between strides, beyond the last record
                      (3, -1), (2, -1), (-1, -1), (0, -1)):                    # 3 -> record 2: just evicted; 4: just kept
        status, _, t_st, t_env = _fork1(ring, 2, rec)
        assert status[0] == want, (rec, status)
        if want >= 0:
            assert np.array_equal(t_st[:, 1], states[want][0][:, 2]) and np.array_equal(t_env[1], states[want][1][2])
        else:
            assert not t_st[:12, 1].any() and (t_st[13, 1] == rn.ST_EMPTY).all() and t_env[1].tolist() == [0, 0, 0, 1]
        assert (t_st[:, [0, 2, 3, 4]] == -7).all() and (t_env[[0, 2, 3, 4]] == -7).all()      # the other target scenes are untouched
    ring.record(*states[9])                                            # record 9 is not stored: nothing moves
    assert ring.span() == (4, 8) and _fork1(ring, 0, 9)[0][0] == 8
    ring.record(*states[10])                                           # record 10 evicts record 4
    assert ring.span() == (6, 10) and _fork1(ring, 0, 5)[0][0] == -1 and _fork1(ring, 0, 6)[0][0] == 6
    for scene in (-1, E, 1 << 20):                                     # scene out of range
        assert _fork1(ring, scene, 8)[0][0] == -1
    # copies > 1: request j fills `copies` consecutive target scenes
    t_st, t_env = np.full((16, 6, N), -7, np.int32), np.full((6, 4), -7, np.int32)
    status, aid = ring.fork(t_st, t_env, 1, [1, 0], [7, 20], copies=2, watch_slots=[0, 1, 2, 3])
    assert status.tolist() == [6, 6, 10, 10]
    for j, (e, r) in enumerate(((1, 6), (1, 6), (0, 10), (0, 10))):
        assert np.array_equal(t_st[:, 1 + j], states[r][0][:, e])
        slot = j
        alive = (states[r][0][13, e, slot] & 0xFF) == rn.ST_ALIVE
        assert aid[j] == (states[r][0][14, e, slot] if alive else -1)
    assert (t_st[:, [0, 5]] == -7).all()
    assert len({int(a) for a in aid}) > 1 and -1 in aid.tolist()       # the hand states hold ALIVE and other watched slots
    # LCF: ALIVE slots only, clamped; NaN keeps the snapshot's
    status, _, t_st, _ = _fork1(ring, 1, 8, lcf=[3.0])
    alive = (states[8][0][13, 1] & 0xFF) == rn.ST_ALIVE
    assert alive.any() and not alive.all()
    assert (t_st[10, 1][alive].view(np.float32) == 1.0).all() and np.array_equal(t_st[10, 1][~alive], states[8][0][10, 1][~alive])
    assert np.array_equal(np.delete(t_st[:, 1], 10, 0), np.delete(states[8][0][:, 1], 10, 0))
    assert np.array_equal(_fork1(ring, 1, 8, lcf=[np.nan])[2][:, 1], states[8][0][:, 1])
    assert (_fork1(ring, 1, 8, lcf=[-0.5])[2][10, 1][alive].view(np.float32) == -0.5).all()
    ring.reset()
    assert ring.span() is None and _fork1(ring, 0, 0)[0][0] == -1
    ring.record(*states[3])
    assert ring.span() == (0, 0) and np.array_equal(_fork1(ring, 0, 5)[2][:, 1], states[3][0][:, 0])


def test_tally_on_hand_flags():
    steps, watch, want = rn.hand_tally_case()
    rows = rn.tally_init(3)
    assert rows.tolist() == [list(rn.TALLY_INIT)] * 3
    for f in steps:
        rn.tally(f, watch, rows)
    assert np.array_equal(rows, want), rows.tolist()
    rows = rn.tally_init(3)
    for f in steps:
        rn.tally(f, None, rows)                                         # no watch at all
    assert np.array_equal(rows[:, :6], want[:, :6]) and rows[:, 6:].tolist() == [[0, -1]] * 3
    rows = rn.tally_init(3)
    rn.tally(steps[0], np.array([5, -2, 0], np.int32), rows)           # slots outside 0..N-1 watch nothing
    assert rows[:, 6:].tolist() == [[0, -1]] * 3


def test_python_surface_without_a_gpu():
    from copo_amd import rewind
    assert rewind.TALLY_KEYS == ("steps", "acted", "arrive", "crash", "out", "maxstep", "watch_flags", "watch_step")
    assert rewind.TALLY_INIT == rn.TALLY_INIT and rewind.TALLY == 8 and rewind.MAX_DEPTH == 64
    assert rewind._per_target(None, 2, 3, np.int32, "x") is None
    assert rewind._per_target(5, 2, 3, np.int32, "x").tolist() == [5] * 6
    assert rewind._per_target([1, 2], 2, 3, np.int32, "x").tolist() == [1, 1, 1, 2, 2, 2]
    assert rewind._per_target(range(6), 2, 3, np.int32, "x").tolist() == list(range(6))
    with pytest.raises(ValueError):
        rewind._per_target([1, 2, 3], 2, 3, np.int32, "x")
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    assert MultiAgentIntersectionEnv.default_config()["rewind"] is None


def test_library_exports_and_null_checks_without_a_gpu():
    from copo_amd import _capi
    names = ["copo_rewind_create", "copo_rewind_record", "copo_rewind_reset", "copo_rewind_count", "copo_rewind_fork", "copo_rewind_tally",
             "copo_rewind_destroy"]
    lib = C.CDLL(_capi.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS and getattr(_capi.lib, name).restype is C.c_int
    assert _capi.lib.copo_version() == 8
    assert C.sizeof(_capi.RewindCfg) == 8 and (_capi.REWIND_MAX_DEPTH, _capi.REWIND_TALLY) == (64, len(rn.TALLY_INIT))
    cfg = _capi.RewindCfg(4, 2)
    h, n = C.c_void_p(), C.c_int32()
    assert _capi.lib.copo_rewind_create(None, C.byref(cfg), C.byref(h)) == -1
    assert b"copo_rewind_create" in _capi.lib.copo_last_error()
    for rc in (_capi.lib.copo_rewind_record(None, None), _capi.lib.copo_rewind_reset(None), _capi.lib.copo_rewind_count(None, C.byref(n)),
               _capi.lib.copo_rewind_fork(None, None, 0, 1, None, None, None, None, None, None, None, None),
               _capi.lib.copo_rewind_tally(None, None, None, 1, 4, None), _capi.lib.copo_rewind_destroy(None)):
        assert rc == -1
