"""Top-down renderer, CPU side: the numpy restatement of the render rules (tests/render_numpy.py) against the maps and the
simulator's spawn poses, the integer colour rules, the PPM / GIF writers and the C entry points' NULL checks (no device needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import render_numpy as rn
from copo_amd.render import PALETTE, read_ppm, write_gif, write_ppm
from copo_amd.sim import SimConfig

MAPS = [dict(map="intersection"), dict(map="roundabout"), dict(map="tollgate", toll_buildings=1), dict(map="tollgate", toll_buildings=2),
        dict(map="bottleneck"), dict(map="parkinglot"), dict(map="pgmap", map_kwargs=dict(sequence="SXCOS", seed=3))]


@pytest.mark.parametrize("kw", MAPS, ids=lambda kw: kw["map"] + str(kw.get("toll_buildings", "")))
def test_every_spawn_pose_lands_on_a_road_pixel(kw):
    cfg = SimConfig(num_envs=1, **kw)
    t, _ = cfg.resolved()
    mp = rn.Map(cfg)
    xy = rn.spawn_poses(t, mp.w)
    assert len(xy) == t.n_spawns > 0
    assert mp.on_road(xy[:, 0], xy[:, 1]).all()
    # and a point 3 lane widths beyond the map's bounding box is not road
    from copo_amd.maps import bounding_box
    x0, x1, y0, y1 = bounding_box(t)
    assert not mp.on_road(np.array([x1 + 3 * mp.w]), np.array([y1 + 3 * mp.w])).any()


def _one_vehicle_state(x, y, th, status=1, aid=0):
    st = np.zeros((16, 1, 1), np.float32)
    st[0, 0, 0], st[1, 0, 0], st[2, 0, 0] = x, y, th
    si = st.view(np.int32)
    si[13, 0, 0] = status | (3 << 16)        # status byte under a non-zero age: only the low byte counts
    si[14, 0, 0] = aid
    return st, np.zeros((1, 4), np.int32)


@pytest.mark.parametrize("th", [0.0, 0.7, -2.1])
def test_body_area(th):
    cfg = SimConfig(num_envs=1, map="intersection")
    mp = rn.Map(cfg)
    m = 0.05
    st, env = _one_vehicle_state(5000.0, -3000.0, th, aid=13)
    rgb, amb = rn.render_frame(mp, st, env, 0, (5000.0, -3000.0, m), 200, 200)
    c = PALETTE[13 % 12].astype(np.int64)
    body = (rgb == c).all(-1) | (rgb == rn.marker(c)).all(-1)
    want = (2 * mp.hl) * (2 * mp.hw) / m ** 2
    assert abs(body.sum() - want) < 0.05 * want, (body.sum(), want)
    marker = (rgb == rn.marker(c)).all(-1).sum()
    assert abs(marker - want / 4) < 0.08 * want / 4, (marker, want / 4)     # the front quarter
    assert amb.sum() < 0.06 * body.sum()      # (th = 0 puts a whole row of pixel centres 1 mm from a long edge)


def test_integer_rules():
    # trail weights w = 160 (K + 1 - a) / (K + 1), integer division: K = 25 -> 153 for the newest snapshot, 6 for the oldest
    K = 25
    w = [160 * (K + 1 - a) // (K + 1) for a in range(1, K + 1)]
    assert w[0] == 153 and w[-1] == 6 and all(x > y for x, y in zip(w, w[1:]))
    below, c = np.array([235, 90, 0]), np.array([31, 119, 255])
    assert (rn.blend(below, c, 0) == below).all() and (rn.blend(below, c, 256) == c).all()
    assert (rn.blend(below, c, 153) == (below * 103 + c * 153) >> 8).all()
    assert tuple(rn.blend(np.array([90]), np.array([255]), 6)) == ((90 * 250 + 255 * 6) >> 8,)
    assert tuple(rn.marker((255, 127, 14))) == (191, 95, 10)
    # dashes: a broken straight line is painted on [6k, 6k + 3) of its length
    L = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 30.0, 0.0, 0, 0, 0, 0, 0])
    s = np.arange(0.05, 30.0, 0.1)
    ex = rn.line_test(L, s, np.zeros_like(s), 0.1)[0]
    assert (ex == (np.fmod(s, 6.0) < 3.0)).all()
    L[0] = 2.0
    assert rn.line_test(L, s, np.zeros_like(s), 0.1)[0].all()
    assert not rn.line_test(L, s, np.full_like(s, 0.11), 0.1)[0].any()


def test_ppm_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    f = rng.randint(0, 256, (3, 7, 5, 4)).astype(np.uint8)
    f[0, 0, 0, :3] = (10, 32, 9)             # whitespace bytes right after the header
    paths = write_ppm(f, str(tmp_path), start=4)
    assert [os.path.basename(p) for p in paths] == ["frame_00004.ppm", "frame_00005.ppm", "frame_00006.ppm"]
    for k, p in enumerate(paths):
        assert (read_ppm(p) == f[k, ..., :3]).all()


def test_gif_writer(tmp_path):
    pytest.importorskip("PIL")
    f = np.zeros((4, 16, 16, 3), np.uint8)
    for k in range(4):
        f[k, :, 4 * k:4 * k + 4] = PALETTE[k]
    p = write_gif(f, str(tmp_path / "a.gif"), fps=5)
    from PIL import Image
    im = Image.open(p)
    assert im.n_frames == 4 and im.size == (16, 16)


def test_render_entry_points_reject_null_handles_without_a_device():
    from copo_amd import _capi
    lib = _capi.lib
    h = C.c_void_p()
    pal = np.ascontiguousarray(PALETTE)
    assert lib.copo_render_create(None, 64, 64, 0, pal.ctypes.data, C.byref(h)) == -1
    assert lib.copo_render_record(None, None) == -1
    assert lib.copo_render_clear(None, None) == -1
    assert lib.copo_render_frames(None, None, 1, None, 0, None, None) == -1
    assert lib.copo_render_destroy(None) == -1
    assert b"copo_render_destroy" in lib.copo_last_error()
