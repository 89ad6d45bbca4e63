"""The CPU oracle against a float64 model of the scene (sim_truth_numpy.py) on crafted scenes (sim_truth_cases.py).

The parity suite holds the HIP kernel to the oracle bit for bit; this file holds the oracle to the geometry it claims to compute.  The
model has known-answer tests of its own first: axis-aligned cases whose answers are written down by hand."""
import math

import numpy as np
import pytest

import sim_truth_cases as tc
import sim_truth_numpy as truth

HL, HW = tc.HL, tc.HW


# ---------------------------------------------------------------------------------------------------------------------------------
# the model's own known answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_ray_meets_a_box_dead_ahead_at_10_m():
    d, face, s = truth.ray_box((0.0, 0.0), 0.0, (10.0 + HL, 0.0), 0.0, HL, HW)
    assert abs(d - 10.0) < 1e-12 and face == 0 and abs(s - 1.0) < 1e-12
    d, face, _ = truth.ray_box((0.0, 0.0), 0.0, (10.0 + HW, 0.0), math.pi / 2, HL, HW)          # the box turned: its side faces the ray
    assert abs(d - 10.0) < 1e-12 and face == 1
    assert truth.ray_box((0.0, 0.0), math.pi, (10.0 + HL, 0.0), 0.0, HL, HW)[0] == np.inf          # looking away
    assert truth.ray_box((0.0, 0.0), -math.pi / 2, (10.0 + HL, 0.0), 0.0, HL, HW)[0] == np.inf      # looking right
    assert truth.ray_box((10.0, 0.3), 1.0, (10.0, 0.0), 0.0, HL, HW)[0] == 0.0                     # origin inside
    # 3-4-5: from (0, 0) along (0.8, 0.6) to the face x = 8 of a box [8, 12] x [5, 7]: t = 10 at y = 6
    d, face, s = truth.ray_box((0.0, 0.0), math.atan2(0.6, 0.8), (10.0, 6.0), 0.0, 2.0, 1.0)
    assert abs(d - 10.0) < 1e-12 and face == 0 and abs(s - 0.8) < 1e-12


def test_model_ray_grazing_a_corner_and_the_stability_mask():
    # box [8, 12] x [-1, 1]: its near left corner is (8, 1), seen from the origin under atan2(1, 8)
    corner = math.atan2(1.0, 8.0)
    d_in, face, _ = truth.ray_box((0.0, 0.0), corner - 1e-6, (10.0, 0.0), 0.0, 2.0, 1.0)
    assert abs(d_in - math.hypot(8.0, 1.0)) < 1e-4 and face == 0
    assert truth.ray_box((0.0, 0.0), corner + 1e-6, (10.0, 0.0), 0.0, 2.0, 1.0)[0] == np.inf
    rel = np.array([corner - 5e-6, corner + 5e-6, 0.0, math.pi])          # two grazing rays, one square on the face, one looking away
    val, hit, stable, clear_miss, clear_hit = truth._beams_vs_boxes(
        np.zeros((1, 2)), np.zeros(1), rel, np.array([[10.0, 0.0]]), np.zeros(1), np.array([2.0]), np.array([1.0]),
        np.ones((1, 1), bool), np.ones(1, bool), 40.0)
    assert hit[0].tolist() == [True, False, True, False]
    assert stable[0].tolist() == [False, False, True, True]
    assert clear_miss[0].tolist() == [False, False, False, True] and clear_hit[0].tolist() == [False, False, True, False]
    assert abs(val[0, 2] - 8.0 / 40.0) < 1e-12 and val[0, 3] == 1.0


def test_model_boxes_separated_on_one_axis_only():
    a = ((0.0, 0.0), 0.0, 2.0, 1.0)
    # b turned by 45 degrees, 4.2 m ahead: its half extent along x and y is (2 + 1) / sqrt 2; seen along b's axes a's is the same
    r = 3.0 / math.sqrt(2.0)
    want = [4.2 - 2.0 - r, -1.0 - r, 4.2 / math.sqrt(2.0) - r - 2.0, 4.2 / math.sqrt(2.0) - r - 1.0]
    got = truth.box_axis_gaps(a, ((4.2, 0.0), math.pi / 4, 2.0, 1.0))
    assert np.allclose(got, want, atol=1e-12) and (got > 0).sum() == 1 and got[0] > 0
    assert abs(truth.box_gap(a, ((4.2, 0.0), math.pi / 4, 2.0, 1.0)) - want[0]) < 1e-12
    assert abs(truth.box_gap(a, ((0.0, 2.3), 0.0, 2.0, 1.0)) - 0.3) < 1e-12          # side by side, 30 cm apart
    assert abs(truth.box_gap(a, ((0.0, 1.8), 0.0, 2.0, 1.0)) + 0.2) < 1e-12          # 20 cm into each other
    assert abs(truth.box_gap(a, ((4.5, 0.0), 0.0, 2.0, 1.0)) - 0.5) < 1e-12          # nose to tail
    assert truth.box_gap(a, ((0.1, 0.1), 0.3, 0.5, 0.2)) < -1.0                      # a small box inside


def _record(x0, y0, th, length, kappa, lanes_field):
    rec = np.zeros(16, np.float32)
    rec[[0, 1, 2, 3, 4, 5, 10]] = [x0, y0, math.cos(th), math.sin(th), length, kappa, lanes_field]
    rec[12] = 0.0 if kappa == 0 else 1.0 / abs(kappa)
    return rec


def test_model_projection_known_answers():
    north = _record(1.0, 2.0, math.pi / 2, 50.0, 0.0, 2.75)
    lon, lat, psi = truth.project(north, 0.0, 5.0, math.pi / 2 + 0.25)
    assert np.allclose([lon, lat, psi], [3.0, 1.0, 0.25], atol=1e-6)                 # west of a road going north = left of it
    # a left quarter turn of radius 10 from the origin heading east: centre (0, 10), end (10, 10) heading north
    left = _record(0.0, 0.0, 0.0, 5.0 * math.pi, 0.1, 2.0)
    lon, lat, psi = truth.project(left, 9.0, 10.0, math.pi / 2)
    assert np.allclose([lon, lat, psi], [5.0 * math.pi, 1.0, 0.0], atol=1e-6)        # inside a left turn = left
    lon, lat, _ = truth.project(left, 0.0, -1.5, 0.0)
    assert np.allclose([lon, lat], [0.0, -1.5], atol=1e-6)
    # a right turn of 350 degrees: nothing wraps between its two ends
    big = _record(0.0, 0.0, 0.0, 10.0 * math.radians(350.0), -0.1, 2.0)
    for deg in (1.0, 100.0, 175.0, 250.0, 349.0):
        # (clockwise about the centre (0, -10), starting above it)
        lon, lat, psi = truth.project(big, 9.0 * math.sin(math.radians(deg)), -10.0 + 9.0 * math.cos(math.radians(deg)), -math.radians(deg))
        assert np.allclose([lon, lat, psi], [10.0 * math.radians(deg), -1.0, 0.0], atol=1e-5), (deg, lon, lat, psi)


def test_model_out_of_road_rule_known_answers():
    class Cfg:
        lane_width, veh_half_len, veh_half_wid, body_margin = 3.5, 2.0, 1.0, 0.75

    class Tables:
        route_meta = np.array([[100.0, 1, -1, 0]], np.float32)
        route_segs = np.zeros((1, 17, 16), np.float32)

    def margin(lanes_field, lat, psi=0.0):
        Tables.route_segs[0, 0] = _record(0.0, 0.0, 0.0, 100.0, 0.0, lanes_field)
        return truth.road_decisions(Cfg, Tables, 0, 0, 50.0, lat, psi)

    # two lanes, lane-0 line on y = 0: the road is y in [-5.25, 1.75].  Continuous edges: the centre keeps 0.75 x the half width
    assert abs(margin(2.75, 0.0)["out_margin"] - (1.75 - 0.75)) < 1e-9
    assert abs(margin(2.75, 1.0)["out_margin"]) < 1e-9 and abs(margin(2.75, -4.5)["out_margin"]) < 1e-9
    assert abs(margin(2.75, 0.0, math.pi / 2)["out_margin"] - (1.75 - 1.5)) < 1e-9              # across the road: half LENGTH counts
    # no continuous line: the centre rule
    assert abs(margin(2.0, 1.75)["out_margin"]) < 1e-9 and abs(margin(2.0, -5.25)["out_margin"]) < 1e-9
    assert margin(2.5, 1.5)["out_margin"] > 0.2 and abs(margin(2.5, -4.5)["out_margin"]) < 1e-9   # right edge only
    d = margin(2.75, -1.74)
    assert d["lane"] == 0 and abs(d["lane_margin"] - 0.01) < 1e-9 and margin(2.75, -1.76)["lane"] == 1
    assert margin(2.75, 3.0)["lane"] == 0 and margin(2.75, -9.0)["lane"] == 1


def test_model_detector_known_answers():
    # heading east at the origin: beam 0 looks SOUTH (90 degrees clockwise), then west, north, east
    lines = np.array([[-5.0, -3.0, 0.0, 10.0, 0.0, 2.0, 0, 0],              # y = -3, continuous
                      [-4.0, -6.0, math.pi / 2, 12.0, 0.0, 1.0, 0, 0],      # x = -4, broken
                      # an arc of radius 7 about the origin from 10 degrees south of east to 10 degrees west of north
                      [7.0 * math.cos(math.radians(-10.0)), 7.0 * math.sin(math.radians(-10.0)), math.radians(80.0), 7.0 * math.radians(110.0), 1.0 / 7.0, 2.0, 0, 0]], np.float64)
    val, hit, stable, _, _ = truth.detector(np.zeros((1, 2)), np.zeros(1), 4, lines, 2.0, 20.0)
    assert np.allclose(val[0], [3.0 / 20.0, 1.0, 7.0 / 20.0, 7.0 / 20.0], atol=1e-12) and stable.all()
    val, _, _, _, _ = truth.detector(np.zeros((1, 2)), np.zeros(1), 4, lines, 1.0, 20.0)
    assert np.allclose(val[0], [3.0 / 20.0, 4.0 / 20.0, 7.0 / 20.0, 7.0 / 20.0], atol=1e-12)
    val, _, _, _, _ = truth.detector(np.zeros((1, 2)), np.array([math.pi / 4]), 4, lines, 2.0, 20.0)          # beams SE, SW, NW, NE
    assert np.allclose(val[0], [3.0 * math.sqrt(2.0) / 20.0, 3.0 * math.sqrt(2.0) / 20.0, 1.0, 7.0 / 20.0], atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# the crafted scenes say what they claim (from the model alone)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_collision_scenes_are_what_they_claim():
    case = tc.get_case("collisions")
    axis_pairs = 0
    for k, (kind, gap, swap) in enumerate(tc.collision_pairs()):
        a, b = case.scenes[k // 7][2 * (k % 7)], case.scenes[k // 7][2 * (k % 7) + 1]
        gaps = truth.box_axis_gaps(((a.x, a.y), a.th, HL, HW), ((b.x, b.y), b.th, HL, HW))
        if kind == "inside":
            assert gaps.max() < -1.0
            continue
        assert abs(gaps.max() - gap) < 1e-9, (kind, gap, gaps)
        if kind.startswith("axis"):          # separated along exactly one of the four axes, one pair for each
            assert (gaps > 0).sum() == 1 and int(gaps.argmax()) == (0 if kind == "axis_len" else 1) + (2 if swap else 0), (kind, swap, gaps)
            axis_pairs += 1
    assert axis_pairs == 4


BEAM_CASES = [n for n in tc.CASES if n.startswith(("lidar", "detectors"))]


@pytest.mark.parametrize("name", BEAM_CASES)
def test_caps_on_unstable_beams_from_the_model_alone(name):
    """The stability filter must not hide a failure: in every scene of a LiDAR or detector case at most 10 % of the beams that hit in the
    model are unstable (25 % in the pile), per block of beams -- LiDAR, side detector, lane-line detector.  No simulator runs here: the
    crafted words are put on an all-zero template (the oracle test below finds this evaluation of the model cached)."""
    case = tc.get_case(name)
    T = tc.case_truth(name, tc.crafted_state(name))
    blocks = ["lidar"] + [k for k, n in (("side", case.cfg.side_lasers), ("lane_col", case.cfg.lane_line_lasers)) if n]
    for key in blocks:
        share, hits = tc.unstable_shares(T, key)
        for e in range(case.cfg.num_envs):
            cap = case.caps.get(e, 0.10) if key == "lidar" else 0.10
            print("%s scene %d: %d %s hits, %.3f unstable" % (name, e, hits[e], key, share[e]))
            assert hits[e] > 0 and share[e] <= cap, (name, key, e, share[e], hits[e])


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle against the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_step(name):
    import oracle_lib as ol
    case = tc.get_case(name)
    o = ol.OracleSim(case.cfg)
    o.reset()
    st, env = case.state(*o.get_state())
    o.set_state(st, env)
    out = o.step(tc.brake_actions(case.cfg))
    obs, flags, info = out["obs"].copy(), out["flags"].copy(), out["info"].copy()
    o.close()
    return case, st, obs, flags, info


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_against_the_float64_model(name):
    """One reset, one set_state, one step of the CPU oracle per case, held to the model: decisions (crash flag, out-of-road flag, lane
    index) wherever the model's margin is more than 1 mm from the threshold, the heading column within 3e-7, stable beams and the side /
    lane columns within 1e-3 m (bound; not widened by the measurements below), unstable beams as `<= 1` plus hit / miss where the model
    is sure by more than 1 cm, the longitudinal coordinate (through the route-completion column of the info row) within 1e-3 m.  The caps
    on the share of unstable beams are asserted from the model alone, in the test above.

    Measured here, oracle against model (largest over all cases):
      distance error of stable beams and columns   2.0e-5 m (a Tollgate side beam; LiDAR 1.1e-5 m) -- 50 times below the 1e-3 m bound
      longitudinal coordinate                      1.2e-5 m
      heading column                               7.3e-8 (bound 3e-7)
      share of unstable beams among the hits       LiDAR rings 1.4 .. 6.2 % per scene (cap 10 %), the pile 2.7 % (cap 25 %),
                                                   detector beams 0 .. 7.9 % (cap 10 %)
    Out-of-road decisions on the straights of Merge / Split blocks are not compared (the model leaves their extra width out).
    """
    case, st, obs, flags, info = _oracle_step(name)
    T = tc.case_truth(name, st)
    stats = tc.check_against_model(case, T, obs, flags, info)
    print(name, {k: v for k, v in stats.items() if not isinstance(v, np.ndarray)})
    crafted = T["acted"].copy()
    crafted[:, case.keeper] = False
    if name.startswith("collisions"):          # no crafted decision is skipped
        assert (np.abs(T["crash_gap"][crafted]) > 0.009).all() and stats["crash_sure"][crafted].all()
        crashed = ((flags & tc.F_CRASH) != 0)[crafted]
        assert crashed.any() and not crashed.all()
    if name.startswith("projection") or name == "headings":          # every crafted row is compared
        assert stats["located"][crafted].all()
    if name.startswith("projection"):
        assert (np.abs(T["out_margin"][crafted]) > 0.009).all() and stats["out_known"][crafted].all()
        assert (T["lane_margin"][crafted] > 0.009).all()
        out = ((flags & tc.F_OUT) != 0)[crafted]
        assert 0.25 < out.mean() < 0.75          # both sides of the thresholds
        inside = crafted & (T["lane_col"][..., 0] > 1e-3) & (T["lane_col"][..., 0] < 1.0 - 1e-3)
        assert stats["lane_seen"][inside].all() and len(set(T["lane"][inside].tolist())) == 2


def test_lidar_beams_are_numbered_clockwise():
    """One target 30 degrees to the RIGHT of the heading: the beams that see it are the clockwise ones -- beam 6 of 72 points at it --, by
    index, and the mirrored beams see nothing."""
    case, st, obs, flags, _ = _oracle_step("lidar-intersection")
    c0 = truth.obs_columns(case.cfg)["lidar"]
    row = obs[tc.HANDED_SCENE, 0, c0:c0 + 72]
    seen = set(np.nonzero(row < 1.0)[0].tolist())
    assert 6 in seen and seen <= set(range(2, 11)), seen
    assert (row[72 - 10:] == 1.0).all()
    assert 12.0 - math.hypot(HL, HW) <= float(row[6]) * 40.0 <= 12.0 - HW          # between the target's circumcircle and its incircle
