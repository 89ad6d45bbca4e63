"""CPU: input attribution (copo_amd/eval/attribution.py, copo_ig_obs_seats_f32, copo_attrib_tally) -- the float64
model's own laws (completeness, the premise that more points close the gap, masked columns, one point = the midpoint gradient), levels
and plans, the frame from hand-made words, the command line's entry and the C ABI's refusals.  No device is touched."""
import ctypes as C
import json

import numpy as np
import pytest

import adversary_cases as ac
import attribution_cases as xc
import attribution_numpy as az
from copo_amd import _capi
from copo_amd.eval import attribution as at
from copo_amd.sim import SimConfig

CFG = SimConfig(map="intersection", num_envs=2, num_agents=4)


@pytest.fixture(scope="module", params=[(64, 91), (128, 92)], ids=lambda p: "h%d-o%d" % p)
def model(request):
    hidden, in_dim = request.param
    ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
    rows, counts = ac.lists()
    listed = [(k, int(r)) for k in range(xc.K) for r in rows[k][:counts[k]]]
    return [ac.net_of(w) for w in ws], obs, xc.baselines(in_dim).astype(np.float64), listed


def test_completeness_masks_and_the_premise(model):
    """sum_j attr + gap == mu(o) - mu(b) to float64 rounding at every level; a NaN column gets an exact 0; and |gap| at 32 points is
    below |gap| at 4 points on EVERY listed row, from either baseline of the GPU cases -- the margin is printed."""
    nets, obs, base, listed = model
    least = np.inf
    for k, r in listed:
        for lv in (1, 2, 3):
            gaps = {}
            for m in (1, 4, 32):
                attr, heads = az.ig_row(nets[k], obs[r], base[lv], m)
                assert np.abs(attr.sum(axis=1) + heads[4:6] - (heads[0:2] - heads[2:4])).max() <= 1e-14
                assert (attr[:, np.isnan(base[lv])] == 0.0).all() and np.isfinite(attr).all()
                gaps[m] = np.abs(heads[4:6])
            assert (gaps[32] < gaps[4]).all(), (k, r, lv, gaps)
            least = min(least, float((gaps[4] / gaps[32]).min()))
    print("least |gap(4)| / |gap(32)| over %d rows x 3 baselines x 2 heads: %.1f" % (len(listed), least))
    assert len(listed) == 18 and least > 4.0          # (the midpoint rule gains 64 at best: 4 leaves room for fp32 on the device)


def test_one_point_is_the_gradient_at_the_midpoint(model):
    nets, obs, base, listed = model
    for k, r in listed[:6]:
        o = obs[r].astype(np.float64)
        b = az.baseline_of(o, base[1])
        attr, _ = az.ig_row(nets[k], o, base[1], 1)
        for a in range(2):
            assert np.allclose(attr[a], (o - b) * az.mean_gradient(nets[k], b + 0.5 * (o - b), a), rtol=1e-13, atol=0.0)


def test_the_case_tables_and_the_fp32_deviation():
    ref = xc.reference(64, 91)
    for t in xc.TABLES:
        m = ref["tables"][t]
        assert (m["index"] >= 0).sum() == xc.ATTRIBUTED[t] and m["listed"].sum() == 18
        assert (m["heads"][m["index"] >= 0][:, 6] == 1.0).all() and (m["heads"][m["index"] < 0] == 0.0).all()
    assert set(ref["tables"]["A"]["index"]) == {-1, 1, 2, 3} and (ref["tables"]["C"]["index"][16:24] == -1).all()
    print("hidden 64 in_dim 91: torch fp32 dev %.3g, tau %.3g" % (ref["dev"], ref["tau"]))
    assert 0.0 < ref["tau"] < 1e-3


def test_levels_are_checked():
    L = at.AttributionLevel
    assert L().is_identity and L().words().tolist() == [0, 0, 0, 0] and L(4, "zeros").words().dtype == np.int32
    for bad in (33, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            L(bad, "zeros")
    for kw in (dict(points=0, baseline="zeros"), dict(points=4), dict(points=4, baseline="night"), dict(points=4, baseline=[0.0, np.inf]),
               dict(points=4, baseline=[1e39, 0.0]), dict(points=4, baseline=np.zeros((2, 3))), dict(points=4, baseline=[])):
        with pytest.raises(ValueError):
            L(**kw)
    row = L.row([0.5, None, np.nan, 1.0], 2)
    assert np.isnan(row.baseline[1:3]).all() and row.baseline.dtype == np.float32 and row.as_dict() == dict(points=2, baseline="row")
    assert row == L(2, [0.5, np.nan, np.nan, 1.0]) and row != L(3, [0.5, np.nan, np.nan, 1.0]) and hash(row) == hash(L(2, [0.5, np.nan, np.nan, 1.0]))
    with pytest.raises(ValueError):
        row.baseline_row(CFG, 5)          # a baseline of the wrong width
    lo, hi = CFG.ego_dim + CFG.navi_dim, CFG.ego_dim + CFG.navi_dim + CFG.num_lasers
    clear = L.clear_road(CFG, 4).baseline_row(CFG, hi)
    assert (clear[lo:hi] == 1.0).all() and np.isnan(clear[:lo]).all() and hi - lo == CFG.num_lasers
    assert (L.zeros(CFG).baseline_row(CFG, hi) == 0.0).all() and np.isnan(L().baseline_row(CFG, hi)).all()


def test_plans_are_checked():
    P, L = at.AttributionPlan, at.AttributionLevel
    levels = [L(), L.clear_road(CFG, 4), L.zeros(CFG, 32)]
    plan = P(levels, np.array([[0, 1], [2, -1]], np.int32))
    assert (plan.L, plan.G, plan.K, plan.max_points) == (3, 2, 2, 32) and plan.words.shape == (3, 4) and plan.words.dtype == np.int32
    assert P([{}], np.zeros((1, 1), np.int32)).max_points == 1 and plan.base is None
    with pytest.raises(ValueError):
        at.AttributionBuffers.tables(plan)          # baselines that are still names
    O = CFG.ego_dim + CFG.navi_dim + CFG.num_lasers
    assert plan.resolve(CFG, O).base.shape == (3, O) and plan.base.dtype == np.float32 and plan.in_dim == O
    arrays, key = at.AttributionBuffers.tables(plan)
    assert key == (3, 2, 2, 32, O) and set(arrays) == {"level_of", "levels", "base"}
    for bad in (np.zeros(3, np.int32), np.zeros((0, 2), np.int32), np.zeros((2, 2, 2), np.int32)):
        with pytest.raises(ValueError):
            P(levels, bad)
    with pytest.raises(ValueError):
        P([], np.zeros((1, 1), np.int32))
    with pytest.raises(ValueError):
        P([L.row(np.zeros(5), 2)], np.zeros((1, 1), np.int32)).resolve(CFG, O)
    seats, sweep = P.sweep(2, levels, 1, 4)
    assert seats.n_groups == 6 and sweep.level_of.shape == (6, 2) and list(sweep.level) == [0, 1, 2, 0, 1, 2]
    with pytest.raises(ValueError):
        plan.check(seats)


def test_load_levels(tmp_path):
    path = tmp_path / "levels.json"
    path.write_text(json.dumps([{}, dict(points=4, baseline="clear_road"), dict(points=2, baseline=[0.5, None])]))
    L = at.AttributionLevel
    assert at.load_levels(str(path)) == [L(), L(4, "clear_road"), L(2, [0.5, np.nan])]
    path.write_text(json.dumps([dict(points=40, baseline="zeros")]))
    with pytest.raises(ValueError):
        at.load_levels(str(path))


def test_frame_from_hand_made_words():
    P, L = at.AttributionPlan, at.AttributionLevel
    levels = [L.clear_road(CFG, 4), L.zeros(CFG, 8)]
    seats, plan = P.sweep(2, levels, 1, 4)
    O = CFG.ego_dim + CFG.navi_dim + CFG.num_lasers + 1
    rng = np.random.RandomState(5)
    cols = rng.randint(1, 1 << 40, (seats.n_groups, 2, 2, O)).astype(np.int64)
    words = np.zeros((seats.n_groups, 2, 8), np.int64)
    words[..., 0], words[..., 1], words[..., 3], words[..., 5] = 10, int(5 * at.Q32), int(0.25 * at.Q32), int(0.125 * at.Q32)
    df = at.attribution_frame(words, cols, np.ones((seats.n_groups, 2, 8), np.int64), seats, plan, CFG, ["a", "b"])
    assert [(r.checkpoint, r.level, r.label) for r in df.itertuples()] == [(0, 0, "a"), (0, 1, "a"), (1, 0, "b"), (1, 1, "b")]
    assert list(df["baseline"]) == ["clear_road", "zeros"] * 2 and list(df["points"]) == [4, 8] * 2
    for head in at.HEADS:
        shares = df[["share_%s_%s" % (b, head) for b in at.BLOCKS]]
        assert np.allclose(shares.sum(axis=1), 1.0, rtol=0, atol=1e-12) and (shares > 0).all().all()
    blocks = at.column_blocks(CFG, O)
    assert sorted(np.concatenate(list(blocks.values())).tolist()) == list(range(O - 1))          # every column but the one behind the LiDAR
    n, lo = CFG.num_lasers, CFG.ego_dim + CFG.navi_dim
    assert lo in blocks["lidar_front"] and lo + n - 1 in blocks["lidar_front"] and lo + n // 4 in blocks["lidar_right"]
    assert lo + n // 2 in blocks["lidar_rear"] and lo + 3 * n // 4 in blocks["lidar_left"] and all(len(blocks[b]) == n // 4 for b in at.BLOCKS[2:])
    g, k = 1, 0
    want = cols[g, k, 0][blocks["navi"]].sum() / sum(cols[g, k, 0][i].sum() for i in blocks.values())
    assert df.iloc[1]["share_navi_steer"] == pytest.approx(want, rel=1e-12)
    assert df.iloc[0]["mean_abs_delta_steer"] == 0.5 and df.iloc[0]["mean_gap_steer"] == 0.025 and df.iloc[0]["max_gap"] == 0.125
    empty = at.attrib_rates(np.zeros(8, np.int64), np.zeros((2, O), np.int64), blocks)
    assert all(np.isnan(v) for v in empty.values())
    prof = at.attribution_profile(words, cols, seats, plan, ["a", "b"])
    assert len(prof) == seats.n_groups * 2 * O and prof.iloc[0]["mean_abs_attr"] == cols[0, 0, 0, 0] / at.Q32 / 10


def test_the_command_line_entry(tmp_path, monkeypatch, capsys):
    from copo_amd.eval import checkpoint_io, evaluate
    study, = (s for s in evaluate.STUDIES if s.option == "attribution")
    assert not any("attribution" in studies for studies in evaluate.GOES_WITH.values())          # no option of its own
    assert (study.option, study.module, study.rows, study.levels, study.share) == ("attribution", "attribution", "attribution_rows", "attribution_levels", None)
    levels = tmp_path / "levels.json"
    levels.write_text(json.dumps([dict(points=4, baseline="clear_road")]))
    table, called = str(tmp_path / "t.csv"), []

    def fake_rows(algo, env, weights_list, levels, **kw):
        called.append((algo, env, list(weights_list), levels, kw))
        seats, plan = at.AttributionPlan.sweep(2, levels, 1, 4)
        O = CFG.ego_dim + CFG.navi_dim + CFG.num_lasers
        return at.attribution_frame(np.ones((seats.n_groups, 2, 8), np.int64), np.ones((seats.n_groups, 2, 2, O), np.int64),
                                    np.ones((seats.n_groups, 2, 8), np.int64), seats, plan, CFG, kw["labels"])

    monkeypatch.setattr(at, "attribution_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])
    base = ["--attribution", "a.npz", "b.npz"]

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        return e.value.code == 2

    assert refused(base + ["--table", table]) and refused(base + ["--attribution-levels", str(levels)])          # its levels and its table
    assert refused(base + ["--attribution-levels", str(levels), "--table", table, "--certify-sweep", "a.npz", "--certify-levels", str(levels)])
    assert "one table per run" in capsys.readouterr().err
    assert refused(base + ["--attribution-levels", str(levels), "--table", table, "--certify-method", "linear"])          # goes with another study
    assert not called
    evaluate.main(base + ["--attribution-levels", str(levels), "--table", table, "--steps", "16", "--scenes-per-pair", "3", "--num-agents", "4", "--share", "0.25"])
    (algo, env, ws, lv, kw), = called
    assert (algo, env, ws) == ("copo", "inter", ["w:a.npz", "w:b.npz"]) and lv == [at.AttributionLevel(4, "clear_road")]
    assert kw == dict(num_agents=4, steps=16, labels=["a.npz", "b.npz"], scenes_per_cell=3)          # no share: the study takes none
    assert "share_lidar_front_steer" in capsys.readouterr().out


def test_symbols_are_declared_exported_and_refuse():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "copo_hip.h")).read()
    for name in ("copo_ig_obs_seats_f32", "copo_attrib_tally"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, name) and ("int %s(" % name) in header
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION
    p = C.c_void_p(64)          # never dereferenced: every call below is refused before any HIP call
    good = dict(flags=p, attr=p, heads=p, seat=p, group=p, E=2, N=4, K=2, G=2, in_dim=91, words=p, cols=p, stream=None)
    tally = lambda **kw: _capi.lib.copo_attrib_tally(*dict(good, **kw).values())  # noqa: E731
    for name in ("flags", "attr", "heads", "seat", "group", "words", "cols"):
        assert tally(**{name: None}) == -1, name
    for kw in (dict(E=-1), dict(N=0), dict(N=257), dict(K=0), dict(G=0), dict(in_dim=0)):
        assert tally(**kw) == -2, kw
    assert tally(E=0) == 0
    cfg = _capi.PpoCfg()
    ig = dict(cfg=C.byref(cfg), theta=p, theta_t=p, stride=1 << 20, K=2, rows=p, counts=p, cap=32, n_out=48, obs=p, attr=p, heads=p, col_lo=0, col_hi=0,
              n_slots=8, group=p, G=2, level_of=p, levels=p, L=2, base=p, max_points=32, stream=None)
    call = lambda **kw: _capi.lib.copo_ig_obs_seats_f32(*dict(ig, **kw).values())  # noqa: E731
    assert call() == -2          # an empty configuration
    for name in ("heads", "base"):
        assert call(**{name: None}) == -1, name
    assert call(cfg=None) == -1
