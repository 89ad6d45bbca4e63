"""Linear probes without a GPU and without the native library (copo_amd/eval/probes.py): the plan's derivation and
refusals, `probe_fit` against the model that works on the rows directly (tests/probe_numpy.py), the planted signals the GPU tests lean
on, the premise of the exact Gram test, and the command-line rules with the study's rows function replaced."""
import numpy as np
import pytest

import probe_cases as pc
import probe_numpy as pn
import similarity_cases as sc

from copo_amd.eval import probes as pr
from copo_amd.eval.crossplay import SeatPlan

# The largest |probe_fit - fit_direct| over r2_train, r2_test and weight_norm of the planted cases, measured: 1.53e-12 (the value
# test_fit_equals_the_direct_model prints).  The two differ only in the expansion of a squared sum in float64, hence the margin of 16.
MEASURED_FIT_DEVIATION = 1.53e-12


def _seats():
    return SeatPlan(sc.SEAT, sc.K, sc.GROUP, sc.G)


def test_plan_derivation():
    plan = pr.ProbePlan(_seats())
    assert list(plan.members) == [0, 1, 2] and (plan.M, plan.K, plan.blocks, plan.rows_of) == (3, 3, 6, -1)
    assert plan.count == sc.COUNT == plan.cap and np.array_equal(plan.rows[:plan.count], sc.rows())
    assert plan.jury.kind == "panel" and (plan.jury.counts == sc.COUNT).all()
    # groups 0, 1, 2 hold scenes (0, 1), (2, 3), (4); scene 5 lies in group 7: train, test, train, test, train, never
    assert plan.folds.tolist() == [0, 1, 0, 1, 0, 255] and plan.folds.dtype == np.uint8
    assert plan.planes(64) == 1          # one chunk of rows: nothing to split
    assert plan.accumulator_shapes(64) == dict(G=(1, 2, 6, 64, 64), C=(1, 2, 6, 64, 16), T=(1, 2, 16, 16))
    assert plan.accumulator_shapes(128, 1) == dict(G=(1, 2, 1, 128, 128), C=(1, 2, 1, 128, 16), T=(1, 2, 16, 16))
    one = 8 * (2 * 6 * 64 * 64 + 2 * 6 * 64 * 16 + 2 * 256)
    assert plan.accumulator_bytes(64) == one == plan.check_bytes(64)
    assert plan.accumulator_bytes(64, 91) == one + 8 * (2 * 128 * 128 + 2 * 128 * 16 + 2 * 256) and pr.padded_width(91) == 128 == pr.padded_width(128)
    solo = pr.ProbePlan(_seats(), members=[2], rows_of=1)          # a panel of ONE member
    assert list(solo.members) == [2] and solo.blocks == 2 and solo.rows_of == 1 and np.array_equal(solo.rows[:solo.count], sc.rows())
    own = pr.ProbePlan(_seats(), folds=[1, 0, 255, 255, 255, 0])
    assert own.folds.tolist() == [1, 0, 255, 255, 255, 0]
    # the row split is a function of the plan alone: doubled while the launch has fewer than 256 workgroups and a plane has a chunk
    big = pr.ProbePlan(SeatPlan.pairs(2, 64, 40, 0.5))
    assert big.cap == 4 * 64 * 40 and big.planes(256) == 4 and big.planes(64) == 8 and big.planes(512) == 1          # 88, 16 and 296 workgroups
    assert big.planes(128, 1) == 8 and pr.ProbePlan(SeatPlan.pairs(16, 2, 40, 0.5)).planes(256) == 1
    assert (pr.default_folds(SeatPlan.pairs(2, 3, 4, 0.5)) == np.tile([0, 1, 0], 4)).all()
    t = pr.trig_table(72)
    assert t.dtype == np.float32 and t.shape == (72, 2) and t[0].tolist() == [1.0, 0.0] and t[18, 1] == 1.0 and np.array_equal(t, pn.trig_table(72))


def test_plan_refusals():
    seats = _seats()
    for bad in (dict(members=[]), dict(members=[0, 0]), dict(members=[0, 3]), dict(members=[-1]), dict(rows_of=3), dict(rows_of=-1),
                dict(hidden=100), dict(hidden=1024), dict(hidden=64, max_bytes=1000), dict(folds=[0, 1, 0]), dict(folds=[0, 1, 2, 0, 1, 0])):
        with pytest.raises(ValueError):
            pr.ProbePlan(seats, **bad)
    with pytest.raises(ValueError, match=str(8 * (2 * 6 * 512 * 512 + 2 * 6 * 512 * 16 + 2 * 256))):          # the figure is named
        pr.ProbePlan(seats, hidden=512, max_bytes=1 << 20)
    with pytest.raises(ValueError, match=r"test fold \(scene groups \[0, 1, 2\]"):          # a fold without a seated scene, and the groups
        pr.ProbePlan(seats, folds=[0, 0, 0, 0, 0, 1])                                          # (scene 5 is in no group of the plan)
    with pytest.raises(ValueError, match="train fold"):
        pr.ProbePlan(seats, folds=[1, 1, 255, 255, 255, 0])
    with pytest.raises(ValueError, match="test fold"):
        pr.ProbePlan(SeatPlan.pairs(2, 1, 4, 0.5))          # one scene per pair: the default folds have no test scene
    with pytest.raises(ValueError):
        pr.ProbePlan(seats).check(SeatPlan(sc.SEAT[:5], sc.K, sc.GROUP[:5], sc.G))          # another shape
    with pytest.raises(ValueError):
        pr.ProbePlan(seats).check_bytes(64, 600)
    assert pr.ProbePlan(seats, hidden=512).max_bytes == 1 << 30


def _fit_block(acc, Q):
    fit = pr.probe_fit(acc, pc.RIDGE, Q)
    return {k: (v[0] if isinstance(v, np.ndarray) and k != "weights" else v) for k, v in fit.items()}


def test_fit_equals_the_direct_model():
    """`probe_fit` (accumulators only) against `fit_direct` (the rows) on the planted cases.  Measured deviation: 1.53e-12 (max over
    r2_train, r2_test and weight_norm); asserted within 16 times that."""
    worst = 0.0
    for seed in pc.PLANTED_SEEDS:
        c = pc.planted(seed)
        got, want = _fit_block(pc.stats_of(c["X"], c["t"], c["fold"]), 3), pn.fit_direct(c["X"], c["t"], c["fold"], pc.RIDGE)
        assert (got["n_train"], got["n_test"]) == (want["n_train"], want["n_test"]) == (320, 320)
        for key in ("r2_train", "r2_test", "weight_norm"):
            assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (seed, key)
            ok = ~np.isnan(want[key])
            worst = max(worst, float(np.abs(got[key][ok] - want[key][ok]).max()))
    print("max |probe_fit - fit_direct| over the planted cases = %.3g, bound %.3g" % (worst, 16 * MEASURED_FIT_DEVIATION))
    assert worst <= 16 * MEASURED_FIT_DEVIATION


def test_planted_signals():
    """The premises: a linear target is found, a hash of the row index is not, a constant is NaN; a pad column and a duplicated column
    do not break the solve."""
    for seed in pc.PLANTED_SEEDS:
        c = pc.planted(seed)
        assert not c["X"][:, 63].any() and np.array_equal(c["X"][:, 62], c["X"][:, 61])
        assert c["fold"][:16].tolist() == [0] * 16 and c["fold"][16:32].tolist() == [1] * 16
        for fit in (_fit_block(pc.stats_of(c["X"], c["t"], c["fold"]), 3), pn.fit_direct(c["X"], c["t"], c["fold"], pc.RIDGE)):
            print("seed %d: r2_test %s, r2_train %s" % (seed, fit["r2_test"], fit["r2_train"]))
            assert fit["r2_test"][0] > 0.99 and fit["r2_train"][0] > 0.99
            assert abs(fit["r2_test"][1]) < 0.1
            assert np.isnan(fit["r2_test"][2]) and np.isnan(fit["r2_train"][2])
            assert np.isfinite(fit["weight_norm"]).all()


def test_fit_is_nan_not_an_exception():
    c = pc.planted(pc.PLANTED_SEEDS[0])
    X, t = c["X"], c["t"]
    nan = lambda fit: np.isnan(fit["r2_train"]).all() and np.isnan(fit["r2_test"]).all()  # noqa: E731
    one = np.full(len(X), 255)
    one[0] = 0
    one[1:40] = 1
    assert nan(_fit_block(pc.stats_of(X, t, one), 3)) and nan(pn.fit_direct(X, t, one))                       # one train row
    no_test = np.where(np.arange(len(X)) < 100, 0, 255)
    fit = _fit_block(pc.stats_of(X, t, no_test), 3)
    assert fit["n_test"] == 0 and np.isnan(fit["r2_test"]).all() and fit["r2_train"][0] > 0.99                 # an empty test fold
    assert nan(_fit_block(pc.stats_of(np.ones_like(X), t, c["fold"]), 3))                                     # features that do not vary
    bad = pc.stats_of(X, t, c["fold"])
    bad["G"][1, 0, 3, 3] = np.inf
    fit = pr.probe_fit(bad)
    assert nan(fit) and np.isnan(fit["weight_norm"]).all() and np.isnan(fit["weights"]).all()                 # a non-finite entry
    for kw in (dict(n_targets=16), dict(n_targets=0), dict(ridge=-1.0), dict(ridge=float("nan"))):
        with pytest.raises(ValueError):
            pr.probe_fit(bad, **kw)
    G = pn.accumulate([np.arange(128.0 * 5).reshape(5, 128)], np.ones((5, 16)), [np.ones(5, bool)] * 2)["G"]
    assert np.array_equal(pr.mirror_tiles(pn.upper_tiles(G)), G) and not pn.upper_tiles(G)[0, 0, 64:, :64].any()


def test_the_end_to_end_premise():
    """The GPU test's planted targets in the float64 model of the same members and rows: found at member 0's h1, and the hash is not."""
    c = pc.rows_case(64, 91, pc.E2E_ROWS)
    h = sc.hidden_of(c["members"], c["obs"])
    t = pc.planted_targets(h[0][:, 0].astype(np.float32), pc.E2E_ROWS)
    fit = pn.fit_direct(h[0][:, 0], t, c["fold"], pc.RIDGE)
    print("r2_test of the planted pair at member 0's h1: %s" % fit["r2_test"])
    assert fit["r2_test"][0] > 0.99 and abs(fit["r2_test"][1]) < 0.1
    for m in (1, 2):
        for layer in range(2):
            assert abs(pn.fit_direct(h[m][:, layer], t, c["fold"], pc.RIDGE)["r2_test"][1]) < 0.1


def test_the_targets_model_and_the_premise_of_the_exact_gram_test():
    for in_dim in (91, 92):
        c = pc.target_rows(in_dim)
        t = pn.targets_of(c["obs"], pc.COL_LO, pc.N_BEAMS, c["flags"], c["reward"])
        assert t.dtype == np.float32 and np.isfinite(t).all() and not t[:, 8:15].any() and (t[:, 15] == 1).all()
        assert t[0, :5].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]                                  # nothing in range
        trig = pn.trig_table(72)
        assert t[1, 0] == 0.25 and t[1, 1] == np.float32(0.75) * trig[7, 0] and t[1, 3] == np.float32(3) / np.float32(72)          # the tie: beam 7
        assert [bool(t[r, 4] == 0.125) for r in range(2, 11)] == [True, True, False, False, False, False, False, True, True]      # front: 63 .. 71, 0 .. 8
        assert t[11, 0] == 0.0 and t[11, 4] == 0.0 and t[12, 0] == 0.5 and t[12, 1] == np.float32(0.5) and t[12, 3] == 1.0
        assert t[[2, 3, 15], 6].tolist() == [1, 0, 1] and t[[2, 3, 15], 7].tolist() == [1, 1, 0]
        assert len(set(c["rows"][:c["count"]].tolist())) == c["count"]
    assert pn.front_beams(72).tolist() == list(range(9)) + list(range(63, 72))
    for D in (64, 512):
        for count in pc.GRID_COUNTS:
            for rows_of in pc.GRID_ROWS_OF:
                for folds in pc.GRID_FOLDS:
                    c = pc.grid_case(D, count, rows_of, folds)
                    for ws, tg, _, masks in c["steps"]:
                        live = masks[0] | masks[1]
                        assert not (masks[0] & masks[1]).any() and not live[count:].any()
                        assert np.isnan(ws[:, ~live]).all() and np.isnan(tg[~live]).all() and np.isin(ws[:, live], pc.GRID_VALUES).all()
                    for k in ("G", "C", "T"):          # quarters below 2^24: exact in fp32 whatever the order
                        assert np.array_equal(c["acc"][k] * 4, np.rint(c["acc"][k] * 4)) and np.abs(c["acc"][k]).max() * 4 < 2 ** 24
                    if folds == "none":
                        assert not any(c["acc"][k].any() for k in ("G", "C", "T"))
                    if folds == "train":
                        assert not c["acc"]["G"][1].any() and not c["acc"]["T"][1].any()
    c = pc.grid_case(64, 320, None, "mixed")
    assert min(c["acc"]["T"][0, 15, 15], c["acc"]["T"][1, 15, 15]) > 0 and pc.grid_case(64, 320, None, "train")["acc"]["T"][0, 15, 15] > 2 * 128
    o = pc.grid_obs_case()
    assert o["acc"]["G"].shape == (2, 1, 128, 128) and o["acc"]["T"][:, 15, 15].min() > 0


def test_frame_from_hand_made_fits():
    Q = len(pr.TARGETS)
    hid = dict(n_train=10, n_test=7, r2_train=np.full((4, Q), 0.5), r2_test=np.arange(4 * Q, dtype=float).reshape(4, Q) / 100, weight_norm=np.ones((4, Q)))
    obs = dict(n_train=10, n_test=7, r2_train=np.full((1, Q), 0.25), r2_test=np.full((1, Q), 0.125), weight_norm=np.full((1, Q), 2.0))
    obs["r2_test"][0, 2] = np.nan
    df = pr.probe_frame(hid, obs, [2, 0], 1, labels=["a", "b", "c"])
    assert list(df.columns) == ["member", "label", "layer", "target", "rows_of", "n_train", "n_test", "r2_train", "r2_test", "gain", "weight_norm"]
    assert len(df) == (2 * 2 + 1) * Q
    assert [(r.member, r.layer) for r in df.itertuples()][::Q] == [(-1, "obs"), (2, "h1"), (2, "h2"), (0, "h1"), (0, "h2")]
    assert list(df["target"][:Q]) == list(pr.TARGETS) and (df["rows_of"] == 1).all() and (df["n_train"] == 10).all() and (df["n_test"] == 7).all()
    assert (df[df.member == -1]["gain"].dropna() == 0).all() and df["label"].iloc[Q] == "c" and df["label"].iloc[0] == "obs"
    row = df[(df.member == 0) & (df.layer == "h2") & (df.target == "nearest_cos")].iloc[0]
    assert row["r2_test"] == (3 * Q + 1) / 100 and row["gain"] == row["r2_test"] - 0.125
    assert np.isnan(df[(df.member == 2) & (df.target == "nearest_sin")]["gain"]).all()          # no control, no gain
    m = pr.probe_matrix(df, 3)
    assert m.shape == (5, Q) and m.loc[(0, "h2"), "nearest_cos"] == row["r2_test"]


def test_the_command_line_entry(tmp_path, monkeypatch, capsys):
    from copo_amd.eval import checkpoint_io, evaluate
    study, = (s for s in evaluate.STUDIES if s.option == "probe")
    assert {o: s for o, s in evaluate.GOES_WITH.items() if "probe" in s} == dict(probe_rows_of=("probe",), probe_ridge=("probe",))
    assert (study.option, study.module, study.rows, study.levels, study.share, study.scenes) == ("probe", "probes", "probe_rows", None, 0.5, "scenes_per_pair")
    table, called = str(tmp_path / "t.csv"), []

    def fake_rows(algo, env, weights_list, **kw):
        called.append((algo, env, list(weights_list), kw))
        Q = len(pr.TARGETS)
        fit = lambda B: dict(n_train=5, n_test=4, r2_train=np.ones((B, Q)), r2_test=np.full((B, Q), 0.5), weight_norm=np.ones((B, Q)))  # noqa: E731
        return pr.probe_frame(fit(4), fit(1), [0, 1], -1 if kw["rows_of"] is None else kw["rows_of"], kw["labels"])

    monkeypatch.setattr(pr, "probe_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])
    base = ["--probe", "a.npz", "b.npz"]

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        return e.value.code == 2

    assert refused(base)                                                                   # its table
    assert refused(base + ["--table", table, "--similarity", "a.npz", "b.npz"])
    assert "one table per run" in capsys.readouterr().err
    assert refused(["--probe-rows-of", "1", "--table", table])                             # without --probe: a usage error
    assert "--probe-rows-of goes with --probe" in capsys.readouterr().err
    assert refused(["--similarity", "a.npz", "b.npz", "--probe-ridge", "0.1", "--table", table])
    assert refused(base + ["--table", table, "--similarity-rows-of", "0"])                 # another study's option
    assert not called
    evaluate.main(base + ["--probe-rows-of", "1", "--probe-ridge", "0.01", "--table", table, "--steps", "16", "--scenes-per-pair", "2", "--num-agents", "4"])
    evaluate.main(base + ["--table", table, "--share", "0.25"])
    (algo, env, ws, kw), (_, _, _, kw2) = called
    assert (algo, env, ws) == ("copo", "inter", ["w:a.npz", "w:b.npz"])
    assert kw == dict(num_agents=4, steps=16, labels=["a.npz", "b.npz"], scenes_per_pair=2, rows_of=1, ridge=0.01, share=0.5)
    assert kw2["rows_of"] is None and kw2["ridge"] == 1e-4 and kw2["share"] == 0.25
    out = capsys.readouterr().out
    assert "r2_test" in out and "nearest_cos" in out and "h2" in out
    import pandas as pd
    assert len(pd.read_csv(table)) == (2 * 2 + 1) * len(pr.TARGETS)
