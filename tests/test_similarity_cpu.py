"""Representation similarity without a GPU and without the native library (copo_amd/eval/similarity.py): the plan's
derivation and refusals, the properties of the float64 model that the GPU tests lean on (tests/similarity_numpy.py), the premise of
the exact Gram test, and the command-line rules with the study's rows function replaced."""
import numpy as np
import pytest

import similarity_cases as sc
import similarity_numpy as sn

from copo_amd.eval import similarity as sim
from copo_amd.eval.crossplay import SeatPlan


def _seats():
    return SeatPlan(sc.SEAT, sc.K, sc.GROUP, sc.G)


def test_plan_derivation():
    plan = sim.SimilarityPlan(_seats())
    assert list(plan.members) == [0, 1, 2] and (plan.M, plan.K, plan.P, plan.rows_of) == (3, 3, 6, -1)
    assert plan.count == sc.COUNT == plan.cap and np.array_equal(plan.rows[:plan.count], sc.rows())
    assert (np.diff(plan.rows[:plan.count]) > 0).all() and plan.count % 16 == 2          # ascending, and a partial last tile
    assert plan.jury.kind == "panel" and (plan.jury.counts == sc.COUNT).all()
    assert [tuple(p) for p in plan.pairs] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert all(sn.pair_index(a, b, 3) == i for i, (a, b) in enumerate(plan.pairs))
    assert plan.planes(64) == 1          # one chunk of rows: nothing to split
    assert plan.accumulator_shapes(64) == dict(S=(1, 6, 2, 64, 64), s=(1, 3, 2, 64), n=(1,))
    assert plan.accumulator_bytes(64) == 8 * (6 * 2 * 64 * 64 + 3 * 2 * 64 + 1) == plan.check_bytes(64)
    sub = sim.SimilarityPlan(_seats(), members=[2, 0], rows_of=1)
    assert list(sub.members) == [2, 0] and sub.P == 3 and sub.rows_of == 1 and np.array_equal(sub.rows[:sub.count], sc.rows())
    assert (sub.jury.counts == np.array([sc.COUNT, 0, sc.COUNT])).all()
    # the row split is a function of the plan alone: doubled while the launch has fewer than 256 workgroups and a plane has a chunk
    big = sim.SimilarityPlan(SeatPlan.pairs(2, 64, 40, 0.5))
    assert big.cap == 4 * 64 * 40 and big.planes(256) == 4 and big.planes(64) == 8 and big.planes(512) == 1          # 96, 6 and 384 tiles
    assert sim.SimilarityPlan(SeatPlan.pairs(16, 1, 40, 0.5)).planes(256) == 1


def test_plan_refusals():
    seats = _seats()
    for bad in (dict(members=[1]), dict(members=[0, 0]), dict(members=[0, 3]), dict(members=[-1, 0]), dict(rows_of=3), dict(rows_of=-1),
                dict(hidden=100), dict(hidden=1024), dict(hidden=64, max_bytes=1000)):
        with pytest.raises(ValueError):
            sim.SimilarityPlan(seats, **bad)
    with pytest.raises(ValueError, match=str(8 * (6 * 2 * 512 * 512 + 3 * 2 * 512 + 1))):          # the figure is named
        sim.SimilarityPlan(seats, hidden=512, max_bytes=1 << 20)
    with pytest.raises(ValueError):
        sim.SimilarityPlan(seats).check(SeatPlan(sc.SEAT[:5], sc.K, sc.GROUP[:5], sc.G))          # another shape
    assert sim.SimilarityPlan(seats, hidden=512).max_bytes == 1 << 30
    with pytest.raises(ValueError):
        sim.similarity_matrix(None, layer="h3")


@pytest.fixture(scope="module")
def case():
    ref = sc.reference(64, 91)
    return ref, sc.workspace_of(ref["hidden64"])


def test_model_properties(case):
    ref, ws = case
    for rows_of in sc.ROWS_OF:
        m = sc.model(ws, rows_of)
        n = m["acc"]["n"]
        assert n == int(m["mask"].sum()) and (2 <= n < sc.COUNT)
        for layer in range(2):
            assert np.allclose(np.diag(m["cka"][:, :, layer]), 1.0, rtol=0, atol=1e-12)          # cka(a, a) == 1
        assert np.array_equal(m["cka"], m["cka"].transpose(1, 0, 2)) and np.array_equal(m["hsic"], m["hsic"].transpose(1, 0, 2))
        assert ((m["cka"] > 0) & (m["cka"] <= 1 + 1e-12)).all()
        # the accumulator form equals the definition on centred features
        for a in range(3):
            for b in range(3):
                for layer in range(2):
                    want = sn.cka_of_activations(ws[a][m["mask"]][:, layer], ws[b][m["mask"]][:, layer])
                    assert abs(m["cka"][a, b, layer] - want) < 1e-9
        # the census: variance and mean straight from the activations
        mean, var = m["mean"], m["var"]
        assert np.allclose(mean[1, 0], ws[1][m["mask"]][:, 0].mean(axis=0), atol=1e-12)
        assert np.allclose(var[1, 1], ws[1][m["mask"]][:, 1].var(axis=0), atol=1e-12)
    assert sc.model(ws, None)["acc"]["n"] > sc.model(ws, 1)["acc"]["n"]


def test_invariances_and_the_twin(case):
    ref, ws = case
    rng = np.random.RandomState(5)
    mask = sc.model(ws, None)["mask"]
    X, Y = ws[0][mask][:, 1], ws[1][mask][:, 1]
    base = sn.cka_of_activations(X, Y)
    Q, _ = np.linalg.qr(rng.randn(X.shape[1], X.shape[1]))
    assert abs(sn.cka_of_activations(X @ Q, Y) - base) < 1e-12          # a random orthogonal map of one side's units
    assert abs(sn.cka_of_activations(3.7 * X, Y) - base) < 1e-12        # isotropic scaling of one side
    assert abs(sn.cka_of_activations(X[:, rng.permutation(X.shape[1])], Y) - base) < 1e-12
    assert base < 0.999                                                 # (the members do differ)
    for hidden in (64, 256):
        r = sc.reference(hidden, 92)
        w0 = r["members"][0]
        twin = sc.twin_of(w0)
        assert sc.weight_distance(w0, twin) > 1.0                       # far away in weight space
        h = sc.workspace_of(sc.hidden_of([w0, twin], r["obs"]))
        m = sc.model(h, None, panel=(0, 1))
        assert np.abs(m["cka"][0, 1] - 1.0).max() < 1e-12               # ... and the same network
        heads = [sn.heads64(sc.ac.net_of(w), sc.hidden_of([w], r["obs"])[0][:, 1]) for w in (w0, twin)]
        assert np.abs(heads[0] - heads[1]).max() < 1e-12                # the same function


def test_fewer_than_two_rows_is_nan(case):
    ref, ws = case
    none = np.zeros_like(sc.jc.flags())
    m = sc.model(ws, None, flags=none)
    assert m["acc"]["n"] == 0 and np.isnan(m["cka"]).all() and not m["hsic"].any() and not m["var"].any()
    one = none.copy()
    one.reshape(-1)[sc.rows()[3]] = sn.F_ACTED
    m = sc.model(ws, None, flags=one)
    assert m["acc"]["n"] == 1 and np.isnan(m["cka"]).all()
    # the package's host rule is the model's: NaN with n < 2 and with a zero norm, never an exception
    hs = sc.model(ws, None)["hsic"]
    assert np.isnan(sim.cka_from_hsic(hs, 1)).all()
    assert np.allclose(sim.cka_from_hsic(hs, 10), sn.cka(hs, 10), rtol=0, atol=1e-15)
    dead = hs.copy()
    dead[1, :, 0] = dead[:, 1, 0] = 0.0          # member 1's first layer is constant on the rows
    got = sim.cka_from_hsic(dead, 10)
    assert np.isnan(got[1, :, 0]).all() and np.isnan(got[:, 1, 0]).all() and np.isfinite(got[:, :, 1]).all() and np.isfinite(got[0, 2, 0])


def test_frames_from_hand_made_numbers():
    plan = sim.SimilarityPlan(_seats(), members=[2, 0], rows_of=1)
    hs = np.zeros((2, 2, 2))
    hs[..., 0] = [[4.0, 1.0], [1.0, 1.0]]
    hs[..., 1] = [[9.0, 0.0], [0.0, 0.0]]
    df = sim.similarity_frame(hs, 12, plan, labels=["a", "b", "c"])
    assert list(df.columns) == ["member_a", "member_b", "label_a", "label_b", "layer", "rows_of", "n", "hsic", "cka"]
    assert [(r.member_a, r.member_b, r.layer) for r in df.itertuples()] == [(a, b, l) for a in (2, 0) for b in (2, 0) for l in sim.LAYERS]
    assert df.iloc[2]["cka"] == 0.5 and df.iloc[0]["cka"] == 1.0 and np.isnan(df.iloc[3]["cka"]) and (df["n"] == 12).all()
    assert (df["label_a"].iloc[0], df["label_b"].iloc[2], df["rows_of"].iloc[0]) == ("c", "a", 1)
    mat = sim.similarity_matrix(df, "h1", 3).to_numpy()
    assert mat[2, 0] == mat[0, 2] == 0.5 and mat[0, 0] == 1.0 and np.isnan(mat[1]).all()
    assert sim.similarity_matrices(df, 3).shape == (6, 3)
    assert np.isnan(sim.similarity_frame(hs, 0, plan)["cka"]).all()          # n == 0: NaN in the frame
    mean, var = np.zeros((2, 2, 4)), np.ones((2, 2, 4))
    mean[0, 0], var[0, 0], var[1, 1] = [0.995, -0.999, 0.5, 0.0], [1e-9, 0.0, 1e-7, 1.0], 0.0
    u = sim.unit_frame(mean, var, 12, plan, labels=["a", "b", "c"])
    assert list(u.columns) == ["member", "label", "layer", "n", "units", "dead_units", "saturated_units", "mean_abs_activation"]
    assert [(r.member, r.layer, r.dead_units, r.saturated_units) for r in u.itertuples()] == [(2, "h1", 2, 2), (2, "h2", 0, 0), (0, "h1", 0, 0), (0, "h2", 4, 0)]
    assert abs(u.iloc[0]["mean_abs_activation"] - (0.995 + 0.999 + 0.5) / 4) < 1e-15
    assert sn.census(mean[0, 0], var[0, 0]) == (2, 2, u.iloc[0]["mean_abs_activation"])


def test_the_premise_of_the_exact_gram_test():
    """On the integer-grid inputs every partial sum stays below 2^24 units of 1/4: fp32 holds every one of them exactly, in any order."""
    for H in (64, 512):
        for count in sc.GRID_COUNTS:
            for rows_of in sc.ROWS_OF:
                c = sc.grid_case(H, count, rows_of)
                assert sc.grid_premise(c) < 2 ** 24
                for ws, _, mask in c["steps"]:
                    assert np.isnan(ws[:, ~mask]).all() and np.isin(ws[:, mask], sc.GRID_VALUES).all() and not mask[count:].any()
                assert np.array_equal(c["acc"]["S"] * 4, np.rint(c["acc"]["S"] * 4)) and np.abs(c["acc"]["S"]).max() * 4 < 2 ** 24
    c = sc.grid_case(64, 320, None)
    assert c["acc"]["n"] > 2 * sc.PROMOTE_ROWS          # 320 rows cross the promotion interval, with one plane twice
    assert -(-320 // sc.CHUNK) // 2 * sc.CHUNK > sc.PROMOTE_ROWS          # ... and with two planes each plane crosses it once
    assert sc.grid_case(64, 320, 1)["acc"]["n"] > 2 and sc.grid_case(64, 13, 1)["acc"]["n"] >= 1


def test_the_command_line_entry(tmp_path, monkeypatch, capsys):
    from copo_amd.eval import checkpoint_io, evaluate
    study, = (s for s in evaluate.STUDIES if s.option == "similarity")
    assert (study.option, study.module, study.rows, study.levels, study.share, study.scenes) == (
        "similarity", "similarity", "similarity_rows", None, 0.5, "scenes_per_pair")
    assert {o: s for o, s in evaluate.GOES_WITH.items() if "similarity" in s} == dict(similarity_rows_of=("similarity",))
    table, called = str(tmp_path / "t.csv"), []

    def fake_rows(algo, env, weights_list, **kw):
        called.append((algo, env, list(weights_list), kw))
        plan = sim.SimilarityPlan(SeatPlan.pairs(2, 1, 4, 0.5), rows_of=kw["rows_of"])
        return sim.similarity_frame(np.ones((2, 2, 2)), 9, plan, kw["labels"])

    monkeypatch.setattr(sim, "similarity_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])
    base = ["--similarity", "a.npz", "b.npz"]

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        return e.value.code == 2

    assert refused(base)                                                                   # its table
    assert refused(base + ["--table", table, "--jury", "a.npz", "b.npz"])
    assert "one table per run" in capsys.readouterr().err
    assert refused(["--similarity-rows-of", "1", "--table", table])                        # without --similarity: a usage error
    assert "--similarity-rows-of goes with --similarity" in capsys.readouterr().err
    assert refused(["--jury", "a.npz", "b.npz", "--similarity-rows-of", "0", "--table", table])
    assert refused(base + ["--table", table, "--jury-plan", "seated"])                     # another study's option
    assert not called
    evaluate.main(base + ["--similarity-rows-of", "1", "--table", table, "--steps", "16", "--scenes-per-pair", "3", "--num-agents", "4"])
    evaluate.main(base + ["--table", table, "--share", "0.25"])
    (algo, env, ws, kw), (_, _, _, kw2) = called
    assert (algo, env, ws) == ("copo", "inter", ["w:a.npz", "w:b.npz"])
    assert kw == dict(num_agents=4, steps=16, labels=["a.npz", "b.npz"], scenes_per_pair=3, rows_of=1, share=0.5)
    assert kw2["rows_of"] is None and kw2["share"] == 0.25
    out = capsys.readouterr().out
    assert "cka" in out and "h2" in out
    import pandas as pd
    assert len(pd.read_csv(table)) == 2 * 2 * 2
