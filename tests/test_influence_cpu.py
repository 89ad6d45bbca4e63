"""CPU: the influence graph (copo_amd/eval/influence.py, copo_influence_*) -- the rule's restatement
(tests/influence_numpy.py) on a table written out by hand: owners, ties, min2, candidate order, truncation, the variant rows, the list
builder and the eight words; the frame's rates, the argument checks of the buffers, the C entries (no device is touched) and the CLI."""
import os
import re

import numpy as np
import pytest

import influence_cases as ic
import influence_numpy as inf
import jury_numpy as jn

from copo_amd import _capi
from copo_amd.eval.crossplay import SeatPlan
from copo_amd.eval.influence import (EDGE_DTYPE, INFLUENCE_WORDS, InfluenceBuffers, edges_array, influence_frame, influence_rates)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_owners_ties_and_min2():
    d, s = ic.table()
    min1, owner, min2 = inf.beams(d, s, ic.RNG)
    assert np.array_equal(owner, ic.WANT_OWNER)
    for (a, b), v in ic.WANT_MIN2.items():
        assert min2[a, b] == F(v), (a, b)
    assert min1[0, 0] == F(7.5) and owner[0, 0] == 1                        # two vehicles at equal distance: the lower slot, min2 == min1
    assert min1[0, 3] == F(20.0) and owner[0, 3] == -1                      # a box tying a vehicle: nobody owns the beam
    assert min1[0, 4] == F(6.0) and owner[0, 4] == -1                       # a box in front of a vehicle
    assert min1[3, 3] == F(ic.RNG) and owner[3, 3] == -1                    # a hit beyond the range is no hit
    assert min1[3, 5] == F(0.0) and owner[3, 5] == 0                        # distance zero is a hit
    assert (min2 >= min1).all() and (min1[2] == F(ic.RNG)).all()


def test_candidate_order_and_truncation():
    d, s = ic.table()
    min1, owner, _ = inf.beams(d, s, ic.RNG)
    who, kept, trunc, hit = inf.candidates(min1, owner, 4)
    assert np.array_equal(who, ic.WANT_WHO4) and kept.tolist() == [2, 4, 0, 1] and not trunc.any()
    assert hit[1].tolist() == [2.0, 5.0, 5.0, 12.5]                          # equal smallest distances: the lower slot first
    who2, kept2, trunc2, _ = inf.candidates(min1, owner, 2)
    assert np.array_equal(who2, ic.WANT_WHO2) and kept2.tolist() == [2, 2, 0, 1] and np.array_equal(trunc2, ic.WANT_TRUNC2)
    assert 3 not in who[0][who[0] >= 0] or owner[0, 2] == 3                  # vehicle 3 is a candidate by beam 2 alone (occluded on beam 1)


def test_variant_rows():
    d, s = ic.table()
    min1, owner, min2 = inf.beams(d, s, ic.RNG)
    who, kept, _, _ = inf.candidates(min1, owner, 4)
    obs = np.arange(4 * 10, dtype=F).reshape(4, 10) + 100.0
    inv = F(1.0) / F(ic.RNG)
    rows = inf.variants(obs, 3, min1, owner, min2, who, inv)
    assert sorted(rows) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3), (3, 0)]
    r = rows[0, 0]                                                           # vehicle 1 out: beam 0 stays (the tie), beam 1 shows vehicle 3
    assert np.array_equal(r[:3], obs[0, :3]) and r[9] == obs[0, 9]
    assert r[3:9].tolist() == [F(7.5) * inv, F(12.0) * inv, F(15.0) * inv, F(20.0) * inv, F(6.0) * inv, F(40.0) * inv]
    assert rows[0, 1][5] == F(40.0) * inv and rows[0, 1][4] == F(9.0) * inv  # vehicle 3 out: only the beam it owns moves
    assert rows[3, 0][3:9].tolist() == [1.0] * 6                             # the only vehicle out: an empty scene


def test_list_builder():
    seat = np.array([[0, 1, 0, -1], [1, 1, 0, 0]])
    plan = SeatPlan(seat, 3)
    kept = np.array([2, 0, 1, 3, 0, 4, 0, 1])                               # (row 3 is nobody's: its count is never read)
    vrows, vcounts = inf.variant_lists(plan.rows, plan.counts, kept, 4)
    assert vcounts.tolist() == [4, 4, 0] and vrows.shape == (3, plan.cap * 4)
    assert vrows[0, :4].tolist() == [0, 1, 8, 28] and vrows[1, :4].tolist() == [20, 21, 22, 23]
    assert (np.diff(vrows[0, :4]) > 0).all()                                 # ascending
    none, zero = inf.variant_lists(plan.rows, plan.counts, np.zeros(8, int), 4)
    assert not zero.any()                                                    # no candidates anywhere: empty lists


def hand_fold():
    """Two scenes of three slots, two members, M = 2."""
    seat, group = np.array([[0, 1, -1], [1, 1, 0]]), np.array([0, 1])
    flags = np.array([1, 1, 1, 0, 1, 1], np.uint8)                           # row 3 is no ego; row 2 is nobody's seat
    who = np.array([[1, 2], [0, -1], [0, 1], [-1, -1], [-1, -1], [3, 4]])
    trunc = np.array([0, 3, 9, 0, 0, 1])
    dist = np.zeros((6, 4), F)
    dist[:, 2:] = -0.5
    v = np.zeros((12, 2, 4), F)
    v[..., 2:] = -0.5
    v[0, 0, 0] = 0.25           # row 0 cand 0, member 0: steer moves by 0.25
    v[1, 0, 1] = -0.03125       # row 0 cand 1: throttle by 1/32 (below the delta)
    v[2, 1, 0] = 2000.0         # row 1 cand 0, member 1: beyond the clamp of q
    v[2, 0, 0] = 7.0            # (another member's plane: never read)
    v[10, 0, :2] = (0.0625, -0.5)
    v[11, 0, 3] = -0.25         # row 5 cand 1: only the log-std moves -- KL, no shift
    want = np.zeros((2, 2, 8), np.int64)
    kl = lambda q: jn.q16(jn.kl(dist[0], q))  # noqa: E731
    want[0, 0] = (1, 2, 1, 16384, 2048, kl(v[0, 0]) + kl(v[1, 0]), 16384, 0)
    want[0, 1] = (1, 1, 1, 1024 * 65536, 0, kl(v[2, 1]), 1024 * 65536, 3)
    want[1, 1] = (1, 0, 0, 0, 0, 0, 0, 0)
    want[1, 0] = (1, 2, 1, 4096, 32768, kl(v[10, 0]) + kl(v[11, 0]), 32768, 1)
    return dict(seat=seat, group=group, flags=flags, who=who, trunc=trunc, dist=dist, verdict_cf=v, want=want)


def test_the_eight_words_on_a_case_written_out_by_hand():
    h = hand_fold()
    got = inf.fold(h["flags"], h["dist"], h["verdict_cf"], h["who"], h["trunc"], h["seat"], h["group"], 2, 2, ic.DELTAS)
    assert np.array_equal(got, h["want"]), (got, h["want"])
    assert h["want"][0, 1, 5] == 1024 * 65536 and h["want"][1, 0, 5] > 0
    twice = inf.fold(h["flags"], h["dist"], h["verdict_cf"], h["who"], h["trunc"], h["seat"], h["group"], 2, 2, ic.DELTAS, got.copy())
    assert np.array_equal(twice[..., [0, 1, 2, 3, 4, 5, 7]], 2 * got[..., [0, 1, 2, 3, 4, 5, 7]]) and np.array_equal(twice[..., 6], got[..., 6])


def test_frame_rates_and_edges():
    r = influence_rates([4, 6, 3, 65536, 32768, 131072, 16384, 2])
    assert r == dict(others_per_ego=1.5, moved_rate=0.5, mean_d_steer=1.0 / 6, mean_d_throttle=0.5 / 6, mean_kl=2.0 / 6, max_dev=0.25,
                     truncated_rate=0.25)
    empty = influence_rates([3, 0, 0, 0, 0, 0, 0, 0])                        # egos without candidates
    assert empty["others_per_ego"] == 0.0 and all(v != v for k, v in empty.items() if k != "others_per_ego")
    assert all(v != v for v in influence_rates([0] * 8).values())
    seats = SeatPlan.pairs(2, 1, 4)
    tally = np.arange(4 * 2 * 8, dtype=np.int64).reshape(4, 2, 8) + 1
    df = influence_frame(tally, seats, ["a", "b"], (0.1, 0.2))
    assert list(df.columns) == ["group", "focal", "partner", "member", "label", "delta_steer", "delta_throttle", *INFLUENCE_WORDS, "others_per_ego",
                                "moved_rate", "mean_d_steer", "mean_d_throttle", "mean_kl", "max_dev", "truncated_rate"]
    assert [(x.focal, x.partner, x.member) for x in df.itertuples()] == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 1)]
    row = df.iloc[2]
    assert [row[w] for w in INFLUENCE_WORDS] == tally[1, 1].tolist() and row["label"] == "b"
    assert row["truncated_rate"] == tally[1, 1, 7] / (tally[1, 1, 1] + tally[1, 1, 7])
    lone = SeatPlan(np.array([[0, 0, -1]]), 2)                               # a member without seats has no row
    assert influence_frame(np.ones((1, 2, 8), np.int64), lone)["member"].tolist() == [0]
    who = np.array([[2, -1], [-1, -1], [0, 1], [-1, -1]])
    edges = np.arange(4 * 2 * 4, dtype=F).reshape(4, 2, 4)
    e = edges_array(who, edges, 2)
    assert e.dtype == EDGE_DTYPE and e["scene"].tolist() == [0, 1, 1] and e["ego_slot"].tolist() == [0, 0, 0]
    assert e["other_slot"].tolist() == [2, 0, 1] and e["kl"].tolist() == [2.0, 18.0, 22.0] and e["hit"].tolist() == [3.0, 19.0, 23.0]


def test_buffers_check_their_arguments():
    seats = SeatPlan(np.array([[0, 1, -1], [1, 1, 0]]), 3)                  # member 2 has no seat
    b = InfluenceBuffers(seats, 91, 72, 4, "cpu")
    assert (b.K, b.cap, b.E, b.N, b.G, b.M, b.O, b.L) == (3, 3, 2, 3, 1, 4, 91, 72) and b.n_out == 6
    assert tuple(b.who.shape) == (6, 4) and int(b.who.max()) == -1 and tuple(b.obs_cf.shape) == (24, 91) and tuple(b.vrows.shape) == (3, 12)
    assert tuple(b.verdict_cf.shape) == (24, 3, 4) and tuple(b.tally.shape) == (1, 3, 8) and tuple(b.edges.shape) == (6, 4, 4)
    assert tuple(b.heading.shape) == (6, 2) and tuple(b.clean.shape) == (6, 72)
    b.tally += 1
    b.heading += 1
    b.clear_tally()
    b.clear_heading()
    assert not b.tally.any() and not b.heading.any()
    for bad in (dict(max_others=0), dict(max_others=9), dict(max_others=2.5), dict(O=0), dict(L=0), dict(L=92), dict(seats=seats.seat)):
        with pytest.raises(ValueError):
            InfluenceBuffers(**dict(dict(seats=seats, O=91, L=72, max_others=4, device="cpu"), **bad))


@pytest.mark.parametrize("shape", ic.TALLY_SHAPES, ids=str)
def test_premise_of_the_stand_alone_fold(shape):
    """What test_gpu_influence.py::test_tally_alone_is_exact relies on, measured on the model alone: every shape has pairs, some moved and
    some not, truncated candidates, a max word at the clamp, out-of-range groups, empty seats, rows that did not act and candidate holes."""
    E, N, K, G, M = shape
    t = ic.tally_tables(shape)
    want = inf.fold(t["flags"], t["dist"], t["verdict_cf"], t["who"], t["ncand"] >> 16, t["seat"], t["group"], K, G, ic.DELTAS)
    pairs, moved = int(want[..., 1].sum()), int(want[..., 2].sum())
    print(shape, "egos %d pairs %d moved %d truncated %d" % (want[..., 0].sum(), pairs, moved, want[..., 7].sum()))
    assert pairs > 0 and 0 < moved < pairs and want[..., 7].sum() > 0 and want[..., 6].max() == 1024 * 65536
    assert (t["seat"] == -1).any() and (t["who"] == -1).any() and not (t["flags"] & inf.F_ACTED).all() and np.isnan(t["verdict_cf"]).any()
    if E >= 3:
        assert len(set(t["seat"][1]) - {-1}) == 1 and 0 <= t["group"][1] < G
        assert all(t["group"][e] == g and g in (-1, G) for e, g in ic.TALLY_BAD_GROUPS[shape].items())
    if K >= 64:
        assert len(set(t["seat"][0, :64])) == 64 and (t["flags"][:64] & inf.F_ACTED).all() and 0 <= t["group"][0] < G
    assert {g for bad in ic.TALLY_BAD_GROUPS.values() for g in bad.values()} == {-1, 1, 5}          # -1 and G both occur


def test_header_declares_the_entries_and_the_bindings_match():
    header = open(os.path.join(ROOT, "include", "copo_hip.h")).read()
    assert "#define COPO_INFL_MAX 8" in header and "#define COPO_INFL_WORDS 8" in header
    for name in ("copo_influence_heading", "copo_influence_obs", "copo_influence_lists", "copo_influence_tally"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_capi._SIGS[name][1]), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, name)
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION
    assert len(INFLUENCE_WORDS) == 8 and inf.F_ACTED == jn.F_ACTED


def test_entries_refuse_before_they_touch_a_device():
    null, dim = -1, -2
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    p += p % 16
    assert _capi.lib.copo_influence_heading(None, p, p, None) == null and _capi.lib.copo_influence_obs(None, p, p, p, 4, p, p + 8, p, p, p, p, None) == null
    lgood = dict(rows=p, counts=p, K=2, cap=8, n_out=16, ncand=p, M=4, vrows=p, vcounts=p, stream=None)
    lists = lambda **kw: _capi.lib.copo_influence_lists(*dict(lgood, **kw).values())  # noqa: E731
    for name in ("rows", "counts", "ncand", "vrows", "vcounts"):
        assert lists(**{name: None}) == null and b"copo_influence_lists" in _capi.lib.copo_last_error(), name
    for bad in (dict(K=0), dict(K=65536), dict(cap=0), dict(n_out=0), dict(M=0), dict(M=9), dict(cap=2 ** 29)):
        assert lists(**bad) == dim, bad
    tgood = dict(flags=p, dist=p, verdict_cf=p, who=p, ncand=p, hit=p, seat=p, group=p, E=4, N=8, K=2, G=3, M=4, ds=0.05, dt=0.05, out=p, edges=p,
                 stream=None)
    tally = lambda **kw: _capi.lib.copo_influence_tally(*dict(tgood, **kw).values())  # noqa: E731
    for name in ("flags", "dist", "verdict_cf", "who", "ncand", "seat", "group", "out"):
        assert tally(**{name: None}) == null and b"copo_influence_tally" in _capi.lib.copo_last_error(), name
    for bad in (dict(E=-1), dict(N=0), dict(N=257), dict(K=0), dict(K=65536), dict(G=0), dict(M=0), dict(M=9), dict(dist=p + 4), dict(verdict_cf=p + 8),
                dict(edges=p + 4)):
        assert tally(**bad) == dim, bad
    assert tally(E=0) == 0


def test_cli_arguments(tmp_path, monkeypatch):
    from copo_amd.eval import checkpoint_io, influence
    from copo_amd.eval.evaluate import main
    table = str(tmp_path / "t.csv")
    for bad in (["--influence", "a.npz", "b.npz"],                                                   # no table
                ["--influence", "a.npz", "--table", table, "--cross-play", "a.npz", "b.npz"],
                ["--influence", "a.npz", "--table", table, "--jury", "a.npz"],
                ["--influence", "a.npz", "--table", table, "--influence-max", "0"],
                ["--influence", "a.npz", "--table", table, "--influence-max", "9"],
                ["--influence", "a.npz", "--table", table, "--influence-deltas", "0.1"],
                ["--influence", "a.npz", "--table", table, "--influence-deltas", "-0.1", "0.1"],
                ["--influence-max", "2", "--table", table], ["--influence-deltas", "0.1", "0.1", "--table", table]):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert e.value.code == 2, bad
    seen = {}
    seats = SeatPlan.pairs(2, 1, 4)

    def fake_rows(algo, env, weights_list, **kw):
        seen.update(kw, algo=algo, env=env, weights=list(weights_list))
        return influence_frame(np.ones((4, 2, 8), np.int64), seats, kw["labels"], kw["deltas"])

    monkeypatch.setattr(influence, "influence_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])
    main(["--algo", "ippo", "--influence", "a.npz", "b.npz", "--influence-max", "6", "--influence-deltas", "0.1", "0.2", "--table", table, "--steps",
          "16", "--scenes-per-pair", "1", "--num-agents", "4", "--share", "0.25"])
    assert seen == dict(algo="ippo", env="inter", weights=["w:a.npz", "w:b.npz"], share=0.25, max_others=6, deltas=(0.1, 0.2), scenes_per_pair=1,
                        num_agents=4, steps=16, labels=["a.npz", "b.npz"])
    assert os.path.getsize(table) > 0
    main(["--influence", "a.npz", "b.npz", "--table", table])
    assert (seen["max_others"], seen["deltas"], seen["share"]) == (4, (0.05, 0.05), 0.5)
