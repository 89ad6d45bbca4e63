"""CPU: the policy jury (copo_amd/eval/jury.py, copo_jury_obs_seats_f32, copo_jury_tally) -- the judges' lists
against a brute-force loop, the refusals of the plan and of the C entries (no device is touched), the PREMISE of the GPU cases measured
on the float64 model alone, the fold's restatement against a case written out by hand, the frames and the CLI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import jury_cases as jc
import jury_numpy as jn
from test_learner_plan_cpu import make_cfg

from copo_amd import _capi
from copo_amd.eval.crossplay import SeatPlan
from copo_amd.eval.jury import JURY_WORDS, VERDICT_WORDS, JuryPlan, jury_frame, jury_matrix, jury_rates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def seat_plans():
    odd = SeatPlan(np.array([[0, -1, 2, 2], [1, 1, -1, -1], [2, 0, 0, 1], [-1, -1, -1, -1]]), 3, np.array([0, 1, 1, 5]), 3)      # group 5: out of range
    return dict(pairs=SeatPlan.pairs(3, 2, 5, 0.4), cells=SeatPlan.cells(2, 2, 1, 4, 0.5)[0], uniform=SeatPlan.uniform([0, 1, 1, 2], 3), odd=odd)


@pytest.mark.parametrize("layout", sorted(seat_plans()))
def test_lists_counts_and_capacity_against_a_brute_force_loop(layout):
    seats = seat_plans()[layout]
    brute_seated = np.zeros((seats.n_groups, seats.K), np.int32)
    for e in range(seats.E):
        for n in range(seats.N):
            if seats.seat[e, n] >= 0 and 0 <= seats.group[e] < seats.n_groups:
                brute_seated[seats.group[e], seats.seat[e, n]] = 1
    panel = np.zeros((seats.n_groups, seats.K), np.int32)
    panel[:, [seats.K - 1, 0]] = 1
    for plan, judges in ((JuryPlan.everyone(seats), np.ones((seats.n_groups, seats.K), np.int32)), (JuryPlan.seated(seats), brute_seated),
                         (JuryPlan.panel(seats, [seats.K - 1, 0]), panel)):
        assert np.array_equal(plan.judges, judges) and plan.judges.dtype == np.int32
        rows, counts, cap = jn.jury_lists(seats.seat, seats.group, judges)
        assert plan.cap == cap and np.array_equal(plan.counts, counts) and plan.counts.dtype == np.int32
        assert np.array_equal(plan.rows, rows) and plan.rows.dtype == np.int64
        assert (plan.G, plan.K, plan.E, plan.N, plan.n_out) == (seats.n_groups, seats.K, seats.E, seats.N, seats.E * seats.N)
        assert plan.check(seats) is plan
    if layout == "pairs":          # focal and partner: two forwards per row where K = 3 would make three, one on the self-play groups
        assert JuryPlan.seated(seats).judges.sum(axis=1).tolist() == [1 if i == j else 2 for i in range(3) for j in range(3)]
        assert JuryPlan.everyone(seats).counts.tolist() == [seats.E * seats.N] * 3


def test_plan_refusals():
    seats = SeatPlan.pairs(2, 1, 4)
    for bad in (np.ones((3, 2)), np.ones((4, 3)), np.ones(8), np.ones((4, 2, 1))):
        with pytest.raises(ValueError):
            JuryPlan(seats, bad)
    for members in ([], [2], [-1], [0, 0]):
        with pytest.raises(ValueError):
            JuryPlan.panel(seats, members)
    with pytest.raises(ValueError):
        JuryPlan.named(seats, "nobody")
    plan = JuryPlan.everyone(seats)
    for other in (SeatPlan.pairs(2, 2, 4), SeatPlan.pairs(2, 1, 5), SeatPlan.pairs(3, 1, 4), SeatPlan(seats.seat, 2, np.zeros(4, np.int32), 1)):
        with pytest.raises(ValueError):
            plan.check(other)
    empty = JuryPlan(seats, np.zeros((4, 2)))          # nobody judges: lists of capacity 1, all empty
    assert empty.cap == 1 and empty.counts.tolist() == [0, 0] and empty.rows.shape == (2, 1)


def test_premise_of_the_gpu_cases():
    """Every list shape the kernel test needs is there, and no distance of the float64 model is near a threshold."""
    assert jc.GROUP.tolist() == [0, 0, 1, 1, 2, 7] and (jc.SEAT == -1).any() and (jc.SEAT[5] >= 0).all()
    lists = {}
    for t in jc.TABLES:
        rows, counts, cap = jn.jury_lists(jc.SEAT, jc.GROUP, jc.JUDGES[t])
        assert tuple(counts) == jc.COUNTS[t] and cap == 17
        lists[t] = [set(rows[j, :counts[j]].tolist()) for j in range(jc.K)]
        assert not any(r >= 40 for li in lists[t] for r in li)                     # scene 5's group is out of range
        assert not any(jc.SEAT.reshape(-1)[r] < 0 for li in lists[t] for r in li)   # nobody's slots are in nobody's list
    judges_of = lambda t, r: [j for j in range(jc.K) if r in lists[t][j]]  # noqa: E731
    assert judges_of("A", 0) == [0, 1, 2]                                            # judged by all three
    assert judges_of("A", 35) == [] and jc.SEAT[4, 3] == 0                           # seated, in a valid group, judged by none
    assert judges_of("A", 16) == [1] == [int(jc.SEAT[2, 0])]                         # only by its own driver
    assert judges_of("B", 2) == [2] == [int(jc.SEAT[0, 2])]
    assert len(lists["B"][0]) == 0                                                   # an empty list
    assert lists["B"][1] == {35}                                                     # a one-row list: a one-row masked tile
    assert len(lists["A"][1]) == len(lists["B"][2]) == 17                            # two tiles, the second a one-row masked tile
    acted = (jc.flags() & jn.F_ACTED) != 0
    assert acted.any() and not acted.all() and not acted[jc.SEAT >= 0].all()
    closest = np.inf
    for hidden in jc.HIDDENS:
        for in_dim in jc.IN_DIMS:
            v = jc.reference(hidden, in_dim)["verdict64"]
            n_apart = 0
            for t in jc.TABLES:
                for r, k, j in jc.judged_pairs(t):
                    d = np.abs(v[r, j, :2] - v[r, k, :2])
                    closest = min(closest, float(np.abs(d - np.array(jc.DELTAS)).min()))
                    n_apart += int(j != k and (d > np.array(jc.DELTAS)).any())
            n_off = sum(j != k for t in jc.TABLES for _, k, j in jc.judged_pairs(t))
            assert 0 < n_apart < n_off, (hidden, in_dim)                             # both outcomes occur in every case
    print("closest |d_a - delta_a| of the float64 model: %.3e" % closest)
    assert closest > jc.MARGIN


def hand_case():
    """Two scenes x four slots, two members, one group (scene 1 is in group 3, out of range), both members judge.  Six counted pairs:
    slots 0, 1 and 3 of scene 0 under both judges; slot 2 did not act.  Deltas (0.2, 0.5)."""
    seat = np.array([[0, 1, 0, 0], [0, 1, 0, 1]], np.int32)
    group = np.array([0, 3], np.int32)
    flags = np.array([[1, 1 | 2, 64, 1], [1, 1, 1, 1]], np.uint8)
    dist = np.zeros((2, 4, 4), F)
    verdict = np.zeros((8, 2, 4), F)
    dist[0, 0] = verdict[0, 0] = (0.5, -0.25, 0.0, 0.0)          # slot 0, driven by 0: its own verdict is its own bits
    verdict[0, 1] = (0.75, -0.25, 0.0, 0.0)                      # judge 1: 0.25 apart in steer, equal stds
    dist[0, 1] = verdict[1, 1] = (0.0, 0.0, 0.0, 0.0)            # slot 1, driven by 1
    verdict[1, 0] = (0.0, 0.5, 0.5, -0.5)                        # judge 0: throttle exactly AT its delta, both log-stds 0.5 away
    dist[0, 2] = (9.0, 9.0, 9.0, 9.0)                            # slot 2 did not act: never read
    verdict[2] = 1.0
    dist[0, 3] = verdict[3, 0] = (0.0, 0.0, 0.0, 0.0)            # slot 3, driven by 0
    verdict[3, 1] = (np.nan, 0.125, 0.0, 0.0)                    # judge 1: a NaN steer mean
    dist[1] = 3.0
    verdict[4:] = -3.0
    e = math.e
    want = np.zeros((1, 2, 2, 8), np.int64)
    want[0, 0, 0] = [2, 0, 0, 0, 0, 0, 0, 0]
    # slot 0: d = (0.25, 0), KL = 0.5 * 0.25^2 both ways; slot 3: d = (NaN -> 0, 0.125), KL NaN -> 0, the max takes the other axis
    want[0, 0, 1] = [2, 1, 16384, 8192, 0, 2048, 2048, 16384]
    # slot 1: d = (0, 0.5), |dlogstd| = 0.5 + 0.5; KL(driver || judge) = 0.5 / e + (-1 + 0.625 e); KL(judge || driver) = (-1 + 0.5 e) + (0.5 / e + 0.125)
    want[0, 1, 0] = [1, 0, 0, 32768, 65536, round((0.5 / e - 1.0 + 0.625 * e) * 65536), round((-0.875 + 0.5 * e + 0.5 / e) * 65536), 32768]
    want[0, 1, 1] = [1, 0, 0, 0, 0, 0, 0, 0]
    return dict(seat=seat, group=group, flags=flags, dist=dist, verdict=verdict, judges=np.ones((1, 2), np.int32), deltas=(0.2, 0.5), want=want)


def test_fold_on_a_hand_made_case():
    h = hand_case()
    out = jn.jury_fold(h["flags"], h["dist"], h["verdict"], h["seat"], h["group"], h["judges"], h["deltas"])
    assert out[..., 0].sum() == 6
    assert np.array_equal(out, h["want"]), (out, h["want"])
    again = jn.jury_fold(h["flags"], h["dist"], h["verdict"], h["seat"], h["group"], h["judges"], h["deltas"], out.copy())
    assert np.array_equal(again[..., :7], 2 * out[..., :7]) and np.array_equal(again[..., 7], out[..., 7])
    none = jn.jury_fold(h["flags"], h["dist"], h["verdict"], h["seat"], h["group"], np.array([[0, 1]], np.int32), h["deltas"])
    assert not none[:, :, 0].any() and np.array_equal(none[:, :, 1], h["want"][:, :, 1])


def test_fold_diagonal_is_zero_and_kl_swaps_with_the_roles():
    v = jc.reference(64, 91)["verdict64"].astype(F)
    seat = jc.SEAT.reshape(-1)
    dist = v[np.arange(len(seat)), np.clip(seat, 0, jc.K - 1)]          # the driver's own numbers
    for t in jc.TABLES:
        out = jn.jury_fold(jc.flags(), dist, v, jc.SEAT, jc.GROUP, jc.JUDGES[t], jc.DELTAS)
        for g in range(jc.G):
            for k in range(jc.K):
                if jc.JUDGES[t][g, k]:
                    assert not out[g, k, k, 1:].any(), (t, g, k)
        assert out[..., 0].sum() > 0 and out[..., 1].sum() > 0 and out[..., 5].sum() > 0
        assert not out[:, :, :, 0][jc.JUDGES[t][:, None, :].repeat(jc.K, 1) == 0].any()
    for r, k, j in jc.judged_pairs("A"):
        a, b = jn.pair_words(v[r, k], v[r, j], jc.DELTAS), jn.pair_words(v[r, j], v[r, k], jc.DELTAS)
        assert a[5] == b[6] and a[6] == b[5] and a[:5] == b[:5] and a[7] == b[7]
        assert jn.kl(v[r, k], v[r, j]) >= 0.0 and (jn.kl(v[r, k], v[r, j]) > 0.0) == (j != k)


def synthetic_words(seats, jury):
    rng = np.random.RandomState(7)
    tally = rng.randint(1, 1 << 20, (seats.n_groups, seats.K, seats.K, 8)).astype(np.int64)
    tally[..., 1] = tally[..., 0] // 2
    for k in range(seats.K):
        tally[:, k, k, 1:] = 0
    return tally


def test_rates_frame_and_matrix_on_synthetic_words():
    r = jury_rates([4, 1, 2 * 65536, 65536, 0, 3 * 65536, 65536, 32768])
    assert r == dict(disagree_rate=0.25, d_steer=0.5, d_throttle=0.25, d_logstd=0.0, kl_driver_judge=0.75, kl_judge_driver=0.25, sym_kl=0.5, max_dev=0.5)
    assert all(math.isnan(v) for v in jury_rates([0] * 8).values())
    assert len(JURY_WORDS) == 8 and len(VERDICT_WORDS) == 4
    seats = SeatPlan.pairs(3, 2, 6, 0.5)
    for kind, per_group in (("seated", lambda i, j: 1 if i == j else 4), ("everyone", lambda i, j: 3 if i == j else 6)):
        jury = JuryPlan.named(seats, kind)
        tally = synthetic_words(seats, jury)
        df = jury_frame(tally, seats, jury, labels=["a", "b", "c"], deltas=(0.05, 0.1))
        assert list(df.columns) == ["group", "focal", "partner", "driver", "judge", "driver_label", "judge_label", "delta_steer", "delta_throttle",
                                    *JURY_WORDS, "disagree_rate", "d_steer", "d_throttle", "d_logstd", "kl_driver_judge", "kl_judge_driver",
                                    "sym_kl", "max_dev"]
        assert len(df) == sum(per_group(i, j) for i in range(3) for j in range(3))          # one row per (pair, driver, judge)
        assert not df.duplicated(["group", "driver", "judge"]).any()
        for row in df.itertuples():
            assert row.driver in (row.focal, row.partner) and jury.judges[row.group, row.judge] == 1
            assert [getattr(row, w) for w in JURY_WORDS] == tally[row.group, row.driver, row.judge].tolist()
            assert row.driver_label == "abc"[row.driver] and row.judge_label == "abc"[row.judge]
        m = jury_matrix(df, 3)
        assert m.shape == (3, 3) and np.allclose(m.to_numpy(), m.to_numpy().T, equal_nan=True) and (np.diag(m.to_numpy()) == 0.0).all()
        kl = np.zeros((3, 3))
        n = np.zeros((3, 3))
        for row in df.itertuples():
            kl[row.driver, row.judge] += row.kl_driver_judge_q16 + row.kl_judge_driver_q16
            n[row.driver, row.judge] += row.pairs
        assert np.allclose(m.to_numpy(), (kl + kl.T) / (2 * 65536.0 * (n + n.T)))
    plain = jury_frame(synthetic_words(seats, jury), SeatPlan(seats.seat, 3, seats.group, 9), JuryPlan.everyone(seats))
    assert "focal" not in plain.columns and "delta_steer" not in plain.columns and plain.driver_label.tolist() == plain.driver.tolist()


def test_cli_arguments(tmp_path, monkeypatch):
    from copo_amd.eval import checkpoint_io, jury
    from copo_amd.eval.evaluate import main
    table = str(tmp_path / "t.csv")
    levels = tmp_path / "levels.json"
    levels.write_text("[{}]")
    for bad in (["--jury", "a.npz", "b.npz"],                                                   # no table
                ["--jury", "a.npz", "--table", table, "--cross-play", "a.npz", "b.npz"],
                ["--jury", "a.npz", "--table", table, "--certify-sweep", "a.npz", "--certify-levels", str(levels)],
                ["--jury", "a.npz", "--table", table, "--fault-sweep", "a.npz", "--fault-levels", str(levels)],
                ["--jury", "a.npz", "--table", table, "--jury-plan", "nobody"],
                ["--jury", "a.npz", "--table", table, "--jury-deltas", "0.1"],
                ["--jury", "a.npz", "--table", table, "--jury-deltas", "-0.1", "0.1"],
                ["--jury-plan", "seated", "--table", table], ["--jury-deltas", "0.1", "0.1", "--table", table]):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert e.value.code == 2, bad
    seen = {}
    seats = SeatPlan.pairs(2, 1, 4)
    plan = JuryPlan.seated(seats)

    def fake_rows(algo, env, weights_list, **kw):
        seen.update(kw, algo=algo, env=env, weights=list(weights_list))
        return jury_frame(synthetic_words(seats, plan), seats, plan, kw["labels"], kw["deltas"])

    monkeypatch.setattr(jury, "jury_rows", fake_rows)
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])
    main(["--algo", "ippo", "--jury", "a.npz", "b.npz", "--jury-plan", "seated", "--jury-deltas", "0.1", "0.2", "--table", table, "--steps", "16",
          "--scenes-per-pair", "1", "--num-agents", "4", "--share", "0.25"])
    assert seen == dict(algo="ippo", env="inter", weights=["w:a.npz", "w:b.npz"], plan="seated", share=0.25, deltas=(0.1, 0.2), scenes_per_pair=1,
                        num_agents=4, steps=16, labels=["a.npz", "b.npz"])
    assert os.path.getsize(table) > 0
    main(["--jury", "a.npz", "b.npz", "--table", table])
    assert (seen["plan"], seen["deltas"], seen["share"]) == ("everyone", (0.05, 0.05), 0.5)


def test_header_declares_both_entries_and_the_bindings_match():
    header = open(os.path.join(ROOT, "include", "copo_hip.h")).read()
    assert "#define COPO_JURY_WORDS 8" in header
    for name in ("copo_jury_obs_seats_f32", "copo_jury_tally"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_capi._SIGS[name][1]), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.lib, name)
    assert _capi.lib.copo_version() == 8 == _capi.ABI_VERSION
    from copo_amd import trainer
    assert jn.F_ACTED == trainer.F_ACTED


def test_entries_refuse_before_they_touch_a_device():
    null, dim = -1, -2
    cfg = make_cfg(hidden=64, in_pol=91, in_val=())
    buf = np.zeros(64, np.int64)          # host memory: a refused call reads none of it
    p = buf.ctypes.data
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p += p % 16
    good = dict(cfg=C.byref(cfg), theta=p, theta_t=p, member_stride=cfg.n_params, n_members=3, rows=p, counts=p, cap=32, n_out=48, obs_src=p,
                verdict=p, stream=None)
    call = lambda **kw: _capi.lib.copo_jury_obs_seats_f32(*dict(good, **kw).values())  # noqa: E731
    for name in ("cfg", "theta", "theta_t", "rows", "counts", "obs_src", "verdict"):
        assert call(**{name: None}) == null, name
    for bad in (dict(n_members=0), dict(n_members=65536), dict(cap=0), dict(n_out=0), dict(member_stride=cfg.n_params - 4),
                dict(member_stride=cfg.n_params + 2), dict(theta_t=p + 4)):
        assert call(**bad) == dim, bad
    assert call(cfg=C.byref(make_cfg(hidden=64, in_pol=91, in_val=(), bf16=True))) == dim          # fp32 operands only, as the adversary pass
    for hidden in (96, 32, 1024):
        c = make_cfg(hidden=hidden, in_pol=91, in_val=())
        assert call(cfg=C.byref(c), member_stride=c.n_params) == dim, hidden
    tgood = dict(flags=p, dist=p, verdict=p, seat=p, group=p, judges=p, E=4, N=8, K=2, G=3, delta_steer=0.05, delta_throttle=0.05, out=p, stream=None)
    tally = lambda **kw: _capi.lib.copo_jury_tally(*dict(tgood, **kw).values())  # noqa: E731
    for name in ("flags", "dist", "verdict", "seat", "group", "judges", "out"):
        assert tally(**{name: None}) == null and b"copo_jury_tally" in _capi.lib.copo_last_error(), name
    for bad in (dict(E=-1), dict(N=0), dict(N=257), dict(K=0), dict(K=65536), dict(G=0), dict(dist=p + 4), dict(verdict=p + 8)):
        assert tally(**bad) == dim, bad
    assert tally(E=0) == 0          # nothing to do, nothing launched
