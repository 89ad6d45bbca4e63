"""CPU: what the evaluation samplers and entry points share -- the tally's derived rates, labels, the scene lookup, the seeds of
replicated scenes and their declaration on a `SeatPlan`, the tables a captured graph reads (on CPU tensors), and the session that
always stops its trainer."""
import math

import numpy as np
import pytest

from copo_amd.eval import evaluate as EV
from copo_amd.eval.bank import DeviceTables, replica_seeds
from copo_amd.eval.crossplay import SEAT_WORDS, PlanBuffers, SeatPlan, tally_rates
from copo_amd.eval.faults import FaultBuffers, FaultLevel, FaultPlan

RATES = ("success", "crash_rate", "out_rate", "reward_per_step")


def test_tally_rates_on_words_written_out_by_hand():
    assert SEAT_WORDS == ("acted", "done", "arrive", "crash", "out", "maxstep", "reward_q16", "spawned")
    #        acted done arrive crash out maxstep reward_q16 spawned
    words = [200, 8, 5, 2, 1, 0, 3 * 65536 + 32768, 9]
    r = tally_rates(words)
    assert tuple(r) == RATES
    assert r == dict(success=5 / 8, crash_rate=2 / 8, out_rate=1 / 8, reward_per_step=3.5 / 200)
    assert tally_rates(np.array(words, np.int64)) == r                       # a row of the device's tally as it comes
    r = tally_rates([200, 0, 0, 0, 0, 0, -65536, 0])                         # nobody finished: the three rates over `done` have no value
    assert all(math.isnan(r[k]) for k in RATES[:3]) and r["reward_per_step"] == -1.0 / 200
    r = tally_rates([0] * 8)                                                 # nobody acted either
    assert all(math.isnan(v) for v in r.values())
    r = tally_rates([0, 4, 4, 0, 0, 0, 0, 0])                                # the two denominators are independent
    assert r["success"] == 1.0 and math.isnan(r["reward_per_step"])


def test_check_labels_default_and_length_error():
    assert EV.check_labels(None, 3) == [0, 1, 2] and EV.check_labels(("a", "b"), 2) == ["a", "b"] and EV.check_labels(None, 0) == []
    with pytest.raises(ValueError, match="2 labels for 3 members"):
        EV.check_labels(["a", "b"], 3)


@pytest.mark.parametrize("name,want", [("MultiAgentRoundaboutEnv", ("MultiAgentRoundaboutEnv", "Round")),
                                       ("CCMultiAgentIntersectionEnv", ("MultiAgentIntersectionEnv", "Inter")),
                                       ("LCFMultiAgentParkingLotEnv", ("MultiAgentParkingLotEnv", "Parking")),
                                       ("MultiAgentBottleneckEnv", ("MultiAgentBottleneckEnv", "Bottle")),
                                       ("MultiAgentTollgateEnv", ("MultiAgentTollgateEnv", "Tollgate"))])
def test_scene_of_every_scene(name, want):
    assert EV.scene_of(name) == want and want[0] in EV.ENVS.values()


def test_scene_of_an_unknown_name_raises_with_the_callers_message():
    with pytest.raises(ValueError) as e:
        EV.scene_of("MultiAgentHighwayEnv")
    assert e.value.args == ()                                                # `get_env`'s bare error
    with pytest.raises(ValueError, match="trial t0: unknown scene"):
        EV.scene_of("MultiAgentHighwayEnv", "trial t0: unknown scene 'MultiAgentHighwayEnv'")


@pytest.mark.parametrize("start_seed,S,E", [(5000, 3, 12), (0, 1, 4), (7, 4, 4), (2 ** 40, 2, 6)])
def test_replica_seeds_are_one_replicas_seeds_tiled(start_seed, S, E):
    got = replica_seeds(start_seed, S, E)
    assert got.dtype == np.uint64 and np.array_equal(got, np.tile(start_seed + np.arange(S), E // S).astype(np.uint64))
    assert len(got) == E and len(set(got.tolist())) == S


def test_replica_scenes_is_declared_validated_and_passed_by_the_builders():
    seat = np.zeros((6, 4), np.int32)
    assert SeatPlan(seat).replica_scenes is None and SeatPlan.uniform(np.arange(6) // 3, 4).replica_scenes is None
    assert SeatPlan(seat, replica_scenes=3).replica_scenes == 3 and SeatPlan(seat, replica_scenes=6).replica_scenes == 6
    for bad in (4, 0, -1, 12):
        with pytest.raises(ValueError, match="replicas"):
            SeatPlan(seat, replica_scenes=bad)
    plan = SeatPlan.pairs(2, 3, 4, 0.5)
    assert plan.replica_scenes == 3 and plan.E == 12 and not hasattr(plan, "scenes_per_pair")
    calls = []
    init = SeatPlan.__init__

    def recording_init(self, *a, **kw):
        calls.append(kw.get("replica_scenes"))
        init(self, *a, **kw)
    SeatPlan.__init__ = recording_init
    try:
        seats, faults = FaultPlan.sweep(2, [FaultLevel(), FaultLevel(sticky=0.5)], 3, 4, 0.5)
    finally:
        SeatPlan.__init__ = init
    assert calls == [3] and seats.replica_scenes == 3 == faults.scenes_per_cell       # through the constructor, not bolted on
    assert FaultPlan([FaultLevel()], [[0]]).scenes_per_cell is None


def _ptrs(tables, names):
    return [getattr(tables, n).data_ptr() for n in names]


def test_device_tables_copy_in_place_or_rebuild_and_tell():
    names = ("rows", "counts", "seat", "group")
    a = SeatPlan(np.array([[0, 1, 1], [1, 0, -1]], np.int32), n_members=2, group=[0, 1])
    b = SeatPlan(np.array([[1, 0, 0], [0, 1, -1]], np.int32), n_members=2, group=[1, 0])          # the same K, cap, E, N, groups
    c = SeatPlan(np.array([[1, 1, 1], [1, 1, 0]], np.int32), n_members=2, group=[1, 0])           # cap 5, not 3
    pb = PlanBuffers(a, "cpu")
    assert isinstance(pb, DeviceTables) and pb.plan is a and (pb.K, pb.cap, pb.E, pb.N, pb.G, pb.n_out) == (2, 3, 2, 3, 2, 6)
    assert pb.same_shape(PlanBuffers.tables(b)[1]) and not pb.same_shape(PlanBuffers.tables(c)[1])
    told = []
    pb.on_replace.append(lambda: told.append(1))
    before = _ptrs(pb, names)
    pb.copy_in(b)
    assert _ptrs(pb, names) == before and pb.plan is b
    for n in names:
        assert np.array_equal(getattr(pb, n).numpy(), getattr(b, n)) and not np.array_equal(getattr(a, n), getattr(b, n)), n
    pb.replace(a)                                                            # the same key: copied in, nobody is told
    assert _ptrs(pb, names) == before and told == [] and pb.plan is a and np.array_equal(pb.seat.numpy(), a.seat)
    old = [getattr(pb, n) for n in names]                                    # (kept alive: a freed block could be handed out again)
    pb.replace(c)                                                            # another key: new tensors, told exactly once
    assert told == [1] and pb.plan is c and pb.cap == 5 and tuple(pb.rows.shape) == (2, 5)
    assert all(p != q for p, q in zip(_ptrs(pb, names), before)) and np.array_equal(old[2].numpy(), a.seat)
    for n in names:
        assert np.array_equal(getattr(pb, n).numpy(), getattr(c, n)), n
    # the fault tables declare other arrays and another key; the level words travel as their bits
    f1 = FaultPlan([FaultLevel(), FaultLevel(lidar_sigma=0.5)], [[0, 1]])
    f2 = FaultPlan([FaultLevel(sticky=1.0), FaultLevel()], [[1, 0]])
    fb = FaultBuffers(f1, "cpu")
    fb.on_replace.append(lambda: told.append(2))
    before = _ptrs(fb, ("level_of", "words"))
    fb.replace(f2)
    assert _ptrs(fb, ("level_of", "words")) == before and told == [1] and fb.faults is f2 and (fb.L, fb.G, fb.K) == (2, 1, 2)
    assert np.array_equal(fb.words.numpy().view(np.uint32), f2.words) and fb.level_of.numpy().tolist() == [[1, 0]]
    fb.replace(FaultPlan([FaultLevel()], [[0, 0]]))
    assert told == [1, 2] and fb.L == 1 and tuple(fb.words.shape) == (1, 8)


class _StubTrainer:
    def __init__(self):
        self.stopped = 0

    def stop(self):
        self.stopped += 1


def test_eval_session_stops_the_trainer_when_the_body_raises(monkeypatch):
    made = []

    def factory(algo, env, num_envs, num_agents, seed, lcf, **extra):
        made.append((_StubTrainer(), (algo, env, num_envs, num_agents, seed, lcf, extra)))
        return made[-1][0]
    monkeypatch.setattr(EV, "make_eval_trainer", factory)
    with pytest.raises(KeyError, match="boom"):
        with EV.eval_session("ippo", "inter", 4, 8, 3, train_batch_size=16) as t:
            assert t is made[0][0] and t.stopped == 0
            raise KeyError("boom")
    assert made[0][0].stopped == 1 and made[0][1] == ("ippo", "inter", 4, 8, 3, None, dict(train_batch_size=16))
    with EV.eval_session("copo", "round", 2, 8, 0, lcf=(0.3, 0.1)) as t:
        pass
    assert t.stopped == 1 and made[1][1][5] == (0.3, 0.1) and len(made) == 2
