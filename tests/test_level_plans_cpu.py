"""The contract the four level plans share (copo_amd/eval/levels.py: `LevelPlan`, `load_levels`), asserted once over the four (plan,
level) pairs.  numpy only; what is particular to a study stays in its own test file."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from copo_amd.eval import adversary, certify, faults, pgd
from copo_amd.eval.levels import LevelPlan, sweep_members

# (module, plan, level, a non-identity level as a dict, the dtype of the words its kernel reads, has roles)
STUDIES = [(faults, faults.FaultPlan, faults.FaultLevel, dict(lidar_sigma=0.1, sticky=0.25), np.uint32, True),
           (adversary, adversary.AdversaryPlan, adversary.AdversaryLevel, dict(eps=0.1, throttle=1.0), np.float32, True),
           (pgd, pgd.PGDPlan, pgd.PGDLevel, dict(eps=0.1, alpha=0.05, iters=3, random_start=True, untargeted=True), np.int32, True),
           (certify, certify.CertifyPlan, certify.CertifyLevel, dict(eps=0.01, delta_steer=0.1), np.float32, False)]
IDS = [s[1].__name__ for s in STUDIES]
LEVEL_OF = np.array([[0, 1], [1, 0], [-1, 1]], np.int32)


@pytest.mark.parametrize("mod,Plan,Level,fields,dtype,roles", STUDIES, ids=IDS)
def test_a_dict_and_a_level_build_equal_plans(mod, Plan, Level, fields, dtype, roles):
    assert issubclass(Plan, LevelPlan) and Plan.LEVEL is Level
    a, b = Plan([{}, fields], LEVEL_OF), Plan([Level(), Level(**fields)], LEVEL_OF)
    assert a.levels == b.levels and all(isinstance(lv, Level) for lv in a.levels)
    assert np.array_equal(a.words, b.words) and np.array_equal(a.level_of, b.level_of) and a.level_of.dtype == np.int32
    assert (a.L, a.G, a.K) == (b.L, b.G, b.K) == (2, 3, 2)
    assert a.words.shape == (a.L, mod.LEVEL_WORDS) and a.words.dtype == dtype
    assert a.levels[1].as_dict() == dict(Level().as_dict(), **fields) and tuple(a.levels[1].as_dict()) == mod.LEVEL_FIELDS
    assert a.checkpoint is a.level is a.share is a.scenes_per_cell is None


@pytest.mark.parametrize("mod,Plan,Level,fields,dtype,roles", STUDIES, ids=IDS)
def test_refusals_name_the_concrete_class(mod, Plan, Level, fields, dtype, roles):
    name = Plan.__name__
    with pytest.raises(ValueError, match="^%s: no levels$" % name):
        Plan([], LEVEL_OF)
    for level_of in (np.zeros(3, np.int32), np.zeros((2, 2, 2), np.int32), np.zeros((0, 2), np.int32)):
        with pytest.raises(ValueError, match=r"^%s: level_of of shape .*\[groups\]\[members\] wanted$" % name):
            Plan([{}], level_of)
    plan = Plan([{}, fields], LEVEL_OF)
    assert plan.check(SimpleNamespace(n_groups=3, K=2)) is plan
    for n_groups, K in ((2, 2), (3, 3)):
        with pytest.raises(ValueError, match="^%s: level_of is 3 groups x 2 members, the seat plan has %d x %d$" % (name, n_groups, K)):
            plan.check(SimpleNamespace(n_groups=n_groups, K=K))
    for bad in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="^%s: %s = .* a finite number wanted$" % (Level.__name__, mod.LEVEL_FIELDS[0])):
            Level(**{mod.LEVEL_FIELDS[0]: bad})


@pytest.mark.parametrize("mod,Plan,Level,fields,dtype,roles", STUDIES, ids=IDS)
def test_sweep_layout_and_its_level_0_rule(mod, Plan, Level, fields, dtype, roles):
    seats, plan = Plan.sweep(2, [{}, fields], 3, 8)          # share 1: a bank of the two checkpoints
    assert isinstance(plan, Plan) and (plan.G, plan.K, plan.L) == (4, 2, 2) and (seats.E, seats.N, seats.n_groups, seats.K) == (12, 8, 4, 2)
    assert plan.check(seats) is plan and plan.doubled is False and plan.share == 1.0 and plan.scenes_per_cell == 3 and plan.n_impaired == 8
    assert list(plan.checkpoint) == [0, 0, 1, 1] and list(plan.level) == [0, 1, 0, 1]
    assert all(plan.level_of[g, plan.checkpoint[g]] == plan.level[g] for g in range(4))
    if not roles:          # a certificate impairs nobody: the layout is always share 1
        with pytest.raises(TypeError):
            Plan.sweep(2, [{}, fields], 3, 8, 0.5)
        return
    seats, plan = Plan.sweep(2, [{}, fields], 3, 8, 0.25)   # share < 1: the bank twice, the impaired seats are members K + k
    assert plan.doubled is True and (plan.K, seats.K) == (4, 4) and plan.n_impaired == 2 and plan.share == 0.25
    assert sweep_members([1, 2], plan) == [1, 2, 1, 2]
    with pytest.raises(ValueError, match=r"^%s\.sweep: with share < 1 the healthy seats drive at level 0, which must be the identity$" % Plan.__name__):
        Plan.sweep(2, [fields, {}], 3, 8, 0.25)
    Plan.sweep(2, [fields, {}], 3, 8, 1.0)                 # at share 1 nobody drives at level 0 for another cell


@pytest.mark.parametrize("mod,Plan,Level,fields,dtype,roles", STUDIES, ids=IDS)
def test_load_levels_round_trip(mod, Plan, Level, fields, dtype, roles, tmp_path):
    path = tmp_path / "levels.json"
    path.write_text(json.dumps([{}, fields]))
    assert mod.load_levels(str(path)) == [Level(), Level(**fields)]
    for bad in ({"levels": [fields]}, [fields, 3], "x"):
        path.write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="a JSON list of objects wanted"):
            mod.load_levels(str(path))
