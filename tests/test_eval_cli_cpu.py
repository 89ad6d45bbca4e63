"""CPU: the study table of `copo_amd.eval.evaluate.main` (`STUDIES`, `GOES_WITH`) -- one table per run, every
study-specific option only next to one of its studies, --table and the levels file wanted, and every entry's `*_rows` the one that is
called, with the keyword arguments it always got and a frame that has the label columns the print leaves out.  Every `*_rows` and
`load_members` are replaced, so no device is touched."""
import importlib
import itertools
import os

import numpy as np
import pytest

from copo_amd.eval import checkpoint_io
from copo_amd.eval.evaluate import GOES_WITH, STUDIES, main

PATHS = ["a.npz", "b.npz"]
GIVEN = dict(jury_plan=["seated"], jury_deltas=["0.1", "0.2"], influence_max=["2"], influence_deltas=["0.1", "0.2"], precisions=["bfloat16"],
             certify_method=["linear"], similarity_rows_of=["1"], probe_rows_of=["1"], probe_ridge=["0.01"])          # every option of GOES_WITH away from its default


def flag(option):
    return "--" + option.replace("_", "-")


def module_of(study):
    return importlib.import_module("copo_amd.eval." + study.module)


def ones(*shape):
    return np.ones(shape, np.int64)


def real_frame(study, levels, kw):
    """A frame of the study's own frame function on a tally of ones (hand-made numbers where the study has no tally): two checkpoints,
    one scene of four slots per pair or cell."""
    from copo_amd.eval.crossplay import SeatPlan, tally_frame
    labels, K = kw["labels"], len(PATHS)
    if study.option == "attribution":
        from copo_amd.eval.attribution import AttributionPlan, attribution_frame
        from copo_amd.sim import SimConfig
        cfg = SimConfig(map="intersection", num_envs=2, num_agents=4)
        seats, plan = AttributionPlan.sweep(K, levels, 1, 4)
        O = cfg.ego_dim + cfg.navi_dim + cfg.num_lasers
        return attribution_frame(ones(seats.n_groups, K, 8), ones(seats.n_groups, K, 2, O), ones(seats.n_groups, K, 8), seats, plan, cfg, labels)
    if study.option == "similarity":
        from copo_amd.eval.similarity import SimilarityPlan, similarity_frame
        return similarity_frame(np.ones((K, K, 2)), 9, SimilarityPlan(SeatPlan.pairs(K, 1, 4, kw["share"]), rows_of=kw["rows_of"]), labels)
    if study.option == "probe":
        from copo_amd.eval.probes import TARGETS, probe_frame
        fit = lambda B: dict(n_train=5, n_test=4, r2_train=np.ones((B, len(TARGETS))), r2_test=np.full((B, len(TARGETS)), 0.5),  # noqa: E731
                             weight_norm=np.ones((B, len(TARGETS))))
        return probe_frame(fit(2 * K), fit(1), range(K), -1 if kw["rows_of"] is None else kw["rows_of"], labels)
    if study.option in ("cross_play", "jury", "influence"):
        seats = SeatPlan.pairs(K, 1, 4, kw["share"])
        if study.option == "cross_play":
            return tally_frame(ones(K * K, K, 8), seats, labels)
        if study.option == "influence":
            from copo_amd.eval.influence import influence_frame
            return influence_frame(ones(K * K, K, 8), seats, labels, kw["deltas"])
        from copo_amd.eval.jury import JuryPlan, jury_frame
        return jury_frame(ones(K * K, K, K, 8), seats, JuryPlan.named(seats, kw["plan"]), labels, kw["deltas"])
    if study.option == "precision_sweep":
        from copo_amd.eval.precision import PrecisionPlan, precision_frame
        seats, plan = PrecisionPlan.sweep(K, kw["precisions"], 1, 4, kw["share"])
        return precision_frame(ones(seats.n_groups, seats.K, 8), ones(seats.n_groups, seats.K, seats.K, 8), seats, plan, labels, kw["deltas"])
    if study.option == "certify_sweep":
        from copo_amd.eval.certify import CertifyPlan, certify_frame
        seats, plan = CertifyPlan.sweep(K, levels, 1, 4)
        return certify_frame(ones(seats.n_groups, seats.K, 8), ones(seats.n_groups, seats.K, 8), seats, plan, labels)
    from copo_amd.eval.levels import sweep_frame
    plan_cls = dict(fault_sweep="FaultPlan", adversary_sweep="AdversaryPlan", pgd_sweep="PGDPlan")[study.option]
    seats, plan = getattr(module_of(study), plan_cls).sweep(K, levels, 1, 4, kw["share"])
    return sweep_frame(ones(seats.n_groups, seats.K, 8), seats, plan, labels)


@pytest.fixture
def cli(tmp_path, monkeypatch):
    """`argv(*studies, table=True, levels=True, extra=())` and `called`, the (option, levels, kwargs, frame) of every `*_rows` that ran."""
    levels_file = tmp_path / "levels.json"
    levels_file.write_text("[{}]")
    table = str(tmp_path / "t.csv")
    called = []

    def fake_of(study):
        def fake_rows(algo, env, weights_list, *levels, **kw):
            assert (algo, env, list(weights_list)) == ("copo", "inter", ["w:" + p for p in PATHS]) and len(levels) == (1 if study.levels else 0)
            called.append((study.option, levels, kw, real_frame(study, levels[0] if levels else None, kw)))
            return called[-1][3]
        return fake_rows

    for study in STUDIES:
        monkeypatch.setattr(module_of(study), study.rows, fake_of(study))
    monkeypatch.setattr(checkpoint_io, "load_members", lambda paths: ["w:" + p for p in paths])

    def argv(*studies, table_given=True, levels_given=True, extra=()):
        out = []
        for s in studies:
            out += [flag(s.option)] + PATHS + ([flag(s.levels), str(levels_file)] if s.levels and levels_given else [])
        return out + (["--table", table] if table_given else []) + list(extra)

    argv.table, argv.called = table, called
    return argv


def refused(argv):
    with pytest.raises(SystemExit) as e:
        main(argv)
    return e.value.code == 2


def test_the_table_names_every_study_once():
    options = [s.option for s in STUDIES]
    assert options == ["cross_play", "fault_sweep", "adversary_sweep", "pgd_sweep", "certify_sweep", "jury", "influence", "precision_sweep",
                       "attribution", "similarity", "probe"]
    assert len(set(s.rows for s in STUDIES)) == len(STUDIES) and all(set(studies) <= set(options) for studies in GOES_WITH.values())
    assert sorted(GOES_WITH) == sorted(GIVEN)


@pytest.mark.parametrize("a, b", list(itertools.combinations(STUDIES, 2)), ids=lambda s: s.option)
def test_two_studies_are_refused(cli, capsys, a, b):
    assert refused(cli(a, b)) and refused(cli(b, a))
    err = capsys.readouterr().err
    assert flag(a.option) in err and flag(b.option) in err and "one table per run" in err
    assert not cli.called and not os.path.exists(cli.table)


@pytest.mark.parametrize("option", sorted(GOES_WITH))
def test_an_option_without_its_study_is_refused(cli, option):
    given = [flag(option)] + GIVEN[option]
    assert refused(cli(extra=given)), option
    for study in STUDIES:
        if study.option in GOES_WITH[option]:
            main(cli(study, extra=given))
            assert cli.called.pop()[0] == study.option
        else:
            assert refused(cli(study, extra=given)), (option, study.option)
    assert not cli.called


@pytest.mark.parametrize("study", STUDIES, ids=lambda s: s.option)
def test_a_study_wants_its_table_and_its_levels(cli, study):
    assert refused(cli(study, table_given=False))
    if study.levels:
        assert refused(cli(study, levels_given=False))
    assert not cli.called


OWN_DEFAULTS = dict(cross_play=dict(share=0.5), fault_sweep=dict(share=1.0), adversary_sweep=dict(share=1.0), pgd_sweep=dict(share=1.0),
                    certify_sweep=dict(method="interval"), jury=dict(plan="everyone", deltas=(0.05, 0.05), share=0.5),
                    influence=dict(max_others=4, deltas=(0.05, 0.05), share=0.5),
                    precision_sweep=dict(precisions=("float32", "bfloat16", "float8_e4m3"), deltas=(0.05, 0.05), share=1.0), attribution=dict(),
                    similarity=dict(rows_of=None, share=0.5), probe=dict(rows_of=None, ridge=1e-4, share=0.5))


@pytest.mark.parametrize("study", STUDIES, ids=lambda s: s.option)
def test_the_named_rows_run_with_the_arguments_they_always_got(cli, capsys, study):
    main(cli(study, extra=["--steps", "16", "--scenes-per-pair", "3", "--num-agents", "4"]))
    (option, levels, kw, frame), = cli.called
    assert option == study.option
    scenes = "scenes_per_pair" if study.option in ("cross_play", "jury", "influence", "similarity", "probe") else "scenes_per_cell"
    assert kw == dict(OWN_DEFAULTS[option], num_agents=4, steps=16, labels=PATHS, **{scenes: 3})
    if study.levels:
        assert levels == (module_of(study).load_levels(cli(study)[4]),)
    assert set(study.drop) and set(study.drop) <= set(frame.columns) and len(frame) > 0
    assert os.path.getsize(cli.table) > 0
    out = capsys.readouterr().out
    assert not any(col in out for col in study.drop) and frame.columns.drop(list(study.drop))[0] in out
    main(cli(study, extra=["--share", "0.25"] if study.share is not None else []))
    assert cli.called[-1][2].get("share") == (0.25 if study.share is not None else None)


def test_a_bad_value_is_a_usage_error(cli):
    jury, influence, precision = (next(s for s in STUDIES if s.option == o) for o in ("jury", "influence", "precision_sweep"))
    for study, extra in ((jury, ["--jury-deltas", "-0.1", "0.1"]), (jury, ["--jury-deltas", "nan", "0.1"]), (precision, ["--jury-deltas", "inf", "0.1"]),
                         (influence, ["--influence-deltas", "0.1", "-1"]), (influence, ["--influence-max", "0"]), (influence, ["--influence-max", "9"]),
                         (precision, ["--precisions", "bfloat16", "bfloat16"])):
        assert refused(cli(study, extra=extra)), extra
    assert not cli.called
