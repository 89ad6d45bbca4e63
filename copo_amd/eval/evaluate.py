"""Vectorised population evaluation on the HIP simulator (the role of `copo/eval.py` + `eval/recoder.py` +
`eval/evaluate_population.py`): load a population (`.npz` in either reference layout, or this build's trainer
checkpoint), roll it in E parallel scenes without learning, report the reference's headline evaluation metrics
(success / crash / out-of-road / max-step rates, episode reward and length, velocity ...).

    python -m copo_amd.eval.evaluate --algo copo --env inter --npz path/to/copo_inter.npz --lcf 0.368 0.088

The sweep of `copo/eval.py:93-241` -- every checkpoint of every trial of an experiment folder, one table -- is `sweep_trials`: the
checkpoints of one algorithm and scene drive their scenes of ONE simulator batch as a policy bank (`evaluate_bank_rows`, eval/bank.py).

    python -m copo_amd.eval.evaluate --root path/to/experiment --num-episodes 20 --table sweep.csv
"""
import argparse
import collections
import contextlib
import json

import numpy as np

ENVS = {"inter": "MultiAgentIntersectionEnv", "round": "MultiAgentRoundaboutEnv", "parking": "MultiAgentParkingLotEnv",
        "tollgate": "MultiAgentTollgateEnv", "bottle": "MultiAgentBottleneckEnv"}


_SCENE_OF = (("Roundabout", "MultiAgentRoundaboutEnv", "Round"), ("Intersection", "MultiAgentIntersectionEnv", "Inter"),
             ("Parking", "MultiAgentParkingLotEnv", "Parking"), ("Bottle", "MultiAgentBottleneckEnv", "Bottle"),
             ("Tollgate", "MultiAgentTollgateEnv", "Tollgate"))


def scene_of(env_name, *error):
    """(wrapper class name, short scene name) of an RLlib env name; an unknown one raises ValueError(*error)."""
    for needle, cls_name, short in _SCENE_OF:
        if needle in env_name:
            return cls_name, short
    raise ValueError(*error)


def get_env(env, should_wrap_copo_env, should_wrap_cc_env, svo_mean=0.0, svo_std=0.0):
    """(RecorderEnv(single-scene env), short scene name) from an RLlib env name, as `copo/eval.py:27-64` builds it: the
    CoPO env gets the population's LCF distribution, the CC env only the neighbour lists."""
    from copo_amd.torch_copo.utils import env_wrappers as W
    from .recoder import RecorderEnv
    cls_name, short = scene_of(env)
    cls = getattr(W, cls_name)
    if should_wrap_copo_env:
        assert should_wrap_cc_env is False
        e = W.get_lcf_env(cls)({})
        e.set_lcf_dist(float(svo_mean), max(float(svo_std), 1e-6))
    elif should_wrap_cc_env:
        e = W.get_ccenv(cls)({})
    else:
        e = cls({})
    return RecorderEnv(e), short


def get_env_and_start_seed(trial_path):
    """(env name, start seed, params) of a Tune trial folder (`params.json`), copo/eval.py:67-80."""
    import os
    path = os.path.join(trial_path, "params.json")
    assert os.path.isfile(path)
    with open(path, "r") as f:
        param = json.load(f)
    if "env_config" not in param:
        raise ValueError()
    return param["env"], param["env_config"]["start_seed"], param


def make_eval_trainer(algo, env, num_envs=64, num_agents=40, seed=0, lcf=None, **extra):
    """A trainer used for its sampler only: same env wrappers, model and observation as training
    (`get_env`, copo/eval.py:27-76: CoPO populations run in the LCF env with the population's LCF distribution)."""
    from copo_amd.torch_copo import algo_ccppo, algo_copo, algo_ippo
    from copo_amd.torch_copo.utils import env_wrappers as W
    base = getattr(W, ENVS[env])
    if algo == "copo":
        cls, e = algo_copo.CoPOTrainer, W.get_rllib_compatible_env(W.get_lcf_env(base))
    elif algo == "ccppo":
        cls, e = algo_ccppo.CCPPOTrainer, algo_ccppo.get_ccppo_env(base)
    else:
        cls, e = algo_ippo.IPPOTrainer, W.get_rllib_compatible_env(base)
    extra = dict(extra)
    cfg = dict(env=e, env_config=dict(extra.pop("env_config", None) or {}, num_agents=num_agents), num_envs=num_envs,
               train_batch_size=num_envs * 25, seed=seed)
    cfg.update(extra)
    t = cls(config=cfg)
    if algo == "copo" and lcf is not None:
        t.env.set_lcf_dist(float(lcf[0]), float(lcf[1]))
    return t


@contextlib.contextmanager
def eval_session(algo, env, num_envs, num_agents, seed, lcf=None, weights=None, **extra):
    """One evaluation session: `make_eval_trainer`, with the population `weights` loaded where given (and the fused learner's mirror in
    step with them), yielded, and stopped whatever the body did."""
    t = make_eval_trainer(algo, env, num_envs, num_agents, seed, lcf, **extra)
    try:
        if weights is not None:
            from .checkpoint_io import load_policy_weights
            load_policy_weights(t.policy.model, weights)
            if t.policy.fused is not None:
                t.policy.fused.sync_mirror()
        yield t
    finally:
        t.stop()


def graph_flag(t):
    """Whether a sampler built next to trainer `t`'s own captures its fragment."""
    return t.config.get("use_hip_graphs", True)


def record_scene_episodes(smp, scene_episodes, horizon):
    """Fragments of `smp` folded by a `DeviceRecorder` until every scene has finished `scene_episodes` whole episodes (or six times their
    length has passed); one host read per fragment, the episode counter.  Returns the recorder: the caller reads it and closes it."""
    from .device_recorder import DeviceRecorder
    n = int(scene_episodes)
    rec = DeviceRecorder(smp.E, smp.N, smp.device, max_rows=smp.E * n, limit=n)
    n_frag = 0
    while n_frag * smp.T <= 6 * (n + 1) * horizon:
        rec.add(smp.sample())
        n_frag += 1
        if int(rec.episodes().min()) >= n:
            break
    return rec


def run_steps(smp, steps):
    """`steps` env steps of `smp`, rounded up to whole fragments.  Returns `smp`."""
    for _ in range(-(-int(steps) // smp.T)):
        smp.sample()
    return smp


def check_labels(labels, K):
    """One label per member; default: the member index."""
    labels = list(range(K)) if labels is None else list(labels)
    if len(labels) != K:
        raise ValueError("%d labels for %d members" % (len(labels), K))
    return labels


def evaluate_population(algo, env, weights=None, lcf=None, num_envs=64, num_agents=40, episodes=2000, seed=0,
                        scene_episodes=None, **extra):
    """Roll a population in `num_envs` scenes.  `scene_episodes` = whole scene episodes (until done["__all__"]: `horizon`
    env steps of respawning, then the scene drains -- the unit of the reference's evaluation,
    eval/evaluate_population.py:57-76) -- every agent that terminates inside them counts; otherwise stop after `episodes`
    terminated agents (quick, but the first agents to terminate are the ones that fail early)."""
    with eval_session(algo, env, num_envs, num_agents, seed, lcf, weights, **extra) as t:
        if scene_episodes:
            return t.evaluate(scene_episodes=int(scene_episodes))
        return t.evaluate(num_fragments=1, min_episodes=episodes)


def evaluate_population_rows(algo, env, weights=None, lcf=None, num_envs=64, num_agents=40, scene_episodes=1, seed=0,
                             recorder_distance=20.0, recorder="torch", **extra):
    """The reference's per-episode evaluation table (`evaluate_once`, eval/evaluate_population.py:21-99: one row of
    `RecorderEnv.get_episode_result` per whole scene episode) for `num_envs` scenes at once: a pandas DataFrame with the
    reference's column names (`vec_recorder.COLUMNS`).  The recorder counts neighbours within its own radius (20 m,
    recoder.py:76), so the scenes are built with that `neighbours_distance` -- the policies do not read it.
    `recorder`: "torch" = `VecRecorder`; "device" = `DeviceRecorder`, which adds the SVO columns (`device_recorder.COLUMNS`), folds a
    fragment in three launches and leaves the loop one host read per fragment, the episode counter."""
    import torch
    from .vec_recorder import F_ENV_RESET, VecRecorder
    if recorder not in ("torch", "device"):
        raise ValueError("recorder=%r: 'torch' or 'device'" % (recorder,))
    extra = dict(extra)
    env_config = dict(extra.pop("env_config", None) or {}, neighbours_distance=float(recorder_distance))
    with eval_session(algo, env, num_envs, num_agents, seed, lcf, weights, env_config=env_config, **extra) as t:
        smp = t.sampler
        horizon = int(t.env.sim.cfg.horizon)
        if recorder == "device":
            rec = record_scene_episodes(smp, scene_episodes, horizon)
            df = rec.frame()
            rec.close()
            return df
        rec = VecRecorder(smp.E, smp.device)
        ep = torch.zeros(smp.E, dtype=torch.int64, device=smp.device)
        n_frag = 0
        while bool((ep < int(scene_episodes)).any()) and n_frag * smp.T <= 6 * (int(scene_episodes) + 1) * horizon:
            b = smp.sample()
            fl = b["flags"]
            ended = ((fl & F_ENV_RESET) > 0).any(-1).to(torch.int64)            # [T, E]
            before = ep[None] + torch.cumsum(ended, 0) - ended                   # whole episodes finished before step t
            rec.add(dict(flags=fl, infos=b["infos"], nbr_cnt=b["nbr_cnt"]), keep=before < int(scene_episodes))
            ep = ep + ended.sum(0)
            n_frag += 1
        return rec.frame()


def evaluate_bank_rows(algo, env, weights_list, lcfs=None, num_envs=64, num_agents=40, scene_episodes=1, seed=0, labels=None,
                       recorder_distance=20.0, **extra):
    """`evaluate_population_rows(recorder="device")` for K populations of one algorithm and scene in one batch: member k drives scenes
    [k E / K, (k + 1) E / K) of `num_envs` = E scenes (`num_envs % K` must be 0) through one eval trainer, one `PolicyBank`, one
    captured rollout and one `DeviceRecorder`; with `algo == "copo"` member k's scenes draw their LCF from `lcfs[k]` = (mean, std)
    (`VecSim.set_lcf_table`).  Every member gets the scene seeds start_seed + arange(E / K) and the same action noise, so the
    evaluation is paired.  Returns the recorder's frame sorted by (scene, episode of the scene), plus `member` = scene // (E / K) and
    `label` = labels[member] (default: the member index)."""
    from .bank import BankSampler, PolicyBank, members_of_scenes
    from .device_recorder import COLUMNS
    import pandas as pd
    weights_list = list(weights_list)
    K = len(weights_list)
    per = members_of_scenes(int(num_envs), K)
    labels = check_labels(labels, K)
    table = None
    if algo == "copo":
        if lcfs is None or len(lcfs) != K:
            raise ValueError("a CoPO bank needs one (mean, std) per member in `lcfs`")
        from copo_amd.sim import lcf_table_array
        table = np.asarray([(float(m), max(float(s), 1e-6)) for m, s in lcfs], np.float32)       # (the floor of `get_env`)
        table = lcf_table_array(np.repeat(table, per, axis=0), num_envs)
    extra = dict(extra)
    env_config = dict(extra.pop("env_config", None) or {}, neighbours_distance=float(recorder_distance))
    with eval_session(algo, env, num_envs, num_agents, seed, env_config=env_config, **extra) as t:
        if table is not None:
            t.env.sim.set_lcf_table(table)
        smp = BankSampler(t.env, t.policy, PolicyBank(t.policy, weights_list), t.sampler.T, use_graph=graph_flag(t))
        rec = record_scene_episodes(smp, scene_episodes, int(t.env.sim.cfg.horizon))
        r = rec.rows().cpu().numpy()
        rec.close()
    r = r[np.lexsort((r[:, len(COLUMNS) + 1], r[:, len(COLUMNS)]))]
    df = pd.DataFrame(r[:, :len(COLUMNS)], columns=list(COLUMNS))
    df["scene"] = r[:, len(COLUMNS)].astype(np.int64)
    df["member"] = df["scene"] // per
    df["label"] = [labels[k] for k in df["member"]]
    return df


def list_checkpoints(root):
    """One dict per checkpoint of every trial folder under `root`, trial by trial and by checkpoint count within a trial
    (copo/eval.py:96-139): path, count, algo (the folder's name), env (the trial's RLlib env name), seed, trial, trial_path and the
    wrapper choice, "CoPO" / "CCPPO" in the trial's name."""
    import os
    root = os.path.abspath(root)
    infos = []
    for trial in sorted(p for p in os.listdir(root) if os.path.isdir(os.path.join(root, p))):
        trial_path = os.path.join(root, trial)
        raw_env, start_seed, _ = get_env_and_start_seed(trial_path)
        ckpts = sorted(((c, int(c.split("_")[1])) for c in os.listdir(trial_path) if "checkpoint" in c), key=lambda p: p[1])
        for ckpt, count in ckpts:
            infos.append(dict(path=os.path.join(trial_path, ckpt, ckpt.replace("_", "-")), count=count, algo=os.path.basename(root),
                              env=raw_env, seed=start_seed, trial=trial, trial_path=trial_path,
                              should_wrap_copo_env="CoPO" in trial, should_wrap_cc_env="CCPPO" in trial))
    return infos


def sweep_trials(root, num_episodes=20, max_members=16, num_agents=40, seed=0, evaluator=None, **extra):
    """The reference's checkpoint sweep (copo/eval.py:93-241) as banks: the checkpoints of `list_checkpoints(root)` are grouped by
    (algorithm, scene) in their listed order, and each group is evaluated `max_members` checkpoints at a time by
    `evaluator` (default `evaluate_bank_rows`) with `num_episodes` scenes of one whole scene episode per checkpoint -- the scene seeds
    start_seed + 0 .. num_episodes - 1, as the reference's env walks them episode after episode.  CoPO trials take their LCF
    distribution from the trial's progress.csv.  Returns one frame: the evaluator's rows with the reference's extra columns `count`,
    `algo`, `env` (the short scene name), `seed`, `trial`; `label` is the checkpoint's path."""
    import pandas as pd
    from .checkpoint_io import checkpoint_policy_weights, get_lcf_from_checkpoint
    evaluator = evaluate_bank_rows if evaluator is None else evaluator
    if int(max_members) < 1 or int(num_episodes) < 1:
        raise ValueError("max_members and num_episodes must be at least 1")
    by_cls = {cls: key for key, cls in ENVS.items()}
    groups = {}
    for info in list_checkpoints(root):
        cls_name, short = scene_of(info["env"], "trial %s: unknown scene %r" % (info["trial"], info["env"]))
        algo = "copo" if info["should_wrap_copo_env"] else ("ccppo" if info["should_wrap_cc_env"] else "ippo")
        groups.setdefault((algo, by_cls[cls_name], short), []).append(info)
    frames = []
    for (algo, env, short), infos in groups.items():
        for lo in range(0, len(infos), int(max_members)):
            chunk = infos[lo:lo + int(max_members)]
            weights = [checkpoint_policy_weights(i["path"]) for i in chunk]
            lcfs = [tuple(float(v) for v in get_lcf_from_checkpoint(i["trial_path"])) for i in chunk] if algo == "copo" else None
            df = evaluator(algo, env, weights, lcfs=lcfs, num_envs=len(chunk) * int(num_episodes), num_agents=num_agents,
                           scene_episodes=1, seed=seed, labels=[i["path"] for i in chunk], **extra)
            member = df["member"].to_numpy()
            for col in ("count", "algo", "seed", "trial"):
                df[col] = [chunk[k][col] for k in member]
            df["env"] = short
            frames.append(df)
    return pd.concat(frames, ignore_index=True) if frames else pd.DataFrame()


def _flag(option):
    return "--" + option.replace("_", "-")


def _deltas(a, option):
    from .jury import check_deltas
    given = getattr(a, option)
    return check_deltas(_flag(option), (0.05, 0.05) if given is None else given)


def _influence_args(a):
    from .influence import check_max_others
    return dict(max_others=check_max_others("--influence-max", 4 if a.influence_max is None else a.influence_max), deltas=_deltas(a, "influence_deltas"))


def _precision_args(a):
    low = ("bfloat16", "float8_e4m3") if a.precisions is None else tuple(a.precisions)
    if len(set(low)) != len(low):
        raise ValueError("--precisions: a precision twice")
    return dict(precisions=("float32",) + low, deltas=_deltas(a, "jury_deltas"))


# The studies of `main` that seat checkpoints and write one table, one entry each: the option that names the checkpoints; the module of
# eval/ and the name of its `*_rows`, looked up when the study runs (a test may have replaced it); the option of its levels file (read by
# the module's `load_levels`) or None; the default --share, None where the study takes none; the name of its scenes keyword; its own
# keyword arguments from its own options (a ValueError is a usage error); the label columns left out of the print; the name of a
# function of the module whose table of (frame, members) is printed too.
# `members`: keyword arguments of `load_members` for the study's checkpoints (the critic audit keeps their value nets).
Study = collections.namedtuple("Study", "option module rows levels share scenes extra drop epilogue members",
                               defaults=(None, None, "scenes_per_cell", lambda a: {}, ("label",), None, {}))
STUDIES = (
    Study("cross_play", "crossplay", "cross_play_rows", share=0.5, scenes="scenes_per_pair"),
    Study("fault_sweep", "faults", "fault_sweep_rows", "fault_levels", 1.0),
    Study("adversary_sweep", "adversary", "adversary_sweep_rows", "adversary_levels", 1.0),
    Study("pgd_sweep", "pgd", "pgd_sweep_rows", "pgd_levels", 1.0),
    Study("certify_sweep", "certify", "certify_sweep_rows", "certify_levels", extra=lambda a: dict(method=a.certify_method)),
    Study("jury", "jury", "jury_rows", share=0.5, scenes="scenes_per_pair", extra=lambda a: dict(plan=a.jury_plan, deltas=_deltas(a, "jury_deltas")),
          drop=("driver_label", "judge_label"), epilogue="jury_matrix"),
    Study("influence", "influence", "influence_rows", share=0.5, scenes="scenes_per_pair", extra=_influence_args),
    Study("precision_sweep", "precision", "precision_sweep_rows", share=1.0, extra=_precision_args),
    Study("attribution", "attribution", "attribution_rows", "attribution_levels"),
    Study("similarity", "similarity", "similarity_rows", share=0.5, scenes="scenes_per_pair", extra=lambda a: dict(rows_of=a.similarity_rows_of),
          drop=("label_a", "label_b"), epilogue="similarity_matrices"),
    Study("probe", "probes", "probe_rows", share=0.5, scenes="scenes_per_pair",
          extra=lambda a: dict(rows_of=a.probe_rows_of, ridge=1e-4 if a.probe_ridge is None else a.probe_ridge), epilogue="probe_matrix"),
)
# the options that belong to some studies only: given (not at its default) without one of them, an option is a usage error
GOES_WITH = dict(jury_plan=("jury",), jury_deltas=("jury", "precision_sweep"), influence_max=("influence",), influence_deltas=("influence",),
                 precisions=("precision_sweep",), certify_method=("certify_sweep",), similarity_rows_of=("similarity",), probe_rows_of=("probe",),
                 probe_ridge=("probe",))


def _critic_args(a):
    from .critics import DEFAULT_RANGE, CriticAudit
    kw = dict(bins=8 if a.critic_bins is None else a.critic_bins, value_range=DEFAULT_RANGE if a.critic_range is None else tuple(a.critic_range),
              pairs=bool(a.cross_play_pairs))
    CriticAudit([1.0], kw["value_range"], kw["bins"])          # (a ValueError is a usage error)
    if a.share is not None:          # (the study's entry names no share of its own: only the pairs layout has one)
        if not kw["pairs"]:
            raise ValueError("--share goes with --cross-play-pairs here: a checkpoint's own scenes have no share")
        kw["share"] = a.share
    return kw


# The studies that read the VALUE nets, entries of the same kind run by the same `run_study`; a table of their own, next to their options,
# so that STUDIES and GOES_WITH stay the list of the policy-net studies.
CRITIC_STUDIES = (
    Study("critic_audit", "critics", "critic_audit_rows", scenes="scenes_per_pair", extra=_critic_args, drop=("label", "head_name"),
          epilogue="calibration_of", members=dict(values=True)),
)
CRITIC_GOES_WITH = dict(critic_bins=("critic_audit",), critic_range=("critic_audit",), cross_play_pairs=("critic_audit",))


def run_study(ap, a, study):
    """One entry of `STUDIES` from the parsed options `a`: its table written to --table and printed."""
    import importlib
    from .checkpoint_io import load_members
    needs = [o for o in (study.levels, "table") if o]
    if not all(getattr(a, o) for o in needs):
        ap.error("%s needs %s" % (_flag(study.option), " and ".join(_flag(o) for o in needs)))
    module = importlib.import_module("." + study.module, __package__)
    try:
        kw = study.extra(a)
    except ValueError as e:
        ap.error(str(e))
    if study.share is not None:
        kw["share"] = study.share if a.share is None else a.share
    paths = getattr(a, study.option)
    levels = [module.load_levels(getattr(a, study.levels))] if study.levels else []
    df = getattr(module, study.rows)("ippo" if a.algo == "cl" else a.algo, a.env, load_members(paths, **study.members), *levels, num_agents=a.num_agents,
                                     steps=a.steps, labels=list(paths), **{study.scenes: a.scenes_per_pair}, **kw)
    df.to_csv(a.table)
    print(df.drop(columns=list(study.drop)).to_string())
    if study.epilogue:
        print(getattr(module, study.epilogue)(df, len(paths)).to_string())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="experiment folder of Tune trial folders: evaluate every checkpoint of every trial "
                                                 "(the reference's copo/eval.py) into --table")
    ap.add_argument("--num-episodes", type=int, default=20, help="with --root: whole scene episodes per checkpoint")
    ap.add_argument("--max-members", type=int, default=16, help="with --root: checkpoints per simulator batch")
    ap.add_argument("--algo", default="copo", choices=["ippo", "ccppo", "copo", "cl"])
    ap.add_argument("--env", default="inter", choices=sorted(ENVS))
    ap.add_argument("--npz", default=None, help="population file in the reference's key layout")
    ap.add_argument("--lcf", type=float, nargs=2, default=None, metavar=("MEAN", "STD"))
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--num-agents", type=int, default=40)
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--table", default=None, metavar="CSV",
                    help="write the reference's per-episode evaluation table (RecorderEnv columns, one row per whole scene episode) "
                         "instead of the headline rates")
    ap.add_argument("--scene-episodes", type=int, default=1)
    ap.add_argument("--recorder", default="torch", choices=["torch", "device"],
                    help="what folds the table: the torch recorder, or the device recorder (adds the SVO estimate columns)")
    ap.add_argument("--cross-play", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints (.npz populations or Tune checkpoint files) of --algo's layout: every ordered pair shares scenes "
                         "(eval/crossplay.py), one row per (pair, member) into --table")
    ap.add_argument("--share", type=float, default=None,
                    help="with --cross-play: the focal member's share of a scene's slots (default 0.5); with --fault-sweep / --adversary-sweep / --pgd-sweep: the "
                         "impaired share (default 1: every slot)")
    ap.add_argument("--scenes-per-pair", type=int, default=4, help="scenes per pair (--cross-play) or per cell (--fault-sweep, --adversary-sweep, --pgd-sweep)")
    ap.add_argument("--steps", type=int, default=1000, help="with --cross-play / --fault-sweep / --adversary-sweep / --pgd-sweep: env steps")
    ap.add_argument("--fault-sweep", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each driven at every level of --fault-levels (eval/faults.py): one row per "
                         "(checkpoint, level, role) into --table")
    ap.add_argument("--fault-levels", default=None, metavar="JSON",
                    help="with --fault-sweep: a JSON list of {lidar_sigma, lidar_dropout, dropout_value, act_sigma, sticky}; the first "
                         "must be the identity {}")
    ap.add_argument("--adversary-sweep", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each attacked at every level of --adversary-levels (eval/adversary.py: one "
                         "gradient-sign step on the LiDAR block): one row per (checkpoint, level, role) into --table")
    ap.add_argument("--adversary-levels", default=None, metavar="JSON",
                    help="with --adversary-sweep: a JSON list of {eps, steer, throttle}; the first must be an identity, e.g. {}")
    ap.add_argument("--pgd-sweep", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each attacked at every level of --pgd-levels (eval/pgd.py: iterated "
                         "gradient-sign steps on the LiDAR block, projected onto the budget): one row per (checkpoint, level, role) into --table")
    ap.add_argument("--pgd-levels", default=None, metavar="JSON",
                    help="with --pgd-sweep: a JSON list of {eps, steer, throttle, alpha, iters, random_start, untargeted}; the first must "
                         "be an identity, e.g. {}")
    ap.add_argument("--certify-sweep", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each certified at every level of --certify-levels (eval/certify.py: interval "
                         "bounds of the action means over the LiDAR budget; nobody's driving changes): one row per (checkpoint, level) "
                         "into --table; takes --scenes-per-pair and --steps")
    ap.add_argument("--certify-levels", default=None, metavar="JSON", help="with --certify-sweep: a JSON list of {eps, delta_steer, delta_throttle}")
    ap.add_argument("--certify-method", default="interval", choices=("interval", "linear"),
                    help="with --certify-sweep: interval propagation (default) or the tighter linear bounds intersected with it; "
                         "\"linear\" adds a `method` column to the table")
    ap.add_argument("--jury", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout on the scenes of --cross-play, each row judged by the others (eval/jury.py: how far "
                         "apart the drivers' and the judges' action distributions are): one row per (pair, driver, judge) into --table; "
                         "takes --share, --scenes-per-pair and --steps")
    ap.add_argument("--jury-plan", default="everyone", choices=("everyone", "seated"),
                    help="with --jury: every checkpoint judges every row (default), or focal and partner judge the rows of their pair")
    ap.add_argument("--jury-deltas", type=float, nargs=2, default=None, metavar=("STEER", "THROTTLE"),
                    help="with --jury: the distances of the two action means above which a pair counts as a disagreement (default 0.05 0.05)")
    ap.add_argument("--influence", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout on the scenes of --cross-play, every driver's row re-read with one LiDAR neighbour "
                         "taken out at a time (eval/influence.py: which neighbour a driver reacts to, and how strongly): one row per (pair, "
                         "member) into --table; takes --share, --scenes-per-pair and --steps")
    ap.add_argument("--influence-max", type=int, default=None, metavar="M", help="with --influence: neighbours removed per driver, 1..8 (default 4)")
    ap.add_argument("--influence-deltas", type=float, nargs=2, default=None, metavar=("STEER", "THROTTLE"),
                    help="with --influence: the shifts of the two action means above which a neighbour counts as one that moved the driver "
                         "(default 0.05 0.05)")
    ap.add_argument("--precision-sweep", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each driven in float32 and in every precision of --precisions (eval/precision.py: "
                         "the policy net on the bfloat16 / float8 matrix instructions, its float32 twin judging the states it drives): one row "
                         "per (checkpoint, precision) into --table; takes --share (default 1), --jury-deltas, --scenes-per-pair and --steps")
    ap.add_argument("--precisions", nargs="+", default=None, choices=("bfloat16", "float8_e4m3"),
                    help="with --precision-sweep: the low precisions of the sweep (default: both)")
    ap.add_argument("--attribution", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout, each attributed at every level of --attribution-levels (eval/attribution.py: "
                         "integrated gradients of the two action means over the observation columns; nobody's driving changes): one row "
                         "per (checkpoint, level) into --table; takes --scenes-per-pair and --steps")
    ap.add_argument("--attribution-levels", default=None, metavar="JSON",
                    help="with --attribution: a JSON list of {points, baseline}; baseline is \"clear_road\", \"zeros\" or a row of numbers "
                         "in which null masks a column")
    ap.add_argument("--similarity", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout on the scenes of --cross-play, compared by linear CKA of both hidden layers on the "
                         "states the scenes visit (eval/similarity.py: what the checkpoints compute inside, not what they do): one row per "
                         "(checkpoint a, checkpoint b, layer) into --table; takes --share, --scenes-per-pair and --steps")
    ap.add_argument("--similarity-rows-of", type=int, default=None, metavar="INDEX",
                    help="with --similarity: count only the rows that checkpoint INDEX drives (default: every acted row)")
    ap.add_argument("--probe", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout on the scenes of --cross-play, both hidden layers probed by ridge regressions for eight "
                         "scene quantities (eval/probes.py: what a layer encodes; the scenes of a pair alternate between the train and the test "
                         "fold, so --scenes-per-pair is at least 2): one row per (checkpoint, layer, quantity) and the observation's own as a "
                         "control into --table; takes --share, --scenes-per-pair and --steps")
    ap.add_argument("--probe-rows-of", type=int, default=None, metavar="INDEX",
                    help="with --probe: count only the rows that checkpoint INDEX drives (default: every acted row)")
    ap.add_argument("--probe-ridge", type=float, default=None, metavar="LAMBDA",
                    help="with --probe: the ridge as a share of the mean feature variance (default 1e-4)")
    ap.add_argument("--critic-audit", nargs="+", default=None, metavar="CKPT",
                    help="checkpoints of --algo's layout WITH their value nets (Tune-style checkpoint files of this build, or .npz files of full "
                         "state-dict keys), every value head compared with the discounted return its agents went on to realise "
                         "(eval/critics.py): one row per (scene group, checkpoint, head) into --table, the reliability diagram printed; takes "
                         "--scenes-per-pair and --steps, and --share with --cross-play-pairs")
    ap.add_argument("--critic-bins", type=int, default=None, metavar="B", help="with --critic-audit: value bins of the reliability diagram, 1..16 (default 8)")
    ap.add_argument("--critic-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --critic-audit: the value range the bins divide (default -20 20)")
    ap.add_argument("--cross-play-pairs", action="store_true",
                    help="with --critic-audit: the scenes of --cross-play (every ordered pair of checkpoints shares scenes) instead of scenes of "
                         "its own per checkpoint: how a critic holds up beside every partner")
    a = ap.parse_args(argv)
    from .checkpoint_io import load_members
    named = [s for s in STUDIES + CRITIC_STUDIES if getattr(a, s.option)]
    if len(named) > 1:
        ap.error("%s: one table per run" % " and ".join(_flag(s.option) for s in named))
    for option, studies in dict(GOES_WITH, **CRITIC_GOES_WITH).items():
        if getattr(a, option) != ap.get_default(option) and not any(s.option in studies for s in named):
            ap.error("%s goes with %s" % (_flag(option), " or ".join(_flag(s) for s in studies)))
    if named:
        return run_study(ap, a, named[0])
    if a.root:
        if not a.table:
            ap.error("--root needs --table")
        df = sweep_trials(a.root, a.num_episodes, a.max_members, num_agents=a.num_agents)
        df.to_csv(a.table)
        print(df.groupby(["trial", "count"])[["success_rate", "crash_rate", "out_rate", "episode_reward_mean"]].mean().to_string())
        return
    w = load_members([a.npz])[0] if a.npz else None
    algo = "ippo" if a.algo == "cl" else a.algo
    if a.table:
        df = evaluate_population_rows(algo, a.env, w, a.lcf, a.num_envs, a.num_agents, scene_episodes=a.scene_episodes, recorder=a.recorder)
        df.to_csv(a.table)
        print(df.mean(numeric_only=True).to_string())
        return
    print(json.dumps(evaluate_population(algo, a.env, w, a.lcf, a.num_envs, a.num_agents, a.episodes), indent=1))


if __name__ == "__main__":
    main()
