"""Host side of the checkpoint sweep without a GPU: `sweep_trials` on a folder tree in the reference's layout (copo/eval.py:93-241)
with the evaluator stubbed out, and the argument checks of the bank, the per-scene LCF table and the binding."""
import json
import os
import types

import numpy as np
import pytest
import torch

import bank_cases as bc
from copo_amd.eval import checkpoint_io as CK
from copo_amd.eval import evaluate as EV


def _cpu_model(kind, odim):
    from copo_amd.engine import Box
    from copo_amd.torch_copo import algo_copo, algo_ippo
    from copo_amd.torch_copo.utils import env_wrappers as W
    base = W.MultiAgentIntersectionEnv
    pcls, ccls, env = dict(ippo=(algo_ippo.IPPOPolicy, algo_ippo.IPPOConfig, W.get_rllib_compatible_env(base)),
                           copo=(algo_copo.CoPOPolicy, algo_copo.CoPOConfig, W.get_rllib_compatible_env(W.get_lcf_env(base))))[kind]
    cfg = ccls()
    cfg.update_from_dict(dict(env=env, device="cpu", use_hip_graphs=False, use_fused_learner=False))
    cfg.validate()
    return pcls(Box(-1, 1, (odim,)), Box(-1, 1, (2,)), cfg).model


def _trial(root, name, env, seed, kind, odim, counts, golden_dir, lcf=None):
    """A Tune trial folder: params.json, progress.csv (CoPO: the LCF columns) and checkpoint_<count>/checkpoint-<count> files whose
    first-layer bias holds the checkpoint count, so that a stub can tell which file it was handed."""
    path = os.path.join(root, name)
    os.makedirs(path)
    with open(os.path.join(path, "params.json"), "w") as f:
        json.dump(dict(env=env, env_config=dict(start_seed=seed)), f)
    with open(os.path.join(path, "progress.csv"), "w") as f:
        if lcf is None:
            f.write("training_iteration\n1\n2\n")
        else:
            f.write("training_iteration,info/learner/svo,info/learner/svo_std\n1,0.0,0.1\n2,%r,%r\n" % lcf)
    model = _cpu_model(kind, odim)
    CK.load_policy_weights(model, bc.golden_population(golden_dir, kind + "_inter"))
    for c in counts:
        with torch.no_grad():
            model.state_dict()["_hidden_layers.0._model.0.bias"].fill_(float(c))
        d = os.path.join(path, "checkpoint_%d" % c)
        os.makedirs(d)
        CK.save_tune_style_checkpoint(model, os.path.join(d, "checkpoint-%d" % c))
    return path


@pytest.fixture()
def tree(tmp_path, golden_dir):
    root = os.path.join(str(tmp_path), "myexp")
    os.makedirs(root)
    _trial(root, "CoPOTrainer_MultiAgentIntersectionEnv_aaaa_00000", "MultiAgentIntersectionEnv", 5000, "copo", 92, (120, 40, 1000),
           golden_dir, lcf=(0.25, 0.0625))
    _trial(root, "IPPOTrainer_MultiAgentIntersectionEnv_bbbb_00000", "MultiAgentIntersectionEnv", 6000, "ippo", 91, (7,), golden_dir)
    with open(os.path.join(root, "experiment_state.json"), "w") as f:          # files next to the trial folders are not trials
        f.write("{}")
    return root


class _Stub:
    """Stands where `evaluate_bank_rows` stands: two rows per scene-less member, remembers what it was asked."""

    def __init__(self):
        self.calls = []

    def __call__(self, algo, env, weights_list, lcfs=None, num_envs=None, num_agents=None, scene_episodes=None, seed=None,
                 labels=None, **extra):
        import pandas as pd
        K = len(weights_list)
        assert num_envs % K == 0
        per = num_envs // K
        self.calls.append(dict(algo=algo, env=env, K=K, lcfs=lcfs, num_envs=num_envs, scene_episodes=scene_episodes, labels=labels,
                               counts=[float(w["_hidden_layers.0._model.0.bias"][0]) for w in weights_list],
                               widths=[w["_hidden_layers.0._model.0.weight"].shape[1] for w in weights_list]))
        scene = np.arange(num_envs)
        return pd.DataFrame(dict(success_rate=scene * 0.5, scene=scene, member=scene // per, label=[labels[s // per] for s in scene]))


def test_sweep_groups_orders_and_chunks(tree):
    stub = _Stub()
    df = EV.sweep_trials(tree, num_episodes=2, max_members=2, evaluator=stub)
    # CoPO's three checkpoints in banks of at most two, by checkpoint count (40, 120 | 1000), then IPPO's one: never mixed in a bank
    assert [(c["algo"], c["env"], c["counts"]) for c in stub.calls] == [
        ("copo", "inter", [40.0, 120.0]), ("copo", "inter", [1000.0]), ("ippo", "inter", [7.0])]
    assert [c["widths"] for c in stub.calls] == [[92, 92], [92], [91]]
    assert [c["num_envs"] for c in stub.calls] == [4, 2, 2] and all(c["scene_episodes"] == 1 for c in stub.calls)
    # the LCF of a CoPO member is the last row of its trial's progress.csv; the others have none
    assert stub.calls[0]["lcfs"] == [(0.25, 0.0625)] * 2 and stub.calls[1]["lcfs"] == [(0.25, 0.0625)] and stub.calls[2]["lcfs"] is None
    assert all(lbl.endswith(os.path.join("checkpoint_%d" % c, "checkpoint-%d" % c))
               for call in stub.calls for lbl, c in zip(call["labels"], call["counts"]))
    # one frame, the reference's extra columns, two rows (episodes) per checkpoint
    assert len(df) == 8 and list(df["count"]) == [40, 40, 120, 120, 1000, 1000, 7, 7]
    assert set(df["algo"]) == {"myexp"} and set(df["env"]) == {"Inter"}
    assert list(df["seed"]) == [5000] * 6 + [6000] * 2
    assert list(df["trial"]) == ["CoPOTrainer_MultiAgentIntersectionEnv_aaaa_00000"] * 6 + ["IPPOTrainer_MultiAgentIntersectionEnv_bbbb_00000"] * 2
    assert list(df["label"]) == [lbl for call in stub.calls for lbl in call["labels"] for _ in range(2)]
    one = _Stub()
    EV.sweep_trials(tree, num_episodes=1, max_members=16, evaluator=one)
    assert [c["counts"] for c in one.calls] == [[40.0, 120.0, 1000.0], [7.0]]
    with pytest.raises(ValueError):
        EV.sweep_trials(tree, num_episodes=1, max_members=0, evaluator=one)


def test_list_checkpoints_follows_the_reference_layout(tree):
    infos = EV.list_checkpoints(tree)
    assert [i["count"] for i in infos] == [40, 120, 1000, 7]
    assert [i["should_wrap_copo_env"] for i in infos] == [True] * 3 + [False] and not any(i["should_wrap_cc_env"] for i in infos)
    assert all(os.path.isfile(i["path"]) and i["algo"] == "myexp" for i in infos)
    w = CK.checkpoint_policy_weights(infos[0]["path"])
    assert not any("value" in k for k in w) and float(w["_hidden_layers.0._model.0.bias"][0]) == 40.0


def test_bank_refuses_members_of_another_shape(golden_dir):
    """The shapes are checked against the model before anything is loaded or any native call is made."""
    from copo_amd.eval.bank import PolicyBank
    model = _cpu_model("copo", 92)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    pol = types.SimpleNamespace(model=model, fused=types.SimpleNamespace(can_forward=True))
    w = bc.golden_population(golden_dir, "copo_inter")
    with pytest.raises(ValueError, match="member 1"):
        PolicyBank(pol, [w, bc.golden_population(golden_dir, "ippo_inter")])
    with pytest.raises(ValueError, match="member 0"):
        PolicyBank(pol, [bc.random_population(92, 64, 0)])
    with pytest.raises(ValueError, match="fused learner"):
        PolicyBank(types.SimpleNamespace(model=model, fused=None), [w])
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())


def test_members_must_divide_the_scenes():
    from copo_amd.eval.bank import members_of_scenes
    assert members_of_scenes(12, 3) == 4
    with pytest.raises(ValueError, match="multiple"):
        members_of_scenes(12, 5)
    with pytest.raises(ValueError, match="multiple"):
        EV.evaluate_bank_rows("ippo", "inter", [{}, {}, {}], num_envs=8)            # refused before a trainer is built
    with pytest.raises(ValueError, match="lcfs"):
        EV.evaluate_bank_rows("copo", "inter", [{}, {}], lcfs=[(0.0, 0.1)], num_envs=8)


def test_lcf_table_is_checked_on_the_host():
    from copo_amd.sim import lcf_table_array
    t = lcf_table_array(bc.lcf_table(), bc.LCF_E)
    assert t.dtype == np.float32 and t.shape == (6, 2) and t.flags["C_CONTIGUOUS"]
    for row, col, v in ((2, 1, 0.0), (2, 1, -0.1), (5, 0, 1.5), (0, 0, float("nan")), (1, 1, float("nan"))):
        bad = bc.lcf_table()
        bad[row, col] = v
        with pytest.raises(ValueError, match="scene %d" % row):
            lcf_table_array(bad, bc.LCF_E)
    with pytest.raises(ValueError, match="shape"):
        lcf_table_array(bc.lcf_table(), 5)


def test_new_entries_are_bound_and_a_missing_symbol_fails_the_load(monkeypatch):
    """The binding lists both new entries, so importing it has resolved them; a symbol the library does not export stops the load with
    the AttributeError every handle of this package relies on."""
    from copo_amd import _capi
    assert {"copo_mlp_forward_bank_f32", "copo_sim_set_lcf_table"} <= set(_capi.EXPORTED_SYMBOLS)
    assert _capi.lib.copo_version() == _capi.ABI_VERSION == 8
    assert _capi.lib.copo_sim_set_lcf_table(None, None) == -1                    # COPO_ERR_NULL: the handle is checked first
    assert b"copo_sim_set_lcf_table" in _capi.lib.copo_last_error()
    assert _capi.lib.copo_mlp_forward_bank_f32(None, None, None, 0, 0, 0, None, None, None, None, None, None, None) != 0
    monkeypatch.setitem(_capi._SIGS, "copo_mlp_forward_bank_f64", _capi._SIGS["copo_mlp_forward_bank_f32"])
    with pytest.raises(AttributeError, match="copo_mlp_forward_bank_f64"):
        _capi._load()
