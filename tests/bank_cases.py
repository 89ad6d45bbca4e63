"""Shared by tests/test_gpu_policy_bank.py and tests/test_policy_bank_cpu.py: the members of a bank and the scene of the per-scene
LCF test.  No GPU and no native library is touched at import."""
import os

import numpy as np

# ---- bank members -----------------------------------------------------------------------------------------------------------------
TORCH_LAYERS = ("_hidden_layers.0._model.0", "_hidden_layers.1._model.0", "_logits._model.0")


def golden_population(golden_dir, key):
    """One population of tests/golden/eval_policy_function.npz in the key layout it was recorded in ("copo_inter": 92 inputs,
    "ippo_inter": 91; hidden 256)."""
    with np.load(os.path.join(golden_dir, "eval_policy_function.npz")) as f:
        pre = key + "/w/"
        return {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}


def perturbed(weights, seed, sigma=0.02):
    """A copy of a population with N(0, sigma) added to every array under a fixed numpy seed."""
    rng = np.random.RandomState(seed)
    return {k: (v + rng.normal(0.0, sigma, v.shape)).astype(np.float32) for k, v in sorted(weights.items())}


def random_population(odim, hidden, seed):
    """Random weights of a two-hidden-layer policy in the torch key layout: tanh layers of unit gain, a small head."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, (rows, cols), scale in zip(TORCH_LAYERS, ((hidden, odim), (hidden, hidden), (4, hidden)), (1.0, 1.0, 0.1)):
        out[name + ".weight"] = (rng.normal(0.0, scale / np.sqrt(cols), (rows, cols))).astype(np.float32)
        out[name + ".bias"] = rng.normal(0.0, 0.05, rows).astype(np.float32)
    return out


def members(golden_dir, key, odim, hidden, K):
    """K members: the golden population (hidden 256) or a random one (other widths), then copies of it perturbed under seeds 1 .. K - 1."""
    base = golden_population(golden_dir, key) if hidden == 256 else random_population(odim, hidden, 100 + odim)
    return [base] + [perturbed(base, s) for s in range(1, K)]


# ---- the per-scene LCF scene --------------------------------------------------------------------------------------------------------
# Intersection, 6 scenes of 8 slots; horizon 50 and wrecks that clear after 5 steps, so that under LCF_ACTIONS every scene spawns both
# inside an episode (terminated agents replaced) and through a whole-scene reset within 80 steps (counted again by the test itself)
LCF_E, LCF_N, LCF_STEPS, LCF_PHASE = 6, 8, 80, 40
LCF_TABLE_ROWS = ((0.0, 0.1), (0.5, 0.2), (-0.3, 0.05))          # scenes {0, 1}, {2, 3}, {4, 5}
LCF_SECOND_DIST = (0.4, 0.3)
LCF_FORCED = 0.5


def lcf_config():
    from copo_amd.sim import SimConfig
    return SimConfig(map="intersection", num_envs=LCF_E, num_agents=LCF_N, horizon=50, delay_done=5)


def lcf_table():
    return np.repeat(np.asarray(LCF_TABLE_ROWS, np.float32), LCF_E // len(LCF_TABLE_ROWS), axis=0)


def lcf_actions():
    """The one action tensor [E, N, 2] every step takes: hard steering at high throttle ends agents quickly."""
    rng = np.random.RandomState(5)
    return np.stack([rng.uniform(-1, 1, (LCF_E, LCF_N)), rng.uniform(0.7, 1.0, (LCF_E, LCF_N))], -1).astype(np.float32)


def lcf_seeds():
    return np.arange(LCF_E, dtype=np.uint64) + np.uint64(5000)
