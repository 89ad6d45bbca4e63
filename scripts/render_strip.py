"""A short frame strip of a population driving, for profiles/: the CoPO Intersection population of tests/golden (through the dict env,
as copo_amd.vis does) and the Tollgate with its booth buildings hidden from the LiDAR (seeded throttle, no population of that scene
is stored in the tree).  Writes OUT/strips.npz (uint8 frames); a GIF is made from it where Pillow is installed.

    python scripts/render_strip.py OUT [--steps 120] [--every 12] [--size 256]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inter_strip(steps, every, size):
    from copo_amd.vis import load_policy, make_env
    np.random.seed(0)
    policy = load_policy("copo", "inter", os.path.join(ROOT, "tests", "golden", "eval_policy_function.npz"), key="copo_inter")
    env = make_env("inter")
    frames = []
    try:
        o, d = env.reset(), {"__all__": False}
        for t in range(steps):
            o, r, d, i = env.step(policy(o, d))
            if (t + 1) % every == 0:
                frames.append(env.render(mode="top_down", num_stack=25, film_size=(size, size)))
    finally:
        env.close()
    return np.stack(frames)


def toll_strip(steps, every, size):
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentTollgateEnv
    rng = np.random.RandomState(0)
    env = MultiAgentTollgateEnv(dict(num_agents=40))
    frames = []
    try:
        o = env.reset()
        env.render(mode="top_down", film_size=(size, size))
        for t in range(steps):
            o, r, d, i = env.step({k: np.array([rng.uniform(-0.05, 0.05), rng.uniform(0.0, 0.6)]) for k in o})
            if (t + 1) % every == 0:
                frames.append(env.render(mode="top_down", num_stack=25, film_size=(size, size)))
    finally:
        env.close()
    return np.stack(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    strips = dict(intersection=inter_strip(a.steps, a.every, a.size), tollgate=toll_strip(a.steps, a.every, a.size))
    np.savez_compressed(os.path.join(a.out, "strips.npz"), **strips)
    from copo_amd.render import write_gif
    for k, v in strips.items():
        try:
            write_gif(v, os.path.join(a.out, "render_%s.gif" % k), fps=4)
        except RuntimeError as err:
            print(err)
    print({k: v.shape for k, v in strips.items()})


if __name__ == "__main__":
    main()
