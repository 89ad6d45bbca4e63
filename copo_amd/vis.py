"""Watch a trained population drive: the reference's `copo/vis.py` loop (PolicyFunction -> env.step -> env.render) with the
top-down frames written to disk.

    python -m copo_amd.vis --env inter --algo copo --weights FILE.npz [--key copo_inter] --steps 300 --out DIR [--gif] [--follow SLOT]
                           [--interaction]

`--weights` is a population file (`{ALGO}_{ENV}.npz` with the reference's key layout); `--key NAME` takes the arrays stored under
`NAME/w/` of a bundle instead.  One PPM per step (`DIR/frame_00000.ppm`, ...), plus `DIR/vis.gif` with `--gif` (needs Pillow).
At the end of every scene episode the reference's summary dict is printed; with `--interaction` the interaction metrics of that
episode's agents (gaps, time to collision, near misses, harsh braking: copo_amd/interact.py) are printed next to it, and those of all
agents of the run, finished or not, at the end.
"""
import argparse
import os

import numpy as np

from copo_amd.eval.evaluate_population import _SCENES
from copo_amd.eval.get_policy_function import PolicyFunction, _gaussian_head, layer_arrays, meta_svo_lookup_table, population_layout


def load_policy(algo, env, weights_path, key=None):
    """PolicyFunction over the arrays of `weights_path` (all of them, or those under `key/w/`)."""
    with np.load(weights_path) as f:
        if key:
            pre = key + "/w/"
            w = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
            if not w:
                raise KeyError("%s holds no arrays under %r" % (weights_path, pre))
        else:
            w = {k: f[k] for k in f.files}
    name = "%s_%s" % (algo, env)
    layout, sfx = population_layout(name)
    layers = layer_arrays(w, layout, "default", sfx)
    pf = PolicyFunction(policy=lambda obs: _gaussian_head(layers, obs, False))
    if algo == "copo":           # the population's trained LCF distribution, appended to the observation (process_svo)
        pf.use_svo, pf.lcf_dist = True, meta_svo_lookup_table[key if key in meta_svo_lookup_table else name]
    return pf


def make_env(env, interaction=False):
    from copo_amd.torch_copo.utils import env_wrappers as W
    cls_name, n = _SCENES[env]
    return getattr(W, cls_name)(dict(num_agents=n, interaction_metrics=bool(interaction)))


def run(env_name, algo, weights, steps, out, key=None, gif=False, follow=None, film_size=(512, 512), seed=0, fps=10, interaction=False):
    """Roll `steps` env steps, writing one frame per step; returns the list of frame paths."""
    from copo_amd.render import write_gif, write_ppm
    np.random.seed(seed)
    policy = load_policy(algo, env_name, weights, key)
    env = make_env(env_name, interaction)
    paths, kept = [], []
    try:
        o, d = env.reset(), {"__all__": False}
        ep_success = ep_step = ep_agent = 0
        for t in range(steps):
            o, r, d, info = env.step(policy(o, d))
            ep_step += 1
            for k, done in d.items():
                if k != "__all__" and done:
                    ep_success += 1 if info[k]["arrive_dest"] else 0
                    ep_agent += 1
            if d["__all__"]:
                print({"total agents": ep_agent, "existing agents": len(o),
                       "success rate": ep_success / ep_agent if ep_agent > 0 else None, "ep step": ep_step},
                      *([{"interaction": env.interaction_summary()}] if interaction else []))
                ep_success = ep_step = ep_agent = 0
                o, d = env.reset(), {"__all__": False}
                policy.reset()
            ids = env._slot_ids or []
            track = ids[follow] if follow is not None and follow < len(ids) else None
            frame = env.render(mode="top_down", num_stack=25, film_size=film_size, track_agent=track)
            paths += write_ppm(frame, out, start=t)
            if gif:
                kept.append(frame)
        if interaction:
            print({"interaction, agents still driving included": env.interaction_summary(flush_open=True)})
    finally:
        env.close()
    if gif and kept:
        write_gif(np.stack(kept), os.path.join(out, "vis.gif"), fps=fps)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="inter", choices=sorted(_SCENES))
    ap.add_argument("--algo", default="copo", choices=["cl", "copo", "ippo", "ccppo"])
    ap.add_argument("--weights", required=True, help="population .npz")
    ap.add_argument("--key", default=None, help="take the arrays under KEY/w/ of a bundle")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--gif", action="store_true", help="also write DIR/vis.gif (needs Pillow)")
    ap.add_argument("--follow", type=int, default=None, help="centre the view on this agent slot")
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("W", "H"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--interaction", action="store_true", help="measure and print the interaction metrics")
    a = ap.parse_args(argv)
    paths = run(a.env, a.algo, a.weights, a.steps, a.out, key=a.key, gif=a.gif, follow=a.follow, film_size=tuple(a.size), seed=a.seed,
                interaction=a.interaction)
    print("wrote %d frames to %s" % (len(paths), a.out))


if __name__ == "__main__":
    main()
