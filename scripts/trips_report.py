"""Per-agent trip table of a population: drive it as `python -m copo_amd.vis` does (one scene of the dict env, the same policy options)
with the trip log and the interaction meter on, and print `TripTable.summary` by route, by outcome and by LCF quartile.

    python scripts/trips_report.py --env inter --algo copo --weights tests/golden/eval_policy_function.npz --key copo_inter --steps 1000 [--out trips.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(env_name, algo, weights, steps, key=None, seed=0, max_rows=65536, stop_speed=0.5):
    """Roll `steps` env steps; returns the `TripTable` of the agents that finished (the ones still driving are left out)."""
    from copo_amd.eval.evaluate_population import _SCENES
    from copo_amd.torch_copo.utils import env_wrappers as W
    from copo_amd.vis import load_policy
    np.random.seed(seed)
    policy = load_policy(algo, env_name, weights, key)
    cls_name, n = _SCENES[env_name]
    env = getattr(W, cls_name)(dict(num_agents=n, interaction_metrics=True, trip_log=dict(max_rows=max_rows, stop_speed=stop_speed)))
    try:
        o, d = env.reset(), {"__all__": False}
        for _ in range(steps):
            o, r, d, info = env.step(policy(o, d))
            if d["__all__"]:
                o, d = env.reset(), {"__all__": False}
                policy.reset()
        return env.trip_log().table()
    finally:
        env.close()


def report(table):
    lines = ["%d finished agents in %d records (%d rows dropped)" % (len(table), table.meta["n_records"], table.meta["dropped"])]
    if len(table):
        edges = np.quantile(table.lcf, [0.0, 0.25, 0.5, 0.75, 1.0])
        for title, by in (("by route", "route"), ("by outcome", "outcome")) + ((("by LCF quartile", edges),) if (np.diff(edges) > 0).all() else ()):
            lines += ["", title, table.text(by)]
    return "\n".join(lines)


def main():
    from copo_amd.eval.evaluate_population import _SCENES
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="inter", choices=sorted(_SCENES))
    ap.add_argument("--algo", default="copo", choices=["cl", "copo", "ippo", "ccppo"])
    ap.add_argument("--weights", required=True, help="population .npz")
    ap.add_argument("--key", default=None, help="take the arrays under KEY/w/ of a bundle")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-rows", type=int, default=65536)
    ap.add_argument("--stop-speed", type=float, default=0.5, metavar="M/S")
    ap.add_argument("--out", default=None, metavar="FILE.npz", help="also write the table")
    a = ap.parse_args()
    table = run(a.env, a.algo, a.weights, a.steps, a.key, a.seed, a.max_rows, a.stop_speed)
    print(report(table))
    if a.out:
        print("wrote", table.save(a.out))


if __name__ == "__main__":
    main()
