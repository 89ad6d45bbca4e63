"""Who met whom in a population: drive it as `python -m copo_amd.vis` does (one scene of the dict env, the same policy options) with the
conflict log and the trip log on, and print `ConflictTable.summary` by type and by outcome and the routes x routes matrix of the encounters.

    python scripts/conflicts_report.py --env inter --algo copo --weights tests/golden/eval_policy_function.npz --key copo_inter --steps 1000 [--out conflicts.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(env_name, algo, weights, steps, key=None, seed=0, max_rows=65536, radius=8.0, leave_radius=10.0):
    """Roll `steps` env steps; returns (the `ConflictTable`, the `TripTable` of the same run), open encounters and trips flushed at the end."""
    from copo_amd.eval.evaluate_population import _SCENES
    from copo_amd.torch_copo.utils import env_wrappers as W
    from copo_amd.vis import load_policy
    np.random.seed(seed)
    policy = load_policy(algo, env_name, weights, key)
    cls_name, n = _SCENES[env_name]
    env = getattr(W, cls_name)(dict(num_agents=n, trip_log=dict(max_rows=max_rows)))
    try:
        o, d = env.reset(), {"__all__": False}
        log = env.conflict_log(max_rows=max_rows, radius=radius, leave_radius=leave_radius)
        for _ in range(steps):
            o, r, d, info = env.step(policy(o, d))
            if d["__all__"]:
                o, d = env.reset(), {"__all__": False}
                policy.reset()
        log.flush()
        env.trip_log().flush()
        return log.table(), env.trip_log().table()
    finally:
        env.close()


def report(table, trips):
    lines = ["%d encounters in %d records (%d rows dropped), radius %g m / %g m" % (len(table), table.meta["n_records"], table.meta["dropped"],
                                                                                    table.meta["radius"], table.meta["leave_radius"])]
    if len(table):
        lines += ["", "by type", table.text("type"), "", "by outcome", table.text("outcome")]
        m = table.route_matrix(trips)
        lines += ["", "encounters by route pair (both crashed in brackets); %d parties without a trip row" % m["missing"],
                  "route " + " ".join("%9d" % r for r in m["routes"])]
        for i, r in enumerate(m["routes"]):
            lines.append("%5d " % r + " ".join("%4d (%2d)" % (m["all"][i, j], m["both_crashed"][i, j]) for j in range(len(m["routes"]))))
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
    ap.add_argument("--radius", type=float, default=8.0, metavar="M")
    ap.add_argument("--leave-radius", type=float, default=10.0, metavar="M")
    ap.add_argument("--out", default=None, metavar="FILE.npz", help="also write the table")
    a = ap.parse_args()
    table, trips = run(a.env, a.algo, a.weights, a.steps, a.key, a.seed, a.max_rows, a.radius, a.leave_radius)
    print(report(table, trips))
    if a.out:
        print("wrote", table.save(a.out))


if __name__ == "__main__":
    main()
