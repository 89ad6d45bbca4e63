"""Who went through the spot another had just left: drive a population as `python -m copo_amd.vis` does (one scene of the dict env, the same
policy options) with the encroachment log on, print `EncroachmentTable.summary` by type and PET band and the share of critical encounters,
and write a frame of the renderer (one PPM) with the map of critical encounters blended over it.

    python scripts/pet_report.py --env inter --algo copo --weights tests/golden/eval_policy_function.npz --key copo_inter --steps 1000 [--out pet.npz] [--frame pet.ppm]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(env_name, algo, weights, steps, key=None, seed=0, max_rows=65536, cell=1.0, window=50, critical_s=1.0, size=512):
    """Roll `steps` env steps; returns (the `EncroachmentTable`, the `aggregates()` dict, an overlay frame uint8 [size, size, 3])."""
    from copo_amd.eval.evaluate_population import _SCENES
    from copo_amd.torch_copo.utils import env_wrappers as W
    from copo_amd.vis import load_policy
    np.random.seed(seed)
    policy = load_policy(algo, env_name, weights, key)
    cls_name, n = _SCENES[env_name]
    env = getattr(W, cls_name)(dict(num_agents=n))
    try:
        o, d = env.reset(), {"__all__": False}
        log = env.encroachment_log(cell=cell, window=window, critical_s=critical_s, max_rows=max_rows)
        for _ in range(steps):
            o, r, d, info = env.step(policy(o, d))
            if d["__all__"]:
                o, d = env.reset(), {"__all__": False}
                policy.reset()
        table, agg = log.table(), log.aggregates()
        from copo_amd.render import map_view
        frame = env.render(mode="top_down", num_stack=1, film_size=(size, size))
        return table, agg, log.heat_overlay(frame, agg["critical"].sum(0), map_view(env.sim.tables, size, size))
    finally:
        env.close()


def report(table, agg):
    m = table.meta
    lines = ["%d encounters in %d records (%d rows dropped), %d x %d cells of %g m, window %d records, critical at %d records or fewer"
             % (len(table), m["n_records"], m["dropped"], m["W"], m["H"], m["cell"], m["window"], m["critical_records"])]
    if len(table):
        lines += ["", table.text(), "", "critical share by type: " + ", ".join(
            "%s %.3f" % (k, v) for k, v in zip(("following", "crossing", "opposing"), agg["critical_frac"][0]) if not np.isnan(v))]
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
    ap.add_argument("--cell", type=float, default=1.0, metavar="M")
    ap.add_argument("--window", type=int, default=50, metavar="RECORDS")
    ap.add_argument("--critical-s", type=float, default=1.0, metavar="S")
    ap.add_argument("--out", default=None, metavar="FILE.npz", help="also write the table")
    ap.add_argument("--frame", default="pet_overlay.ppm", metavar="FILE.ppm", help="the overlay frame")
    a = ap.parse_args()
    table, agg, frame = run(a.env, a.algo, a.weights, a.steps, a.key, a.seed, a.max_rows, a.cell, a.window, a.critical_s)
    print(report(table, agg))
    if a.out:
        print("wrote", table.save(a.out))
    with open(a.frame, "wb") as fh:              # (binary PPM, as `render.write_ppm` writes its numbered frames)
        fh.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
        fh.write(frame.tobytes())
    print("wrote", a.frame)


if __name__ == "__main__":
    main()
