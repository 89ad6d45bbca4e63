"""Watch a trained population drive: the reference's `copo/vis.py` loop (PolicyFunction -> env.step -> env.render) with the
top-down frames written to disk.

    python -m copo_amd.vis --env inter --algo copo --weights FILE.npz [--key copo_inter] --steps 300 --out DIR [--gif] [--follow SLOT]
                           [--interaction] [--clips [--clip-pre N] [--clip-post N] [--clip-on crash,out,ttc<1.0,gap<0.5]]
                           [--heatmap LAYER [--heatmap-out FILE.ppm]] [--gates [--gate-inset METRES]]
    python -m copo_amd.vis --replay FILE.npz --out DIR [--size W H] [--follow SLOT]

`--weights` is a population file (`{ALGO}_{ENV}.npz` with the reference's key layout); `--key NAME` takes the arrays stored under
`NAME/w/` of a bundle instead.  One PPM per step (`DIR/frame_00000.ppm`, ...), plus `DIR/vis.gif` with `--gif` (needs Pillow).
At the end of every scene episode the reference's summary dict is printed; with `--interaction` the interaction metrics of that
episode's agents (gaps, time to collision, near misses, harsh braking: copo_amd/interact.py) are printed next to it, and those of all
agents of the run, finished or not, at the end.

`--clips` runs the flight recorder (copo_amd/clips.py) next to the rollout: the `--clip-pre` steps before and `--clip-post` after every
event of `--clip-on` -- step flags by name, `ttc<SECONDS`, `gap<METRES` -- are kept as clips, written at the end to `DIR/clips.npz` and,
played back, to `DIR/clip_000/frame_00000.ppm`, ...  `--replay FILE.npz` renders the clips of such a file again: no policy, no
simulator run, no `--weights`.

`--heatmap LAYER` runs the field maps (copo_amd/fields.py, 1 m cells over the map) next to the rollout and writes, after the run, the map
view with that layer -- one of the ten integer layers, `mean_speed` or `occupancy_s` -- blended over it to `--heatmap-out` (default
`DIR/heatmap_LAYER.ppm`); `critical` counts the steps below a time to collision of 1.5 s.

`--gates` runs the traffic gates (copo_amd/gates.py: an entry and an exit gate per route, `--gate-inset` metres from its ends) next to
the rollout, draws them into every frame and prints the per-gate and per-section table -- crossings, vehicles per hour, mean speed,
completed trips and mean travel time -- at the end.
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


def make_env(env, interaction=False, clips=None, fields=None, gates=None):
    from copo_amd.torch_copo.utils import env_wrappers as W
    cls_name, n = _SCENES[env]
    return getattr(W, cls_name)(dict(num_agents=n, interaction_metrics=bool(interaction), event_clips=clips, field_maps=fields, traffic_gates=gates))


HEATMAP_LAYERS = ("occupancy", "wreck", "visits", "speed_q", "vx_q", "vy_q", "crash", "out", "arrive", "critical", "mean_speed", "occupancy_s")


def write_heatmap(env, layer, path, film_size=(512, 512)):
    """The map view of scene 0 without a trail, `layer` of the env's field maps (group 0) blended over it, as one PPM; returns the path."""
    from copo_amd.render import map_view
    fm = env.field_maps()
    frame = env.render(mode="top_down", num_stack=1, film_size=film_size)
    out = fm.heat_overlay(frame, fm.read()[layer][0], map_view(env.sim.tables, int(film_size[0]), int(film_size[1])))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:                 # (binary PPM, as `render.write_ppm` writes its numbered frames)
        fh.write(b"P6\n%d %d\n255\n" % (out.shape[1], out.shape[0]))
        fh.write(out.tobytes())
    return path


def parse_clip_on(spec):
    """`crash,out,ttc<1.0,gap<0.5` -> dict(flags, ttc_below, gap_below) of `ClipRecorder`."""
    from copo_amd.clips import FLAG_BITS
    flags, kw = [], dict(ttc_below=0.0, gap_below=0.0)
    for item in (x.strip() for x in spec.split(",") if x.strip()):
        name, lt, value = item.partition("<")
        if lt and name in ("ttc", "gap") and float(value) > 0.0:
            kw[name + "_below"] = float(value)
        elif not lt and name in FLAG_BITS:
            flags.append(name)
        else:
            raise ValueError("--clip-on item %r: a flag of %s, ttc<SECONDS or gap<METRES" % (item, "/".join(FLAG_BITS)))
    return dict(flags=tuple(flags), **kw)


def write_clips(clipset, out, film_size=(512, 512), follow=None, device=0):
    """Play every clip of `clipset` back and write `out/clip_000/frame_00000.ppm`, ...; returns the paths."""
    from copo_amd.clips import ClipPlayer
    from copo_amd.render import write_ppm
    paths = []
    if not len(clipset):
        return paths
    player = ClipPlayer(clipset, device=device)
    try:
        for c in range(len(clipset)):
            frames = player.render(c, film_size=film_size, view="map" if follow is None else "follow", follow_slot=follow)
            paths += write_ppm(frames, os.path.join(out, "clip_%03d" % c))
            print("clip %d:" % c, clipset.info(c))
    finally:
        player.close()
    return paths


def replay(path, out, film_size=(512, 512), follow=None):
    """Render the clips of a saved clip set; returns the list of frame paths."""
    from copo_amd.clips import ClipSet
    return write_clips(ClipSet.load(path), out, film_size, follow)


def run(env_name, algo, weights, steps, out, key=None, gif=False, follow=None, film_size=(512, 512), seed=0, fps=10, interaction=False,
        clips=None, heatmap=None, heatmap_out=None, gates=None):
    """Roll `steps` env steps, writing one frame per step; returns the list of frame paths.  `clips`: the arguments of a `ClipRecorder`
    (then `out/clips.npz` and the played-back clips are written too)."""
    from copo_amd.render import write_gif, write_ppm
    np.random.seed(seed)
    policy = load_policy(algo, env_name, weights, key)
    fields = None
    if heatmap is not None:
        if heatmap not in HEATMAP_LAYERS:
            raise ValueError("--heatmap %r: one of %s" % (heatmap, ", ".join(HEATMAP_LAYERS)))
        fields = dict(cell=1.0, ttc_below=1.5 if heatmap == "critical" else 0.0)
    env = make_env(env_name, interaction or bool(clips and (clips.get("ttc_below") or clips.get("gap_below"))) or heatmap == "critical", clips,
                   fields, gates)
    clipset = None
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
            if gates is not None and track is None:      # (the map view; a followed agent's view moves with it)
                from copo_amd.render import map_view
                frame = env.traffic_gates().gate_overlay(np.asarray(frame), map_view(env.sim.tables, int(film_size[0]), int(film_size[1])))
            paths += write_ppm(frame, out, start=t)
            if gif:
                kept.append(frame)
        if interaction:
            print({"interaction, agents still driving included": env.interaction_summary(flush_open=True)})
        if clips is not None:
            clipset = env.event_clips(flush=True)
        if gates is not None:
            print(env.traffic_gates().table())
        if heatmap is not None:
            p = write_heatmap(env, heatmap, heatmap_out or os.path.join(out, "heatmap_%s.ppm" % heatmap), film_size)
            print("wrote the %s map of %d records to %s" % (heatmap, env.field_maps().n_records, p))
    finally:
        env.close()
    if gif and kept:
        write_gif(np.stack(kept), os.path.join(out, "vis.gif"), fps=fps)
    if clipset is not None:
        os.makedirs(out, exist_ok=True)
        clipset.save(os.path.join(out, "clips.npz"))
        clip_paths = write_clips(clipset, out, film_size, follow)
        print("wrote %d clips (%d frames) to %s" % (len(clipset), len(clip_paths), out))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="inter", choices=sorted(_SCENES))
    ap.add_argument("--algo", default="copo", choices=["cl", "copo", "ippo", "ccppo"])
    ap.add_argument("--weights", default=None, help="population .npz (not needed with --replay)")
    ap.add_argument("--key", default=None, help="take the arrays under KEY/w/ of a bundle")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--gif", action="store_true", help="also write DIR/vis.gif (needs Pillow)")
    ap.add_argument("--follow", type=int, default=None, help="centre the view on this agent slot")
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("W", "H"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--interaction", action="store_true", help="measure and print the interaction metrics")
    ap.add_argument("--clips", action="store_true", help="record event clips: DIR/clips.npz and DIR/clip_NNN/frame_*.ppm")
    ap.add_argument("--clip-pre", type=int, default=24, help="steps kept before an event")
    ap.add_argument("--clip-post", type=int, default=8, help="steps kept after an event")
    ap.add_argument("--clip-on", default="crash", help="events: step flags by name, ttc<SECONDS, gap<METRES, comma separated")
    ap.add_argument("--heatmap", default=None, metavar="LAYER", help="field maps: write the map view with this layer over it (%s)" % ", ".join(HEATMAP_LAYERS))
    ap.add_argument("--heatmap-out", default=None, metavar="FILE.ppm", help="where the overlay goes (default DIR/heatmap_LAYER.ppm)")
    ap.add_argument("--gates", action="store_true", help="traffic gates: draw them into the frames, print the flow table at the end")
    ap.add_argument("--gate-inset", type=float, default=10.0, metavar="METRES", help="distance of the gates from the ends of every route")
    ap.add_argument("--replay", default=None, metavar="FILE.npz", help="render the clips of a saved clip set instead of running a policy")
    a = ap.parse_args(argv)
    if a.replay:
        paths = replay(a.replay, a.out, film_size=tuple(a.size), follow=a.follow)
        print("wrote %d frames to %s" % (len(paths), a.out))
        return
    if not a.weights:
        ap.error("--weights is required (unless --replay)")
    clips = dict(pre=a.clip_pre, post=a.clip_post, **parse_clip_on(a.clip_on)) if a.clips else None
    paths = run(a.env, a.algo, a.weights, a.steps, a.out, key=a.key, gif=a.gif, follow=a.follow, film_size=tuple(a.size), seed=a.seed,
                interaction=a.interaction, clips=clips, heatmap=a.heatmap, heatmap_out=a.heatmap_out,
                gates=dict(inset=a.gate_inset) if a.gates else None)
    print("wrote %d frames to %s" % (len(paths), a.out))


if __name__ == "__main__":
    main()
