"""What if: drive every crash of a shipped population again, from before it happened, under other LCFs.

The reference's CoPO Intersection population (tests/golden/eval_policy_function.npz, deterministic actions) drives `--scenes` scenes
with the env keys `event_clips` (crash, `--pre` / `--post`) and `rewind` (stride 1, a ring deep enough to hold a clip's first record
when the clip is committed).  For every crash clip, as soon as it is committed, the scene is forked at the clip's `first_rec` into one
CONTROL branch (LCF unchanged, the source's seed, deterministic actions) and `--copies` branches per LCF of `--lcf` (that LCF for the
agents driving at the fork, a seed of their own, Gaussian action noise `--noise`); the slot that triggered the clip is watched.  Clips
whose watched slot does not hold the triggering agent at `first_rec` (it spawned inside the clip) are skipped and counted.  The branches
run `pre + post + margin` steps; printed per LCF: the share of branches in which the watched agent ends without the CRASH bit (or does
not end at all).  Self-check: the control branch must crash again in the step that leads to the clip's trigger record.

    python scripts/whatif_crashes.py [--scenes 8] [--steps 300] [--lcf -1 0 1] [--copies 8] [--noise 0.1] [--pre 10] [--post 2] [--margin 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_policy(torch, device, model="copo_inter"):
    """obs [..., O] -> the Gaussian head's mean [..., 2] on the device, in float64 and rounded once: a row's actions do not depend on
    how many rows a call holds, so a branch and its source decide alike"""
    from copo_amd.eval.get_policy_function import layer_arrays, population_layout
    with np.load(os.path.join(ROOT, "tests", "golden", "eval_policy_function.npz")) as f:
        pre = model + "/w/"
        w = {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
    layout, sfx = population_layout(model)
    layers = [(torch.from_numpy(a.astype(np.float64)).to(device), torch.from_numpy(b.astype(np.float64)).to(device))
              for a, b in layer_arrays(w, layout, "default", sfx)]

    def act(obs):
        x = obs.reshape(-1, obs.shape[-1]).to(torch.float64)
        for d, (a, b) in enumerate(layers):
            x = x @ a + b
            if d < len(layers) - 1:
                x = torch.tanh(x)
        return x[:, :2].to(torch.float32).reshape(obs.shape[:-1] + (2,)).contiguous()
    return act


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=5000)
    ap.add_argument("--lcf", type=float, nargs="+", default=[-1.0, 0.0, 1.0])
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--pre", type=int, default=10)
    ap.add_argument("--post", type=int, default=2)
    ap.add_argument("--margin", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "whatif_crashes needs a GPU"
    from copo_amd.clips import HEADER_KEYS
    from copo_amd.eval.get_policy_function import meta_svo_lookup_table
    from copo_amd.rewind import Branches
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv, get_lcf_env
    mean, std = meta_svo_lookup_table["copo_inter"]
    env = get_lcf_env(MultiAgentIntersectionEnv)(dict(
        num_envs=a.scenes, start_seed=a.seed, lcf_mean=float(mean), lcf_std=float(std), lcf_normal_std=float(std),
        event_clips=dict(pre=a.pre, post=a.post, max_clips=4096, flags=("crash",)),
        rewind=dict(depth=a.pre + a.post + 2, stride=1, keep_obs=True)))
    buf = env.rewind_buffer()
    L, K = len(a.lcf), a.copies
    B = 1 + L * K
    br = Branches(buf, B)
    br.sim.set_lcf_dist(float(mean), float(std))
    policy = torch_policy(torch, env.sim.device)
    gen = torch.Generator(device=env.sim.device).manual_seed(a.seed)
    noisy = torch.ones(B, 1, 1, device=env.sim.device)
    noisy[0] = 0.0                                         # branch 0 is the control

    def branch_policy(obs):
        act = policy(obs)
        return act + noisy * a.noise * torch.randn(act.shape, device=act.device, generator=gen)
    lcfs = np.r_[np.nan, np.repeat(np.asarray(a.lcf, np.float32), K)].astype(np.float32)
    escaped, branches, done_clips, skipped, out_of_ring = np.zeros(L), 0, 0, 0, 0
    try:
        out = env.vec_reset()
        n_seen = 0
        for t in range(a.steps):
            out = env.vec_step(policy(out["obs"]))
            n_now, _ = env.observer("event_clips").count()
            if n_now == n_seen:
                continue
            cs = env.event_clips()
            for c in range(n_seen, n_now):
                h = dict(zip(HEADER_KEYS, cs.header[c].tolist()))
                lo, _ = buf.span()
                if h["first_rec"] < lo or h["first_rec"] >= h["trig_rec"]:
                    out_of_ring += 1
                    continue
                seeds = np.r_[np.uint64(a.seed + h["scene"]), np.arange(1, B, dtype=np.uint64) * np.uint64(7919) + np.uint64(1000003 * (c + 1))]
                status, aid = br.fork([h["scene"]] * B, [h["first_rec"]] * B, lcf=lcfs, seeds=seeds, watch_slots=h["trig_slot"])
                assert (status == h["first_rec"]).all()
                if int(aid[0]) != h["trig_aid"]:
                    skipped += 1
                    continue
                br.rollout(branch_policy, a.pre + a.post + a.margin)
                o = br.outcomes()
                # self-check: the control repeats the source -- its watched agent crashes in the step that leads to trig_rec
                assert o["watch_flags"][0] & 0x08 and o["watch_step"][0] == h["trig_rec"] - h["first_rec"] - 1, (h, o["watch_flags"][0], o["watch_step"][0])
                ok = ((o["watch_flags"][1:] & 0x08) == 0).reshape(L, K)
                escaped += ok.sum(1)
                branches += K
                done_clips += 1
            n_seen = n_now
        print("%d scenes x %d steps: %d crash clips driven again (%d skipped: the watched slot held another agent at first_rec; %d not forkable), "
              "%d branches per LCF" % (a.scenes, a.steps, done_clips, skipped, out_of_ring, branches))
        rows = []
        for v, n in zip(a.lcf, escaped):
            share = n / branches if branches else float("nan")
            print("  LCF %+.2f: the watched agent ends without a crash in %5.1f %% of the branches" % (v, 100.0 * share))
            rows.append(dict(lcf=float(v), no_crash_share=round(float(share), 4)))
        print(json.dumps(dict(metric="whatif_no_crash_share", clips=done_clips, skipped=skipped, branches_per_lcf=branches, noise=a.noise, rows=rows)))
    finally:
        br.close()
        env.close()


if __name__ == "__main__":
    main()
