"""Top-down renderer throughput: 256 Intersection scenes x 40 slots, 512 x 512 frames, a 25-snapshot trail, every scene in one call.

Prints the device-event time per batch after warm-up, the bytes written (S * H * W * 4) against the store floor at 6.3 TB/s, and the
numpy restatement's time for one frame (tests/render_numpy.py) for scale.  One JSON line at the end.

    python scripts/bench_render.py [--scenes 256] [--size 512] [--trail 25] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STORE_RATE = 6.3e12      # achievable HBM store rate, bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--agents", type=int, default=40)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--trail", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_render needs a GPU"
    from copo_amd.render import TopDownRenderer
    from copo_amd.sim import SimConfig, VecSim
    cfg = SimConfig(map="intersection", num_envs=a.scenes, num_agents=a.agents)
    sim = VecSim(cfg)
    r = TopDownRenderer(sim, a.size, a.size, trail=a.trail)
    rng = np.random.RandomState(0)
    sim.reset()
    for _ in range(a.trail + 5):          # populated scenes and a full trail ring
        act = np.zeros((a.scenes, sim.N, 2), np.float32)
        act[..., 0] = rng.uniform(-0.3, 0.3, act.shape[:2])
        act[..., 1] = rng.uniform(0.0, 1.0, act.shape[:2])
        sim.step(torch.from_numpy(act).cuda())
        r.record()
    views = r.views(np.arange(a.scenes), "map")
    for _ in range(a.warmup):
        r.frames(views=views)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f = r.frames(views=views)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)       # us
    S, H, W = a.scenes, a.size, a.size
    nbytes = S * H * W * 4
    floor_us = nbytes / STORE_RATE * 1e6
    med = float(np.median(times))
    st, env = sim.get_state()
    import render_numpy as rn
    mp = rn.Map(cfg)
    stn, envn = st.cpu().numpy(), env.cpu().numpy()
    t = time.perf_counter()
    rn.render_frame(mp, stn, envn, 0, views[0], W, H)
    np_ms = (time.perf_counter() - t) * 1e3
    alive = int(((stn.view(np.int32)[13] & 0xFF) == 1).sum())
    print("frames %d x %d x %d, trail %d, %d alive vehicles" % (S, H, W, a.trail, alive))
    print("device time per batch: median %.1f us (min %.1f, max %.1f over %d)" % (med, min(times), max(times), a.iters))
    print("bytes written %.1f MB, store floor %.1f us at %.1f TB/s: kernel at %.2f x the floor (%.0f %% of it)"
          % (nbytes / 1e6, floor_us, STORE_RATE / 1e12, med / floor_us, 100.0 * floor_us / med))
    print("numpy restatement, one frame: %.1f ms" % np_ms)
    print(json.dumps(dict(metric="render_batch_us", scenes=S, size=H, trail=a.trail, median_us=round(med, 2), min_us=round(min(times), 2),
                          bytes=nbytes, floor_us=round(floor_us, 2), floor_share=round(floor_us / med, 4), numpy_frame_ms=round(np_ms, 1),
                          frames_per_s=round(S / med * 1e6, 1))))
    r.close()
    sim.close()
    del f


if __name__ == "__main__":
    main()
