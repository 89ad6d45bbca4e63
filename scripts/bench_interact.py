"""Cost of one interaction-meter record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes.

Both are timed with device events around batches of launches after warm-up, on populated scenes (30 steps of random driving first).
One line per shape and a JSON line at the end.

    python scripts/bench_interact.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, iters, batch):
    """median, min microseconds per call over `iters` batches of `batch` back-to-back calls"""
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(batch):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / batch)
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--agents", type=int, default=40)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_interact needs a GPU"
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import SimConfig, VecSim
    rows = []
    for E in a.scenes:
        sim = VecSim(SimConfig(map="intersection", num_envs=E, num_agents=a.agents))
        meter = InteractionMeter(sim)
        rng = np.random.RandomState(0)
        act = np.zeros((E, sim.N, 2), np.float32)
        act[..., 0] = rng.uniform(-0.3, 0.3, act.shape[:2])
        act[..., 1] = rng.uniform(0.0, 1.0, act.shape[:2])
        act = torch.from_numpy(act).cuda()
        sim.reset()
        for _ in range(30):
            sim.step(act)
            meter.record()
        torch.cuda.synchronize()
        # record alone on a standing state (the accumulators move on, the poses do not), then the step alone, then both in turn
        rec_us, rec_min = timed(torch, meter.record, a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, _ = timed(torch, lambda: (sim.step(act), meter.record()), a.iters, a.batch)
        st, _ = sim.get_state()
        status = st.view(torch.int32)[13] & 0xFF
        alive, wreck = int((status == 1).sum()), int((status == 2).sum())
        summary = meter.summary(flush_open=True)
        print("%6d scenes x %d slots (%d driving, %d wrecks): record %.1f us (min %.1f), step %.1f us (min %.1f), step + record %.1f us; "
              "record / step = %.2f" % (E, sim.N, alive, wreck, rec_us, rec_min, step_us, step_min, both_us, rec_us / step_us))
        rows.append(dict(scenes=E, slots=sim.N, driving=alive, wrecks=wreck, record_us=round(rec_us, 2), step_us=round(step_us, 2),
                         step_plus_record_us=round(both_us, 2), record_over_step=round(rec_us / step_us, 3),
                         tet_frac=summary["tet_frac"], min_gap_mean=summary["min_gap_mean"]))
        meter.close()
        sim.close()
    print(json.dumps(dict(metric="interact_record_us", rows=rows)))


if __name__ == "__main__":
    main()
