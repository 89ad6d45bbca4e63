"""Cost of one trip-log record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes, fed with the step's
flags and rewards and the interaction meter's gap / ttc arrays.

Timed with device events after warm-up on populated scenes (30 steps of random driving first), medians of `--iters` batches of `--batch`
back-to-back calls:
  record   the record alone (three launches; the state stands still, so nothing closes: the memory traffic is that of any record)
  step     the step alone, and step + record
One line per shape and a JSON line at the end.

    python scripts/bench_trips.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10]
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
    assert torch.cuda.is_available(), "bench_trips needs a GPU"
    from copo_amd.interact import InteractionMeter
    from copo_amd.sim import SimConfig, VecSim
    from copo_amd.trips import TripLog
    rows = []
    for E in a.scenes:
        sim = VecSim(SimConfig(map="intersection", num_envs=E, num_agents=a.agents))
        rng = np.random.RandomState(0)
        act = np.zeros((E, sim.N, 2), np.float32)
        act[..., 0] = rng.uniform(-0.3, 0.3, act.shape[:2])
        act[..., 1] = rng.uniform(0.0, 1.0, act.shape[:2])
        act = torch.from_numpy(act).cuda()
        sim.reset()
        log, meter = TripLog(sim, max_rows=1 << 20), InteractionMeter(sim)
        gap, ttc = meter.record()
        log.record(None, None, gap, ttc)
        for _ in range(30):
            out = sim.step(act)
            meter.record()
            log.record(out["flags"], out["rew"], gap, ttc)
        torch.cuda.synchronize()
        flags, rew = out["flags"].clone(), out["rew"].clone()
        flags &= 0x01                                         # (the state stands still: an end would be booked again in every call)

        def both():
            o = sim.step(act)
            log.record(o["flags"], o["rew"], gap, ttc)
        rec_us, rec_min = timed(torch, lambda: log.record(flags, rew, gap, ttc), a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, both_min = timed(torch, both, a.iters, a.batch)
        n_rows, dropped = log.count()
        print("%6d scenes x %d slots: record %.1f us (min %.1f), step %.1f us (min %.1f), step + record %.1f us (min %.1f), record / step = %.3f "
              "(%d rows, %d dropped in %d records)"
              % (E, sim.N, rec_us, rec_min, step_us, step_min, both_us, both_min, rec_us / step_us, n_rows, dropped, log.n_records))
        rows.append(dict(scenes=E, slots=sim.N, record_us=round(rec_us, 2), step_us=round(step_us, 2), step_plus_record_us=round(both_us, 2),
                         record_over_step=round(rec_us / step_us, 3), rows=n_rows, dropped=dropped, records=log.n_records))
        log.close()
        meter.close()
        sim.close()
    print(json.dumps(dict(metric="trip_record_us", rows=rows)))


if __name__ == "__main__":
    main()
