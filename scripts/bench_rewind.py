"""Cost of one rewind record and of a fork next to the simulator step: Intersection, 40 slots, 256 and 16 384 scenes, depth 8.

Per shape, timed with device events after warm-up on populated scenes (30 steps of random driving first): a STORED record (stride 1:
every record is one), the step alone, step + record with stride 1 and with stride 4 (three records of four launch nothing), and a fork
of `--branches` target scenes from random scenes and stored records.  One line per shape and a JSON line at the end.

    python scripts/bench_rewind.py [--scenes 256 16384] [--agents 40] [--depth 8] [--branches 1024] [--iters 20] [--batch 10]
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
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--branches", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_rewind needs a GPU"
    from copo_amd import _capi
    from copo_amd.rewind import Branches, RewindBuffer
    from copo_amd.sim import SimConfig, VecSim
    rows = []
    for E in a.scenes:
        sim = VecSim(SimConfig(map="intersection", num_envs=E, num_agents=a.agents))
        rng = np.random.RandomState(0)
        act = np.zeros((E, sim.N, 2), np.float32)
        act[..., 0] = rng.uniform(-0.3, 0.3, act.shape[:2])
        act[..., 1] = rng.uniform(0.0, 1.0, act.shape[:2])
        act = torch.from_numpy(act).cuda()
        sim.reset()
        for _ in range(30):
            sim.step(act)
        b1, b4 = RewindBuffer(sim, depth=a.depth, stride=1), RewindBuffer(sim, depth=a.depth, stride=4)
        for _ in range(a.depth + 2):
            b1.record()
        torch.cuda.synchronize()
        rec_us, rec_min = timed(torch, b1.record, a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)

        def both(buf):
            sim.step(act)
            buf.record()
        both1_us, _ = timed(torch, lambda: both(b1), a.iters, 4 * a.batch)
        both4_us, _ = timed(torch, lambda: both(b4), a.iters, 4 * a.batch)
        # ---- fork: the raw entry point on device arrays made once (RewindBuffer.fork uploads its requests on every call) ----
        br = Branches(b1, a.branches)
        lo, hi = b1.span()
        scene = torch.from_numpy(rng.randint(0, E, a.branches).astype(np.int32)).cuda()
        recs = torch.from_numpy(rng.randint(lo, hi + 1, a.branches).astype(np.int32)).cuda()
        status = torch.empty(a.branches, dtype=torch.int32, device="cuda")
        st = _capi.current_stream()

        def fork():
            _capi.check(_capi.lib.copo_rewind_fork(b1._h, br.sim._h, 0, a.branches, scene.data_ptr(), recs.data_ptr(), None, None, None,
                                                   status.data_ptr(), None, st))
        fork()
        assert (status >= lo).all()
        fork_us, fork_min = timed(torch, fork, a.iters, a.batch)
        ring_mb = (64 * sim.N * E * a.depth + 16 * E * a.depth) / 1e6
        moved_mb = 2 * 64 * sim.N * E / 1e6
        print("%6d scenes x %d slots: stored record %.1f us (min %.1f, %.1f MB moved, ring %.0f MB), step %.1f us (min %.1f), record / step = "
              "%.3f; step + record %.1f us at stride 1, %.1f us at stride 4; fork of %d branches %.1f us (min %.1f)"
              % (E, sim.N, rec_us, rec_min, moved_mb, ring_mb, step_us, step_min, rec_us / step_us, both1_us, both4_us, a.branches, fork_us,
                 fork_min))
        rows.append(dict(scenes=E, slots=sim.N, depth=a.depth, record_us=round(rec_us, 2), step_us=round(step_us, 2),
                         record_over_step=round(rec_us / step_us, 3), step_plus_record_stride1_us=round(both1_us, 2),
                         step_plus_record_stride4_us=round(both4_us, 2), branches=a.branches, fork_us=round(fork_us, 2),
                         ring_mb=round(ring_mb, 1)))
        br.close()
        b1.close()
        b4.close()
        sim.close()
    print(json.dumps(dict(metric="rewind_record_us", rows=rows)))


if __name__ == "__main__":
    main()
