"""Cost of one event-clip record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes.

Two cases per shape, timed with device events after warm-up on populated scenes (30 steps of random driving first):
  idle    no scene fires: the snapshot into the rings, the trigger test, the id pass and a commit launch that finds nothing to do --
          batches of back-to-back records, and the step alone and step + record for comparison
  commit  EVERY scene fires with post = 0 and a pool that holds a clip per scene: the record that copies `pre` + 1 snapshots of
          every scene into the pool (the worst case; one record per measurement, the recorder is reset in between)
One line per shape and a JSON line at the end.

    python scripts/bench_clips.py [--scenes 256 16384] [--agents 40] [--pre 24] [--post 8] [--iters 20] [--batch 10]
"""
import numpy as np

from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(pre=24, post=8).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_clips needs a GPU"
    from copo_amd.clips import ClipRecorder
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        quiet = torch.zeros(E, sim.N, dtype=torch.uint8, device="cuda")
        fire = torch.full((E, sim.N), 0x08, dtype=torch.uint8, device="cuda")
        for _ in range(30):
            sim.step(act)
        # ---- idle ----
        rec = ClipRecorder(sim, pre=a.pre, post=a.post, max_clips=256, flags=("crash",))
        for _ in range(a.pre + a.post + 1):
            rec.record(flags=quiet)
        torch.cuda.synchronize()
        rec_us, rec_min = timed(torch, lambda: rec.record(flags=quiet), a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, _ = timed(torch, lambda: rec.record(flags=sim.step(act)["flags"]), a.iters, a.batch)
        stored, dropped = rec.count()
        rec.close()
        # ---- commit: every scene, pre + 1 snapshots each ----
        rec = ClipRecorder(sim, pre=a.pre, post=0, max_clips=E, flags=("crash",))
        times = []
        for _ in range(a.iters):
            rec.reset()
            for _ in range(a.pre):
                rec.record(flags=quiet)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rec.record(flags=fire)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3)
        assert rec.count() == (E, 0)
        commit_us, commit_min = float(np.median(times)), float(min(times))
        moved_mb = 2 * 24 * E * sim.N * (a.pre + 1) / 1e6
        rec.close()
        print("%6d scenes x %d slots: record %.1f us (min %.1f), step %.1f us (min %.1f), step + record %.1f us, record / step = %.3f "
              "(%d clips, %d dropped on the way); record with every scene committing %d snapshots %.1f us (min %.1f, %.0f MB moved)"
              % (E, sim.N, rec_us, rec_min, step_us, step_min, both_us, rec_us / step_us, stored, dropped, a.pre + 1, commit_us, commit_min, moved_mb))
        rows.append(dict(scenes=E, slots=sim.N, pre=a.pre, post=a.post, record_us=round(rec_us, 2), step_us=round(step_us, 2),
                         step_plus_record_us=round(both_us, 2), record_over_step=round(rec_us / step_us, 3),
                         commit_all_us=round(commit_us, 2), commit_moved_mb=round(moved_mb, 1)))
        sim.close()
    emit("clip_record_us", rows)


if __name__ == "__main__":
    main()
