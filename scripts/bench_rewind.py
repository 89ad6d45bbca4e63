"""Cost of one rewind record and of a fork next to the simulator step: Intersection, 40 slots, 256 and 16 384 scenes, depth 8.

Per shape, timed with device events after warm-up on populated scenes (30 steps of random driving first): a STORED record (stride 1:
every record is one), the step alone, step + record with stride 1 and with stride 4 (three records of four launch nothing), and a fork
of `--branches` target scenes from random scenes and stored records.  One line per shape and a JSON line at the end.

    python scripts/bench_rewind.py [--scenes 256 16384] [--agents 40] [--depth 8] [--branches 1024] [--iters 20] [--batch 10]
"""
import numpy as np

from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(depth=8, branches=1024).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_rewind needs a GPU"
    from copo_amd import _capi
    from copo_amd.rewind import Branches, RewindBuffer
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
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
        rng = np.random.RandomState(0)
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
    emit("rewind_record_us", rows)


if __name__ == "__main__":
    main()
