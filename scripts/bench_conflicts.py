"""Cost of one conflict-log record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes, fed with the
step's flags.

Timed with device events after warm-up on populated scenes (30 steps of random driving first), medians of `--iters` batches of `--batch`
back-to-back calls:
  record   the record alone (three launches; the state stands still, so nothing closes or opens: every open pair accumulates)
  step     the step alone, and step + record
One line per shape and a JSON line at the end.

    python scripts/bench_conflicts.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10] [--radius 8] [--leave_radius 10]
"""
from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(radius=8.0, leave_radius=10.0).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_conflicts needs a GPU"
    from copo_amd.conflicts import ConflictLog
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        log = ConflictLog(sim, max_rows=1 << 20, radius=a.radius, leave_radius=a.leave_radius)
        log.record()
        for _ in range(30):
            out = sim.step(act)
            log.record(out["flags"])
        torch.cuda.synchronize()
        flags = out["flags"].clone()
        flags &= 0x01                                         # (the state stands still: an end would be booked again in every call)

        def both():
            log.record(sim.step(act)["flags"])
        rec_us, rec_min = timed(torch, lambda: log.record(flags), a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, both_min = timed(torch, both, a.iters, a.batch)
        n_rows, dropped = log.count()
        print("%6d scenes x %d slots: record %.1f us (min %.1f), step %.1f us (min %.1f), step + record %.1f us (min %.1f), record / step = %.3f "
              "(%d rows, %d dropped in %d records, %.1f MB of state)"
              % (E, sim.N, rec_us, rec_min, step_us, step_min, both_us, both_min, rec_us / step_us, n_rows, dropped, log.n_records, log.state_bytes / 1e6))
        rows.append(dict(scenes=E, slots=sim.N, record_us=round(rec_us, 2), step_us=round(step_us, 2), step_plus_record_us=round(both_us, 2),
                         record_over_step=round(rec_us / step_us, 3), rows=n_rows, dropped=dropped, records=log.n_records, state_bytes=log.state_bytes))
        log.close()
        sim.close()
    emit("conflict_record_us", rows)


if __name__ == "__main__":
    main()
