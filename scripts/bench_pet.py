"""Cost of one encroachment-log record next to the simulator step it follows and to the conflict log's record: Intersection, 40 slots, 256
and 16 384 scenes, a grid of `--cell` metres over the map.

Timed with device events after warm-up on populated scenes (30 steps of random driving first), medians of `--iters` batches of `--batch`
back-to-back calls, all in one run:
  record     the encroachment record alone (four launches; the state stands still, so every body rests on its own stamps)
  conflicts  the conflict log's record on the same scenes
  step       the step alone, and step + record
One line per shape and a JSON line at the end.

    python scripts/bench_pet.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10] [--cell 1.0] [--window 50]
"""
from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(cell=1.0, window=50).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pet needs a GPU"
    from copo_amd.conflicts import ConflictLog
    from copo_amd.encroach import EncroachmentLog
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        log = EncroachmentLog.for_map(sim, cell=a.cell, window=a.window, max_rows=1 << 20)
        conf = ConflictLog(sim, max_rows=1 << 20)
        log.record()
        conf.record()
        for _ in range(30):
            out = sim.step(act)
            log.record()
            conf.record(out["flags"])
        torch.cuda.synchronize()
        flags = out["flags"].clone()
        flags &= 0x01                                         # (the state stands still: an end would be booked again in every call)

        def both():
            sim.step(act)
            log.record()
        rec_us, rec_min = timed(torch, log.record, a.iters, a.batch)
        conf_us, conf_min = timed(torch, lambda: conf.record(flags), a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, both_min = timed(torch, both, a.iters, a.batch)
        n_rows, dropped = log.count()
        print("%6d scenes x %d slots, %d x %d cells: record %.1f us (min %.1f), conflict record %.1f us (min %.1f), step %.1f us (min %.1f), "
              "step + record %.1f us (min %.1f), record / step = %.3f (%d rows, %d dropped in %d records, %.1f MB of state)"
              % (E, sim.N, log.W, log.H, rec_us, rec_min, conf_us, conf_min, step_us, step_min, both_us, both_min, rec_us / step_us, n_rows, dropped,
                 log.n_records, log.state_bytes / 1e6))
        rows.append(dict(scenes=E, slots=sim.N, W=log.W, H=log.H, record_us=round(rec_us, 2), conflict_record_us=round(conf_us, 2), step_us=round(step_us, 2),
                         step_plus_record_us=round(both_us, 2), record_over_step=round(rec_us / step_us, 3), rows=n_rows, dropped=dropped,
                         records=log.n_records, state_bytes=log.state_bytes))
        log.close()
        conf.close()
        sim.close()
    emit("pet_record_us", rows)


if __name__ == "__main__":
    main()
