"""Cost of one traffic-gate record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes, `for_map` gates
(8 gates, 16 sections), one group.

Timed with device events after warm-up on populated scenes (30 steps of random driving first), medians of `--iters` batches of `--batch`
back-to-back calls:
  record   the record alone (one launch)
  step     the step alone, and step + record
One line per shape and a JSON line at the end.

    python scripts/bench_gates.py [--scenes 256 16384] [--agents 40] [--inset 10.0] [--iters 20] [--batch 10]
"""
from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(inset=10.0).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_gates needs a GPU"
    from copo_amd.gates import TrafficGates
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        tg = TrafficGates.for_map(sim, inset=a.inset)
        tg.record()
        for _ in range(30):
            sim.step(act)
            tg.record()
        torch.cuda.synchronize()

        def both():
            sim.step(act)
            tg.record()
        rec_us, rec_min = timed(torch, tg.record, a.iters, a.batch)        # (the state stands still: the memory traffic is that of any record)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both_us, both_min = timed(torch, both, a.iters, a.batch)
        d = tg.read()
        crossings, trips, recs = int(d["count"].sum()), int(d["sec_count"].sum()), int(d["scene_records"][0])
        print("%6d scenes x %d slots, %d gates, %d sections: record %.1f us (min %.1f), step %.1f us (min %.1f), step + record %.1f us (min %.1f), "
              "record / step = %.3f (%d crossings and %d trips in %d scene-records)"
              % (E, sim.N, tg.L, tg.S, rec_us, rec_min, step_us, step_min, both_us, both_min, rec_us / step_us, crossings, trips, recs))
        rows.append(dict(scenes=E, slots=sim.N, gates=tg.L, sections=tg.S, record_us=round(rec_us, 2), step_us=round(step_us, 2),
                         step_plus_record_us=round(both_us, 2), record_over_step=round(rec_us / step_us, 3), crossings=crossings,
                         scene_records=recs))
        tg.close()
        sim.close()
    emit("gate_record_us", rows)


if __name__ == "__main__":
    main()
