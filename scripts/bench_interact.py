"""Cost of one interaction-meter record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes.

Both are timed with device events around batches of launches after warm-up, on populated scenes (30 steps of random driving first).
One line per shape and a JSON line at the end.

    python scripts/bench_interact.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10]
"""
from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser().parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_interact needs a GPU"
    from copo_amd.interact import InteractionMeter
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        meter = InteractionMeter(sim)
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
    emit("interact_record_us", rows)


if __name__ == "__main__":
    main()
