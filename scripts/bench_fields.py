"""Cost of one field-map record next to the simulator step it follows: Intersection, 40 slots, 256 and 16 384 scenes, 1 m cells over
the map, one group.

Timed with device events after warm-up on populated scenes (30 steps of random driving first), medians of `--iters` batches of `--batch`
back-to-back calls, fed with the step's own flags:
  record   the record that accumulates (tile bits cleared, events + last-seen pass, tile pass) and the one that does not (events only)
  step     the step alone, and step + record at stride 1 and stride 4
One line per shape and a JSON line at the end.

    python scripts/bench_fields.py [--scenes 256 16384] [--agents 40] [--cell 1.0] [--iters 20] [--batch 10]
"""
from _bench_common import base_parser, driven_sim, emit, timed


def main():
    a = base_parser(cell=1.0).parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_fields needs a GPU"
    from copo_amd.fields import FieldMaps
    rows = []
    for E in a.scenes:
        sim, act = driven_sim(torch, E, a.agents)
        for _ in range(30):
            out = sim.step(act)
        flags = out["flags"]
        every, fourth, never = (FieldMaps.for_map(sim, cell=a.cell, stride=s) for s in (1, 4, 1 << 30))
        never.record(flags=flags)                  # (record 0 accumulates whatever the stride: the events-only record starts after it)
        for fm in (every, fourth):
            for _ in range(4):
                fm.record(flags=flags)
        torch.cuda.synchronize()
        acc_us, acc_min = timed(torch, lambda: every.record(flags=flags), a.iters, a.batch)
        ev_us, ev_min = timed(torch, lambda: never.record(flags=flags), a.iters, a.batch)
        step_us, step_min = timed(torch, lambda: sim.step(act), a.iters, a.batch)
        both1_us, _ = timed(torch, lambda: every.record(flags=sim.step(act)["flags"]), a.iters, a.batch)
        both4_us, _ = timed(torch, lambda: fourth.record(flags=sim.step(act)["flags"]), a.iters, a.batch)
        m, r = every.maps()
        visits, events = int(m[0, 2].sum()), int(m[0, 6:9].sum())
        print("%6d scenes x %d slots, %d x %d cells of %g m: record %.1f us (min %.1f), events-only record %.1f us (min %.1f), step %.1f us (min %.1f), "
              "step + record %.1f us at stride 1 and %.1f us at stride 4, record / step = %.3f (%d visits and %d events in %d scene-records)"
              % (E, sim.N, every.W, every.H, a.cell, acc_us, acc_min, ev_us, ev_min, step_us, step_min, both1_us, both4_us, acc_us / step_us, visits, events,
                 int(r[0])))
        rows.append(dict(scenes=E, slots=sim.N, W=every.W, H=every.H, cell=a.cell, record_us=round(acc_us, 2), events_only_us=round(ev_us, 2),
                         step_us=round(step_us, 2), step_plus_record_stride1_us=round(both1_us, 2), step_plus_record_stride4_us=round(both4_us, 2),
                         record_over_step=round(acc_us / step_us, 3)))
        for fm in (every, fourth, never):
            fm.close()
        sim.close()
    emit("field_record_us", rows)


if __name__ == "__main__":
    main()
