"""Cost of folding one sampler fragment into the evaluation table: `VecRecorder.add` (a Python loop over the steps, about 45 framework
kernels and two host stops per step) next to `DeviceRecorder.add` (three launches per fragment, no host stop) on the SAME fragments:
Intersection, 40 slots, 64 and 1 024 scenes, `--steps` steps per fragment, recorded from random driving with a short horizon so that
agents terminate and scene episodes end inside the fragments.

Both are timed with device events around `--batch` back-to-back calls, medians of `--iters` batches after one warm-up call;
`VecRecorder.add` stops the host inside every step, so its figure is host and device time together, which is what the evaluation loop
pays.  One line per shape and a JSON line at the end.

    python scripts/bench_recorder.py [--scenes 64 1024] [--agents 40] [--steps 25] [--iters 10] [--batch 4]
"""
import numpy as np

from _bench_common import base_parser, emit, timed


def fragments(torch, sim, act, steps, count):
    """`count` fragments of `steps` steps each in the sampler's layout (dicts of [T, E, N] tensors)"""
    out = []
    for _ in range(count):
        rows = dict(flags=[], infos=[], rewards=[], nei_rewards=[], nbr_cnt=[])
        for _ in range(steps):
            o = sim.step(act)
            for key, src in (("flags", "flags"), ("infos", "info"), ("rewards", "rew"), ("nei_rewards", "nei_rew"), ("nbr_cnt", "nbr_cnt")):
                rows[key].append(o[src].clone())
        out.append({k: torch.stack(v).contiguous() for k, v in rows.items()})
    return out


def main():
    ap = base_parser(steps=25, horizon=60)
    ap.set_defaults(scenes=[64, 1024], iters=10, batch=4)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_recorder needs a GPU"
    from copo_amd.eval.device_recorder import DeviceRecorder
    from copo_amd.eval.vec_recorder import VecRecorder
    from copo_amd.sim import SimConfig, VecSim
    rows = []
    for E in a.scenes:
        sim = VecSim(SimConfig(map="intersection", num_envs=E, num_agents=a.agents, horizon=a.horizon))
        rng = np.random.RandomState(0)
        act = np.stack([rng.uniform(-0.3, 0.3, (E, sim.N)), rng.uniform(0.0, 1.0, (E, sim.N))], -1).astype(np.float32)
        act = torch.from_numpy(act).cuda()
        sim.reset()
        frags = fragments(torch, sim, act, a.steps, 4)
        vec, dev = VecRecorder(E, sim.device), DeviceRecorder(E, sim.N, sim.device, max_rows=1 << 16)
        state = dict(k=0)

        def feed(rec):
            rec.add(frags[state["k"] % len(frags)])
            state["k"] += 1
        feed(vec)
        feed(dev)
        torch.cuda.synchronize()
        vec_us, vec_min = timed(torch, lambda: feed(vec), a.iters, a.batch)
        dev_us, dev_min = timed(torch, lambda: feed(dev), a.iters, a.batch)
        n_rows, dropped = dev.count()
        print("%6d scenes x %d slots, fragments of %d steps: VecRecorder.add %.1f us (min %.1f), DeviceRecorder.add %.1f us (min %.1f), "
              "ratio %.1f (%d rows, %d dropped; VecRecorder %d rows)"
              % (E, sim.N, a.steps, vec_us, vec_min, dev_us, dev_min, vec_us / dev_us, n_rows, dropped, len(vec.rows)))
        rows.append(dict(scenes=E, slots=sim.N, steps=a.steps, vec_add_us=round(vec_us, 1), device_add_us=round(dev_us, 2),
                         ratio=round(vec_us / dev_us, 1), rows=n_rows, dropped=dropped))
        dev.close()
        sim.close()
    emit("recorder_add_us", rows)


if __name__ == "__main__":
    main()
