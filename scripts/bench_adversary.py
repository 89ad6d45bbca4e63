"""The adversarial-observation launch next to what surrounds it: Intersection, 256 scenes x 40 slots, a bank of K members (default 2 and
16) whose seats alternate over the rows, four scene groups -- one at the identity, three at an attack level -- so three quarters of the
rows take the whole forward + backward-to-input pass and a quarter is copied.

  adversary    `copo_adv_obs_seats_f32`: one step's observation [E N][O] -> obs_seen, one gradient-sign step on the LiDAR block
  forward      the seat forward (`copo_mlp_forward_seats_f32`) on the same row lists
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls, both issued one by one (which at 256 scenes measures the host issuing
the launches as much as the kernels) and replayed from one captured graph of `--batch` calls, as the sampler runs them.  The whole
measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_adversary.py [--scenes 256] [--agents 40] [--members 2 16] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed, timed


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_adversary needs a GPU"
    from copo_amd.eval import adversary as A
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    levels = [A.AdversaryLevel(), A.AdversaryLevel(0.05, 0.0, 1.0), A.AdversaryLevel(0.1, 1.0, 0.0), A.AdversaryLevel(0.1, -1.0, -1.0)]
    rows = []
    for E in a.scenes:
        for K in a.members:
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                seats = SeatPlan((np.arange(E * sim.N, dtype=np.int32) % K).reshape(E, sim.N), n_members=K, group=np.arange(E) % 4, n_groups=4)
                plan = A.AdversaryPlan(levels, np.repeat(np.arange(4, dtype=np.int32)[:, None], K, axis=1))
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                smp = A.AdversarialSeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, plan, 2, use_graph=False)
                smp.sample()                                # real observations and actions in the buffers
                EN, O = E * sim.N, smp.O
                sim.flush()
                adv_fn = lambda: smp._policy_obs(1)  # noqa: E731
                fwd_fn = lambda: smp.seated.act(smp.obs_seen[1].view(EN, O), smp.eps[1].view(EN, 2), smp.actions[1], smp.logp[1],  # noqa: E731
                                                smp.dist_inputs[1], smp.clipped[1])
                step_fn = lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
                runs = []
                for _ in range(a.runs):
                    eager = [timed(torch, fn, a.iters, a.batch)[0] for fn in (adv_fn, fwd_fn, lambda: sim.step(smp.clipped[1]))]
                    runs.append(eager + [replayed(torch, fn, a.iters, a.batch) for fn in (adv_fn, fwd_fn, step_fn)])
            finally:
                t.stop()
            adv_us, fwd_us, step_us, g_adv, g_fwd, g_step = (float(v) for v in np.median(np.asarray(runs), axis=0))
            row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, cap=int(seats.cap), runs=a.runs, adversary_us=round(adv_us, 1), forward_us=round(fwd_us, 1),
                       step_us=round(step_us, 1), graph_adversary_us=round(g_adv, 1), graph_forward_us=round(g_fwd, 1), graph_step_us=round(g_step, 1),
                       graph_adversary_over_forward=round(g_adv / g_fwd, 2), graph_adversary_over_step=round(g_adv / g_step, 2))
            print("%d scenes x %d slots (O = %d), K = %d: replayed from a graph: adversary %.1f us, seat forward %.1f us (%.2f of it), step %.1f us; "
                  "issued one by one: adversary %.1f us, seat forward %.1f us, step %.1f us" % (
                      E, sim.N, O, K, g_adv, g_fwd, g_adv / g_fwd, g_step, adv_us, fwd_us, step_us))
            rows.append(row)
    emit("adversary_over_forward", rows)


if __name__ == "__main__":
    main()
