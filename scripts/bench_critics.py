"""The value launch and the audit record next to what surrounds them: Intersection (CoPO: three value heads), 256 scenes x 40 slots on the
`SeatPlan.pairs` layout of K bank members (default 2, 4 and 16: K^2 pair groups of 256 / K^2 scenes, half of a scene's seats each).

  values       `copo_value_obs_seats_f32`: one step's observation [E N][O] -> values [E N][heads], one launch for every member and head
  yardstick    K calls of `FusedLearner.values(rows=...)`, call k with member k's list (`copo_mlp_forward_rows_f32`): the same nets, the
               way a single member could already run them (the yardstick, not the code under test; it runs one member's weights K
               times, which costs what K members' weights cost)
  forward      the seat forward of the drive (every row once, the policy net of the member that drives it)
  record       `copo_audit_record`: a step's flags, values and three reward streams into the per-slot state and the accumulator
  seat_tally   `copo_seat_tally` of the same step
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_critics.py [--scenes 256] [--agents 40] [--members 2 4 16] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_critics needs a GPU"
    from copo_amd.eval import critics as CR
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, seat_tally
    rows = []
    for E in a.scenes:
        for K in a.members:
            if E % (K * K):
                raise SystemExit("bench_critics: %d scenes are not a multiple of the %d pairs of %d members" % (E, K * K, K))
            seats = SeatPlan.pairs(K, E // (K * K), a.agents, 0.5)
            t = EV.make_eval_trainer("copo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim, fz = t.env.sim, t.policy.fused
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items()}
                audit = CR.CriticAudit(t.policy.gae_gammas())
                smp = CR.CriticSeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K, values=True), seats, audit, 2, use_graph=False)
                smp.sample()                                # real observations, values, rewards and flags in the buffers
                EN, O, pb = E * sim.N, smp.O, smp.seated.buffers
                obs, eps = smp.obs[1].view(EN, O), smp.eps[1].view(EN, 2)
                lists = [pb.rows[k, :int(seats.counts[k])].contiguous() for k in range(K)]
                scratch = torch.zeros(audit.heads, EN, device=smp.device)
                fz.sync_mirror()
                sim.flush()

                def yard_fn():
                    for k in range(K):
                        fz.values(obs, None, out=scratch, rows=lists[k])

                value_fn = lambda: smp._policy_obs(1)  # noqa: E731
                fwd_fn = lambda: smp.seated.act(obs, eps, smp.actions[1], smp.logp[1], smp.dist_inputs[1], smp.clipped[1])  # noqa: E731
                record_fn = lambda: smp.fold.record(smp.flags[1], smp.values[1], smp.rew3[0, 1], smp.rew3[1, 1], smp.glob[1], pb.seat, pb.group)  # noqa: E731
                tally_fn = lambda: seat_tally(smp.flags[1], smp.rew3[0, 1], pb, smp.tally)  # noqa: E731
                step_fn = lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (value_fn, yard_fn, fwd_fn, record_fn, tally_fn, step_fn)] for _ in range(a.runs)]
                smp.fold.close()
            finally:
                t.stop()
            value_us, yard_us, fwd_us, record_us, tally_us, step_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
            row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, heads=audit.heads, cap=int(seats.cap), runs=a.runs, graph_values_us=round(value_us, 1),
                       graph_yardstick_us=round(yard_us, 1), graph_forward_us=round(fwd_us, 1), graph_record_us=round(record_us, 1),
                       graph_seat_tally_us=round(tally_us, 1), graph_step_us=round(step_us, 1), graph_values_over_yardstick=round(value_us / yard_us, 2),
                       graph_values_over_forward_x_heads=round(value_us / (fwd_us * audit.heads), 2))
            print("%d scenes x %d slots (O = %d), K = %d, %d heads, replayed from a graph: values %.1f us (%.2f of the yardstick's %.1f us, %.2f of "
                  "the seat forward's %.1f us x heads), record %.1f us (seat tally %.1f us), step %.1f us" % (
                      E, sim.N, O, K, audit.heads, value_us, value_us / yard_us, yard_us, value_us / (fwd_us * audit.heads), fwd_us, record_us, tally_us,
                      step_us))
            rows.append(row)
    emit("values_over_yardstick", rows)


if __name__ == "__main__":
    main()
