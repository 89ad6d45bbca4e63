"""The launches of the influence pass next to what surrounds them: Intersection, 256 and 16 384 scenes x 40 slots on the `SeatPlan.pairs`
layout of K bank members (default 2 and 16), `--max-others` variants per ego, after `--drive` env steps of traffic.

  obs          `copo_influence_obs`: the counterfactual rows of one step, one launch.  Yardstick: the simulator step on the same scenes
               (the launch redoes one of the step's phases, for the egos only)
  lists        `copo_influence_lists`
  forward_cf   `copo_jury_obs_seats_f32` on the variant lists.  Yardstick: the seat forward times the candidates per seated row
  tally        `copo_influence_tally`
  heading      `copo_influence_heading`
  forward      the seat forward of the drive on the same plan
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_influence.py [--scenes 256 16384] [--agents 40] [--members 2 16] [--max-others 4] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed


def main():
    ap = base_parser(runs=2, drive=40)
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    ap.add_argument("--max-others", type=int, default=4)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_influence needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import influence as I
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    rows = []
    for E in a.scenes:
        for K in a.members:
            if E % (K * K):
                raise SystemExit("bench_influence: %d scenes are not a multiple of the %d pairs of %d members" % (E, K * K, K))
            seats = SeatPlan.pairs(K, E // (K * K), a.agents, 0.5)
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                smp = I.InfluenceSeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, 2, use_graph=False, max_others=a.max_others)
                for _ in range(max(a.drive // 2, 1)):
                    smp.sample()                                # traffic, real observations, actions and flags in the buffers
                torch.cuda.synchronize()
                b, pb, bank, lib, capi = smp.influence, smp.seated.buffers, smp.seated.bank, sim._capi.lib, sim._capi
                EN, O = E * sim.N, smp.O
                obs, eps = smp.obs[2].view(EN, O), smp.eps[1].view(EN, 2)
                I._obs_launch(sim, pb.seat, b, obs)             # the lists of the state the simulator is in
                torch.cuda.synchronize()
                kept = (b.ncand & 0xffff).double()
                egos = float((b.ego != 0).sum())
                cand_per_ego = float(kept.sum()) / max(egos, 1.0)
                cand_per_row = float(kept.sum()) / float(seats.counts.sum())
                sim.flush()
                st = capi.current_stream
                obs_fn = lambda: I._obs_launch(sim, pb.seat, b, obs)  # noqa: E731
                lists_fn = lambda: capi.check(lib.copo_influence_lists(pb.rows.data_ptr(), pb.counts.data_ptr(), b.K, b.cap, b.n_out,  # noqa: E731
                                                                       b.ncand.data_ptr(), b.M, b.vrows.data_ptr(), b.vcounts.data_ptr(), st()))
                cf_fn = lambda: capi.check(lib.copo_jury_obs_seats_f32(C.byref(bank.cfg), bank.theta.data_ptr(), bank.theta_t.data_ptr(), bank.stride,  # noqa: E731
                                                                       bank.K, b.vrows.data_ptr(), b.vcounts.data_ptr(), b.cap * b.M, b.n_out * b.M,
                                                                       b.obs_cf.data_ptr(), b.verdict_cf.data_ptr(), st()))
                tally_fn = lambda: capi.check(lib.copo_influence_tally(b.ego.data_ptr(), smp.dist_inputs[1].data_ptr(), b.verdict_cf.data_ptr(),  # noqa: E731
                                                                       b.who.data_ptr(), b.ncand.data_ptr(), b.hit.data_ptr(), pb.seat.data_ptr(),
                                                                       pb.group.data_ptr(), b.E, b.N, b.K, b.G, b.M, 0.05, 0.05, b.tally.data_ptr(),
                                                                       b.edges.data_ptr(), st()))
                head_fn = lambda: I.influence_heading(sim, b, smp.clipped[1])  # noqa: E731
                fwd_fn = lambda: smp.seated.act(obs, eps, smp.actions[1], smp.logp[1], smp.dist_inputs[1], smp.clipped[1])  # noqa: E731
                step_fn = lambda: capi.check(lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
                # (the step last: it moves the scene on)
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (obs_fn, lists_fn, cf_fn, tally_fn, head_fn, fwd_fn, step_fn)]
                        for _ in range(a.runs)]
            finally:
                t.stop()
            obs_us, lists_us, cf_us, tally_us, head_us, fwd_us, step_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
            row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, max_others=a.max_others, egos=int(egos), candidates_per_ego=round(cand_per_ego, 2),
                       runs=a.runs, graph_obs_us=round(obs_us, 1), graph_lists_us=round(lists_us, 1), graph_forward_cf_us=round(cf_us, 1),
                       graph_tally_us=round(tally_us, 1), graph_heading_us=round(head_us, 1), graph_forward_us=round(fwd_us, 1),
                       graph_step_us=round(step_us, 1), graph_obs_over_step=round(obs_us / step_us, 2),
                       graph_forward_cf_over_forward_x_candidates=round(cf_us / (fwd_us * max(cand_per_row, 1e-9)), 2))
            print("%d scenes x %d slots (O = %d), K = %d, M = %d, %.2f candidates per ego, replayed from a graph: obs %.1f us (%.2f of the step's "
                  "%.1f us), lists %.1f us, forward_cf %.1f us (%.2f of the seat forward's %.1f us x candidates per seated row), tally %.1f us, "
                  "heading %.1f us" % (E, sim.N, O, K, a.max_others, cand_per_ego, obs_us, obs_us / step_us, step_us, lists_us, cf_us,
                                       cf_us / (fwd_us * max(cand_per_row, 1e-9)), fwd_us, tally_us, head_us))
            rows.append(row)
    emit("influence_launches_us", rows)


if __name__ == "__main__":
    main()
