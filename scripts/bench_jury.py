"""The jury launch and its fold next to what surrounds them: Intersection, 256 scenes x 40 slots on the `SeatPlan.pairs` layout of K bank
members (default 2, 4 and 16: K^2 pair groups of 256 / K^2 scenes, half of a scene's seats each), judged under the `everyone` plan
(K forwards per row) and the `seated` plan (focal and partner: two per row, one on the self-play groups).

  jury         `copo_jury_obs_seats_f32`: one step's observation [E N][O] -> verdict [E N][K][4], one launch
  yardstick    K launches of `copo_mlp_forward_seats_f32`, launch j with member j alone seated on judge j's list: the same forwards, the
               way the bank could already run them (the yardstick, not the code under test)
  forward      the seat forward of the drive (every row once, by the member that drives it)
  fold         `copo_jury_tally`: a step's flags, dist_inputs and verdicts into [G][K][K][8]
  seat_tally   `copo_seat_tally` of the same step
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_jury.py [--scenes 256] [--agents 40] [--members 2 4 16] [--runs 2] [--iters 20] [--batch 10]
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
    assert torch.cuda.is_available(), "bench_jury needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import jury as J
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, seat_tally
    rows = []
    for E in a.scenes:
        for K in a.members:
            if E % (K * K):
                raise SystemExit("bench_jury: %d scenes are not a multiple of the %d pairs of %d members" % (E, K * K, K))
            seats = SeatPlan.pairs(K, E // (K * K), a.agents, 0.5)
            for kind in J.PLANS:
                t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
                try:
                    sim = t.env.sim
                    sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                    jury = J.JuryPlan.named(seats, kind)
                    smp = J.JurySeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, jury, 2, use_graph=False)
                    smp.sample()                                # real observations, actions and flags in the buffers
                    EN, O, jb = E * sim.N, smp.O, smp.jury_buffers
                    obs, eps = smp.obs[1].view(EN, O), smp.eps[1].view(EN, 2)
                    # launch j of the yardstick: judge j's list, every other member's count zero
                    alone = [SimpleBuffers(jb, torch.where(torch.arange(K, device=smp.device) == j, jb.counts, torch.zeros_like(jb.counts)))
                             for j in range(K)]
                    scratch = dict(action=torch.zeros(EN, 2, device=smp.device), logp=torch.zeros(EN, device=smp.device),
                                   dist_inputs=torch.zeros(EN, 4, device=smp.device))
                    sim.flush()

                    def yard_fn():
                        for j in range(K):
                            smp.seated.bank.act_seats(alone[j], obs, eps, **scratch)

                    jury_fn = lambda: smp._policy_obs(1)  # noqa: E731
                    fwd_fn = lambda: smp.seated.act(obs, eps, smp.actions[1], smp.logp[1], smp.dist_inputs[1], smp.clipped[1])  # noqa: E731
                    fold_fn = lambda: J.jury_tally(smp.flags[1], smp.dist_inputs[1], smp.verdict[1], smp.seated.buffers, jb, smp.deltas,  # noqa: E731
                                                   smp.jury_tally)
                    tally_fn = lambda: seat_tally(smp.flags[1], smp.rew3[0, 1], smp.seated.buffers, smp.tally)  # noqa: E731
                    step_fn = lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
                    runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (jury_fn, yard_fn, fwd_fn, fold_fn, tally_fn, step_fn)] for _ in range(a.runs)]
                finally:
                    t.stop()
                jury_us, yard_us, fwd_us, fold_us, tally_us, step_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
                per_row = float(jury.counts.sum()) / float(seats.counts.sum())          # mean number of judges per seated row
                row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, plan=kind, cap=int(jury.cap), judges_per_row=round(per_row, 2), runs=a.runs,
                           graph_jury_us=round(jury_us, 1), graph_yardstick_us=round(yard_us, 1), graph_forward_us=round(fwd_us, 1),
                           graph_fold_us=round(fold_us, 1), graph_seat_tally_us=round(tally_us, 1), graph_step_us=round(step_us, 1),
                           graph_jury_over_yardstick=round(jury_us / yard_us, 2), graph_jury_over_forward_x_judges=round(jury_us / (fwd_us * per_row), 2))
                print("%d scenes x %d slots (O = %d), K = %d, %s (%.2f judges per row), replayed from a graph: jury %.1f us (%.2f of the yardstick's "
                      "%.1f us, %.2f of the seat forward's %.1f us x judges per row), fold %.1f us (seat tally %.1f us), step %.1f us" % (
                          E, sim.N, O, K, kind, per_row, jury_us, jury_us / yard_us, yard_us, jury_us / (fwd_us * per_row), fwd_us, fold_us, tally_us,
                          step_us))
                rows.append(row)
    emit("jury_over_yardstick", rows)


class SimpleBuffers:
    """A jury plan's lists with other counts, as `PolicyBank.act_seats` reads a plan's buffers."""

    def __init__(self, jb, counts):
        self.K, self.cap, self.n_out, self.rows, self.counts = jb.K, jb.cap, jb.n_out, jb.rows, counts.contiguous()


if __name__ == "__main__":
    main()
