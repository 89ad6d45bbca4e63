"""The seat forward of cross-play against its alternatives, and the seat tally next to the simulator step: Intersection, 256 scenes x 40
slots, K = 2, 4, 16 members (IPPO layout, random weights), every slot seated, the members scattered evenly over the slots.

  seats        `copo_mlp_forward_seats_f32`: one launch, grid ceil(cap / 16) x K
  rows_x_K     K launches of `copo_mlp_forward_rows_f32` (policy net) with the same per-member row lists: what a caller without the seat
               mode would do for the hidden layers (it writes values only, no sampling)
  dense_bank   `copo_mlp_forward_bank_f32` over the same number of rows, scenes [k E / K, (k + 1) E / K) to member k
  tally, step  `copo_seat_tally` of one step's flags and rewards, and the simulator step it follows
Device events, medians of `--iters` batches of `--batch` calls.  One JSON line at the end.

    python scripts/bench_crossplay.py [--scenes 256] [--agents 40] [--members 2 4 16] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, timed


def main():
    ap = base_parser()
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 16])
    ap.set_defaults(scenes=[256])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_crossplay needs a GPU"
    from copo_amd import _capi
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan, seat_tally
    rows = []
    for E in a.scenes:
        t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None)
        smp, sim = t.sampler, t.env.sim
        smp.sample()
        EN, N = E * smp.N, smp.N
        sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
        rng = np.random.RandomState(0)
        obs, eps = smp.obs[0].view(EN, smp.O), smp.eps[0].view(EN, 2)
        step_us, _ = timed(torch, lambda: sim.step(smp.clipped[0]), a.iters, a.batch)
        for K in a.members:
            bank = PolicyBank(t.policy, [{k: (v + rng.normal(0, 0.05, v.shape)).astype(np.float32) for k, v in sd.items()} for _ in range(K)])
            bank.sync_mirror()
            plan = SeatPlan(rng.permutation(EN).reshape(E, N) % K, n_members=K, group=np.arange(E) % 4, n_groups=4)
            pb = PlanBuffers(plan, smp.device)
            out = (smp.actions[0], smp.logp[0], smp.dist_inputs[0], smp.clipped[0])
            seats_us, _ = timed(torch, lambda: bank.act_seats(pb, obs, eps, *out), a.iters, a.batch)
            values = torch.zeros(1, EN, device=smp.device)
            st = _capi.current_stream()

            def k_launches():
                for k in range(K):
                    _capi.check(_capi.lib.copo_mlp_forward_rows_f32(C.byref(bank.cfg), bank.theta[k].data_ptr(), bank.theta_t[k].data_ptr(),
                                                                    obs.data_ptr(), None, pb.rows[k].data_ptr(), int(plan.counts[k]), EN, 0, 1,
                                                                    values.data_ptr(), st))
            rows_us, _ = timed(torch, k_launches, a.iters, a.batch)
            dense_us = float("nan")
            if EN % K == 0:
                dense_us, _ = timed(torch, lambda: bank.act(obs, eps, *out), a.iters, a.batch)
            tally = torch.zeros(plan.n_groups, K, 8, dtype=torch.int64, device=smp.device)
            tally_us, _ = timed(torch, lambda: seat_tally(smp.flags[0], smp.rew3[0, 0], pb, tally), a.iters, a.batch)
            row = dict(scenes=E, slots=N, members=K, cap=plan.cap, seats_us=round(seats_us, 1), rows_x_K_us=round(rows_us, 1),
                       dense_bank_us=round(dense_us, 1), rows_x_K_over_seats=round(rows_us / seats_us, 2), tally_us=round(tally_us, 1),
                       step_us=round(step_us, 1))
            print("%d scenes x %d slots, K = %d (cap %d): seats %.1f us, K row-list launches %.1f us (x %.2f), dense bank %.1f us; tally %.1f us "
                  "next to a step of %.1f us" % (E, N, K, plan.cap, seats_us, rows_us, rows_us / seats_us, dense_us, tally_us, step_us))
            rows.append(row)
        t.stop()
    emit("crossplay_rows_x_K_over_seats", rows)


if __name__ == "__main__":
    main()
