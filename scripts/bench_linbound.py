"""The linear-bound launch next to what it is made of: Intersection, 256 scenes x 40 slots, a bank of K members (default 2 and 16) whose
seats alternate over the rows, four scene groups -- one at eps = 0, three at a budget -- so every row takes the whole pass (the budget
does not change the work).

  linear       `copo_lin_obs_seats_f32`: one step's observation [E N][O] -> bounds [E N][8] (no `parts`, as the sampler launches it)
  certify      `copo_cert_obs_seats_f32` on the same inputs: the three-tile forward
  adversary    `copo_adv_obs_seats_f32` on the same row lists: a one-tile forward and one backward pass to the input
  forward      the seat forward (`copo_mlp_forward_seats_f32`) on the same row lists
  fold         `copo_certify_tally`: a step's bounds and flags into [G][K][8]
  step         the simulator step
The YARDSTICK is certify + adversary - forward: the interval kernel's forward plus one backward pass, all three measured in this call.
The linear launch runs the same forward, the layer-1 GEMM of two tiles again, and a two-tile backward.
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_linbound.py [--scenes 256] [--agents 40] [--members 2 16] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_linbound needs a GPU"
    from copo_amd.eval import adversary as A
    from copo_amd.eval import certify as Z
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    levels = [Z.CertifyLevel(), Z.CertifyLevel(0.0005, 0.05, 0.05), Z.CertifyLevel(0.002, 0.05, 0.05), Z.CertifyLevel(0.01, 0.05, 0.05)]
    attack = [A.AdversaryLevel(0.05, 0.0, 1.0)] * 4          # every row takes the whole forward + backward pass
    rows = []
    for E in a.scenes:
        for K in a.members:
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                seats = SeatPlan((np.arange(E * sim.N, dtype=np.int32) % K).reshape(E, sim.N), n_members=K, group=np.arange(E) % 4, n_groups=4)
                level_of = np.repeat(np.arange(4, dtype=np.int32)[:, None], K, axis=1)
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                smp = Z.CertifySeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, Z.CertifyPlan(levels, level_of), 2, use_graph=False,
                                           method="linear")
                smp.sample()                                # real observations, actions and flags in the buffers
                EN, O = E * sim.N, smp.O
                adv = A.AdversaryBuffers(A.AdversaryPlan(attack, level_of), smp.device)
                seen, other = torch.zeros(EN, O, device=smp.device), torch.zeros(EN, len(Z.BOUND_WORDS), device=smp.device)
                sim.flush()
                lin_fn = lambda: smp._policy_obs(1)  # noqa: E731
                cert_fn = lambda: smp.seated.certify_seats(smp.cert_buffers, smp.obs[1].view(EN, O), other, smp.col_lo, smp.col_hi, smp.pad)  # noqa: E731
                fold_fn = lambda: Z.certify_tally(smp.flags[1], smp.bounds[1], smp.seated.buffers, smp.cert_buffers, smp.cert_tally)  # noqa: E731
                fwd_fn = lambda: smp.seated.act(smp.obs[1].view(EN, O), smp.eps[1].view(EN, 2), smp.actions[1], smp.logp[1],  # noqa: E731
                                                smp.dist_inputs[1], smp.clipped[1])
                adv_fn = lambda: smp.seated.perturb_seats(adv, smp.obs[1].view(EN, O), seen, smp.col_lo, smp.col_hi)  # noqa: E731
                step_fn = lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (lin_fn, cert_fn, adv_fn, fwd_fn, fold_fn, step_fn)] for _ in range(a.runs)]
            finally:
                t.stop()
            lin_us, cert_us, adv_us, fwd_us, fold_us, step_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
            yard = cert_us + adv_us - fwd_us
            row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, cap=int(seats.cap), runs=a.runs, graph_linear_us=round(lin_us, 1),
                       graph_certify_us=round(cert_us, 1), graph_adversary_us=round(adv_us, 1), graph_forward_us=round(fwd_us, 1),
                       graph_fold_us=round(fold_us, 1), graph_step_us=round(step_us, 1), yardstick_us=round(yard, 1),
                       graph_linear_over_yardstick=round(lin_us / yard, 2), graph_linear_over_certify=round(lin_us / cert_us, 2))
            print("%d scenes x %d slots (O = %d), K = %d, replayed from a graph: linear %.1f us = %.2f of the yardstick's %.1f us (certify %.1f + "
                  "adversary %.1f - forward %.1f), %.2f of certify; fold %.1f us, step %.1f us" % (
                      E, sim.N, O, K, lin_us, lin_us / yard, yard, cert_us, adv_us, fwd_us, lin_us / cert_us, fold_us, step_us))
            rows.append(row)
    emit("linear_over_yardstick", rows)


if __name__ == "__main__":
    main()
