"""The iterated adversarial-observation launch next to what surrounds it: Intersection, 256 scenes x 40 slots, a bank of K members
(default 2 and 16) whose seats alternate over the rows, four scene groups -- one at the identity, three at an attack level (targeted,
targeted from a random start, untargeted) -- so three quarters of the rows iterate and a quarter is copied.

  pgd N        `copo_pgd_obs_seats_f32` with every attack level at `iters` = N (1, 2, 4, 8): obs [E N][O] -> obs_seen
  adversary    `copo_adv_obs_seats_f32`, the one-step kernel, on the same lists (three quarters of the rows attacked)
  forward      the seat forward (`copo_mlp_forward_seats_f32`) on the same row lists
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  The yardstick is N x the
one-step kernel's time in the same call: one resident launch gathers, looks up and stores once.  One JSON line at the end.

    python scripts/bench_pgd.py [--scenes 256] [--agents 40] [--members 2 16] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed

ITERS = (1, 2, 4, 8)


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pgd needs a GPU"
    from copo_amd.eval import adversary as A
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import pgd as P
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    one_step = [A.AdversaryLevel(), A.AdversaryLevel(0.05, 0.0, 1.0), A.AdversaryLevel(0.1, 1.0, 0.0), A.AdversaryLevel(0.1, -1.0, -1.0)]

    def levels(n):
        return [P.PGDLevel(), P.PGDLevel(0.05, 0.0, 1.0, 0.05 / n, n), P.PGDLevel(0.1, 1.0, 0.0, 0.1 / n, n, random_start=True),
                P.PGDLevel(0.1, 0.0, 0.0, 0.1 / n, n, random_start=True, untargeted=True)]
    rows = []
    for E in a.scenes:
        for K in a.members:
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                seats = SeatPlan((np.arange(E * sim.N, dtype=np.int32) % K).reshape(E, sim.N), n_members=K, group=np.arange(E) % 4, n_groups=4)
                level_of = np.repeat(np.arange(4, dtype=np.int32)[:, None], K, axis=1)
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                bank = PolicyBank(t.policy, [sd] * K)
                smp = P.PGDSeatSampler(t.env, t.policy, bank, seats, P.PGDPlan(levels(ITERS[-1]), level_of), 2, use_graph=False)
                smp.sample()                                # real observations and actions in the buffers
                EN, O = E * sim.N, smp.O
                sim.flush()
                obs, seen = smp.obs[1].view(EN, O), smp.obs_seen[1].view(EN, O)
                tables = {n: P.PGDBuffers(P.PGDPlan(levels(n), level_of), smp.device) for n in ITERS}
                adv = A.AdversaryBuffers(A.AdversaryPlan(one_step, level_of), smp.device)
                fns = [lambda gb=tables[n]: smp.seated.pgd_seats(gb, obs, seen, smp.col_lo, smp.col_hi, 0, smp.tick) for n in ITERS]
                fns.append(lambda: smp.seated.perturb_seats(adv, obs, seen, smp.col_lo, smp.col_hi))
                fns.append(lambda: smp.seated.act(seen, smp.eps[1].view(EN, 2), smp.actions[1], smp.logp[1], smp.dist_inputs[1], smp.clipped[1]))
                fns.append(lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream())))
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in fns] for _ in range(a.runs)]
            finally:
                t.stop()
            med = [float(v) for v in np.median(np.asarray(runs), axis=0)]
            pgd_us, (adv_us, fwd_us, step_us) = med[:len(ITERS)], med[len(ITERS):]
            row = dict(scenes=E, slots=sim.N, obs_dim=O, members=K, cap=int(seats.cap), runs=a.runs, graph_adversary_us=round(adv_us, 1),
                       graph_forward_us=round(fwd_us, 1), graph_step_us=round(step_us, 1))
            for n, us in zip(ITERS, pgd_us):
                row["graph_pgd%d_us" % n] = round(us, 1)
                row["pgd%d_over_iters_x_adversary" % n] = round(us / (n * adv_us), 2)
            print("%d scenes x %d slots (O = %d), K = %d, replayed from a graph: pgd %s us at iters %s (%s of iters x the one-step kernel's %.1f us), "
                  "seat forward %.1f us, step %.1f us" % (E, sim.N, O, K, " / ".join("%.1f" % u for u in pgd_us), " / ".join(map(str, ITERS)),
                                                           " / ".join("%.2f" % (u / (n * adv_us)) for n, u in zip(ITERS, pgd_us)), adv_us, fwd_us, step_us))
            rows.append(row)
    emit("pgd_over_iters_x_adversary", rows)


if __name__ == "__main__":
    main()
