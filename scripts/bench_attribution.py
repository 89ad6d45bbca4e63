"""The integrated-gradients launch next to what surrounds it: Intersection, 256 scenes x 40 slots, hidden 256, a bank of K members
(default 2 and 16) whose seats alternate over the rows, four scene groups -- one at the identity, three at a level (clear road, zeros,
clear road) -- so three quarters of the rows are attributed and a quarter gets zeros.

  ig M         `copo_ig_obs_seats_f32` with every level at `points` = M (4, 8, 16): obs [E N][O] -> attr, heads
  adversary    `copo_adv_obs_seats_f32`, the one-step kernel, with `grad` on the same lists (three quarters of the rows)
  pgd M        `copo_pgd_obs_seats_f32` at `iters` = M on the same lists
  forward      the seat forward (`copo_mlp_forward_seats_f32`) on the same row lists
  fold         `copo_attrib_tally`: a step's attr, heads and flags into words [G][K][8] and cols [G][K][2][O]
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  The yardstick is 2 M x the
one-step kernel's time in the same call: two heads, each with one backward pass per point.  One JSON line at the end.

    python scripts/bench_attribution.py [--scenes 256] [--agents 40] [--members 2 16] [--runs 2] [--iters 20] [--batch 10]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed

POINTS = (4, 8, 16)


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_attribution needs a GPU"
    from copo_amd.eval import adversary as A
    from copo_amd.eval import attribution as X
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import pgd as P
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    one_step = [A.AdversaryLevel(), A.AdversaryLevel(0.0, 0.0, 1.0), A.AdversaryLevel(0.0, 1.0, 0.0), A.AdversaryLevel(0.0, -1.0, -1.0)]

    def ig_levels(m):
        return [X.AttributionLevel(), X.AttributionLevel(m, "clear_road"), X.AttributionLevel(m, "zeros"), X.AttributionLevel(m, "clear_road")]

    def pgd_levels(n):
        return [P.PGDLevel(), P.PGDLevel(0.05, 0.0, 1.0, 0.05 / n, n), P.PGDLevel(0.1, 1.0, 0.0, 0.1 / n, n), P.PGDLevel(0.1, -1.0, -1.0, 0.1 / n, n)]
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
                smp = X.AttributionSeatSampler(t.env, t.policy, bank, seats, X.AttributionPlan(ig_levels(POINTS[-1]), level_of), 2, use_graph=False)
                smp.sample()                                # real observations, actions and flags in the buffers
                EN, O = E * sim.N, smp.O
                sim.flush()
                obs, attr, heads = smp.obs[1].view(EN, O), smp.attr[1].view(EN, 2, O), smp.heads[1].view(EN, 8)
                seen, grad = torch.zeros(EN, O, device=smp.device), torch.zeros(EN, O, device=smp.device)
                ig = {m: X.AttributionBuffers(X.AttributionPlan(ig_levels(m), level_of).resolve(sim.cfg, O), smp.device) for m in POINTS}
                pg = {m: P.PGDBuffers(P.PGDPlan(pgd_levels(m), level_of), smp.device) for m in POINTS}
                adv = A.AdversaryBuffers(A.AdversaryPlan(one_step, level_of), smp.device)
                fns = [lambda b=ig[m]: smp.seated.attribute_seats(b, obs, attr, heads) for m in POINTS]
                fns += [lambda b=pg[m]: smp.seated.pgd_seats(b, obs, seen, smp.col_lo, smp.col_hi, 0, None) for m in POINTS]
                fns.append(lambda: smp.seated.perturb_seats(adv, obs, seen, smp.col_lo, smp.col_hi, grad))
                fns.append(lambda: smp.seated.act(obs, smp.eps[1].view(EN, 2), smp.actions[1], smp.logp[1], smp.dist_inputs[1], smp.clipped[1]))
                fns.append(lambda: X.attrib_tally(smp.flags[1], smp.attr[1], smp.heads[1], smp.seated.buffers, smp.attrib_words, smp.attrib_cols))
                fns.append(lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream())))
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in fns] for _ in range(a.runs)]
            finally:
                t.stop()
            med = [float(v) for v in np.median(np.asarray(runs), axis=0)]
            n = len(POINTS)
            ig_us, pgd_us, (adv_us, fwd_us, fold_us, step_us) = med[:n], med[n:2 * n], med[2 * n:]
            row = dict(scenes=E, slots=sim.N, obs_dim=O, hidden=int(bank.cfg.hidden), members=K, cap=int(seats.cap), runs=a.runs,
                       graph_adversary_grad_us=round(adv_us, 1), graph_forward_us=round(fwd_us, 1), graph_fold_us=round(fold_us, 1),
                       graph_step_us=round(step_us, 1))
            for m, us, pus in zip(POINTS, ig_us, pgd_us):
                row["graph_ig%d_us" % m], row["graph_pgd%d_us" % m] = round(us, 1), round(pus, 1)
                row["ig%d_over_2m_x_adversary" % m] = round(us / (2 * m * adv_us), 2)
            print("%d scenes x %d slots (O = %d), K = %d, replayed from a graph: ig %s us at points %s (%s of 2 m x the one-step kernel's %.1f us), "
                  "pgd at iters = m %s us, seat forward %.1f us, fold %.1f us, step %.1f us" % (
                      E, sim.N, O, K, " / ".join("%.1f" % u for u in ig_us), " / ".join(map(str, POINTS)),
                      " / ".join("%.2f" % (u / (2 * m * adv_us)) for m, u in zip(POINTS, ig_us)), adv_us, " / ".join("%.1f" % u for u in pgd_us),
                      fwd_us, fold_us, step_us))
            rows.append(row)
    emit("ig_over_2m_x_adversary", rows)


if __name__ == "__main__":
    main()
