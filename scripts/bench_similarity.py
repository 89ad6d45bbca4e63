"""The three launches of representation similarity (eval/similarity.py) next to their yardsticks: Intersection, 256 scenes x 40 slots on
the `SeatPlan.pairs` layout of K bank members (default 2, 4 and 16), every member on the panel, hidden 256.

  hidden       `copo_hidden_obs_seats_f32`: one step's observation [E N][O] -> hidden [K][cap][2][H], one launch
  jury         `copo_jury_obs_seats_f32` on the same lists.  Yardstick of `hidden`: a ratio near 1 -- the same forward, the heads left
               out and the two tiles stored
  gram         `copo_cka_accumulate` of the step: its time, and its 4 P H^2 n FLOP (P pairs, both layers, n counted rows) as a fraction
               of the fp32 MFMA peak (157.3 TFLOP/s).  Yardstick: the 47 % the README states for the weight-gradient GEMM
  finish       `copo_cka_finish`
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_similarity.py [--scenes 256] [--agents 40] [--members 2 4 16] [--runs 2] [--iters 20] [--batch 10]
"""
import numpy as np

from _bench_common import base_parser, emit, replayed

PEAK_FP32_MFMA = 157.3e12


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_similarity needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import similarity as S
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    rows = []
    for E in a.scenes:
        for K in a.members:
            if E % (K * K):
                raise SystemExit("bench_similarity: %d scenes are not a multiple of the %d pairs of %d members" % (E, K * K, K))
            seats = SeatPlan.pairs(K, E // (K * K), a.agents, 0.5)
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                plan = S.SimilarityPlan(seats, max_bytes=8 << 30)
                smp = S.SimilaritySeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, plan, 2, use_graph=False)
                smp.sample()                                # real observations, activations and flags in the buffers
                EN, O, jb, acc = E * sim.N, smp.O, smp.jury_buffers, smp.acc
                H = acc.H
                obs = smp.obs[1].view(EN, O)
                verdict = torch.zeros(EN, K, 4, device=smp.device)
                n = int(np.count_nonzero((smp.flags[1].cpu().numpy().reshape(-1)[plan.rows[:plan.count]] & 1) != 0))
                sim.flush()
                hidden_fn = lambda: smp.seated.hidden_seats(jb, obs, smp.hidden)  # noqa: E731
                jury_fn = lambda: smp.seated.jury_seats(jb, obs, verdict)  # noqa: E731
                gram_fn = lambda: S.cka_accumulate(smp.hidden, smp.panel, smp._rows, smp._count, smp.flags[1].view(-1),  # noqa: E731
                                                   smp.seated.buffers.seat.view(-1), plan.rows_of, acc.S, acc.s, acc.n)
                finish_fn = lambda: S.cka_finish(acc.S, acc.s, acc.n, acc.hsic, acc.n_out, acc.mean, acc.var)  # noqa: E731
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (hidden_fn, jury_fn, gram_fn, finish_fn)] for _ in range(a.runs)]
            finally:
                t.stop()
            hidden_us, jury_us, gram_us, finish_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
            flop = 4.0 * plan.P * H * H * n
            share = flop / (gram_us * 1e-6) / PEAK_FP32_MFMA
            row = dict(scenes=E, slots=sim.N, obs_dim=O, hidden=H, members=K, pairs=plan.P, cap=int(plan.cap), counted_rows=n, planes=acc.R, runs=a.runs,
                       accumulator_mib=round(plan.accumulator_bytes(H) / 2 ** 20, 1), graph_hidden_us=round(hidden_us, 1), graph_jury_us=round(jury_us, 1),
                       graph_hidden_over_jury=round(hidden_us / jury_us, 2), graph_gram_us=round(gram_us, 1), gram_gflop=round(flop / 1e9, 2),
                       gram_share_of_fp32_mfma_peak=round(share, 3), graph_finish_us=round(finish_us, 1))
            print("%d scenes x %d slots (O = %d, hidden %d), K = %d (%d pairs, %d planes, %d counted rows), replayed from a graph: hidden %.1f us (%.2f of "
                  "the jury's %.1f us), gram %.1f us (%.2f GFLOP: %.1f %% of the fp32 MFMA peak), finish %.1f us" % (
                      E, sim.N, O, H, K, plan.P, acc.R, n, hidden_us, hidden_us / jury_us, jury_us, gram_us, flop / 1e9, 100.0 * share, finish_us))
            rows.append(row)
    emit("similarity_launches", rows)


if __name__ == "__main__":
    main()
