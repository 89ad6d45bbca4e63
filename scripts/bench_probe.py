"""The launches of the linear probes (eval/probes.py) next to their yardstick: Intersection, 256 scenes x 40 slots on the `SeatPlan.pairs`
layout of K bank members (default 2, 4 and 16), every member on the panel, hidden 256, the scenes alternating between the two folds.

  targets      `copo_probe_targets`: one step's observation, flags and reward -> targets [cap][16] and xobs [cap][Op], one launch
  gram_hidden  `copo_probe_accumulate` on the 2 M hidden blocks: its time, and its 2 folds x 2 M x (nt (nt + 1) / 2 + 1) x 64 x 64 x 2 n FLOP
               (every workgroup walks all n counted rows of the step; a row is zero in the fold it does not belong to) as a fraction of
               the fp32 MFMA peak (157.3 TFLOP/s)
  cka          `copo_cka_accumulate` on the same workspace and panel.  Yardstick of `gram_hidden`: this time scaled by the ratio of the
               workgroup counts, 2 x 2 M x (nt (nt + 1) / 2 + 1) against P x 2 x nt^2
  gram_obs     `copo_probe_accumulate` on the observation block (B = 1, D = Op)
  fit          one host read of the accumulators and `probe_fit` of both sets, host clock
Device events, medians of `--iters` batches of `--batch` calls replayed from one captured graph of `--batch` calls, as the sampler runs
them.  The whole measurement is taken `--runs` times (default 2); the medians over the runs are reported.  One JSON line at the end.

    python scripts/bench_probe.py [--scenes 256] [--agents 40] [--members 2 4 16] [--runs 2] [--iters 20] [--batch 10]
"""
import time

import numpy as np

from _bench_common import base_parser, emit, replayed

PEAK_FP32_MFMA = 157.3e12


def main():
    ap = base_parser(runs=2)
    ap.set_defaults(scenes=[256])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_probe needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import probes as P
    from copo_amd.eval import similarity as S
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    rows = []
    for E in a.scenes:
        for K in a.members:
            if E % (K * K):
                raise SystemExit("bench_probe: %d scenes are not a multiple of the %d pairs of %d members" % (E, K * K, K))
            seats = SeatPlan.pairs(K, E // (K * K), a.agents, 0.5)
            t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
            try:
                sim = t.env.sim
                sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
                plan = P.ProbePlan(seats, folds=np.arange(E) % 2, max_bytes=8 << 30)
                cka = S.SimilarityPlan(seats, max_bytes=8 << 30)
                smp = P.ProbeSeatSampler(t.env, t.policy, PolicyBank(t.policy, [sd] * K), seats, plan, 2, use_graph=False)
                smp.sample()                                # real observations, activations, targets and flags in the buffers
                EN, O, acc = E * sim.N, smp.O, smp.acc
                H, Op = acc.hidden.D, acc.obs.D
                sacc = S.SimilarityAccumulators(cka.M, H, cka.planes(H), smp.device)
                panel = torch.from_numpy(cka.members.copy()).to(smp.device)
                flags, seat = smp.flags[1].view(-1), smp.seated.buffers.seat.view(-1)
                n = int(np.count_nonzero((flags.cpu().numpy()[plan.rows[:plan.count]] & 1) != 0))
                sim.flush()
                targets_fn = lambda: P.probe_targets(smp.obs[1].view(EN, O), smp.lidar_lo, smp.num_lasers, smp.trig, flags,  # noqa: E731
                                                     smp.rew3[0, 1].view(-1), smp._rows, smp._count, smp.targets, smp.xobs)
                hidden_fn = lambda: P.probe_accumulate(smp.hidden, smp.block_base, 2 * H, H, smp.targets, smp._rows, smp._count, flags, seat,  # noqa: E731
                                                       smp.fold, plan.rows_of, *acc.hidden.tensors())
                cka_fn = lambda: S.cka_accumulate(smp.hidden, panel, smp._rows, smp._count, flags, seat, cka.rows_of, sacc.S, sacc.s, sacc.n)  # noqa: E731
                obs_fn = lambda: P.probe_accumulate(smp.xobs, smp.obs_base, Op, Op, smp.targets, smp._rows, smp._count, flags, seat, smp.fold,  # noqa: E731
                                                    plan.rows_of, *acc.obs.tensors())
                runs = [[replayed(torch, fn, a.iters, a.batch) for fn in (targets_fn, hidden_fn, cka_fn, obs_fn)] for _ in range(a.runs)]
                fits = []
                for _ in range(a.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    smp.read()
                    fits.append((time.perf_counter() - t0) * 1e3)
            finally:
                t.stop()
            targets_us, hidden_us, cka_us, obs_us = (float(v) for v in np.median(np.asarray(runs), axis=0))
            nt = H // P.TILE
            wg_probe, wg_cka = 2 * 2 * plan.M * (nt * (nt + 1) // 2 + 1), cka.P * 2 * nt * nt
            flop = wg_probe * 64.0 * 64.0 * 2.0 * n
            share = flop / (hidden_us * 1e-6) / PEAK_FP32_MFMA
            yardstick_us = cka_us * wg_probe / wg_cka
            row = dict(scenes=E, slots=sim.N, obs_dim=O, obs_width=Op, hidden=H, members=K, cap=int(plan.cap), counted_rows=n, runs=a.runs,
                       planes_hidden=acc.hidden.R, planes_obs=acc.obs.R, planes_cka=sacc.R, workgroups_probe=wg_probe, workgroups_cka=wg_cka,
                       accumulator_mib=round(plan.accumulator_bytes(H, O) / 2 ** 20, 1), graph_targets_us=round(targets_us, 1),
                       graph_gram_hidden_us=round(hidden_us, 1), gram_hidden_gflop=round(flop / 1e9, 2), gram_hidden_share_of_fp32_mfma_peak=round(share, 3),
                       graph_cka_us=round(cka_us, 1), yardstick_us=round(yardstick_us, 1), gram_hidden_over_yardstick=round(hidden_us / yardstick_us, 2),
                       graph_gram_obs_us=round(obs_us, 1), host_fit_ms=round(float(np.median(fits)), 1))
            print("%d scenes x %d slots (O = %d, hidden %d), K = %d (%d counted rows; planes %d / %d, CKA %d), replayed from a graph: targets %.1f us, "
                  "hidden-block gram %.1f us (%.2f GFLOP: %.1f %% of the fp32 MFMA peak; yardstick %.1f us = the CKA launch's %.1f us x %d / %d workgroups: "
                  "%.2f of it), observation-block gram %.1f us; host read and fit %.1f ms" % (
                      E, sim.N, O, H, K, n, acc.hidden.R, acc.obs.R, sacc.R, targets_us, hidden_us, flop / 1e9, 100.0 * share, yardstick_us, cka_us, wg_probe,
                      wg_cka, hidden_us / yardstick_us, obs_us, float(np.median(fits))))
            rows.append(row)
    emit("probe_launches", rows)


if __name__ == "__main__":
    main()
