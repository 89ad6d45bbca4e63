"""The two fault kernels next to what they surround: Intersection, 256 and 16 384 scenes x 40 slots, one member, four scene groups at
the identity, a mild, and (two of them) a harsh level: a quarter of the rows is copied, a quarter gets noise, half get everything.

  fault_obs    `copo_fault_obs` of one step's observation [E N][O] -> obs_seen; with it the share of the HBM streaming rate for the
               2 E N O 4 bytes it moves at the least (`--hbm-tbs`, default 6.3: what a float4 copy reaches on an MI355X; the table
               reads are not counted)
  fault_act    `copo_fault_act` on one step's clipped actions, with the previous step's flags
  forward      the seat forward (`copo_mlp_forward_seats_f32`) on obs_seen
  step         the simulator step
Device events, medians of `--iters` batches of `--batch` calls, issued one by one (which at 256 scenes measures the host issuing the
launches as much as the kernels) and, for the two fault kernels and the step, replayed from one captured graph of `--batch` calls, as
the sampler runs them.  One JSON line at the end.

    python scripts/bench_faults.py [--scenes 256 16384] [--agents 40] [--iters 20] [--batch 10] [--hbm-tbs 6.3]
"""
import ctypes as C

import numpy as np

from _bench_common import base_parser, emit, replayed, timed


def main():
    ap = base_parser()
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_faults needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval import faults as F
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan
    levels = [F.FaultLevel(), F.FaultLevel(lidar_sigma=0.02, act_sigma=0.05),
              F.FaultLevel(lidar_sigma=0.1, lidar_dropout=0.1, dropout_value=1.0, act_sigma=0.2, sticky=0.25)]
    rows = []
    for E in a.scenes:
        t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, train_batch_size=2 * E)
        try:
            sim = t.env.sim
            seats = SeatPlan(np.zeros((E, sim.N), np.int32), n_members=1, group=np.arange(E) % 4, n_groups=4)
            faults = F.FaultPlan(levels, [[0], [1], [2], [2]])
            sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
            bank = PolicyBank(t.policy, [sd])
            smp = F.FaultySeatSampler(t.env, t.policy, bank, seats, faults, 2, use_graph=False)
            smp.sample()                                # real observations, actions and flags in the buffers
            EN, O = E * sim.N, smp.O
            pb, fb = smp.seated.buffers, smp.fault_buffers
            sim.flush()
            obs_us, _ = timed(torch, lambda: F.fault_obs(smp.obs[1], smp.obs_seen[1], smp.col_lo, smp.col_hi, pb, fb, smp.tick, 1), a.iters, a.batch)
            act = smp.clipped[1].clone()
            act_us, _ = timed(torch, lambda: F.fault_act(act, smp.prev, smp.flags[0], pb, fb, smp.tick, 1), a.iters, a.batch)
            fwd_us, _ = timed(torch, lambda: smp.seated.act(smp.obs_seen[1].view(EN, O), smp.eps[1].view(EN, 2), smp.actions[1], smp.logp[1],
                                                            smp.dist_inputs[1], smp.clipped[1]), a.iters, a.batch)
            step_us, _ = timed(torch, lambda: sim.step(smp.clipped[1]), a.iters, a.batch)
            obs_fn = lambda: F.fault_obs(smp.obs[1], smp.obs_seen[1], smp.col_lo, smp.col_hi, pb, fb, smp.tick, 1)  # noqa: E731
            act_fn = lambda: F.fault_act(act, smp.prev, smp.flags[0], pb, fb, smp.tick, 1)  # noqa: E731
            step_fn = lambda: sim._capi.check(sim._capi.lib.copo_sim_step(sim._h, smp.clipped[1].data_ptr(), C.byref(smp._outs[1]), sim._stream()))  # noqa: E731
            g_obs, g_act, g_step = (replayed(torch, fn, a.iters, a.batch) for fn in (obs_fn, act_fn, step_fn))
        finally:
            t.stop()
        moved = 2.0 * EN * O * 4
        share = moved / (obs_us * 1e-6) / (a.hbm_tbs * 1e12)
        row = dict(scenes=E, slots=sim.N, obs_dim=O, fault_obs_us=round(obs_us, 1), fault_act_us=round(act_us, 1), forward_us=round(fwd_us, 1),
                   step_us=round(step_us, 1), faults_over_step=round((obs_us + act_us) / step_us, 2), obs_mbytes=round(moved / 1e6, 2),
                   obs_hbm_share=round(share, 3), hbm_tbs=a.hbm_tbs, graph_fault_obs_us=round(g_obs, 1), graph_fault_act_us=round(g_act, 1),
                   graph_step_us=round(g_step, 1), graph_faults_over_step=round((g_obs + g_act) / g_step, 2))
        print("%d scenes x %d slots (O = %d): fault_obs %.1f us (%.2f MB, %.1f %% of %.1f TB/s), fault_act %.1f us, both %.2f of a step of %.1f us; "
              "seat forward %.1f us; replayed from a graph: fault_obs %.1f us, fault_act %.1f us, step %.1f us (%.2f of it)" % (
                  E, sim.N, O, obs_us, moved / 1e6, 100 * share, a.hbm_tbs, act_us, (obs_us + act_us) / step_us, step_us, fwd_us, g_obs, g_act,
                  g_step, (g_obs + g_act) / g_step))
        rows.append(row)
    emit("fault_kernels_over_step", rows)


if __name__ == "__main__":
    main()
