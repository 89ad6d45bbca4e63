"""The low-precision seat forwards next to the fp32 seat forward on the same row lists: Intersection, 256 scenes x 40 slots, K = 2 and 16
members (IPPO layout, hidden 256, random weights), every slot seated, the members scattered evenly over the slots.

  fp32         `copo_mlp_forward_seats_f32`: the yardstick (this study does not touch it)
  bf16, e4m3   `copo_lowp_forward_seats` in either format on the same lists: one launch, grid ceil(cap / 16) x K
  pack         `copo_lowp_pack` of the K members in either format (outside the rollout: once per bank)
  step         the simulator step the forwards sit next to
Replayed from a graph of `--batch` calls (the cost inside a captured fragment), medians of `--iters` replays.  One JSON line at the end.

    python scripts/bench_lowp.py [--scenes 256] [--agents 40] [--members 2 16] [--iters 20] [--batch 10]
"""
import numpy as np

from _bench_common import base_parser, emit, replayed, timed


def main():
    ap = base_parser()
    ap.add_argument("--members", type=int, nargs="+", default=[2, 16])
    ap.set_defaults(scenes=[256])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_lowp needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    from copo_amd.eval.precision import LowpBank
    rows = []
    for E in a.scenes:
        t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None)
        smp, sim = t.sampler, t.env.sim
        smp.sample()
        EN, N = E * smp.N, smp.N
        sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
        rng = np.random.RandomState(0)
        obs, eps = smp.obs[0].view(EN, smp.O), smp.eps[0].view(EN, 2)
        out = (smp.actions[0], smp.logp[0], smp.dist_inputs[0], smp.clipped[0])
        step_us, _ = timed(torch, lambda: sim.step(smp.clipped[0]), a.iters, a.batch)
        for K in a.members:
            bank = PolicyBank(t.policy, [{k: (v + rng.normal(0, 0.05, v.shape)).astype(np.float32) for k, v in sd.items()} for _ in range(K)])
            bank.sync_mirror()
            plan = SeatPlan(rng.permutation(EN).reshape(E, N) % K, n_members=K)
            pb = PlanBuffers(plan, smp.device)
            low = {fmt: LowpBank(bank, fmt) for fmt in ("bfloat16", "float8_e4m3")}
            us = dict(fp32=replayed(torch, lambda: bank.act_seats(pb, obs, eps, *out), a.iters, a.batch))
            for name, fmt in (("bf16", "bfloat16"), ("e4m3", "float8_e4m3")):
                us[name] = replayed(torch, lambda lb=low[fmt]: lb.act_seats(pb, obs, eps, *out), a.iters, a.batch)
                us["pack_" + name], _ = timed(torch, low[fmt].pack, a.iters, a.batch)
            row = dict(scenes=E, slots=N, members=K, cap=plan.cap, hidden=int(bank.cfg.hidden), step_us=round(step_us, 1),
                       **{k + "_us": round(v, 1) for k, v in us.items()}, bf16_over_fp32=round(us["bf16"] / us["fp32"], 2),
                       e4m3_over_fp32=round(us["e4m3"] / us["fp32"], 2))
            print("%d scenes x %d slots, K = %d (cap %d): fp32 seats %.1f us, bf16 %.1f us (x %.2f), e4m3 %.1f us (x %.2f); pack %.1f / %.1f us; "
                  "a step %.1f us" % (E, N, K, plan.cap, us["fp32"], us["bf16"], us["bf16"] / us["fp32"], us["e4m3"], us["e4m3"] / us["fp32"],
                                      us["pack_bf16"], us["pack_e4m3"], step_us))
            rows.append(row)
        t.stop()
    emit("lowp_over_fp32_seat_forward", rows)


if __name__ == "__main__":
    main()
