"""A checkpoint sweep as one bank against the same checkpoints one after the other: Intersection, 40 slots, K = 16 members (IPPO layout,
random weights), at 16 and at 64 scenes per member, one whole scene episode each at a `--horizon` of 200 steps.

  batched      `evaluate_bank_rows`: K members x S scenes in one simulator batch, one captured rollout, one recorder
  sequential   K calls of `evaluate_population_rows(recorder="device")` at S scenes, each of which builds its own trainer;
               `construct` is what one such trainer costs to build and stop, so K x construct of the sequential figure is not evaluation
Wall-clock seconds of the whole calls (they end in a host read), then per fragment of 25 steps the median over `--iters` fragments of the
batched and of one sequential rollout (sample + recorder + the episode-counter read), and the batched fragment split into its forward,
step and recorder launches (device events, medians of `--iters` batches of `--batch` calls).  One JSON line at the end.

    python scripts/bench_sweep.py [--members 16] [--scenes 16 64] [--agents 40] [--horizon 200] [--iters 20] [--batch 10]
"""
import time

import numpy as np

from _bench_common import base_parser, emit, timed


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _fragment_us(torch, smp, rec, iters):
    def one():
        rec.add(smp.sample())
        return int(rec.episodes().min())
    for _ in range(3):
        one()
    return float(np.median([_wall(torch, one)[0] for _ in range(iters)])) * 1e6


def main():
    ap = base_parser(members=16, horizon=200)
    ap.set_defaults(scenes=[16, 64])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_sweep needs a GPU"
    from copo_amd.eval import evaluate as EV
    from copo_amd.eval.bank import BankSampler, PolicyBank
    from copo_amd.eval.device_recorder import DeviceRecorder
    K = a.members
    kw = dict(num_agents=a.agents, scene_episodes=1, seed=0)
    env_config = dict(horizon=a.horizon, neighbours_distance=20.0)
    rows = []
    for S in a.scenes:
        E = K * S
        build_s, t = _wall(torch, lambda: EV.make_eval_trainer("ippo", "inter", S, a.agents, 0, None, env_config=dict(env_config)))
        sd = {k: v.detach().cpu().numpy() for k, v in t.policy.model.state_dict().items() if "value" not in k}
        rng = np.random.RandomState(0)
        weights = [{k: (v + rng.normal(0, 0.05, v.shape)).astype(np.float32) for k, v in sd.items()} for _ in range(K)]
        rec = DeviceRecorder(S, t.sampler.N, t.sampler.device, max_rows=1 << 16)
        single_us = _fragment_us(torch, t.sampler, rec, a.iters)
        rec.close()
        stop_s, _ = _wall(torch, t.stop)
        seq_s, _ = _wall(torch, lambda: [EV.evaluate_population_rows("ippo", "inter", w, None, S, recorder="device",
                                                                      env_config=dict(horizon=a.horizon), **kw) for w in weights])
        bat_s, df = _wall(torch, lambda: EV.evaluate_bank_rows("ippo", "inter", weights, num_envs=E, env_config=dict(horizon=a.horizon), **kw))
        assert len(df) == E
        # the batched fragment and its three parts
        t = EV.make_eval_trainer("ippo", "inter", E, a.agents, 0, None, env_config=dict(env_config))
        bank = PolicyBank(t.policy, weights)
        smp = BankSampler(t.env, t.policy, bank, t.sampler.T)
        rec = DeviceRecorder(E, smp.N, smp.device, max_rows=1 << 16)
        bank_us = _fragment_us(torch, smp, rec, a.iters)
        b = smp.sample()
        EN = E * smp.N
        fwd_us, _ = timed(torch, lambda: bank.act(smp.obs[0].view(EN, smp.O), smp.eps[0].view(EN, 2), smp.actions[0], smp.logp[0],
                                                  smp.dist_inputs[0], smp.clipped[0]), a.iters, a.batch)
        step_us, _ = timed(torch, lambda: t.env.sim.step(smp.clipped[0]), a.iters, a.batch)
        rec_us, _ = timed(torch, lambda: rec.add(b), a.iters, a.batch)
        rec.close()
        t.stop()
        row = dict(members=K, scenes_per_member=S, slots=smp.N, horizon=a.horizon, batched_s=round(bat_s, 3), sequential_s=round(seq_s, 3),
                   construct_s=round(build_s + stop_s, 3), sequential_over_batched=round(seq_s / bat_s, 2),
                   fragment_batched_us=round(bank_us, 1), fragment_single_us=round(single_us, 1),
                   fragments_sequential_over_batched=round(K * single_us / bank_us, 2),
                   forward_us=round(fwd_us, 1), step_us=round(step_us, 1), recorder_add_us=round(rec_us, 1), steps_per_fragment=smp.T)
        print("K = %d x %d scenes: batched %.2f s, sequential %.2f s (%.2f s of it per trainer built and stopped), ratio %.2f; fragment of %d "
              "steps: batched %.0f us, one member alone %.0f us (x K / batched = %.2f); forward %.1f us, step %.1f us, recorder add %.1f us"
              % (K, S, bat_s, seq_s, build_s + stop_s, seq_s / bat_s, smp.T, bank_us, single_us, K * single_us / bank_us, fwd_us, step_us, rec_us))
        rows.append(row)
    emit("sweep_sequential_over_batched", rows)


if __name__ == "__main__":
    main()
