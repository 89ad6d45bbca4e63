"""What the observer benchmarks (`bench_interact`, `bench_clips`, `bench_rewind`, `bench_fields`, `bench_gates`, `bench_trips`, `bench_conflicts`, `bench_pet`) share:
the timing loop, the command line, the scene they measure on and the JSON line they end with; `bench_faults`, `bench_adversary`, `bench_pgd`, `bench_certify` and
`bench_jury` and `bench_influence` also take the graph-replay timer from here."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, iters, batch):
    """median, min microseconds per call over `iters` batches of `batch` back-to-back calls"""
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(batch):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / batch)
    return float(np.median(times)), float(min(times))


def replayed(torch, fn, iters, batch):
    """median microseconds per call of `batch` calls captured into one graph and replayed: the cost inside the sampler's captured
    fragment, without the host's share of issuing each launch"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batch):
            fn()
    return timed(torch, g.replay, iters, 1)[0] / batch


def base_parser(**extra):
    """--scenes --agents --iters --batch, then one `--name` per keyword of the type of its default"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--agents", type=int, default=40)
    for name, default in extra.items():
        ap.add_argument("--" + name, type=type(default), default=default)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    return ap


def driven_sim(torch, E, agents):
    """(an Intersection `VecSim` of `E` scenes after `reset()`, the random action tensor [E, N, 2] that drives it)"""
    from copo_amd.sim import SimConfig, VecSim
    sim = VecSim(SimConfig(map="intersection", num_envs=E, num_agents=agents))
    rng = np.random.RandomState(0)
    act = np.zeros((E, sim.N, 2), np.float32)
    act[..., 0] = rng.uniform(-0.3, 0.3, act.shape[:2])
    act[..., 1] = rng.uniform(0.0, 1.0, act.shape[:2])
    act = torch.from_numpy(act).cuda()
    sim.reset()
    return sim, act


def emit(metric, rows):
    print(json.dumps(dict(metric=metric, rows=rows)))
