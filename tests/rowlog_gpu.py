"""What the GPU tests of the trip log and the conflict log share (tests/test_gpu_trips.py, tests/test_gpu_conflicts.py): the simulator's
state to and from numpy, a log's rows and count, the simulator of the hand sequences and what their `run_hand` clears and flushes."""
import numpy as np

from copo_amd.sim import SimConfig


def _np_state(sim):
    st, env = sim.get_state()
    return st.cpu().numpy(), env.cpu().numpy()


def _set_state(sim, st, env):
    import torch
    sim.set_state(torch.from_numpy(np.ascontiguousarray(st)).cuda(), torch.from_numpy(np.ascontiguousarray(env)).cuda())


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _read(log):
    return log.rows().cpu().numpy().view(np.uint32), log.count()


def _sim64(E, N):
    from copo_amd.sim import VecSim
    kw = dict(map="intersection", num_envs=E, num_agents=N)
    return VecSim(SimConfig(map_kwargs=dict(exit_length=80.0), **kw) if N == 64 else SimConfig(**kw))


class Both:
    """`clear` and `flush` of the device's log and of the restatement next to it"""

    def __init__(self, *logs):
        self.logs = logs

    def clear(self):
        for log in self.logs:
            log.clear()

    def flush(self):
        for log in self.logs:
            log.flush()
