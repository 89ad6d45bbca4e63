"""The HIP simulator against the float64 model of motion, rewards and lifecycle (sim_motion_numpy.py) on the crafted scenes of
sim_motion_cases.py, in three launch shapes.  The model is the only reference here: the comparison with the CPU oracle is the parity
suite's.  Bounds and assertions are those of test_sim_motion_cpu.py (`check_motion`, `check_lifecycle`); the model of a case is evaluated
once and shared by the shapes."""
import numpy as np
import pytest

import sim_motion_cases as mc

pytestmark = pytest.mark.gpu

SHAPES = (64, 1024, -8)


class HipAdapter:
    def __init__(self, cfg, block):
        import torch
        from copo_amd.sim import VecSim
        self.torch = torch
        self.g = VecSim(cfg)
        try:
            self.g.set_block(block)          # (every case is one that the packed shape takes: an error fails the test)
        except Exception:
            self.g.close()
            raise

    def reset(self):
        self.g.reset()

    def get_state(self):
        st, env = self.g.get_state()
        return st.cpu().numpy(), env.cpu().numpy()

    def set_state(self, st, env):
        self.g.set_state(self.torch.from_numpy(np.ascontiguousarray(st)).cuda(), self.torch.from_numpy(np.ascontiguousarray(env)).cuda())

    def set_capacity(self, c):
        self.g.set_capacity(c)

    def step(self, act):
        out = self.g.step(self.torch.from_numpy(np.ascontiguousarray(act, np.float32)).cuda())
        return {k: out[k].cpu().numpy() for k in ("obs", "flags", "info", "rew")}

    def close(self):
        self.g.close()


def _run(name, block, capacity=None):
    case = mc.get_case(name)
    sim = HipAdapter(case.cfg, block)
    try:
        return (case,) + mc.drive(case, sim, capacity)
    finally:
        sim.close()


@pytest.mark.parametrize("block", SHAPES)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_hip_against_the_motion_model(name, block):
    """One reset, one set_state, up to 10 steps per case and launch shape, held to the model after every step; no row is skipped."""
    case, st, env, records = _run(name, block)
    stats = mc.check_motion(case, st, records)
    print(name, block, {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in stats.items()})
    assert stats["skipped"] == 0 and stats["rows"] >= 6


@pytest.mark.parametrize("block", SHAPES)
@pytest.mark.parametrize("capacity", [None, 3])
def test_hip_lifecycle_against_the_model(capacity, block):
    """30 steps of four standing scenes: wreck timers, arrival, respawn into eligible places only, drain, reset, the capacity."""
    case, st, env, records = _run(mc.LIFECYCLE, block, capacity)
    stats = mc.check_lifecycle(case, st, env, records, capacity)
    cap = 8 if capacity is None else capacity
    assert stats["skipped"] == 0
    assert stats["spawns"].tolist() == [min(4, cap), 0, 0, 0] and stats["resets"].tolist() == [0, 0, 0, 1]
    assert stats["max_slot"].tolist() == [min(4, cap) - 1, -1, -1, cap - 1]          # no slot at or beyond the capacity is ever filled
    tr = stats["status_trace"]
    assert (tr[:25, 2, 4] == 2).all() and (tr[25:, 2, 4] == 0).all() and (tr[:, 2, 0] == 1).all()
