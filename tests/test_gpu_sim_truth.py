"""The HIP simulator against the float64 model of the scene (sim_truth_numpy.py) on the crafted scenes of sim_truth_cases.py, in three
launch shapes.  The model is the only reference here: the comparison with the CPU oracle is the parity suite's."""
import numpy as np
import pytest

import sim_truth_cases as tc
import sim_truth_numpy as truth

pytestmark = pytest.mark.gpu

SHAPES = (64, 1024, -8)


def _hip_step(name, block):
    import torch
    from copo_amd.sim import VecSim
    case = tc.get_case(name)
    g = VecSim(case.cfg)
    try:
        g.set_block(block)          # (every case is one that the packed shape takes: an error fails the test)
        g.reset()
        st, env = g.get_state()
        st, env = case.state(st.cpu().numpy(), env.cpu().numpy())
        g.set_state(torch.from_numpy(st).cuda(), torch.from_numpy(env).cuda())
        out = g.step(torch.from_numpy(tc.brake_actions(case.cfg)).cuda())
        return case, st, out["obs"].cpu().numpy(), out["flags"].cpu().numpy(), out["info"].cpu().numpy()
    finally:
        g.close()


@pytest.mark.parametrize("block", SHAPES)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_hip_against_the_float64_model(name, block):
    """One reset, one set_state, one step per case and launch shape; the same assertions as test_sim_truth_cpu.py makes of the oracle:
    decisions beyond 1 mm of their threshold, heading column within 3e-7, stable beams and the side / lane columns within 1e-3 m."""
    case, st, obs, flags, info = _hip_step(name, block)
    T = tc.case_truth(name, st)
    stats = tc.check_against_model(case, T, obs, flags, info)
    print(name, block, {k: v for k, v in stats.items() if not isinstance(v, np.ndarray)})
    crafted = T["acted"].copy()
    crafted[:, case.keeper] = False
    if name.startswith("collisions"):
        assert stats["crash_sure"][crafted].all()
    if name.startswith("projection"):
        assert stats["out_known"][crafted].all()
    if name.startswith("projection") or name == "headings":
        assert stats["located"][crafted].all()


@pytest.mark.parametrize("block", SHAPES)
def test_lidar_beams_are_numbered_clockwise(block):
    """One target 30 degrees to the RIGHT of the heading is seen by the clockwise beams, by index."""
    case, st, obs, flags, _ = _hip_step("lidar-intersection", block)
    c0 = truth.obs_columns(case.cfg)["lidar"]
    row = obs[tc.HANDED_SCENE, 0, c0:c0 + 72]
    seen = set(np.nonzero(row < 1.0)[0].tolist())
    assert 6 in seen and seen <= set(range(2, 11)), seen
    assert (row[72 - 10:] == 1.0).all()
