"""Lifetime of the library's handles on the GPU (copo_amd/_handle.py, copo_amd/csrc/capi_common.h): every observer of a simulator is
created, used, reset and closed twice; closed AFTER its simulator, which only the destroy call may be; and a create that the device
refuses leaves no error behind for the next launch.  What the observers compute is pinned by their own tests."""
import ctypes as C

import pytest

import sim_config_cases as scc

pytestmark = pytest.mark.gpu

E, N = 2, 12


def _renderer(sim):
    from copo_amd.render import TopDownRenderer
    return TopDownRenderer(sim, 16, 16, trail=2)


def _meter(sim):
    from copo_amd.interact import InteractionMeter
    return InteractionMeter(sim)


def _clips(sim):
    from copo_amd.clips import ClipRecorder
    return ClipRecorder(sim, pre=1, post=1, max_clips=2)


def _rewind(sim):
    from copo_amd.rewind import RewindBuffer
    return RewindBuffer(sim, depth=2, stride=1)


def _fields(sim):
    from copo_amd.fields import FieldMaps
    return FieldMaps(sim, -20.0, -20.0, 8, 8, cell=5.0, groups=1)


def _gates(sim):
    from copo_amd.gates import TrafficGates
    return TrafficGates(sim, [[0.0, -5.0, 0.0, 5.0]])


def _trips(sim):
    from copo_amd.trips import TripLog
    return TripLog(sim, max_rows=8)


OBSERVERS = [_renderer, _meter, _clips, _rewind, _fields, _gates, _trips]


def _sim():
    from copo_amd.sim import VecSim
    sim = VecSim(scc.sim_config("intersection", E, N))
    sim.reset()
    return sim


@pytest.mark.parametrize("make", OBSERVERS)
def test_lifecycle(make):
    sim = _sim()
    try:
        obs = make(sim)
        assert obs._h.value and obs.sim is sim
        obs.record()
        obs.clear() if make is _renderer else obs.reset()
        obs.close()
        assert not obs._h.value
        obs.close()                                    # a no-op
        assert not obs._h.value
    finally:
        sim.close()
    sim.close()
    assert not sim._h.value


@pytest.mark.parametrize("make", OBSERVERS)
def test_observer_closed_after_its_simulator(make):
    import torch
    sim = _sim()
    obs = make(sim)
    obs.record()
    torch.cuda.synchronize()
    sim.close()
    obs.close()                                        # reads the handle alone, not the simulator that is gone
    assert not obs._h.value
    sim = _sim()
    try:
        obs = make(sim)
        obs.record()
        torch.cuda.synchronize()
        if make in (_fields, _gates):                  # the one record: every scene once, in group 0
            assert int(obs.read()["scene_records"][0]) == E
        if make is _trips:                             # the one record: counted, and no trip has ended in it
            assert obs.n_records == 1 and obs.count() == (0, 0)
        obs.close()
    finally:
        sim.close()


def test_refused_create_leaves_no_sticky_error():
    """A clip pool of 66 TB is refused by its size alone (COPO_ERR_DEVICE); the next launch on the same stream must not report it.  (The
    renderer refuses every size beyond its limit before it allocates, and the meter's buffers follow the simulator's size, so the clip
    pool is the request that can be refused here; all seven handle types allocate through the same owner.)"""
    import torch
    from copo_amd import _capi
    lib = _capi.lib
    sim = _sim()
    try:
        h = C.c_void_p()
        big = _capi.ClipCfg(200, 55, 2 ** 31 - 1, 8, 0.0, 0.0)
        assert lib.copo_clip_create(sim._h, C.byref(big), C.byref(h)) == -3 and not h.value
        assert lib.copo_last_error().startswith(b"copo_clip_create")
        act = torch.zeros(E, N, 2, device="cuda")
        assert lib.copo_sim_step(sim._h, act.data_ptr(), C.byref(sim._step_out), sim._stream()) == 0
        torch.cuda.synchronize()
    finally:
        sim.close()
