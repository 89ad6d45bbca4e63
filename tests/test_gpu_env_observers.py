"""The env drives its observers through `copo_amd.observers.ObserverList`: with every key on, what they hold is bit for bit what the same
observers hold when they are created directly over a second simulator and driven by the sequence written out below -- the env's code from
before the list existed, frozen here as the specification (order: renderer, meter, clips, rewind, fields, gates, trips; a reset by hand
means clear / reset / flush / invalidate / nothing / forget / nothing)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILM = (64, 64)


def _keys():
    return dict(interaction_metrics=True, event_clips=dict(pre=2, post=1, max_clips=16, flags=("maxstep",), ttc_below=1.0),
                rewind=dict(depth=3, stride=2), field_maps=dict(cell=2.0, ttc_below=1.5), traffic_gates=dict(inset=30.0),
                trip_log=dict(max_rows=256))


class _ByHand:
    """The seven observers over `sim`, created as the env creates them from `_keys()` and recorded as the env recorded them."""

    def __init__(self, sim):
        from copo_amd.clips import ClipRecorder
        from copo_amd.fields import FieldMaps
        from copo_amd.gates import TrafficGates
        from copo_amd.interact import InteractionMeter
        from copo_amd.rewind import RewindBuffer
        from copo_amd.trips import TripLog
        self.sim, self.renderer, self.clips_records = sim, None, 0
        self.meter = InteractionMeter(sim)
        self.clips = ClipRecorder(sim, pre=2, post=1, max_clips=16, flags=("maxstep",), ttc_below=1.0)
        self.rewind = RewindBuffer(sim, depth=3, stride=2)
        self.fields = FieldMaps.for_map(sim, cell=2.0, ttc_below=1.5)
        self.gates = TrafficGates.for_map(sim, inset=30.0)
        self.trips = TripLog(sim, max_rows=256)

    def first_render(self):
        from copo_amd.render import MAX_TRAIL, TopDownRenderer
        self.renderer = TopDownRenderer(self.sim, FILM[0], FILM[1], trail=MAX_TRAIL)
        self.renderer.record()

    def frame(self):
        from copo_amd.render import to_numpy_rgb
        return to_numpy_rgb(self.renderer.frames(scenes=[0], view="map", trail=24))[0]

    def after_reset(self):
        m = self.meter
        if self.renderer is not None:
            self.renderer.clear()
            self.renderer.record()
        m.reset()
        m.record()
        if self.clips_records:
            self.clips.flush()
        self.clips.record(flags=None, ttc=m.ttc, gap=None)             # ttc_below > 0, gap_below == 0
        self.clips_records += 1
        if self.rewind.n_records:
            self.rewind.invalidate()
        self.rewind.record()
        assert self.rewind.n_records == self.clips_records
        self.fields.record(flags=None, ttc=m.ttc)
        self.gates.forget()
        self.gates.record()
        self.trips.record(flags=None, rew=None, gap=m.gap, ttc=m.ttc)

    def after_step(self, out):
        m = self.meter
        if self.renderer is not None:
            self.renderer.record()
        m.record()
        self.clips.record(flags=out["flags"], ttc=m.ttc, gap=None)
        self.clips_records += 1
        self.rewind.record()
        assert self.rewind.n_records == self.clips_records
        self.fields.record(flags=out["flags"], ttc=m.ttc)
        self.gates.record()
        self.trips.record(flags=out["flags"], rew=out["rew"], gap=m.gap, ttc=m.ttc)

    def close(self):
        for o in (self.renderer, self.meter, self.clips, self.rewind, self.fields, self.gates, self.trips):
            if o is not None:
                o.close()


def test_vector_env_matches_the_sequence_by_hand():
    import torch
    from copo_amd.sim import VecSim
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    from copo_amd.trips import KIND_DONE
    env = MultiAgentIntersectionEnv(dict(num_envs=2, num_agents=8, horizon=12, delay_done=2, **_keys()))
    sim = VecSim(env.sim_config)
    hand = _ByHand(sim)
    try:
        assert env.observers.names() == ["interaction_metrics", "event_clips", "rewind", "field_maps", "traffic_gates", "trip_log"]
        g = torch.Generator().manual_seed(7)
        act = torch.rand(2, env.sim.N, 2, generator=g)
        act[..., 0] = act[..., 0] * 0.6 - 0.3
        act = act.cuda().contiguous()
        for seeds, steps, render in ((np.array([21, 22], np.uint64), 18, True), (np.array([905, 33], np.uint64), 12, False)):
            env.vec_reset(seeds)
            sim.reset(seeds)
            hand.after_reset()
            if render:                                             # the renderer joins after the first reset, on both sides
                env.render(film_size=FILM)
                hand.first_render()
                assert env.observers.names()[0] == "renderer"
            for _ in range(steps):
                mine = env.vec_step(act)
                out = sim.step(act)
                assert torch.equal(mine["flags"], out["flags"])   # (the premise: two simulators in step)
                hand.after_step(out)
        m = env.observer("interaction_metrics")
        assert torch.equal(m.gap.view(torch.int32), hand.meter.gap.view(torch.int32))
        assert torch.equal(m.ttc.view(torch.int32), hand.meter.ttc.view(torch.int32))
        np.testing.assert_equal(env.interaction_summary(True), hand.meter.summary(True))
        assert np.array_equal(env.render(film_size=FILM), hand.frame())
        hand.clips.flush()
        a, b = env.event_clips(flush=True), hand.clips.clips()
        assert len(b) >= 1                                         # premise: horizon 12 ends every agent that drives 12 steps with MAXSTEP
        assert np.array_equal(a.header, b.header) and np.array_equal(a.snaps, b.snaps) and np.array_equal(a.envw, b.envw)
        assert env.rewind_buffer().n_records == hand.rewind.n_records == 32 and env.observers.records == 32
        assert env.rewind_buffer().span() == hand.rewind.span() and hand.rewind.span() is not None
        np.testing.assert_equal(env.field_maps().read(), hand.fields.read())
        np.testing.assert_equal(env.traffic_gates().read(), hand.gates.read())
        assert env.trip_log().count() == hand.trips.count()
        rows = hand.trips.rows()
        assert torch.equal(env.trip_log().rows(), rows)
        assert (hand.trips.table().kind == KIND_DONE).sum() >= 1   # premise, as above
    finally:
        hand.close()
        sim.close()
        env.close()


def test_dict_env_info_renderer_first_accessors_close():
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    env = MultiAgentIntersectionEnv(dict(num_envs=1, num_agents=8, horizon=12, delay_done=2, **_keys()))
    plain = MultiAgentIntersectionEnv(dict(num_envs=1, num_agents=8))
    try:
        o = env.reset()
        seen, resets = 0, 1
        for t in range(15):
            if t == 5:
                frame = env.render(film_size=FILM)
                assert frame.shape == (64, 64, 3) and env.observers.names()[0] == "renderer"
            o, r, d, info = env.step({a: np.array([0.0, 0.6], np.float32) for a in o})
            meter = env.observer("interaction_metrics")
            gap, ttc = meter.gap[0].cpu().numpy(), meter.ttc[0].cpu().numpy()
            for a, i in info.items():
                if not i:                                          # (a respawned agent's first step)
                    continue
                if d[a]:
                    assert i["min_gap"] == np.inf and i["ttc"] == np.inf
                elif not d["__all__"]:
                    s = env.vehicles[a].slot
                    assert i["min_gap"] == float(gap[s]) and i["ttc"] == float(ttc[s])
                    seen += 1
            if d["__all__"]:
                o = env.reset()
                resets += 1
        assert seen >= 8 and resets == 2                           # horizon 12: one episode ends within the 15 steps
        assert env.observers.names() == ["renderer", "interaction_metrics", "event_clips", "rewind", "field_maps", "traffic_gates", "trip_log"]
        assert env.rewind_buffer().n_records == env.observers.records == env.trip_log().n_records == resets + 15
        for call, text in ((plain.interaction_summary, "set interaction_metrics=True in the env config"),
                           (plain.event_clips, "set event_clips={...} in the env config"),
                           (plain.rewind_buffer, "set rewind={...} in the env config"),
                           (plain.field_maps, "set field_maps={...} in the env config"),
                           (plain.traffic_gates, "set traffic_gates={...} in the env config"),
                           (plain.trip_log, "set trip_log={...} in the env config")):
            with pytest.raises(AssertionError) as e:
                call()
            assert str(e.value) == text
        assert plain.observers.names() == [] and plain.observer("trip_log") is None
    finally:
        plain.close()
        env.close()
    assert all(env.observer(k) is None for k in env.observers.names() + ["renderer"] + list(_keys()))
    env.close()                                                    # harmless
    assert env.observers.names() == []
