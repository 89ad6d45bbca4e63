"""Interaction metrics of the simulator's scenes (host side of `copo_interact_*`).

`InteractionMeter` owns one `copo_interact` handle over a `VecSim`.  `record()` measures the current state on the GPU -- per driving
slot the minimum body-to-body gap and the minimum time to collision (TTC) against the other vehicles and wrecks of its scene -- and
updates per-agent accumulators on the device: minimum gap, minimum TTC, steps below the critical TTC (time exposed, TET), the
time-integrated shortfall (TIT), near-miss events and harsh-braking steps.  Agents that left their slot are folded into per-scene
totals; `summary()` reduces those over the scenes.  The definitions are DESIGN.md section 8b; `tests/interact_numpy.py` restates
them in float64.
"""
import ctypes as C

from ._handle import Handle

COUNT_KEYS = ("agents", "steps", "tet_steps", "near_events", "brake_events", "agents_with_finite_ttc")
SUM_KEYS = ("min_gap", "min_ttc", "tit")


def summarise(counts, sums):
    """The summary dict of count rows [..., 6] and sum rows [..., 3] (numpy), reduced over the rows in float64."""
    import numpy as np
    c = np.asarray(counts, np.int64).reshape(-1, len(COUNT_KEYS)).sum(0)
    s = np.asarray(sums, np.float64).reshape(-1, len(SUM_KEYS)).sum(0)
    agents, steps, tet, near, brake, finite = (int(v) for v in c)
    nan = float("nan")
    return dict(
        agents=agents, steps=steps,
        min_gap_mean=float(s[0]) / agents if agents else nan,
        min_ttc_mean=float(s[1]) / finite if finite else nan,
        ttc_finite_frac=finite / agents if agents else nan,
        tet_frac=tet / steps if steps else nan,
        tit_mean=float(s[2]) / agents if agents else nan,
        near_events_per_agent=near / agents if agents else nan,
        brake_events_per_agent=brake / agents if agents else nan)


class InteractionMeter(Handle):
    """Surrogate safety measures of a `VecSim`'s agents: TTC beyond `horizon` seconds counts as none, a step is critical below
    `ttc_crit` seconds, near below that or below `gap_near` metres, harsh braking above `brake` m/s^2.  `close()` it when done
    (before or after its simulator; no other call once the simulator is closed); every call is asynchronous on torch's current
    stream."""

    _prefix = "copo_interact_"

    def __init__(self, sim, horizon=6.0, ttc_crit=1.5, gap_near=0.5, brake=4.0):
        self._attach(sim)
        self.horizon, self.ttc_crit, self.gap_near, self.brake = float(horizon), float(ttc_crit), float(gap_near), float(brake)
        cfg = self._capi.InteractCfg(self.horizon, self.ttc_crit, self.gap_near, self.brake)
        self._create(self._capi.lib.copo_interact_create, sim._h, C.byref(cfg))
        torch = sim._torch
        self.gap = torch.empty(sim.E, sim.N, dtype=torch.float32, device=sim.device)
        self.ttc = torch.empty(sim.E, sim.N, dtype=torch.float32, device=sim.device)

    @classmethod
    def from_env(cls, sim, value):
        """The env's meter (config key `interaction_metrics`: on or off, no arguments)."""
        return cls(sim)

    def env_record(self, feed):
        """One measurement of the state after reset and after every step; a reset empties the accumulators first."""
        if feed.after_reset:
            self.reset()
        self.record()

    def record(self):
        """Measure the current state: (gap, ttc), float32 [E, N] device tensors owned by the meter (overwritten by the next call);
        +inf for a slot that does not drive or has no partner."""
        self._capi.check(self._capi.lib.copo_interact_record(self._h, self.gap.data_ptr(), self.ttc.data_ptr(), self._stream()))
        return self.gap, self.ttc

    def totals(self, flush_open=False):
        """(counts int64 [E, 6], sums float64 [E, 3]) device tensors, columns `COUNT_KEYS` / `SUM_KEYS`, over the agents that have
        left their slot; `flush_open`: also those still driving, as if they ended now (the meter goes on unchanged)."""
        torch = self.sim._torch
        counts = torch.empty(self.sim.E, len(COUNT_KEYS), dtype=torch.int64, device=self.sim.device)
        sums = torch.empty(self.sim.E, len(SUM_KEYS), dtype=torch.float64, device=self.sim.device)
        self._call("totals", counts.data_ptr(), sums.data_ptr(), 1 if flush_open else 0)
        return counts, sums

    def summary(self, flush_open=False):
        """Dict over all scenes: `agents`, `steps`, `min_gap_mean` (m), `min_ttc_mean` (s, over the agents whose minimum TTC is
        finite), `ttc_finite_frac`, `tet_frac` (critical steps per step), `tit_mean` (s^2 per agent), `near_events_per_agent`,
        `brake_events_per_agent`; NaN where the denominator is 0."""
        counts, sums = self.totals(flush_open)
        return summarise(counts.cpu().numpy(), sums.cpu().numpy())

    def reset(self):
        """Empty every accumulator and the totals (after a manual reset or set_state)."""
        self._call("reset")
