"""Scene rewind: go back to a past record of one scene and drive it again, many times (host side of `copo_rewind_*`).

`RewindBuffer` owns one `copo_rewind` handle over a source `VecSim`.  `record()` copies, on the GPU, everything a scene resumes from --
the 16 state words of every slot and the scene's four env words -- into that scene's ring of the last `depth` stored records (every
`stride`-th record is stored); `fork()` puts one scene at one past record into scenes of ANOTHER simulator, optionally with another
LCF for the agents driving at that moment and another seed for the draws that follow.  `Branches` owns such a target simulator and a
tally of how its scenes end: `fork`, then `step` / `rollout`, then `outcomes()`.  `Branches.sim` is an ordinary `VecSim`:
`TopDownRenderer` and `InteractionMeter` attach to it unchanged.  Records count as `ClipRecorder`'s do, so a clip header's `first_rec` /
`trig_rec` name rewind records when both are recorded every time (the dict env's `event_clips` + `rewind` keys do).  Eager only.  The
rules are DESIGN.md section 8d; `tests/rewind_numpy.py` restates them.
"""
import ctypes as C
import dataclasses

import numpy as np

from ._abi import REWIND_MAX_DEPTH as MAX_DEPTH, REWIND_TALLY as TALLY
from ._handle import Handle

TALLY_KEYS = ("steps", "acted", "arrive", "crash", "out", "maxstep", "watch_flags", "watch_step")
TALLY_INIT = (0, 0, 0, 0, 0, 0, 0, -1)


def _per_target(x, S, copies, dtype, name):
    """None, one value, one per request (repeated over its copies) or one per target scene -> numpy [S * copies] (or None)"""
    if x is None:
        return None
    a = np.asarray(x, dtype).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, S * copies)
    elif a.size == S and copies > 1:
        a = np.repeat(a, copies)
    if a.size != S * copies:
        raise ValueError("%s: one value, %d (one per request) or %d (one per target scene), not %d" % (name, S, S * copies, a.size))
    return np.ascontiguousarray(a)


class RewindBuffer(Handle):
    """Ring of the last `depth` (1..64) stored records of every scene of `sim`; record r is stored iff `r % stride == 0`.  Memory:
    `64 N E depth + 16 E depth` bytes.  `keep_obs`: the observation of every stored record is kept next to it (`368 N E depth` bytes more
    at 92 columns), so that `Branches.rollout` has the policy's first input -- a snapshot holds state, not observations.  `close()` it
    when done (before or after its simulator; no other call once the simulator is closed); `record` and `fork` are asynchronous on
    torch's current stream."""

    _prefix = "copo_rewind_"

    def __init__(self, sim, depth=8, stride=4, keep_obs=False):
        self._attach(sim)
        self.depth, self.stride, self.keep_obs = int(depth), int(stride), bool(keep_obs)
        cfg = self._capi.RewindCfg(self.depth, self.stride)
        self._create(self._capi.lib.copo_rewind_create, sim._h, C.byref(cfg))
        self._floor = 0            # first record a fork may take (`invalidate`)
        self._obs = None
        if self.keep_obs:
            torch = sim._torch
            self._obs = torch.zeros(self.depth, sim.E, sim.N, sim.O, dtype=torch.float32, device=sim.device)

    @classmethod
    def from_env(cls, sim, value):
        """The env's buffer (config key `rewind`: None, or the arguments of `RewindBuffer`)."""
        return cls(sim, **dict(value))

    def env_record(self, feed):
        """One record of the state after reset and after every step, next to the clip recorder's, so that a clip header's first_rec /
        trig_rec name rewind records.  The clip recorder counts on over a reset by hand, so the buffer does too; the records from
        before that reset can no longer be forked (`invalidate`)."""
        if feed.after_reset and self.n_records:
            self.invalidate()
        self.record()

    @property
    def n_records(self):
        """Records made since creation / `reset()`."""
        n = C.c_int32()
        self._capi.check(self._capi.lib.copo_rewind_count(self._h, C.byref(n)))
        return n.value

    def span(self):
        """(oldest, newest) stored record still in the ring, or None before the first record."""
        n = self.n_records
        if n == 0:
            return None
        q = (n - 1) // self.stride
        lo = max(max(0, q - self.depth + 1), -(-self._floor // self.stride)) * self.stride
        return (lo, q * self.stride) if lo <= q * self.stride else None

    def record(self, obs=None):
        """One record of the current state of every scene.  `obs` (with `keep_obs`): the observation that belongs to this state,
        float32 [E, N, O]; default: the simulator's own output tensor, which holds it right after `reset()` / `step()`."""
        r = self.n_records
        self._capi.check(self._capi.lib.copo_rewind_record(self._h, self._stream()))
        if self._obs is not None and r % self.stride == 0:
            self._obs[(r // self.stride) % self.depth].copy_(self.sim.out["obs"] if obs is None else obs)

    def reset(self):
        """Forget everything; records count from 0 again."""
        self._capi.check(self._capi.lib.copo_rewind_reset(self._h))           # (takes no stream)
        self._floor = 0

    def invalidate(self):
        """The records made so far can no longer be forked (status -1), the count goes on: for a source that was reset by hand --
        a fork takes the source scene's CURRENT seed, which no longer belongs to those records -- while another recorder
        (`ClipRecorder`) keeps counting the same records."""
        self._floor = self.n_records

    def fork(self, target, scenes, records, copies=1, lcf=None, seeds=None, watch_slots=None, first=0):
        """Request j: scene `scenes[j]` at the newest stored record <= `records[j]` becomes scenes `first + j * copies ...` (`copies`
        of them) of the `VecSim` `target` -- same map and slots, not the source.  `lcf`: NaN keeps the snapshot's, another value is
        given (clamped to [-1, 1]) to the agents ALIVE in the snapshot; agents spawned later draw from the target's own distribution.
        `seeds`: the target scenes' seeds (default: the source scene's, so a branch repeats the source's draws).  `lcf`, `seeds` and
        `watch_slots` take one value, one per request or one per target scene.  Returns `status` int32 [S * copies] on the device --
        the record taken, -1 for a request that cannot be served (nothing recorded, a record < 0 or already out of the ring, a scene
        outside the source: that target scene is left all-EMPTY) -- and, with `watch_slots`, `(status, watch_aid)`: the agent id in that
        slot of the snapshot, -1 when the slot is not ALIVE there."""
        torch, dev = self.sim._torch, self.sim.device
        sc = np.asarray(scenes, np.int32).reshape(-1)
        rc = np.asarray(records, np.int32).reshape(-1)
        if rc.size == 1:
            rc = np.repeat(rc, sc.size)
        if sc.size < 1 or rc.size != sc.size or copies < 1:
            raise ValueError("scenes / records: %d / %d requests, copies=%d" % (sc.size, rc.size, copies))
        S, copies = int(sc.size), int(copies)
        T = S * copies
        if self._floor:            # a request that would take a record from before `invalidate()` is sent as record -1
            taken = np.minimum(rc, self.n_records - 1) // self.stride * self.stride
            rc = np.where(taken < self._floor, -1, rc).astype(np.int32)

        def dev_arr(a, tdtype):
            return None if a is None else torch.from_numpy(a).to(dev).view(tdtype)
        t_sc = dev_arr(np.ascontiguousarray(np.repeat(sc, copies)), torch.int32)
        t_rc = dev_arr(np.ascontiguousarray(np.repeat(rc, copies)), torch.int32)
        t_lcf = dev_arr(_per_target(lcf, S, copies, np.float32, "lcf"), torch.float32)
        sd = _per_target(seeds, S, copies, np.uint64, "seeds")
        t_seeds = dev_arr(None if sd is None else sd.view(np.int64), torch.int64)
        t_ws = dev_arr(_per_target(watch_slots, S, copies, np.int32, "watch_slots"), torch.int32)
        status = torch.empty(T, dtype=torch.int32, device=dev)
        aid = torch.empty(T, dtype=torch.int32, device=dev) if t_ws is not None else None
        p = self._capi.ptr
        self._call("fork", target._h, int(first), T, p(t_sc), p(t_rc), p(t_lcf), p(t_seeds), p(t_ws), p(status), p(aid))
        self._last_fork = dict(scene=t_sc, lcf=t_lcf, watch_slot=t_ws)
        return status if aid is None else (status, aid)

    def fork_obs(self, status, out, lcf_col=-1):
        """With `keep_obs`: the kept observations of the records a fork took (`status`, and the scenes / LCFs of that fork) into `out`
        float32 [len(status), N, O]; rows of unserved requests are 0.  The `lcf` column of a scene whose LCF was overridden is set to
        `(lcf + 1) / 2` as the step kernel would write it (in every row: rows of slots without an agent mean nothing)."""
        assert self._obs is not None, "RewindBuffer(keep_obs=True) keeps the observations"
        torch, f = self.sim._torch, self._last_fork
        ok = status >= 0
        place = (torch.clamp(status, min=0) // self.stride) % self.depth
        scene = torch.clamp(f["scene"], 0, self.sim.E - 1)
        rows = self._obs[place.long(), scene.long()]
        rows = torch.where(ok.view(-1, 1, 1), rows, torch.zeros_like(rows))
        if f["lcf"] is not None and lcf_col >= 0:
            lv = f["lcf"]
            col = (torch.clamp(lv, -1.0, 1.0) + 1.0) * 0.5
            over = (ok & ~torch.isnan(lv)).view(-1, 1)
            rows[:, :, lcf_col] = torch.where(over, col.view(-1, 1), rows[:, :, lcf_col])
        out.copy_(rows)


def tally(flags, watch_slots, rows):
    """One step's `flags` (uint8 [B, N], a step's output) into the tally `rows` (int32 [B, 8], columns `TALLY_KEYS`, initialised to
    `TALLY_INIT`); `watch_slots` int32 [B] or None.  One launch on torch's current stream."""
    import torch
    from . import _capi
    B, N = flags.shape
    assert flags.is_cuda and flags.dtype == torch.uint8 and flags.is_contiguous()
    assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and tuple(rows.shape) == (B, TALLY)
    assert watch_slots is None or (watch_slots.is_cuda and watch_slots.dtype == torch.int32 and watch_slots.is_contiguous() and watch_slots.numel() == B)
    _capi.check(_capi.lib.copo_rewind_tally(flags.data_ptr(), _capi.ptr(watch_slots), rows.data_ptr(), B, N,
                                            torch.cuda.current_stream(flags.device).cuda_stream))
    return rows


class Branches:
    """`num_branches` scenes to re-roll forks of `buffer`'s simulator in: a `VecSim` of its own (`sim`) built from the source's
    `SimConfig`, and the tally of how each scene ends (`tally`, int32 [num_branches, 8] on the device).  `close()` when done."""

    def __init__(self, buffer, num_branches):
        from .sim import VecSim
        src = buffer.sim
        self.buffer, self._torch = buffer, src._torch
        torch = self._torch
        self.sim = VecSim(dataclasses.replace(src.cfg, num_envs=int(num_branches)), device=src.device.index, with_info=False)
        self.B = self.sim.E
        self.sim.reset()           # every scene is a valid one to step, forked into or not
        self._init = torch.tensor(TALLY_INIT, dtype=torch.int32, device=self.sim.device)
        self.tally = self._init.repeat(self.B, 1).contiguous()
        self.watch_slots = torch.full((self.B,), -1, dtype=torch.int32, device=self.sim.device)
        self._forked = False

    def fork(self, scenes, records, copies=1, lcf=None, seeds=None, watch_slots=None, first=0):
        """`RewindBuffer.fork` into this simulator, same arguments and return value; the tally rows of the written scenes start over
        and watch the given slots.  With a `keep_obs` buffer the scenes' rows of `sim.out["obs"]` become the forked records'
        observations."""
        res = self.buffer.fork(self.sim, scenes, records, copies=copies, lcf=lcf, seeds=seeds, watch_slots=watch_slots, first=first)
        status = res[0] if isinstance(res, tuple) else res
        lo, hi = int(first), int(first) + status.numel()
        self.tally[lo:hi] = self._init
        ws = self.buffer._last_fork["watch_slot"]
        self.watch_slots[lo:hi] = -1 if ws is None else ws
        if self.buffer.keep_obs:
            self.buffer.fork_obs(status, self.sim.out["obs"][lo:hi], self.sim.cfg.lcf_col)
        self._forked = True
        return res

    def step(self, act):
        """Step every scene with `act` float32 [num_branches, N, A] and add the step's flags to the tally; returns the step's outputs."""
        out = self.sim.step(act)
        tally(out["flags"], self.watch_slots, self.tally)
        return out

    def rollout(self, policy, steps, obs=None):
        """`steps` steps under `policy`, a callable from the observation tensor float32 [num_branches, N, O] to the action tensor
        [num_branches, N, A] (rows of slots without an agent are ignored by the simulator).  The first input is `obs`, or -- with a
        `keep_obs` buffer -- the forked records' observations."""
        torch = self._torch
        assert self._forked, "fork() first"
        if obs is None:
            if not self.buffer.keep_obs:
                raise ValueError("a snapshot holds no observation: pass obs=, or record with RewindBuffer(keep_obs=True)")
            obs = self.sim.out["obs"]
        out = None
        for _ in range(int(steps)):
            act = torch.as_tensor(policy(obs), dtype=torch.float32, device=self.sim.device).reshape(self.B, self.sim.N, self.sim.A).contiguous()
            out = self.step(act)
            obs = out["obs"]
        return out

    def outcomes(self):
        """The tally as a dict of numpy int32 [num_branches] by column name (`TALLY_KEYS`); waits for the stream."""
        t = self.tally.cpu().numpy()
        return {k: t[:, i].copy() for i, k in enumerate(TALLY_KEYS)}

    def close(self):
        if getattr(self, "sim", None) is not None:
            self.sim.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
