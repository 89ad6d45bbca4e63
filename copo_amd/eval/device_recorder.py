"""Device evaluation recorder (host side of `copo_recorder_*`): the reference's per-episode evaluation table
(`RecorderEnv.get_episode_result`, copo/eval/recoder.py:188-349) for E scenes at once, with its SVO estimate (:108-115, :326-347).

`DeviceRecorder.add(batch)` consumes one sampler fragment -- `flags`, `infos`, `rewards`, `nei_rewards`, `nbr_cnt`, the tensors
`VecSampler.sample()` returns, read in place -- in three launches whatever `T` is and without a host read; a finished whole scene
episode leaves ONE row of `COLUMNS` (+ scene, episode index) in a pool of `max_rows` rows on the device (later ones are counted as
dropped).  The accumulators are carried across fragments, and every sum over slots has one fixed order, so the rows do not depend on
how a stream of steps is cut into fragments.  With `limit` > 0 the steps of a scene that has finished `limit` episodes are ignored.

The 25 columns of `vec_recorder.COLUMNS` follow `VecRecorder`'s definitions one for one.  The SVO estimate: per agent
`own` = sum of its reward and `nei` = sum of its neighbourhood reward (its own reward in a step with nobody in range) over the rows it
is present in; when it terminates, `alpha = degrees(atan2(nei, own))`, `svo = clip(alpha, 0, 90)` and `svo_reward` gains
`hypot(nei, own) * cos(radians(svo - alpha))`; the row holds mean / min / max of `svo` over the agents that terminated in the episode and
`svo_reward` = sum / `num_agents_total`.

DEVIATION from the reference: in the step an agent is spawned into a slot whose occupant just terminated (flags `F_DONE | F_SPAWNED`)
the reference adds the NEW agent's neighbourhood reward of that step to the new agent; the simulator's row of that step holds the
terminating agent's numbers, so the row counts for the agent that acted and the new occupant starts at zero sums.  The energy columns
stay out (MetaDrive's energy model is out of scope).  The rules: include/copo_hip.h, DESIGN.md section 8j;
tests/recorder_numpy.py restates them."""
import ctypes as C

import numpy as np

from .._handle import Handle
from . import vec_recorder

SVO_COLUMNS = ("svo_estimate_deg_mean", "svo_estimate_deg_min", "svo_estimate_deg_max", "svo_reward")
COLUMNS = vec_recorder.COLUMNS + SVO_COLUMNS
NCOL = len(COLUMNS) + 2          # + scene, + episode index of the scene
_INPUTS = (("flags", "uint8", 1), ("infos", "float32", 8), ("rewards", "float32", 1), ("nei_rewards", "float32", 1), ("nbr_cnt", "int32", 1))


class DeviceRecorder(Handle):
    _prefix = "copo_recorder_"

    def __init__(self, E, N, device, max_rows=4096, limit=0):
        import torch
        from .. import _capi
        assert NCOL == _capi.RECORDER_NCOL
        self._capi, self._torch, self.sim = _capi, torch, None
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.E, self.N, self.max_rows, self.limit = int(E), int(N), int(max_rows), int(limit)
        with torch.cuda.device(self.device):
            self._create(_capi.lib.copo_recorder_create, self.E, self.N, self.max_rows, self.limit)

    def add(self, batch):
        """Consume one sampler fragment: contiguous tensors [T, E, N] (`infos` [T, E, N, 8]) on the recorder's device."""
        torch = self._torch
        T = int(batch["flags"].shape[0])
        ptrs = []
        for key, dtype, last in _INPUTS:
            t = batch[key]
            if not (t.is_cuda and t.device == self.device and t.dtype == getattr(torch, dtype) and t.is_contiguous() and
                    t.numel() == T * self.E * self.N * last):
                raise ValueError("%s must be a contiguous %s tensor of %d x %d x %d%s on %s" % (
                    key, dtype, T, self.E, self.N, " x 8" if last > 1 else "", self.device))
            ptrs.append(t.data_ptr())
        self._capi.check(self._capi.lib.copo_recorder_add(self._h, *ptrs, T, self._stream()))

    def episodes(self):
        """Finished episodes per scene, device int64 [E] (a copy; no host read)."""
        out = self._torch.empty(self.E, dtype=self._torch.int64, device=self.device)
        self._call("episodes", out.data_ptr())
        return out

    def count(self):
        """(rows stored, rows dropped); waits for the stream."""
        out = (C.c_int64 * 2)()
        self._call("count", out)
        return int(out[0]), int(out[1])

    def rows(self):
        """The stored rows, device float64 [n, NCOL] (a copy): `COLUMNS`, scene, episode index of the scene."""
        torch = self._torch
        n, _ = self.count()
        out = torch.empty(n, NCOL, dtype=torch.float64, device=self.device)
        if n:
            self._call("read", 0, n, out.data_ptr())
        return out

    def clear(self):
        """Empty the pool and the dropped count; the open episodes and the episode counts stay."""
        self._call("clear")

    def reset(self):
        """Forget every row, counter, open episode and episode count."""
        self._call("reset")

    def frame(self):
        """The rows as a pandas DataFrame: `COLUMNS` and `scene`, as `VecRecorder.frame()` names them."""
        import pandas as pd
        r = self.rows().cpu().numpy()
        df = pd.DataFrame(r[:, :len(COLUMNS)], columns=list(COLUMNS))
        df["scene"] = r[:, len(COLUMNS)].astype(np.int64)
        return df

    def means(self):
        r = self.rows().cpu().numpy()
        if not len(r):
            return {}
        return {c: float(np.mean(r[:, k])) for k, c in enumerate(COLUMNS)}
