"""Base class of everything that owns a handle of libcopo_hip.so on one GPU: `VecSim` and the observers of one."""
import ctypes as C


class Handle:
    """`_h` is the library's handle, made by `_create` and given to the library's `<_prefix>destroy` by `close()`; `device` and
    `_torch` name where its calls run.  An observer calls `_attach(sim)` first.  `close()` is idempotent, and an observer's may come
    after its simulator's; every other call on an observer whose simulator is closed is undefined."""

    _prefix = None                 # "copo_<handle>_": the library's entry points for this handle are `<_prefix>record` ...

    def _attach(self, sim):
        from . import _capi
        self._capi, self.sim, self._torch, self.device = _capi, sim, sim._torch, sim.device

    def _create(self, fn, *args):
        h = C.c_void_p()
        self._capi.check(fn(*args, C.byref(h)))
        self._h = h

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, name, *args):
        """`<_prefix><name>(handle, *args, torch's current stream)`, checked.  Not for `record()`: a call per step spells itself out."""
        self._capi.check(getattr(self._capi.lib, self._prefix + name)(self._h, *args, self._stream()))

    def _en_arg(self, t, dtype, name):
        if t is None:
            return None
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == self.sim.E * self.sim.N):
            raise ValueError("%s must be a contiguous %s cuda tensor [E, N]" % (name, dtype))
        return t.data_ptr()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._capi.lib, self._prefix + "destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Grouped:
    """Mixin of an observer with scene groups: scene e adds to group[e], a value outside 0..groups-1 to nothing; all 0 at first."""

    def set_groups(self, group):
        """Scene groups: int32 [E] (torch tensor on the simulator's device, or anything numpy reads)."""
        import numpy as np
        torch = self._torch
        if not hasattr(group, "is_cuda"):
            group = torch.from_numpy(np.ascontiguousarray(np.asarray(group, np.int32).reshape(-1)))
        group = group.to(device=self.device, dtype=torch.int32).contiguous()
        if group.numel() != self.sim.E:
            raise ValueError("one group per scene: %d values for %d scenes" % (group.numel(), self.sim.E))
        self._call("set_groups", group.data_ptr())
