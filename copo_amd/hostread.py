"""The one way the trainer and the policies bring the results of an iteration to the host.

  HostRead       named 1-D device tensors packed into one tensor, read once (optionally through an asynchronous copy into a pinned
                 buffer) and decoded by name.
  PinnedBuffer   the pinned host memory of such copies, kept by whoever issues the same read every iteration.
  PendingResult  a HostRead plus the function that builds the caller's result dict from its parts: what `run_sgd(defer=True)` and
                 `run_meta(defer=True)` return.
"""
import torch


class PinnedBuffer:
    """Pinned host memory for one recurring read, allocated at its first use (and again should the read change its size or type)."""

    def __init__(self):
        self.buf = None

    def fit(self, packed):
        if self.buf is None or self.buf.numel() != packed.numel() or self.buf.dtype != packed.dtype:
            self.buf = torch.empty(packed.numel(), dtype=packed.dtype, pin_memory=True)
        return self.buf


class HostRead:
    """`parts`: ordered (name, 1-D device tensor) pairs.  Parts of one dtype are packed as they are (a single part is not even
    concatenated), parts of several dtypes as float64.  `get()` returns {name: list of floats}."""

    def __init__(self, parts, pin=None):
        self.names = [name for name, _ in parts]
        assert len(set(self.names)) == len(self.names), self.names
        tensors = [t.detach().reshape(-1) for _, t in parts]
        self.sizes = [t.numel() for t in tensors]
        if len({t.dtype for t in tensors}) > 1:
            tensors = [t.double() for t in tensors]
        self.packed = tensors[0] if len(tensors) == 1 else torch.cat(tensors)
        self._pin = pin if pin is not None else PinnedBuffer()
        self._event = None
        self._parts = None

    def start(self):
        """GPU: queue the copy to the host behind what the current stream holds now; `get()` then waits for ITS event, not for the
        stream, and later writes to the parts on this stream do not reach it.  CPU: nothing to do."""
        if self.packed.is_cuda and self._event is None and self._parts is None:
            self._pin.fit(self.packed).copy_(self.packed, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()

    def _read(self):
        """The device -> host read itself (the only place that waits for the device)."""
        if self._event is not None:
            self._event.synchronize()
            return self._pin.buf.tolist()
        return self.packed.tolist()

    def get(self, values=None):
        """`values`: the packed numbers, already on the host (they rode along in another read).  A second call returns the first
        call's dict and touches no device."""
        if self._parts is None:
            values = self._read() if values is None else list(values)
            assert len(values) == sum(self.sizes), (len(values), self.sizes)
            self._parts, o = {}, 0
            for name, n in zip(self.names, self.sizes):
                self._parts[name] = values[o:o + n]
                o += n
        return self._parts


class PendingResult:
    """Calling it resolves `read` and returns `build(parts)`, once; `parts` are the decoded host values themselves (riders included)."""

    def __init__(self, read, build):
        self.read, self._build, self._result = read, build, None

    def start(self):
        self.read.start()

    @property
    def parts(self):
        return self.read.get()

    def __call__(self, values=None):
        if self._result is None:
            self._result = self._build(self.read.get(values))
        return self._result
