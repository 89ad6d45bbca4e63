"""What the trip log, the conflict log and the encroachment log share on the host (`trips.py`, `conflicts.py`, `encroach.py`; the device side is `csrc/rowlog_common.h`): a
table of raw 16-word rows with its `.npz` file, and the handle calls over a bounded pool of such rows.  DESIGN.md section 8g."""
import ctypes as C

import numpy as np

from . import _npz
from ._handle import Handle

WORDS = 16


class RowTable:
    """Rows as numpy: `raw` uint32 [n, 16] as the device wrote them, `meta` (dict), and the columns of the subclass's
    `_decode(raw, meta)` as attributes / items."""

    def __init__(self, raw, meta):
        self.raw = np.ascontiguousarray(np.asarray(raw).reshape(-1, WORDS)).view(np.uint32).copy()
        self.meta = dict(meta)
        self.columns = self._decode(self.raw, self.meta)

    def __len__(self):
        return len(self.raw)

    def __getitem__(self, key):
        return self.columns[key]

    def __getattr__(self, key):
        cols = self.__dict__.get("columns")
        if cols is not None and key in cols:
            return cols[key]
        raise AttributeError(key)

    def save(self, path):
        """One `.npz` without pickled objects (`np.load(path, allow_pickle=False)` reads it): the raw rows and `meta` as JSON."""
        return _npz.save(path, self.meta, rows=self.raw)

    @classmethod
    def load(cls, path):
        return cls(*_npz.load(path, "rows"))


class RowLog(Handle):
    """A handle whose `record()` commits rows into a pool of `max_rows` (later ones are counted as dropped).  The subclass supplies
    `_prefix`, `_table_cls`, `_meta(dropped)` and `record`, and counts `n_records`."""

    def flush(self):
        """Close everything that is open as it stands (the last kind, outcome "open"); what goes on opens anew in the next record."""
        self._call("flush")

    def count(self):
        """(rows stored, rows dropped); waits for the stream."""
        out = (C.c_int64 * 2)()
        self._call("count", out)
        return int(out[0]), int(out[1])

    def clear(self):
        """Empty the pool and the dropped count; what is open and the record count stay."""
        self._call("clear")

    def reset(self):
        """Forget every row, counter and everything open; records count from 0 again."""
        self._call("reset")
        self.n_records = 0

    def rows(self):
        """The stored rows, device int32 [n, 16] (a copy)."""
        torch = self._torch
        n, _ = self.count()
        out = torch.empty(n, WORDS, dtype=torch.int32, device=self.device)
        if n:
            self._call("read", 0, n, out.data_ptr())
        return out

    def table(self):
        """The stored rows as a table of `_table_cls`."""
        _, dropped = self.count()
        return self._table_cls(self.rows().cpu().numpy(), self._meta(dropped))

    def drain(self):
        """`table()`, then `clear()`: what a long run calls now and then to keep a bounded pool from overflowing."""
        t = self.table()
        self.clear()
        return t
