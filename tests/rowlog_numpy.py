"""The pool under the restatements of the trip log and the conflict log (tests/trip_numpy.py, tests/conflict_numpy.py; DESIGN.md section
8g) and what the two share.  The rows closed in one record take the ids n_rows, n_rows + 1, ... in the order the restatement commits
them; an id >= max_rows is dropped, what it stood for is closed all the same.  `clear` empties the pool and the dropped count only."""
import numpy as np

ST_EMPTY, ST_ALIVE, ST_WRECK = 0, 1, 2
F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = (1 << i for i in range(8))
WORDS = 16
f32 = np.float32
M32 = 0xFFFFFFFF


class RowPool:
    """The subclass sets `max_rows` and, in its `reset`, `total_closed = 0` (what the tests' premises need, not part of the rules)."""

    def clear(self):
        self._rows, self.close_rec, self.dropped = [], [], 0

    n_rows = property(lambda self: len(self._rows))

    def rows(self):
        return np.array(self._rows, np.uint32).reshape(-1, WORDS)

    def _store(self, row, close_rec):
        self.total_closed += 1
        if len(self._rows) >= self.max_rows:
            self.dropped += 1
            return
        self._rows.append(row)
        self.close_rec.append(close_rec)


def compare(got_rows, got_count, ref):
    """the device's rows (anything numpy reads as [n, 16] words) and (n_rows, dropped) equal the restatement's, word for word"""
    a, b = np.ascontiguousarray(np.asarray(got_rows).reshape(-1, WORDS)).view(np.uint32), ref.rows()
    assert tuple(int(v) for v in got_count) == (ref.n_rows, ref.dropped), (got_count, ref.n_rows, ref.dropped)
    assert a.shape == b.shape and np.array_equal(a, b), (a.shape, b.shape, np.argwhere(a != b)[:8].tolist() if a.shape == b.shape else None)
