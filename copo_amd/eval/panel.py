"""What representation similarity (`similarity.py`) and linear probes (`probes.py`) share: a panel of bank members that all read the same
rows of a seated evaluation, and the hidden activations `copo_hidden_obs_seats_f32` keeps of them there.

Pieces: `PanelPlan` (numpy only: the members, the `JuryPlan.panel` whose lists the hidden launch reads, the one common row list, the row
split of the float64 accumulators), `PanelSeatSampler` (a `SeatSampler` that keeps h1 and h2 of every panel member on the observation the
policy reads), `hidden_activations` / `every_row` (the same on a plain observation array, every row counted) and `want` (the tensor check
of the thin wrappers).  The Gram kernels under both studies share csrc/gram_common.h in the same way.
"""
import numpy as np

from .crossplay import SeatPlan, SeatSampler
from .jury import JuryBuffers, JuryPlan

LAYERS = ("h1", "h2")
CHUNK, MAX_PLANES, MAX_PANEL, TILE = 32, 8, 255, 64          # include/copo_hip.h, COPO_CKA_*; csrc/gram_common.h
FILL_WORKGROUPS = 256          # the row split stops once the Gram launch has this many workgroups: one per compute unit of the target


class PanelPlan:
    """A panel of bank members on the seated rows of the seat plan `seats`.  `members`: the panel, bank members in the order of the
    tables (default: all K).  `rows_of`: None, or the member whose DRIVEN rows alone are counted.  Derived: `jury`, the `JuryPlan.panel`
    whose lists the hidden launch reads (every panel member's list is `rows`, the one common ascending list of the seated rows e * N + n
    of the groups in [0, G); `count`, `cap`); `row_split(tiles)`, the fixed row split R of an accumulator set whose launch has `tiles`
    workgroups per plane (a power of two up to 8: doubled while the launch has fewer than 256 workgroups and every plane still gets a chunk
    of 32 rows -- a property of the plan, never of the device).  A refusal starts with the name of the class that refuses.  Nothing here
    touches a device."""

    def __init__(self, seats, members=None, rows_of=None, max_bytes=1 << 30):
        who = type(self).__name__
        members = list(range(seats.K)) if members is None else [int(m) for m in members]
        if len(members) > MAX_PANEL:
            raise ValueError("%s: a panel of %d, %d at the most" % (who, len(members), MAX_PANEL))
        self.jury = JuryPlan.panel(seats, members)          # (refuses an empty panel, members outside the bank and duplicates)
        self.members, self.M, self.K = np.asarray(members, np.int32), len(members), seats.K
        self.rows_of = -1 if rows_of is None else int(rows_of)
        if rows_of is not None and not 0 <= self.rows_of < seats.K:
            raise ValueError("%s: rows_of = %r of a bank of %d" % (who, rows_of, seats.K))
        first = members[0]
        self.rows, self.count, self.cap = self.jury.rows[first], int(self.jury.counts[first]), self.jury.cap
        self.E, self.N, self.n_out, self.G = seats.E, seats.N, seats.E * seats.N, seats.n_groups
        self.max_bytes = int(max_bytes)

    def check(self, seats):
        self.jury.check(seats)
        return self

    def row_split(self, tiles):
        chunks, R = -(-self.cap // CHUNK), 1
        while R < MAX_PLANES and tiles * R < FILL_WORKGROUPS and 2 * R <= chunks:
            R *= 2
        return R

    def check_width(self, hidden, most):
        H = int(hidden)
        if H < TILE or H > most or H % TILE:
            raise ValueError("%s: hidden = %d, a multiple of %d up to %d wanted" % (type(self).__name__, H, TILE, most))
        return H

    @staticmethod
    def bytes_of(*shape_sets):
        """The bytes of float64 / int64 accumulators of the shapes in the dicts `shape_sets`."""
        return 8 * sum(int(np.prod(shape)) for shapes in shape_sets for shape in shapes.values())


def want(who, name, t, shape, dtype):
    """Refuses a tensor that is not contiguous, of `shape` and of `dtype`, in the name of the wrapper `who`."""
    if t is None or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != dtype:
        raise ValueError("%s: %s of shape %s and dtype %s, contiguous %s %s wanted" % (
            who, name, None if t is None else tuple(t.shape), None if t is None else t.dtype, dtype, list(shape)))


class PanelSeatSampler(SeatSampler):
    """`SeatSampler` with a panel (`PanelPlan`): per env step `hidden_seats` on the observation the policy reads leaves h1 and h2 of every
    panel member in `hidden` float32 [K][cap][2][H], listed by `_rows` / `_count` (the common list on the device).  Actions, flags and the
    seat tally are a plain `SeatSampler`'s.  A subclass sets `acc`, the accumulators that `clear_tally()` clears, and adds to them in
    `_step`."""

    def __init__(self, vec_env, policy, bank, plan, panel, T, use_graph=True):
        import torch
        panel.check(plan)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.jury_buffers = JuryBuffers(panel.jury, self.device)
        self.jury_buffers.on_replace.append(self._loop.reset)
        self.hidden = torch.zeros(bank.K, panel.cap, 2, int(bank.cfg.hidden), dtype=torch.float32, device=self.device)
        first = int(panel.members[0])
        self._rows, self._count = self.jury_buffers.rows[first], self.jury_buffers.counts[first:first + 1]

    def clear_tally(self):
        super().clear_tally()
        self.acc.clear()

    def _policy_obs(self, t):
        obs = super()._policy_obs(t)
        self.seated.hidden_seats(self.jury_buffers, obs.view(-1, self.O), self.hidden)
        return obs


def hidden_activations(bank, obs):
    """`hidden` [K][n][2][H] of every member of `bank` on every row of obs [n][O]: one launch with every member reading every row."""
    import torch
    n = int(obs.shape[0])
    seats = SeatPlan(np.zeros((1, n), np.int32), bank.K)
    jb = JuryBuffers(JuryPlan.everyone(seats), obs.device)
    hidden = torch.zeros(bank.K, n, 2, int(bank.cfg.hidden), dtype=torch.float32, device=obs.device)
    bank.sync_mirror()
    bank.hidden_seats(jb, obs, hidden)
    torch.cuda.current_stream().synchronize()          # (the plan's tables die with this call)
    return hidden


def every_row(n, device):
    """(rows, count, flags, seat, rows_of) under which every row of a plain array of `n` rows counts: the list 0 .. n - 1, ACTED
    everywhere, every seat 0 and no `rows_of`."""
    import torch
    return (torch.arange(n, dtype=torch.int64, device=device), torch.full((1,), n, dtype=torch.int32, device=device),
            torch.ones(n, dtype=torch.uint8, device=device), torch.zeros(n, dtype=torch.int32, device=device), -1)
