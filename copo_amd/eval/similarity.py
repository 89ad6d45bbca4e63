"""Representation similarity: linear centred kernel alignment (CKA) between the hidden layers of bank members on the same states.

The other studies of seated evaluation compare what checkpoints DO; `jury.py` compares the outputs of two checkpoints on the same
states.  Here what they compute inside: is a 0.3 nat gap between CoPO and IPPO a different head on the same features, or a different
first layer?  Are two seeds with a large weight distance the same network up to a permutation of hidden units?  Linear CKA of the
activations of two nets on the same inputs,
    cka(a, b) = hsic(a, b) / sqrt(hsic(a, a) hsic(b, b)),    hsic(a, b) = || Ha^T Hb - (1^T Ha)^T (1^T Hb) / n ||_F^2,
is invariant to permutation, rotation and isotropic scaling of the units, which weight distance and unit-by-unit correlation are not.

A `SimilarityPlan` is a panel of members that all read the same rows: the seated rows of the scene groups of a seat plan (a `PanelPlan`
of `panel.py`, shared with `probes.py`: internally a `JuryPlan.panel`, so every member's list is the one common ascending list).  Per env step `copo_hidden_obs_seats_f32`
(csrc/learn_hidden.inc, the fourth mode of the bank's forward: the jury pass stopped behind layer 2) keeps h1 and h2 of every panel member
on those rows, and `copo_cka_accumulate` (csrc/cka_kernels.hip) adds the step's H x H cross-products of every member pair, the unit sums
and the row count to float64 accumulators -- over the rows that ACTED in the step (the seat tally's rule), optionally only over the rows
one member drives (`rows_of`).  `copo_cka_finish` turns the accumulators into the centred norms when the frame is read.  Nothing here
changes anybody's driving: the drive and the seat tally are a plain `SeatSampler`'s, bit for bit.

`cka` is NaN where fewer than two rows were counted or either norm is zero (a member whose every unit is constant on the rows); it is
never an exception.

Pieces: `SimilarityPlan` (numpy only), `PolicyBank.hidden_seats` / `SeatedBank.hidden_seats`, `cka_accumulate` / `cka_finish` (thin
checked wrappers), `SimilarityAccumulators`, `SimilaritySeatSampler` (forward, step, seat tally, hidden launch and accumulate of a
fragment stay one captured graph; finish is issued when the frame is read), `similarity_frame` / `similarity_matrix` / `unit_frame`,
`similarity_rows` (`evaluate --similarity`) and `hidden_activations` / `cka_of` (one launch on a plain observation array).
"""
import numpy as np

from .crossplay import SeatPlan, run_pairs
from .panel import CHUNK, FILL_WORKGROUPS, LAYERS, MAX_PANEL, MAX_PLANES, TILE, PanelPlan, PanelSeatSampler, every_row, want      # noqa: F401
from .panel import hidden_activations      # noqa: F401  (its home is panel.py; it stays importable from here)

PROMOTE_ROWS, MAX_HIDDEN = 128, 512          # include/copo_hip.h, COPO_CKA_*
DEAD_VARIANCE, SATURATED_MEAN = 1e-8, 0.99


class SimilarityPlan(PanelPlan):
    """A `PanelPlan` of bank members compared on the seated rows of the seat plan `seats`.  `members`: default all K; otherwise at least
    two distinct members.  Its own: `pairs` int32 [P][2], the unordered pairs a <= b of PANEL indices in the accumulators' order;
    `planes(hidden)`, the row split R of the accumulators (`PanelPlan.row_split` of the Gram launch's P * 2 * (hidden / 64)^2
    workgroups); `accumulator_shapes(hidden)`, `accumulator_bytes(hidden)`.  `check_bytes(hidden)` refuses accumulators beyond `max_bytes`
    (default 1 GiB) with the figure; it runs at construction where `hidden` is given.  Nothing here touches a device."""

    def __init__(self, seats, members=None, rows_of=None, hidden=None, max_bytes=1 << 30):
        members = list(range(seats.K)) if members is None else [int(m) for m in members]
        if members != list(range(seats.K)) and len(members) < 2:
            raise ValueError("SimilarityPlan: a panel of %d, at least two members wanted" % len(members))
        super().__init__(seats, members, rows_of, max_bytes)
        self.pairs = np.array([(a, b) for a in range(self.M) for b in range(a, self.M)], np.int32)
        self.P = len(self.pairs)
        if hidden is not None:
            self.check_bytes(hidden)

    def planes(self, hidden):
        return self.row_split(self.P * 2 * (int(hidden) // TILE) ** 2)

    def accumulator_shapes(self, hidden):
        H, R = int(hidden), self.planes(hidden)
        return dict(S=(R, self.P, 2, H, H), s=(R, self.M, 2, H), n=(R,))

    def accumulator_bytes(self, hidden):
        return self.bytes_of(self.accumulator_shapes(hidden))

    def check_bytes(self, hidden):
        H = self.check_width(hidden, MAX_HIDDEN)
        need = self.accumulator_bytes(H)
        if need > self.max_bytes:
            raise ValueError("SimilarityPlan: %d pairs x 2 layers x %d x %d float64 in %d planes are %d bytes of accumulators, max_bytes = %d" % (
                self.P, H, H, self.planes(H), need, self.max_bytes))
        return need


def cka_accumulate(hidden, panel, rows, count, flags, seat, rows_of, S, s, n):
    """One step's `hidden` float32 [K][cap][2][H] (`PolicyBank.hidden_seats`) added to the accumulators `S` float64 [R][P][2][H][H], `s`
    float64 [R][M][2][H] and `n` int64 [R] over the counted positions of the common list `rows` int64 [cap] / `count` int32 [1]:
    position p counts when p < count, `flags` uint8 [n_out] carry ACTED at rows[p] and (`rows_of` < 0 or `seat` int32 [n_out] is
    `rows_of` there).  `panel` int32 [M]: the members compared, P = M (M + 1) / 2.  R is read off `S`.  The outputs accumulate; the
    caller clears them.  One launch on the current stream."""
    import torch
    from .. import _capi
    who = "cka_accumulate"
    if hidden is None or hidden.dim() != 4 or hidden.shape[2] != 2:
        raise ValueError("%s: hidden of shape %s, [K][cap][2][H] wanted" % (who, None if hidden is None else tuple(hidden.shape)))
    K, cap, _, H = (int(v) for v in hidden.shape)
    if panel is None or panel.dim() != 1:
        raise ValueError("%s: panel of shape %s, [M] wanted" % (who, None if panel is None else tuple(panel.shape)))
    M = int(panel.shape[0])
    P = M * (M + 1) // 2
    if S is None or S.dim() != 5:
        raise ValueError("%s: S of shape %s, [R][P][2][H][H] wanted" % (who, None if S is None else tuple(S.shape)))
    R = int(S.shape[0])
    if flags is None or seat is None or flags.numel() != seat.numel() or flags.numel() < 1:
        raise ValueError("%s: flags and seat must cover the same rows" % who)
    want(who, "hidden", hidden, (K, cap, 2, H), torch.float32)
    want(who, "panel", panel, (M,), torch.int32)
    want(who, "rows", rows, (cap,), torch.int64)
    want(who, "count", count, (1,), torch.int32)
    want(who, "flags", flags, flags.shape, torch.uint8)
    want(who, "seat", seat, seat.shape, torch.int32)
    want(who, "S", S, (R, P, 2, H, H), torch.float64)
    want(who, "s", s, (R, M, 2, H), torch.float64)
    want(who, "n", n, (R,), torch.int64)
    _capi.check(_capi.lib.copo_cka_accumulate(hidden.data_ptr(), K, cap, H, panel.data_ptr(), M, rows.data_ptr(), count.data_ptr(), flags.data_ptr(),
                                              seat.data_ptr(), int(flags.numel()), int(rows_of), R, S.data_ptr(), s.data_ptr(), n.data_ptr(),
                                              _capi.current_stream()))


def cka_finish(S, s, n, hsic, n_out, mean, var):
    """The accumulators of `cka_accumulate` -> `hsic` float64 [M][M][2] (both triangles), `n_out` int64 [1], `mean` and `var` float64
    [M][2][H] of the units; zeros with fewer than two counted rows.  One launch on the current stream."""
    import torch
    from .. import _capi
    who = "cka_finish"
    if S is None or S.dim() != 5 or s is None or s.dim() != 4:
        raise ValueError("%s: S [R][P][2][H][H] and s [R][M][2][H] wanted" % who)
    R, P, _, H, _ = (int(v) for v in S.shape)
    M = int(s.shape[1])
    want(who, "S", S, (R, M * (M + 1) // 2, 2, H, H), torch.float64)
    want(who, "s", s, (R, M, 2, H), torch.float64)
    want(who, "n", n, (R,), torch.int64)
    want(who, "hsic", hsic, (M, M, 2), torch.float64)
    want(who, "n_out", n_out, (1,), torch.int64)
    want(who, "mean", mean, (M, 2, H), torch.float64)
    want(who, "var", var, (M, 2, H), torch.float64)
    _capi.check(_capi.lib.copo_cka_finish(S.data_ptr(), s.data_ptr(), n.data_ptr(), M, H, R, hsic.data_ptr(), n_out.data_ptr(), mean.data_ptr(),
                                          var.data_ptr(), _capi.current_stream()))


def cka_from_hsic(hsic, n):
    """cka [M][M][2] = hsic[a][b] / sqrt(hsic[a][a] hsic[b][b]) from `hsic` [M][M][2] (numpy float64); NaN everywhere with n < 2, and
    wherever either norm is zero."""
    hsic = np.asarray(hsic, np.float64)
    diag = np.einsum("aal->al", hsic)
    with np.errstate(invalid="ignore", divide="ignore"):
        cka = hsic / np.sqrt(diag[:, None, :] * diag[None, :, :])
    cka[~np.isfinite(cka)] = np.nan
    if int(n) < 2:
        cka[:] = np.nan
    return cka


class SimilarityAccumulators:
    """The float64 accumulators of a panel of M members at hidden width H in R planes, and what `cka_finish` writes from them."""

    def __init__(self, M, H, R, device):
        import torch
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
        self.M, self.H, self.R = int(M), int(H), int(R)
        self.S, self.s, self.n = z(R, M * (M + 1) // 2, 2, H, H), z(R, M, 2, H), z(R, dtype=torch.int64)
        self.hsic, self.n_out, self.mean, self.var = z(M, M, 2), z(1, dtype=torch.int64), z(M, 2, H), z(M, 2, H)

    def clear(self):
        for t in (self.S, self.s, self.n):
            t.zero_()

    def finish(self):
        """`cka_finish` on the current stream, then one host read: dict(n, hsic, cka, mean, var) as numpy."""
        import torch
        cka_finish(self.S, self.s, self.n, self.hsic, self.n_out, self.mean, self.var)
        torch.cuda.current_stream().synchronize()
        n, hsic = int(self.n_out.cpu()[0]), self.hsic.cpu().numpy()
        return dict(n=n, hsic=hsic, cka=cka_from_hsic(hsic, n), mean=self.mean.cpu().numpy(), var=self.var.cpu().numpy())


class SimilaritySeatSampler(PanelSeatSampler):
    """`PanelSeatSampler` with a similarity panel: per env step `hidden_seats` on the observation the policy reads, the seated forward on
    the same observation, the simulator step, the seat tally and `cka_accumulate` of the step's flags -- the whole fragment is still one
    captured graph.  `acc` (`SimilarityAccumulators`) accumulates until `clear_tally()`; `read()` issues the finish and returns its
    numbers, `frame()` / `units()` the tables."""

    def __init__(self, vec_env, policy, bank, plan, similarity, T, use_graph=True):
        import torch
        H = int(bank.cfg.hidden)
        similarity.check(plan).check_bytes(H)
        super().__init__(vec_env, policy, bank, plan, similarity, T, use_graph=use_graph)
        self.similarity = similarity
        self.panel = torch.from_numpy(similarity.members.copy()).to(self.device)
        self.acc = SimilarityAccumulators(similarity.M, H, similarity.planes(H), self.device)

    def _step(self, t):
        super()._step(t)
        cka_accumulate(self.hidden, self.panel, self._rows, self._count, self.flags[t].view(-1), self.seated.buffers.seat.view(-1),
                       self.similarity.rows_of, self.acc.S, self.acc.s, self.acc.n)

    def read(self):
        return self.acc.finish()

    def frame(self, labels=None):
        r = self.read()
        return similarity_frame(r["hsic"], r["n"], self.similarity, labels)

    def units(self, labels=None):
        r = self.read()
        return unit_frame(r["mean"], r["var"], r["n"], self.similarity, labels)


def similarity_frame(hsic, n, plan, labels=None):
    """`hsic` [M][M][2] and the row count `n` of a panel as a frame: one row per (member a, member b, layer), both orders and the
    diagonal.  Columns: `member_a`, `member_b`, `label_a`, `label_b`, `layer` ("h1" / "h2"), `rows_of` (-1: every acted row), `n`,
    `hsic`, `cka` (NaN with n < 2 or a zero norm)."""
    import pandas as pd
    labels = list(range(plan.K)) if labels is None else list(labels)
    cka = cka_from_hsic(hsic, n)
    rows = []
    for a, ma in enumerate(plan.members):
        for b, mb in enumerate(plan.members):
            for li, layer in enumerate(LAYERS):
                rows.append(dict(member_a=int(ma), member_b=int(mb), label_a=labels[int(ma)], label_b=labels[int(mb)], layer=layer,
                                 rows_of=int(plan.rows_of), n=int(n), hsic=float(hsic[a, b, li]), cka=float(cka[a, b, li])))
    return pd.DataFrame(rows)


def similarity_matrix(frame, layer="h2", n_members=None):
    """The K x K CKA table of one layer of a `similarity_frame`; NaN for members outside the panel."""
    import pandas as pd
    if layer not in LAYERS:
        raise ValueError("similarity_matrix: layer = %r, one of %s wanted" % (layer, ", ".join(repr(v) for v in LAYERS)))
    K = int(max(frame["member_a"].max(), frame["member_b"].max())) + 1 if n_members is None else int(n_members)
    m = np.full((K, K), np.nan)
    sub = frame[frame["layer"] == layer]
    for a, b, v in zip(sub["member_a"], sub["member_b"], sub["cka"]):
        m[int(a), int(b)] = float(v)
    return pd.DataFrame(m, index=range(K), columns=range(K))


def similarity_matrices(frame, n_members=None):
    """Both layers' `similarity_matrix` under one another, the layer as the outer index (what `evaluate --similarity` prints)."""
    import pandas as pd
    return pd.concat({layer: similarity_matrix(frame, layer, n_members) for layer in LAYERS})


def unit_frame(mean, var, n, plan, labels=None):
    """The census of hidden units that comes free from the accumulators, `mean` / `var` [M][2][H]: one row per (member, layer) with
    `units`, `dead_units` (variance below 1e-8 on the counted rows), `saturated_units` (|mean| above 0.99) and `mean_abs_activation`
    (the mean over the units of |mean activation|); NaN / zero counts with n < 2."""
    import pandas as pd
    labels = list(range(plan.K)) if labels is None else list(labels)
    rows = []
    for a, ma in enumerate(plan.members):
        for li, layer in enumerate(LAYERS):
            ok = int(n) >= 2
            rows.append(dict(member=int(ma), label=labels[int(ma)], layer=layer, n=int(n), units=int(mean.shape[2]),
                             dead_units=int((var[a, li] < DEAD_VARIANCE).sum()) if ok else 0,
                             saturated_units=int((np.abs(mean[a, li]) > SATURATED_MEAN).sum()) if ok else 0,
                             mean_abs_activation=float(np.abs(mean[a, li]).mean()) if ok else float("nan")))
    return pd.DataFrame(rows)


def similarity_rows(algo, env, weights_list, rows_of=None, members=None, share=0.5, scenes_per_pair=4, num_agents=40, steps=1000, seed=0,
                    labels=None, max_bytes=1 << 30, **extra):
    """The K populations `weights_list` (one layout) on the `SeatPlan.pairs` layout of `cross_play_rows`, compared by linear CKA of both
    hidden layers on the states the scenes visit: every acted row of every pair's scenes, or with `rows_of` = k only the rows member k
    drives, for `steps` env steps (rounded up to whole fragments).  `members`: the panel (default: all).  Returns the
    `similarity_frame`: one row per (member a, member b, layer)."""
    def check():
        K = len(list(weights_list))
        if K < 2:
            raise ValueError("similarity_rows: %d member, at least two wanted" % K)
        if rows_of is not None and not 0 <= int(rows_of) < K:
            raise ValueError("similarity_rows: rows_of = %r of %d members" % (rows_of, K))

    weights_list = list(weights_list)
    return run_pairs("similarity_rows", algo, env, weights_list,
                     lambda t, bank, seats, use_graph: SimilaritySeatSampler(
                         t.env, t.policy, bank, seats, SimilarityPlan(seats, members, rows_of, max_bytes=max_bytes), t.sampler.T, use_graph=use_graph),
                     lambda smp, seats, labels: smp.frame(labels),
                     share=share, scenes_per_pair=scenes_per_pair, num_agents=num_agents, steps=steps, seed=seed, labels=labels, extra=extra,
                     check=check)


def cka_of(bank, obs):
    """dict(n, hsic, cka, mean, var) of every member pair of `bank` on the rows of obs [n][O] (every row counts): the hidden launch, one
    accumulate and the finish."""
    import torch
    n = int(obs.shape[0])
    plan = SimilarityPlan(SeatPlan(np.zeros((1, n), np.int32), bank.K))
    H = int(bank.cfg.hidden)
    plan.check_bytes(H)
    hidden = hidden_activations(bank, obs)
    acc = SimilarityAccumulators(plan.M, H, plan.planes(H), obs.device)
    cka_accumulate(hidden, torch.from_numpy(plan.members.copy()).to(obs.device), *every_row(n, obs.device), acc.S, acc.s, acc.n)
    return acc.finish()
