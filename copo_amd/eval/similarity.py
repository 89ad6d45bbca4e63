"""Representation similarity: linear centred kernel alignment (CKA) between the hidden layers of bank members on the same states.

The other studies of seated evaluation compare what checkpoints DO; `jury.py` compares the outputs of two checkpoints on the same
states.  Here what they compute inside: is a 0.3 nat gap between CoPO and IPPO a different head on the same features, or a different
first layer?  Are two seeds with a large weight distance the same network up to a permutation of hidden units?  Linear CKA of the
activations of two nets on the same inputs,
    cka(a, b) = hsic(a, b) / sqrt(hsic(a, a) hsic(b, b)),    hsic(a, b) = || Ha^T Hb - (1^T Ha)^T (1^T Hb) / n ||_F^2,
is invariant to permutation, rotation and isotropic scaling of the units, which weight distance and unit-by-unit correlation are not.

A `SimilarityPlan` is a panel of members that all read the same rows: the seated rows of the scene groups of a seat plan (internally a
`JuryPlan.panel`, so every member's list is the one common ascending list).  Per env step `copo_hidden_obs_seats_f32`
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

from .crossplay import SeatPlan, SeatSampler, run_pairs
from .jury import JuryBuffers, JuryPlan

LAYERS = ("h1", "h2")
CHUNK, PROMOTE_ROWS, MAX_PLANES, MAX_PANEL, MAX_HIDDEN, TILE = 32, 128, 8, 255, 512, 64      # include/copo_hip.h, COPO_CKA_*
DEAD_VARIANCE, SATURATED_MEAN = 1e-8, 0.99
FILL_WORKGROUPS = 256          # the row split stops once the Gram launch has this many workgroups: one per compute unit of the target


class SimilarityPlan:
    """A panel of bank members compared on the seated rows of the seat plan `seats`.  `members`: the panel, bank members in the order of
    the tables (default: all K; otherwise at least two distinct members).  `rows_of`: None, or the member whose DRIVEN rows alone are
    counted.  Derived: `jury`, the `JuryPlan.panel` whose lists the hidden launch reads (every panel member's list is `rows`, the one
    common ascending list of the seated rows e * N + n of the groups in [0, G); `count`, `cap`); `pairs` int32 [P][2], the unordered
    pairs a <= b of PANEL indices in the accumulators' order; `planes(hidden)`, the fixed row split R of the accumulators (a power of
    two up to 8: doubled while the Gram launch has fewer than 256 workgroups and every plane still gets a chunk of 32 rows -- a property
    of the plan, never of the device); `accumulator_bytes(hidden)`.  `check_bytes(hidden)` refuses accumulators beyond `max_bytes`
    (default 1 GiB) with the figure; it runs at construction where `hidden` is given.  Nothing here touches a device."""

    def __init__(self, seats, members=None, rows_of=None, hidden=None, max_bytes=1 << 30):
        members = list(range(seats.K)) if members is None else [int(m) for m in members]
        if members != list(range(seats.K)) and len(members) < 2:
            raise ValueError("SimilarityPlan: a panel of %d, at least two members wanted" % len(members))
        if len(members) > MAX_PANEL:
            raise ValueError("SimilarityPlan: a panel of %d, %d at the most" % (len(members), MAX_PANEL))
        self.jury = JuryPlan.panel(seats, members)          # (refuses members outside the bank and duplicates)
        self.members, self.M, self.K = np.asarray(members, np.int32), len(members), seats.K
        self.rows_of = -1 if rows_of is None else int(rows_of)
        if rows_of is not None and not 0 <= self.rows_of < seats.K:
            raise ValueError("SimilarityPlan: rows_of = %r of a bank of %d" % (rows_of, seats.K))
        first = members[0]
        self.rows, self.count, self.cap = self.jury.rows[first], int(self.jury.counts[first]), self.jury.cap
        self.pairs = np.array([(a, b) for a in range(self.M) for b in range(a, self.M)], np.int32)
        self.P = len(self.pairs)
        self.E, self.N, self.n_out, self.G = seats.E, seats.N, seats.E * seats.N, seats.n_groups
        self.max_bytes = int(max_bytes)
        if hidden is not None:
            self.check_bytes(hidden)

    def check(self, seats):
        self.jury.check(seats)
        return self

    def planes(self, hidden):
        tiles, chunks, R = self.P * 2 * (int(hidden) // TILE) ** 2, -(-self.cap // CHUNK), 1
        while R < MAX_PLANES and tiles * R < FILL_WORKGROUPS and 2 * R <= chunks:
            R *= 2
        return R

    def accumulator_shapes(self, hidden):
        H, R = int(hidden), self.planes(hidden)
        return dict(S=(R, self.P, 2, H, H), s=(R, self.M, 2, H), n=(R,))

    def accumulator_bytes(self, hidden):
        return 8 * sum(int(np.prod(shape)) for shape in self.accumulator_shapes(hidden).values())

    def check_bytes(self, hidden):
        H = int(hidden)
        if H < TILE or H > MAX_HIDDEN or H % TILE:
            raise ValueError("SimilarityPlan: hidden = %d, a multiple of %d up to %d wanted" % (H, TILE, MAX_HIDDEN))
        need = self.accumulator_bytes(H)
        if need > self.max_bytes:
            raise ValueError("SimilarityPlan: %d pairs x 2 layers x %d x %d float64 in %d planes are %d bytes of accumulators, max_bytes = %d" % (
                self.P, H, H, self.planes(H), need, self.max_bytes))
        return need


def _want(who, name, t, shape, dtype):
    if t is None or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != dtype:
        raise ValueError("%s: %s of shape %s and dtype %s, contiguous %s %s wanted" % (
            who, name, None if t is None else tuple(t.shape), None if t is None else t.dtype, dtype, list(shape)))


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
    _want(who, "hidden", hidden, (K, cap, 2, H), torch.float32)
    _want(who, "panel", panel, (M,), torch.int32)
    _want(who, "rows", rows, (cap,), torch.int64)
    _want(who, "count", count, (1,), torch.int32)
    _want(who, "flags", flags, flags.shape, torch.uint8)
    _want(who, "seat", seat, seat.shape, torch.int32)
    _want(who, "S", S, (R, P, 2, H, H), torch.float64)
    _want(who, "s", s, (R, M, 2, H), torch.float64)
    _want(who, "n", n, (R,), torch.int64)
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
    _want(who, "S", S, (R, M * (M + 1) // 2, 2, H, H), torch.float64)
    _want(who, "s", s, (R, M, 2, H), torch.float64)
    _want(who, "n", n, (R,), torch.int64)
    _want(who, "hsic", hsic, (M, M, 2), torch.float64)
    _want(who, "n_out", n_out, (1,), torch.int64)
    _want(who, "mean", mean, (M, 2, H), torch.float64)
    _want(who, "var", var, (M, 2, H), torch.float64)
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


class SimilaritySeatSampler(SeatSampler):
    """`SeatSampler` with a similarity panel: per env step `hidden_seats` on the observation the policy reads, the seated forward on the
    same observation, the simulator step, the seat tally and `cka_accumulate` of the step's flags -- the whole fragment is still one
    captured graph.  Actions, flags and the seat tally are a plain `SeatSampler`'s.  `acc` (`SimilarityAccumulators`) accumulates until
    `clear_tally()`; `read()` issues the finish and returns its numbers, `frame()` / `units()` the tables."""

    def __init__(self, vec_env, policy, bank, plan, similarity, T, use_graph=True):
        import torch
        similarity.check(plan)
        H = int(bank.cfg.hidden)
        similarity.check_bytes(H)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.similarity = similarity
        self.jury_buffers = JuryBuffers(similarity.jury, self.device)
        self.jury_buffers.on_replace.append(self._loop.reset)
        self.panel = torch.from_numpy(similarity.members.copy()).to(self.device)
        self.hidden = torch.zeros(bank.K, similarity.cap, 2, H, dtype=torch.float32, device=self.device)
        self.acc = SimilarityAccumulators(similarity.M, H, similarity.planes(H), self.device)
        first = int(similarity.members[0])
        self._rows, self._count = self.jury_buffers.rows[first], self.jury_buffers.counts[first:first + 1]

    def clear_tally(self):
        super().clear_tally()
        self.acc.clear()

    def _policy_obs(self, t):
        obs = super()._policy_obs(t)
        self.seated.hidden_seats(self.jury_buffers, obs.view(-1, self.O), self.hidden)
        return obs

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


def cka_of(bank, obs):
    """dict(n, hsic, cka, mean, var) of every member pair of `bank` on the rows of obs [n][O] (every row counts): the hidden launch, one
    accumulate and the finish."""
    import torch
    n = int(obs.shape[0])
    plan = SimilarityPlan(SeatPlan(np.zeros((1, n), np.int32), bank.K))
    H = int(bank.cfg.hidden)
    plan.check_bytes(H)
    hidden = hidden_activations(bank, obs)
    dev = obs.device
    acc = SimilarityAccumulators(plan.M, H, plan.planes(H), dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cka_accumulate(hidden, up(plan.members), up(plan.rows), up(np.array([plan.count], np.int32)), torch.ones(n, dtype=torch.uint8, device=dev),
                   torch.zeros(n, dtype=torch.int32, device=dev), -1, acc.S, acc.s, acc.n)
    return acc.finish()
