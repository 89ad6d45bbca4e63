"""An influence graph: whose presence moves whose action.

`jury.py` says how far two policies are apart on the same states, the LiDAR studies how a policy reacts to a corrupted sensor.  Here what
CoPO is about: which neighbour a driver reacts to, and how strongly.  A policy learns of other vehicles only through the LiDAR block of
its observation row (SPEC 3.4), so the effect of vehicle j on driver i has an exact counterfactual: i's row with j taken out of the scene.

The rule (restated by tests/influence_numpy.py).  An EGO is a seated row whose slot is ALIVE.  Per beam, `min1` is
the minimum over the static boxes and the other vehicles, its OWNER the vehicle that attains it strictly below the boxes (ties: the lower
slot), `min2` the minimum over everything but the owner.  The CANDIDATES of an ego are the owners of at least one beam, by (smallest
owned distance, slot); the first `max_others` = M are kept, the rest counted as truncated.  Variant c of row r is row r M + c of `obs_cf`:
obs[r] with min2 on the beams the candidate owns.  A vehicle that owns nothing is occluded: removing it changes no bit.

Per env step five launches.  Before the forward's step: `copo_influence_obs` (one pass over the pairs for all M + 1 observations),
`copo_influence_lists` (the variant rows of every member's seats, ascending), `copo_jury_obs_seats_f32` UNCHANGED on the lists -- so a
variant's four numbers are the bits the seat forward would write for that member on that row -- and `copo_influence_tally` into eight
int64 words per (scene group, member), `INFLUENCE_WORDS`.  Right before the simulator step: `copo_influence_heading`, which keeps the
heading unit vectors the step is about to give the vehicles; the step's LiDAR reads them and the simulator's state does not hold them,
so the NEXT pass needs them to repeat that LiDAR bit for bit.  After `VecSim.set_state` clear them (`InfluenceBuffers.clear_heading`).

Pieces: `InfluenceBuffers`, `influence_pass`, `influence_heading`, `influence_obs` (the first launch alone, on plain arrays),
`InfluenceSeatSampler` (one captured graph; the drive, the batch and the seat tally are a plain `SeatSampler`'s), `influence_rates` /
`influence_frame`, `influence_edges` and `influence_rows` (`evaluate --influence`).
"""
import numpy as np

from .bank import DeviceTables
from .crossplay import SeatPlan, SeatSampler, run_pairs
from .jury import Q16, check_deltas

INFLUENCE_WORDS = ("egos", "pairs", "moved", "d_steer_q16", "d_throttle_q16", "kl_q16", "max_dev_q16", "truncated")
EDGE_WORDS = ("d_steer", "d_throttle", "kl", "hit")
EDGE_DTYPE = np.dtype([("scene", np.int32), ("ego_slot", np.int32), ("other_slot", np.int32), ("d_steer", np.float32),
                       ("d_throttle", np.float32), ("kl", np.float32), ("hit", np.float32)])
MAX_OTHERS = 8          # COPO_INFL_MAX


def check_max_others(who, max_others):
    M = int(max_others)
    if M != max_others or not 1 <= M <= MAX_OTHERS:
        raise ValueError("%s: max_others = %r, an integer in 1..%d wanted" % (who, max_others, MAX_OTHERS))
    return M


class InfluenceBuffers(DeviceTables):
    """What the influence pass writes, sized from a `SeatPlan`, the row width O, the beams L and M = `max_others`, allocated ONCE: a
    captured graph holds the addresses.  `who` int32 [n_out][M] (-1 = none), `ncand` int32 [n_out] (kept | truncated << 16), `ego` uint8
    [n_out] (COPO_F_ACTED on an ego), `hit` [n_out][M], `clean` [n_out][L], `obs_cf` [n_out M][O], `vrows` int64 [K][cap M], `vcounts`
    int32 [K], `verdict_cf` [n_out M][K][4], `edges` [n_out][M][4] (`EDGE_WORDS`), `heading` [n_out][2] and `tally` int64 [G][K][8]
    (`INFLUENCE_WORDS`; accumulates until `clear_tally`).  `verdict_cf` entries that no list names keep what they held."""
    KEY = ("K", "cap", "E", "N", "G", "M", "O", "L")
    seats = property(lambda self: self.source[0])
    n_out = property(lambda self: self.E * self.N)

    def __init__(self, seats, O, L, max_others=4, device="cuda"):
        M = check_max_others("InfluenceBuffers", max_others)
        if not isinstance(seats, SeatPlan):
            raise ValueError("InfluenceBuffers: a SeatPlan wanted, not %r" % (type(seats).__name__,))
        if int(O) < 1 or int(L) < 1 or int(L) > int(O):
            raise ValueError("InfluenceBuffers: O = %r columns with L = %r beams" % (O, L))
        if seats.cap * M >= 2 ** 31:
            raise ValueError("InfluenceBuffers: %d seats x %d variants per member, fewer than 2^31 wanted" % (seats.cap, M))
        super().__init__((seats, int(O), int(L), M), device)

    @staticmethod
    def tables(source):
        p, O, L, M = source
        n = p.E * p.N
        z = lambda *s, dtype=np.float32: np.zeros(s, dtype)  # noqa: E731
        return dict(who=np.full((n, M), -1, np.int32), ncand=z(n, dtype=np.int32), ego=z(n, dtype=np.uint8), hit=z(n, M), clean=z(n, L),
                    obs_cf=z(n * M, O), vrows=z(p.K, p.cap * M, dtype=np.int64), vcounts=z(p.K, dtype=np.int32), verdict_cf=z(n * M, p.K, 4),
                    edges=z(n, M, 4), heading=z(n, 2), tally=z(p.n_groups, p.K, len(INFLUENCE_WORDS), dtype=np.int64)), (
                        p.K, p.cap, p.E, p.N, p.n_groups, M, O, L)

    def clear_tally(self):
        self.tally.zero_()

    def clear_heading(self):
        """Forget the kept heading vectors (after `VecSim.set_state`): the next pass reads sin / cos of the stored headings."""
        self.heading.zero_()


def _check_sim(who, sim, buffers):
    if (sim.E, sim.N, sim.O, int(sim.cfg.num_lasers)) != (buffers.E, buffers.N, buffers.O, buffers.L):
        raise ValueError("%s: buffers for %d x %d rows of %d columns and %d beams, the simulator has %d x %d of %d and %d" % (
            who, buffers.E, buffers.N, buffers.O, buffers.L, sim.E, sim.N, sim.O, int(sim.cfg.num_lasers)))


def influence_heading(sim, buffers, act):
    """BEFORE the step that reads `act` [E][N][act_dim]: `buffers.heading` := the heading unit vectors that step will give the vehicles.
    One launch on the current stream."""
    _check_sim("influence_heading", sim, buffers)
    sim._capi.check(sim._capi.lib.copo_influence_heading(sim._h, act.data_ptr(), buffers.heading.data_ptr(), sim._capi.current_stream()))


def _obs_launch(sim, seat, buffers, obs):
    b = buffers
    sim._capi.check(sim._capi.lib.copo_influence_obs(sim._h, seat.data_ptr(), b.heading.data_ptr(), obs.data_ptr(), b.M, b.who.data_ptr(),
                                                     b.obs_cf.data_ptr(), b.ncand.data_ptr(), b.ego.data_ptr(), b.hit.data_ptr(),
                                                     b.clean.data_ptr(), sim._capi.current_stream()))


def influence_pass(sim, bank, plan_buffers, buffers, obs, dist, flags=None, deltas=(0.05, 0.05)):
    """The four launches of one step on the current stream: the counterfactual rows of `obs` [n_out][O] (the simulator's state must be
    the one that wrote it), the members' variant lists, the bank's jury forward on them and the fold of the variants against the drivers'
    own `dist` [n_out][4] into `buffers.tally` and `buffers.edges`.  `flags` uint8 [n_out]: which rows count (COPO_F_ACTED); None: the
    egos the first launch found.  The bank's mirror must be in step (`sync_mirror`)."""
    import torch
    pb, b = plan_buffers, buffers
    _check_sim("influence_pass", sim, b)
    if (pb.K, pb.cap, pb.E, pb.N, pb.G) != (b.K, b.cap, b.E, b.N, b.G) or bank.K != b.K:
        raise ValueError("influence_pass: a plan of %d members (cap %d) on %d x %d seats in %d groups, buffers for %d (cap %d) on %d x %d in %d, "
                         "a bank of %d" % (pb.K, pb.cap, pb.E, pb.N, pb.G, b.K, b.cap, b.E, b.N, b.G, bank.K))
    for name, t, numel, dtype in (("obs", obs, b.n_out * b.O, torch.float32), ("dist", dist, b.n_out * 4, torch.float32),
                                  ("flags", flags, b.n_out, torch.uint8)):
        if t is not None and (t.numel() != numel or not t.is_contiguous() or t.dtype != dtype):
            raise ValueError("influence_pass: %s of shape %s, %d contiguous %s wanted" % (name, tuple(t.shape), numel, dtype))
    lib, st = sim._capi.lib, sim._capi.current_stream()
    _obs_launch(sim, pb.seat, b, obs)
    sim._capi.check(lib.copo_influence_lists(pb.rows.data_ptr(), pb.counts.data_ptr(), b.K, b.cap, b.n_out, b.ncand.data_ptr(), b.M,
                                             b.vrows.data_ptr(), b.vcounts.data_ptr(), st))
    import ctypes as C
    sim._capi.check(lib.copo_jury_obs_seats_f32(C.byref(bank.cfg), bank.theta.data_ptr(), bank.theta_t.data_ptr(), bank.stride, bank.K,
                                                b.vrows.data_ptr(), b.vcounts.data_ptr(), b.cap * b.M, b.n_out * b.M, b.obs_cf.data_ptr(),
                                                b.verdict_cf.data_ptr(), st))
    sim._capi.check(lib.copo_influence_tally((b.ego if flags is None else flags).data_ptr(), dist.data_ptr(), b.verdict_cf.data_ptr(),
                                             b.who.data_ptr(), b.ncand.data_ptr(), b.hit.data_ptr(), pb.seat.data_ptr(), pb.group.data_ptr(),
                                             b.E, b.N, b.K, b.G, b.M, float(deltas[0]), float(deltas[1]), b.tally.data_ptr(), b.edges.data_ptr(), st))


def influence_obs(sim, seats, obs, max_others=4, heading=None, buffers=None):
    """The first launch alone, on plain arrays: `seats` a `SeatPlan` (or an int [E][N] seat table), `obs` [E N][O] on the device, written
    by the simulator's last step or reset.  `heading` [E N][2]: what `influence_heading` kept before that step (None: `buffers`' own, or
    nothing kept -- exact for vehicles that stood still).  `buffers`: `InfluenceBuffers` to write into (default: new ones of
    `max_others`).  Returns a dict of device tensors: `who`, `kept`, `truncated`, `ego`, `hit`, `clean`, `obs_cf`."""
    import torch
    if not isinstance(seats, SeatPlan):
        seats = SeatPlan(np.asarray(seats))
    b = InfluenceBuffers(seats, sim.O, int(sim.cfg.num_lasers), max_others, obs.device) if buffers is None else buffers
    _check_sim("influence_obs", sim, b)
    if (seats.E, seats.N) != (b.E, b.N) or obs.numel() != b.n_out * b.O or not obs.is_contiguous() or obs.dtype != torch.float32:
        raise ValueError("influence_obs: %d x %d seats and obs of shape %s, contiguous float32 [%d, %d] wanted" % (
            seats.E, seats.N, tuple(obs.shape), b.n_out, b.O))
    if heading is not None:
        b.heading.copy_(heading.view(b.n_out, 2))
    seat = torch.from_numpy(np.ascontiguousarray(seats.seat)).to(obs.device)
    _obs_launch(sim, seat, b, obs)
    torch.cuda.current_stream().synchronize()          # (the seat table dies with this call)
    return dict(who=b.who, kept=b.ncand & 0xffff, truncated=b.ncand >> 16, ego=b.ego, hit=b.hit, clean=b.clean, obs_cf=b.obs_cf)


class InfluenceSeatSampler(SeatSampler):
    """`SeatSampler` with the influence pass: per env step the seated forward, `influence_pass` on the observation and the distribution
    inputs it just read and wrote, `influence_heading` on the clipped action, the simulator step and the seat tally -- the whole fragment
    is still one captured graph.  Actions, flags and the seat tally are a plain `SeatSampler`'s.  `influence.tally` int64 [G][K][8]
    (`INFLUENCE_WORDS`) accumulates until `clear_tally()`; `influence.edges` / `who` hold the fragment's last step (`influence_edges`)."""

    def __init__(self, vec_env, policy, bank, plan, T, use_graph=True, max_others=4, deltas=(0.05, 0.05)):
        self.deltas = check_deltas("InfluenceSeatSampler", deltas)
        M = check_max_others("InfluenceSeatSampler", max_others)
        super().__init__(vec_env, policy, bank, plan, T, use_graph=use_graph)
        self.influence = InfluenceBuffers(plan, self.O, int(self.sim.cfg.num_lasers), M, self.device)
        self.seated.on_replace.append(self._replan)

    def _replan(self):
        self.influence.replace((self.seated.plan, self.O, self.influence.L, self.influence.M))

    def set_deltas(self, deltas):
        """Other thresholds, OUTSIDE captured graphs: they are launch arguments, so the graph is dropped."""
        self.deltas = check_deltas("InfluenceSeatSampler.set_deltas", deltas)
        self._loop.reset()

    def clear_tally(self):
        super().clear_tally()
        self.influence.clear_tally()

    def reset(self, seeds=None):
        super().reset(seeds)
        self.influence.clear_heading()

    def _act(self, t):
        super()._act(t)
        influence_pass(self.sim, self.seated.bank, self.seated.buffers, self.influence, self.obs[t].view(-1, self.O),
                       self.dist_inputs[t], None, self.deltas)

    def _step(self, t):
        influence_heading(self.sim, self.influence, self.clipped[t])
        super()._step(t)


def influence_rates(words):
    """The derived columns of one tally cell (the eight `INFLUENCE_WORDS`): `others_per_ego` = pairs / egos, `moved_rate` = moved / pairs,
    the means `mean_d_steer`, `mean_d_throttle`, `mean_kl` over the pairs, `max_dev`, `truncated_rate` = truncated / (pairs + truncated);
    NaN where a denominator is 0."""
    w = dict(zip(INFLUENCE_WORDS, (int(v) for v in words)))
    ratio = lambda a, b: float(a) / float(b) if b > 0 else float("nan")  # noqa: E731
    n = w["pairs"]
    return dict(others_per_ego=ratio(n, w["egos"]), moved_rate=ratio(w["moved"], n), mean_d_steer=ratio(w["d_steer_q16"] / Q16, n),
                mean_d_throttle=ratio(w["d_throttle_q16"] / Q16, n), mean_kl=ratio(w["kl_q16"] / Q16, n),
                max_dev=w["max_dev_q16"] / Q16 if n > 0 else float("nan"), truncated_rate=ratio(w["truncated"], n + w["truncated"]))


def influence_frame(tally, seats, labels=None, deltas=None):
    """The influence tally [G][K][8] (numpy int64) as a frame: one row per (group, member seated in it).  Columns: `group` (a `pairs` plan:
    also `focal`, `partner`), `member`, `label`, `delta_steer` / `delta_throttle` where `deltas` is given, the eight raw words
    (`INFLUENCE_WORDS`) and `influence_rates`."""
    import pandas as pd
    labels = list(range(seats.K)) if labels is None else list(labels)
    rows = []
    for g in range(seats.n_groups):
        in_group = seats.seat[seats.group == g]
        pair = {} if seats.focal is None else dict(focal=int(seats.focal[g]), partner=int(seats.partner[g]))
        for k in (k for k in range(seats.K) if (in_group == k).any()):
            w = [int(v) for v in tally[g, k]]
            rows.append(dict(group=g, **pair, member=k, label=labels[k],
                             **({} if deltas is None else dict(delta_steer=float(deltas[0]), delta_throttle=float(deltas[1]))),
                             **dict(zip(INFLUENCE_WORDS, w)), **influence_rates(w)))
    return pd.DataFrame(rows)


def edges_array(who, edges, N):
    """`who` int [n_out][M] and `edges` float [n_out][M][4] (numpy) as the structured array of `influence_edges`."""
    who = np.asarray(who)
    r, c = np.nonzero(who >= 0)
    out = np.zeros(len(r), EDGE_DTYPE)
    out["scene"], out["ego_slot"], out["other_slot"] = r // N, r % N, who[r, c]
    for k, name in enumerate(EDGE_WORDS):
        out[name] = np.asarray(edges)[r, c, k]
    return out


def influence_edges(buffers):
    """The directed graph of the last pass: a structured numpy array (`EDGE_DTYPE`), one entry "ego <- other" per kept candidate:
    `scene`, `ego_slot`, `other_slot`, `d_steer`, `d_throttle`, `kl`, `hit` (the candidate's smallest owned distance over the range)."""
    return edges_array(buffers.who.cpu().numpy(), buffers.edges.cpu().numpy(), buffers.N)


def influence_rows(algo, env, weights_list, share=0.5, max_others=4, deltas=(0.05, 0.05), scenes_per_pair=4, num_agents=40, steps=1000, seed=0,
                   labels=None, **extra):
    """The K populations `weights_list` (one layout) on the `SeatPlan.pairs` layout of `cross_play_rows` with the influence pass, for
    `steps` env steps (rounded up to whole fragments).  Returns the `influence_frame`: one row per (pair, member)."""
    return run_pairs("influence_rows", algo, env, weights_list,
                     lambda t, bank, seats, use_graph: InfluenceSeatSampler(t.env, t.policy, bank, seats, t.sampler.T, use_graph=use_graph,
                                                                            max_others=max_others, deltas=deltas),
                     lambda smp, seats, labels: influence_frame(smp.influence.tally.cpu().numpy(), seats, labels, smp.deltas),
                     share=share, scenes_per_pair=scenes_per_pair, num_agents=num_agents, steps=steps, seed=seed, labels=labels, extra=extra,
                     check=lambda: (check_deltas("influence_rows", deltas), check_max_others("influence_rows", max_others)))
