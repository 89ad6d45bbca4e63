"""The influence graph on the GPU (copo_influence_*, copo_amd/eval/influence.py).  The counterfactual rows are held
to the simulator itself, in BITS: the clean row is the simulator's own LiDAR block, a variant row is the observation of a second
simulator with that vehicle emptied.  The forward is the jury's, compared in bits; the fold's integer words equal tests/influence_numpy.py
exactly, its KL word within one unit per pair (as tests/test_gpu_jury.py treats the jury's).  Scenes and outputs are computed once."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

import bank_cases as bc
import influence_cases as ic
import influence_numpy as inf
import sim_truth_cases as tc
import sim_truth_numpy as truth

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

F = np.float32
POISON = ic.POISON


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _crafted_step(case, st_env=None, edit=None):
    """A fresh simulator of the case, its crafted state (after `edit`) set, ONE step of brake actions.  Returns (sim, obs [E N][O])."""
    from copo_amd.sim import VecSim
    g = VecSim(case.cfg)
    g.reset()
    st, env = g.get_state()
    st, env = case.state(st.cpu().numpy(), env.cpu().numpy())
    if edit is not None:
        edit(st)
    g.set_state(torch.from_numpy(st).cuda(), torch.from_numpy(env).cuda())
    out = g.step(torch.from_numpy(tc.brake_actions(case.cfg)).cuda())
    torch.cuda.synchronize()
    return g, out["obs"].reshape(g.E * g.N, g.O).clone()


def _all_seated(cfg):
    from copo_amd.eval.crossplay import SeatPlan
    return SeatPlan(np.zeros((cfg.num_envs, cfg.num_agents), np.int32), 1)


def _alive(g):
    st, _ = g.get_state()
    return ((st[13].view(torch.int32) & 0xFF) == truth.ALIVE).reshape(-1).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _crafted(name, M=4):
    from copo_amd.eval.influence import influence_obs
    case = tc.get_case(name)
    g, obs = _crafted_step(case)
    try:
        res = {k: v.cpu().numpy() for k, v in influence_obs(g, _all_seated(case.cfg), obs, M).items()}
        return dict(case=case, obs=obs.cpu().numpy(), alive=_alive(g), col=truth.obs_columns(case.cfg)["lidar"],
                    lcf=g.get_state()[0][10].cpu().numpy(), **res)
    finally:
        g.close()


def _check_clean(tag, obs, col, L, clean, ego, alive, stats):
    assert np.array_equal(ego != 0, alive), tag                                   # every row is seated: the egos are the ALIVE slots
    block = _u32(obs[:, col:col + L])
    assert np.array_equal(_u32(clean)[alive], block[alive]), "%s: the clean row is not the simulator's LiDAR block" % tag
    stats["below"] += int((obs[alive, col:col + L] < 1.0).sum())


@pytest.mark.parametrize("name", ["lidar-intersection", "lidar-tollgate-visible", "lidar-parkinglot"])
def test_clean_row_is_the_simulators_lidar_block_on_crafted_scenes(name):
    """(1) After the one step `clean` equals the simulator's LiDAR block bit for bit on every ego; the variants of a beam's owner hold
    something behind it."""
    c = _crafted(name)
    L, stats = c["case"].cfg.num_lasers, dict(below=0)
    _check_clean(name, c["obs"], c["col"], L, c["clean"], c["ego"], c["alive"], stats)
    assert stats["below"] > 0 and c["alive"].sum() >= c["case"].cfg.num_envs
    assert (c["kept"][c["alive"]] >= 2).any()                                     # some ego has at least two candidates
    assert not c["kept"][~c["alive"]].any() and (c["who"][~c["alive"]] == -1).all()
    # some beam has min2 < range behind its owner: a variant row differs from the clean row on it and is still below 1
    M, behind = c["who"].shape[1], 0
    cf = c["obs_cf"].reshape(-1, M, c["obs"].shape[1])[:, :, c["col"]:c["col"] + L]
    for r in np.nonzero(c["kept"] > 0)[0]:
        for k in range(c["kept"][r]):
            moved = _u32(cf[r, k]) != _u32(c["clean"][r])
            assert moved.any() and (cf[r, k][moved] > c["clean"][r][moved]).all(), (name, r, k)          # a candidate owns a beam; min2 >= min1
            behind += int((cf[r, k][moved] < 1.0).sum())
    print(name, "beams below range:", stats["below"], "beams with something behind the owner:", behind)
    if name != "lidar-parkinglot":
        assert behind > 0


def _rollout(steps=20, E=4, N=12, M=4, seed=5):
    """Random actions on the Intersection; the heading launch before every step.  Yields (t, sim, buffers, obs [E N][O]) at every step."""
    from copo_amd.eval.influence import InfluenceBuffers, influence_heading
    from copo_amd.sim import SimConfig, VecSim
    cfg = SimConfig(map="intersection", num_envs=E, num_agents=N, horizon=500)
    g = VecSim(cfg)
    try:
        b = InfluenceBuffers(_all_seated(cfg), g.O, cfg.num_lasers, M, "cuda")
        rng = np.random.RandomState(seed)
        obs = g.reset()["obs"]
        for t in range(steps + 1):
            torch.cuda.synchronize()
            yield t, g, b, obs.reshape(E * N, g.O).clone()
            act = _dev(np.stack([rng.normal(0, 0.3, (E, N)), rng.uniform(-0.2, 1.0, (E, N))], -1).astype(F))
            influence_heading(g, b, act)
            obs = g.step(act)["obs"]
    finally:
        g.close()


def test_clean_row_on_a_rollout_of_moving_vehicles():
    """(1, rollout) 20 steps of random actions on the Intersection with 12 slots: the clean row is the simulator's LiDAR block at the
    reset and after every step, vehicles that turn while they drive included (the heading launch keeps the step's own vectors)."""
    from copo_amd.eval.influence import influence_obs
    stats, two, moving = dict(below=0), 0, 0
    for t, g, b, obs in _rollout():
        res = {k: v.cpu().numpy() for k, v in influence_obs(g, b.seats, obs, buffers=b).items()}
        col = truth.obs_columns(g.cfg)["lidar"]
        _check_clean("step %d" % t, obs.cpu().numpy(), col, g.cfg.num_lasers, res["clean"], res["ego"], _alive(g), stats)
        two += int((res["kept"] >= 2).sum())
        st, _ = g.get_state()
        moving += int((st[3].abs() > 1.0).sum())
    print("rollout: beams below range %d, egos with two candidates or more %d, slot-steps faster than 1 m/s %d" % (stats["below"], two, moving))
    assert stats["below"] > 0 and two > 0 and moving > 0


def test_removal_against_the_simulator_itself():
    """(2) One ego of the ring of 23 targets (the ring's own centre vehicle touches its nearest target and ends as a wreck, so the ego is
    the surviving vehicle of that scene that has the most owners): for every other vehicle of the scene a second simulator runs the same
    scene with that slot emptied.  Its observation row of the ego equals the variant row bit for bit, all columns, for every kept
    candidate; the owners are the vehicles whose removal changes the row, and `truncated` is exactly owners - 4."""
    c = _crafted("lidar-intersection")
    case, N, M = c["case"], c["case"].cfg.num_agents, 4
    n_ego = int(np.argmax(np.where(c["alive"][:N - 1], c["truncated"][:N - 1], -1)))          # scene 0; not the keeper
    r = n_ego
    assert c["alive"][r] and c["kept"][r] == M and c["truncated"][r] > 0
    targets = [j for j in list(range(len(case.scenes[0]))) + [N - 1] if j != n_ego]
    ring = dataclasses.replace(case, cfg=dataclasses.replace(case.cfg, num_envs=len(targets)), scenes=[case.scenes[0]] * len(targets))

    def state(st, env):          # the ring scene in every scene, vehicle targets[e] emptied in scene e, the keeper as the case sets it
        st, env = tc.Case.state(ring, st, env)
        iw = st.view(np.int32)
        k = tc.spawn_vehicle(case.cfg.tables(), 0)
        st[0, :, N - 1], st[1, :, N - 1], st[2, :, N - 1] = k.x, k.y, k.th
        st[3:10, :, N - 1] = 0.0
        iw[12, :, N - 1], iw[13, :, N - 1] = k.route | (k.road << 16), truth.ALIVE
        for e, j in enumerate(targets):
            iw[13, e, j] = 0
            st[0:4, e, j] = 0.0
            iw[12, e, j] = 0
        st[10] = c["lcf"][0][None, :]          # (the LCF word is the reset's draw, per scene: the ego's own observation column)
        return st, env
    ring.state = state
    g2, obs2 = _crafted_step(ring)
    g2.close()
    obs2 = obs2.cpu().numpy().reshape(len(targets), N, -1)
    base = _u32(c["obs"][r])
    owners = [j for e, j in enumerate(targets) if not np.array_equal(_u32(obs2[e, n_ego]), base)]
    cf = c["obs_cf"].reshape(-1, M, c["obs"].shape[1])
    for k in range(M):
        j = int(c["who"][r, k])
        assert j in owners, (k, j)
        assert np.array_equal(_u32(cf[r, k]), _u32(obs2[targets.index(j), n_ego])), "variant %d (slot %d) is not the simulator's row without it" % (k, j)
    print("ring: ego slot %d, %d owners among %d vehicles, kept %s, truncated %d" % (n_ego, len(owners), len(targets), c["who"][r].tolist(), c["truncated"][r]))
    assert c["truncated"][r] == len(owners) - M


def test_candidates_are_in_the_order_of_the_float64_models_nearest_hit():
    """(3) Targets at radii 3 m apart in scrambled slot order: `who` lists them by the float64 model's nearest owned hit over the stable
    beams."""
    from copo_amd.eval.influence import influence_obs
    cfg = tc._cfg("intersection", 1, 10)
    t = cfg.tables()
    ego, keeper = tc.spawn_vehicle(t, 7), tc.spawn_vehicle(t, 0)                  # an ego on its road: it comes through the step alive
    c0, h = (ego.x, ego.y), ego.th
    radii = [15.0, 6.0, 21.0, 9.0, 18.0, 12.0]
    scene = [ego]
    for k, rad in enumerate(radii):
        b = h + math.radians(20.0 + 57.0 * k)
        scene.append(tc.V(c0[0] + rad * math.cos(b), c0[1] + rad * math.sin(b), 0.3 + 0.9 * k))
    case = tc._finish("influence-order", cfg, [scene], keeper)
    g, obs = _crafted_step(case)
    try:
        res = {k: v.cpu().numpy() for k, v in influence_obs(g, _all_seated(cfg), obs, 8).items()}
    finally:
        g.close()
    T = truth.step_truth(cfg, t, case.state(np.zeros((16, 1, 10), F), np.zeros((1, 4), np.int32))[0])
    rel = truth.lidar_rel_angles(cfg)
    slots = list(range(1, 7)) + [cfg.num_agents - 1]                              # the targets and the keeper
    others = scene[1:] + [keeper]
    pos = np.array([[v.x, v.y] for v in others])
    ang = np.array([v.th for v in others])
    d = truth.ray_box(np.array(c0)[None, None], (h + rel)[:, None], pos[None], ang[None], tc.HL, tc.HW)[0]          # [beam][vehicle]
    d = np.where(d < cfg.lidar_range, d, np.inf)
    stable = T["lidar_stable"][0, 0]
    nearest = {}
    for bm in np.nonzero(stable & np.isfinite(d.min(-1)))[0]:
        j = slots[int(d[bm].argmin())]
        nearest[j] = min(nearest.get(j, np.inf), d[bm].min())
    order = sorted(nearest, key=nearest.get)
    gaps = np.diff([nearest[j] for j in order])
    print("order:", order, "nearest owned hits:", [round(nearest[j], 3) for j in order])
    n = len(order)
    assert set(range(1, 7)) <= set(order) and gaps.min() > 0.1                    # far beyond what fp32 and the choice of beams could swap
    assert res["ego"][0] and res["kept"][0] == n and res["truncated"][0] == 0
    assert res["who"][0, :n].tolist() == order and (res["who"][0, n:] == -1).all()
    assert np.allclose(res["hit"][0, :n] * cfg.lidar_range, [nearest[j] for j in order], atol=1e-3)


@functools.lru_cache(maxsize=None)
def _pass_case(golden_dir):
    """The rollout's last scene under a two-member seat plan: one `influence_pass` on poisoned outputs."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    from copo_amd.eval.influence import InfluenceBuffers, influence_pass
    for t, g, b, obs in _rollout():
        if t < 20:
            continue
        E, N, M = g.E, g.N, b.M
        seat = (np.arange(E * N).reshape(E, N) % 3 - 1).astype(np.int32)          # -1, 0, 1 in turn
        seat[3] = 1                                                               # a scene of one member
        plan = SeatPlan(seat, 2, np.array([0, 1, 1, 0], np.int32), 2)
        bank = PolicyBank(_policy("ippo", g.O, 64, False), bc.members(golden_dir, "ippo_inter", g.O, 64, 2))
        bank.sync_mirror()
        pb = PlanBuffers(plan, "cuda")
        ib = InfluenceBuffers(plan, g.O, g.cfg.num_lasers, M, "cuda")
        ib.heading.copy_(b.heading)
        ib.verdict_cf.copy_(_poison(*ib.verdict_cf.shape))
        ib.obs_cf.copy_(_poison(*ib.obs_cf.shape))
        dist = torch.zeros(E * N, 4, device="cuda")
        bank.act_seats(pb, obs, torch.zeros(E * N, 2, device="cuda"), torch.zeros(E * N, 2, device="cuda"), torch.zeros(E * N, device="cuda"), dist)
        for _ in range(2):          # the tally accumulates
            influence_pass(g, bank, pb, ib, obs, dist, None, ic.DELTAS)
        torch.cuda.synchronize()
        keep = {k: getattr(ib, k).cpu().numpy() for k in ("who", "ncand", "ego", "obs_cf", "vrows", "vcounts", "verdict_cf", "edges", "tally", "hit")}
        return dict(plan=plan, bank=bank, dist=dist.cpu().numpy(), alive=_alive(g), M=M, **keep)


def test_forward_and_fold(golden_dir):
    """(4) verdict_cf on the listed rows is `jury_verdicts(bank, obs_cf)` on them in bits, every other entry keeps the poison; the lists
    are influence_numpy's; the eight words are influence_numpy's from the device's own p / q."""
    from copo_amd.eval.influence import edges_array
    from copo_amd.eval.jury import jury_verdicts
    c = _pass_case(golden_dir)
    plan, M = c["plan"], c["M"]
    kept, trunc = c["ncand"] & 0xffff, c["ncand"] >> 16
    seated = plan.seat.reshape(-1) >= 0
    assert np.array_equal(c["ego"] != 0, seated & c["alive"]) and not kept[~(seated & c["alive"])].any()
    vrows, vcounts = inf.variant_lists(plan.rows, plan.counts, kept, M)
    assert np.array_equal(c["vcounts"], vcounts) and vcounts.min() > 0
    for k in range(2):
        assert np.array_equal(c["vrows"][k, :vcounts[k]], vrows[k, :vcounts[k]])
    obs_cf = c["obs_cf"].copy()
    obs_cf[_u32(obs_cf) == POISON] = 0.0
    every = jury_verdicts(c["bank"], _dev(obs_cf)).cpu().numpy()
    listed = np.zeros((len(obs_cf), 2), bool)
    for k in range(2):
        listed[vrows[k, :vcounts[k]], k] = True
    got = _u32(c["verdict_cf"])
    assert np.array_equal(got[listed], _u32(every)[listed]) and (got[~listed] == POISON).all()
    written = np.repeat(kept, M).reshape(-1, M) > np.arange(M)[None]
    assert (_u32(c["obs_cf"]).reshape(len(kept), M, -1)[~written] == POISON).all()          # variant rows that do not exist are left alone
    q = c["verdict_cf"].copy()
    q[~listed] = 0.0
    want = inf.fold(c["ego"], c["dist"], q, c["who"], trunc, plan.seat, plan.group, 2, 2, ic.DELTAS)
    tally = c["tally"]
    exact = [0, 1, 2, 3, 4, 7]
    assert np.array_equal(tally[..., exact], 2 * want[..., exact]) and np.array_equal(tally[..., 6], want[..., 6])
    off = np.abs(tally[..., 5] - 2 * want[..., 5])
    print("pairs %d, moved %d, truncated %d; KL word off by at most %d units (bound %d)" % (
        want[..., 1].sum(), want[..., 2].sum(), want[..., 7].sum(), off.max(), 2 * want[..., 1].max()))
    assert (off <= 2 * want[..., 1]).all() and (tally[..., 5] % 2 == 0).all()
    assert want[..., 0].min() > 0 and want[..., 1].sum() > 10 and want[..., 5].sum() > 0 and want[..., 6].max() > 0
    e = edges_array(c["who"], c["edges"], plan.N)
    assert len(e) == kept.sum() and (e["hit"] < 1.0).all() and (e["d_steer"] >= 0).all()
    r = e["scene"] * plan.N + e["ego_slot"]
    assert (c["ego"][r] != 0).all() and (e["other_slot"] != e["ego_slot"]).all()


@pytest.mark.parametrize("shape", ic.TALLY_SHAPES, ids=str)
def test_tally_alone_is_exact(shape):
    """(4, the fold alone) `copo_influence_tally` on random tables (influence_cases.tally_tables: out-of-range groups, empty seats, a scene
    of one member, candidate holes, truncated counts, NaN and beyond-clamp verdicts, rows without ACTED), folded twice: the integer words
    are twice influence_numpy's, the max word is its max, the KL word within one unit per pair and fold (`test_forward_and_fold`'s bound
    and reason: the device's exp differs from numpy's by an ulp, which can move a value across a rounding boundary of q16).  The edges of
    the counted candidates hold the model's d0, d1 and the hit; every other edge keeps its poison."""
    from copo_amd import _capi
    E, N, K, G, M = shape
    t = ic.tally_tables(shape)
    want = inf.fold(t["flags"], t["dist"], t["verdict_cf"], t["who"], t["ncand"] >> 16, t["seat"], t["group"], K, G, ic.DELTAS)
    assert want[..., 1].sum() > 0 and 0 < want[..., 2].sum() < want[..., 1].sum() and want[..., 7].sum() > 0 and want[..., 6].max() == 1024 * 65536
    d = {k: _dev(v) for k, v in t.items()}
    out = torch.zeros(G, K, 8, dtype=torch.int64, device="cuda")
    edges = _poison(E * N, M, 4)
    for _ in range(2):          # the tally accumulates
        _capi.check(_capi.lib.copo_influence_tally(d["flags"].data_ptr(), d["dist"].data_ptr(), d["verdict_cf"].data_ptr(), d["who"].data_ptr(),
                                                   d["ncand"].data_ptr(), d["hit"].data_ptr(), d["seat"].data_ptr(), d["group"].data_ptr(), E, N, K, G, M,
                                                   ic.DELTAS[0], ic.DELTAS[1], out.data_ptr(), edges.data_ptr(), _capi.current_stream()))
    torch.cuda.synchronize()
    tally, edges = out.cpu().numpy(), edges.cpu().numpy()
    exact = [0, 1, 2, 3, 4, 7]
    off = np.abs(tally[..., 5] - 2 * want[..., 5])
    print(shape, "egos %d pairs %d moved %d truncated %d; KL word off by at most %d units (bound %d)" % (
        want[..., 0].sum(), want[..., 1].sum(), want[..., 2].sum(), want[..., 7].sum(), off.max(), 2 * want[..., 1].max()))
    assert np.array_equal(tally[..., exact], 2 * want[..., exact]) and np.array_equal(tally[..., 6], want[..., 6])
    assert (off <= 2 * want[..., 1]).all() and (tally[..., 5] % 2 == 0).all()
    seat = t["seat"].reshape(-1)
    ok = np.repeat((t["group"] >= 0) & (t["group"] < G), N)
    counted = ok & (seat >= 0) & ((t["flags"] & inf.F_ACTED) != 0)
    written = counted[:, None] & (t["who"] >= 0)
    assert written.any() and not written.all() and (_u32(edges)[~written] == POISON).all()
    r, c = np.nonzero(written)
    own, v = t["dist"][r], t["verdict_cf"][r * M + c, seat[r]]
    with np.errstate(invalid="ignore"):
        d0, d1 = np.abs(F(v[:, 0] - own[:, 0])), np.abs(F(v[:, 1] - own[:, 1]))
    assert np.array_equal(edges[r, c, 0], d0, equal_nan=True) and np.array_equal(edges[r, c, 1], d1, equal_nan=True)
    assert np.array_equal(edges[r, c, 3], t["hit"][r, c]) and (np.isnan(d0) | np.isnan(d1)).any()


def test_nobody_near(golden_dir):
    """(5) One vehicle per scene: no candidates, empty lists, words 1 .. 7 zero, obs_cf and verdict_cf untouched."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers, SeatPlan
    from copo_amd.eval.influence import InfluenceBuffers, influence_pass
    from copo_amd.sim import SimConfig, VecSim
    cfg = SimConfig(map="intersection", num_envs=5, num_agents=1, horizon=500)
    g = VecSim(cfg)
    try:
        obs = g.reset()["obs"].reshape(5, g.O).clone()
        plan = SeatPlan(np.array([[0], [1], [0], [1], [1]], np.int32), 2)
        bank = PolicyBank(_policy("ippo", g.O, 64, False), bc.members(golden_dir, "ippo_inter", g.O, 64, 2))
        bank.sync_mirror()
        ib = InfluenceBuffers(plan, g.O, cfg.num_lasers, 4, "cuda")
        ib.verdict_cf.copy_(_poison(*ib.verdict_cf.shape))
        ib.obs_cf.copy_(_poison(*ib.obs_cf.shape))
        ib.vcounts.fill_(7)
        influence_pass(g, bank, PlanBuffers(plan, "cuda"), ib, obs, torch.zeros(5, 4, device="cuda"), None, ic.DELTAS)
        torch.cuda.synchronize()
        assert ib.vcounts.tolist() == [0, 0] and ib.ego.tolist() == [1] * 5 and int(ib.ncand.abs().sum()) == 0 and int(ib.who.max()) == -1
        assert ib.tally[0, :, 0].tolist() == [2, 3] and int(ib.tally[..., 1:].abs().sum()) == 0
        assert (_u32(ib.obs_cf) == POISON).all() and (_u32(ib.verdict_cf) == POISON).all()
        assert (ib.clean == 1.0).all()
    finally:
        g.close()


def _fragments(smp, n_frag, keys, seed=3):
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    keep = []
    for _ in range(n_frag):
        smp.sample()
        torch.cuda.synchronize()
        keep.append({k: (getattr(smp.influence, k[5:]) if k.startswith("infl_") else getattr(smp, k)).clone() for k in keys})
    return keep


def test_sampler_captured_equals_eager_and_the_drive_is_untouched(golden_dir):
    """(6) A captured fragment gives the tally of the eager one; the batch and the seat tally are a plain `SeatSampler`'s bit for bit on
    the same seeds; two runs give identical `vrows`; the clean rows of the last step are the simulator's LiDAR block (the sampler keeps
    the headings across steps and fragments)."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import SeatPlan, SeatSampler
    from copo_amd.eval.evaluate import make_eval_trainer
    from copo_amd.eval.influence import InfluenceSeatSampler, influence_edges
    N, T = 8, 4
    plan = SeatPlan.pairs(2, 1, N, 0.5)
    t = make_eval_trainer("copo", "inter", plan.E, N, 0)
    try:
        bank = PolicyBank(_policy("copo", t.sampler.O, 64, False), bc.members(golden_dir, "copo_inter", t.sampler.O, 64, 2))
        drive = ("tally", "actions", "clipped", "flags", "obs", "dist_inputs", "logp")
        keys = drive + ("infl_tally", "infl_vrows", "infl_vcounts", "infl_who", "infl_clean", "infl_edges")
        runs = {}
        for mode in (False, True, "again"):
            smp = InfluenceSeatSampler(t.env, t.policy, bank, plan, T, use_graph=bool(mode), max_others=3, deltas=ic.DELTAS)
            smp._loop.warmup = 0          # capture at the first fragment: both fragments replay
            runs[mode] = _fragments(smp, 3, keys)
            assert (smp._loop.graph is not None) == bool(mode)
        for f in range(3):
            for k in keys:
                a, b = runs[False][f][k], runs[True][f][k]
                if k == "infl_vrows":          # (beyond the counts the lists hold what earlier steps left)
                    for m in range(2):
                        n = int(runs[True][f]["infl_vcounts"][m])
                        assert torch.equal(a[m, :n], b[m, :n]) and torch.equal(b[m, :n], runs["again"][f][k][m, :n]), (f, k)
                else:
                    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (f, k)
                    assert torch.equal(b.view(torch.uint8), runs["again"][f][k].view(torch.uint8)), (f, k)
        plain = _fragments(SeatSampler(t.env, t.policy, bank, plan, T, use_graph=False), 3, drive)
        for f in range(3):
            for k in drive:
                assert torch.equal(plain[f][k].view(torch.uint8), runs[True][f][k].view(torch.uint8)), (f, k)          # the drive is untouched
        last = runs[True][2]
        col, L = truth.obs_columns(t.sampler.sim.cfg)["lidar"], int(t.sampler.sim.cfg.num_lasers)
        ego = (last["flags"][T - 1].reshape(-1).cpu().numpy() & 1) != 0          # every seat is taken: an ego at obs[T - 1] acts in the step after it
        block = _u32(last["obs"][T - 1].reshape(plan.E * N, -1)[:, col:col + L])
        assert ego.any() and np.array_equal(_u32(last["infl_clean"])[ego], block[ego])
        tally = last["infl_tally"].cpu().numpy()
        seat_tally = last["tally"].cpu().numpy()
        assert np.array_equal(tally[..., 0], seat_tally[..., 0]) and tally[..., 1].sum() > 0          # an ego is a seat that acts
        assert len(influence_edges(smp.influence)) == int((smp.influence.who >= 0).sum())
        smp.clear_tally()
        assert int(smp.influence.tally.abs().sum()) == 0 and int(smp.tally.abs().sum()) == 0
        graph = smp._loop.graph
        smp.set_deltas((0.1, 0.2))
        assert graph is not None and smp._loop.graph is None and smp.deltas == (0.1, 0.2)
    finally:
        t.stop()
