"""Premises of test_gpu_sim_config_parity.py, on the oracle alone (no GPU): with the seeds, actions and setter calls of the GPU
cases (tests/sim_config_cases.py) the configurations really take the branches those cases are there for -- a bit-exact comparison
of two simulators that both never enter a branch would pass vacuously.  The thresholds are conditions on the inputs, not tolerances."""
import numpy as np
import pytest

import sim_config_cases as sc


def _first_difference(a, b, keys):
    for t, (x, y) in enumerate(zip(a, b)):
        if any(not np.array_equal(x[k].view(np.uint32) if x[k].dtype == np.float32 else x[k],
                                  y[k].view(np.uint32) if y[k].dtype == np.float32 else y[k]) for k in keys):
            return t - 1                          # record 0 is the reset, record t + 1 is step t
    return None


@pytest.mark.parametrize("N,lasers", sorted({(N, lasers) for _, _, _, N, lasers, _ in sc.VISIBLE_SHAPES}))
def test_visible_buildings_change_the_lidar_and_nothing_else(N, lasers):
    """Buildings the LiDAR sees against buildings it does not, same actions: the same flags at every step (the agents end alike), and
    plenty of LiDAR cells that differ -- what the parity cases compare is not an idle branch."""
    E = 3
    vis = sc.oracle_rollout(sc.visible_config(E, N, lasers, 1), sc.STEPS_A)
    hid = sc.oracle_rollout(sc.visible_config(E, N, lasers, 2), sc.STEPS_A)
    cols = sc.lidar_cols(sc.visible_config(E, N, lasers))
    cells = 0
    for t, (v, h) in enumerate(zip(vis, hid)):
        assert np.array_equal(v["flags"], h["flags"]), t
        present = (v["flags"] & 0x41) != 0            # rows of absent slots are not written
        cells += int((v["obs"][..., cols][present].view(np.uint32) != h["obs"][..., cols][present].view(np.uint32)).sum())
    print("%d beams, %d agents: %d LiDAR cells differ" % (lasers, N, cells))
    assert cells >= sc.VISIBLE_MIN_CELLS[lasers], cells


def _knob(name):
    return next(c for c in sc.knob_cases() if c[0] == name)


def _knob_rollout(name, **override):
    _, map_name, N, kw, sigma = _knob(name)
    kw = dict(kw, **override)
    return sc.oracle_rollout(sc.sim_config(map_name, sc.KNOB_E, N, **kw), sc.STEPS_B, sigma, sc.KNOB_CALLS.get(name))


def test_friction_limit_changes_the_observations_early():
    t = _first_difference(_knob_rollout("lat_acc_max3"), _knob_rollout("lat_acc_max3", lat_acc_max=0.0), ("obs",))
    print("lat_acc_max 3 against 0: observations first differ at step", t)
    assert t is not None and t <= 60, t


def test_respawn_cooldown_changes_the_flags():
    t = _first_difference(_knob_rollout("respawn_cooldown8"), _knob_rollout("respawn_cooldown8", respawn_cooldown=0), ("flags",))
    print("respawn_cooldown 8 against 0: flags first differ at step", t)
    assert t is not None and t <= 90, t


@pytest.mark.parametrize("name,other", [("substeps2", dict(substeps=5)), ("substeps7", dict(substeps=5)),
                                        ("lidar_counterclockwise", dict(lidar_clockwise=True)), ("body_margin0", dict(body_margin=1.0)),
                                        ("body_margin0", dict(body_margin=0.75)), ("body_margin1", dict(body_margin=0.75)),
                                        ("mf6_nbr25", dict(mf_distance=10.0, neighbours_distance=40.0))])
def test_knob_changes_the_rollout(name, other):
    keys = ("obs", "flags", "mf_cnt", "nbr_cnt") if name == "mf6_nbr25" else ("obs", "flags")
    _, map_name, N, kw, sigma = _knob(name)
    a = sc.oracle_rollout(sc.sim_config(map_name, sc.KNOB_E, N, **kw), sc.STEPS_B, sigma, keys=keys)
    b = sc.oracle_rollout(sc.sim_config(map_name, sc.KNOB_E, N, **dict(kw, **other)), sc.STEPS_B, sigma, keys=keys)
    t = _first_difference(a, b, keys)
    print("%s against %r: first difference at step %r" % (name, other, t))
    assert t is not None


def test_round5_scene_differs_from_the_default_tollgate():
    _, map_name, N, kw, sigma = _knob("tollgate_round5")
    a = sc.oracle_rollout(sc.sim_config(map_name, sc.KNOB_E, N, **kw), sc.STEPS_B, sigma, keys=("obs", "flags", "rew"))
    b = sc.oracle_rollout(sc.sim_config(map_name, sc.KNOB_E, N), sc.STEPS_B, sigma, keys=("obs", "flags", "rew"))
    assert _first_difference(a, b, ("rew",)) is not None and _first_difference(a, b, ("flags",)) is not None


def test_forced_lcf_is_what_spawning_agents_draw():
    """set_force_lcf(0.5) before the reset, -0.8 at step 30, back to the distribution's mean at 60, set_lcf_dist(0.4, 0.3) at 80."""
    rec = _knob_rollout("forced_lcf")
    cfg = sc.sim_config("intersection", sc.KNOB_E, 30)

    def mean_lcf(steps, mask_bits):
        v = np.concatenate([rec[t + 1]["lcf"][(rec[t + 1]["flags"] & mask_bits) != 0] for t in steps])
        return float(v.mean()), len(v)

    m0, n0 = mean_lcf(range(5, 30), 0x41)              # everybody present was spawned under the forced 0.5
    print("present agents, steps 5..29: mean lcf %.4f over %d" % (m0, n0))
    assert n0 > 500 and abs(m0 - 0.5) < 0.1, (m0, n0)
    # agents present after step 70 were spawned under 0.5, -0.8, the mean 0 and (from 80) 0.4: the mean over the PRESENT ones is no
    # statement about the forced value being lifted (it drifts from +0.17 at step 60 to -0.43 at step 92 as the early agents leave).
    # What is one: the LCF of the agents that SPAWN under each setting.
    m1, n1 = mean_lcf(range(30, 60), 0x40)
    m2, n2 = mean_lcf(range(61, 80), 0x40)
    m3, n3 = mean_lcf(range(81, sc.STEPS_B), 0x40)
    print("spawned 30..59: %.4f over %d; 61..79: %.4f over %d; 81..: %.4f over %d" % (m1, n1, m2, n2, m3, n3))
    assert n1 >= 8 and abs(m1 - (-0.8)) < 0.1, (m1, n1)
    assert n2 >= 8 and abs(m2 - cfg.lcf_mean) < 0.1, (m2, n2)      # (std 0.1: the mean of 8 draws is within 0.1 at 2.8 sigma)
    assert n3 >= 1, n3        # somebody draws from (0.4, 0.3) too; at std 0.3 a handful of draws says nothing about the mean
    col = cfg.lcf_col                                  # the observation column carries (lcf + 1) / 2 of the same draw
    t = 20
    present = (rec[t + 1]["flags"] & 0x41) != 0
    assert np.array_equal(rec[t + 1]["obs"][..., col][present], ((rec[t + 1]["lcf"] + np.float32(1.0)) * np.float32(0.5))[present])


def test_captured_step_schedule_is_drawn_from():
    """The captured-step case (3 eager steps, then 120 + 20 replays with setter calls at replays 40, 60, 80): agents spawn under every
    setting, every scene is reset after the last one, and capacity 20 leaves slots 20.. without spawns."""
    calls = {r + 3: c for r, c in sc.GRAPH_CALLS.items()}
    rec = sc.oracle_rollout(sc.sim_config("intersection", sc.GRAPH_E, sc.GRAPH_N, horizon=sc.GRAPH_HORIZON), 3 + sc.GRAPH_STEPS + sc.GRAPH_EXTRA, calls=calls)
    spawned = [int(((r["flags"] & 64) != 0).sum()) for r in rec[1:]]
    counts = [sum(spawned[3 + a:3 + b]) for a, b in ((0, 40), (40, 60), (60, 80), (80, sc.GRAPH_STEPS + sc.GRAPH_EXTRA))]
    print("spawns per setting:", counts)
    assert all(c > 0 for c in counts), counts
    late = rec[1 + 3 + 80:]
    assert np.logical_or.reduce([(r["flags"] & 128).any(1) for r in late]).all()                   # every scene is reset ...
    assert counts[3] >= sc.GRAPH_E * 20 and not any((r["flags"][:, 20:] & 64).any() for r in late)      # ... into capacity 20
    lifted = np.concatenate([r["lcf"][(r["flags"] & 64) != 0] for r in late])
    assert abs(float(lifted.mean()) - 0.4) < 0.1, lifted.mean()              # set_lcf_dist(0.4, 0.3) again, 80 draws at std 0.3
    forced = np.concatenate([r["lcf"][(r["flags"] & 64) != 0] for r in rec[1 + 3 + 60:1 + 3 + 80]])
    assert (forced > 0.0).all() and abs(float(forced.mean()) - 0.5) < 0.3, forced        # drawn around the forced 0.5 at std 0.3


def test_crafted_building_poses_do_what_they_are_named_for():
    """The crafted scenes of the GPU file on the oracle: which poses have a beam shortened by a building (visible against hidden
    buildings on the same state), which body touches one."""
    import oracle_lib as ol
    outs = {}
    for b in (1, 2):
        cfg = sc.visible_config(sc.CRAFT_E, sc.CRAFT_N, 72, b)
        o = ol.OracleSim(cfg)
        o.reset(sc.seeds(sc.CRAFT_E))
        st, env = o.get_state()
        st = st.copy()
        named = sc.crafted_building_scenes(cfg, st)
        o.set_state(st, env)
        out = o.step(sc.crafted_actions())
        outs[b] = {k: out[k].copy() for k in ("obs", "flags")}
        o.close()
    cols = sc.lidar_cols(cfg)
    assert np.array_equal(outs[1]["flags"], outs[2]["flags"]) and not (outs[1]["flags"] & 128).any()      # no scene was reset
    vis, hid = outs[1]["obs"][..., cols], outs[2]["obs"][..., cols]
    assert (vis <= hid).all()
    shortened = {k: int((vis[e, n] < hid[e, n]).sum()) for k, (e, n) in named.items()}
    print(shortened)
    for k in ("reach_in_long", "reach_in_short", "parallel_along", "parallel_across", "parallel_end_face", "behind_vehicle",
              "before_building", "touching", "clear"):
        assert shortened[k] > 0, (k, shortened)
    # on the cull radius the nearest face is range + min(half_len, half_wid) away: nothing to see on either side of it
    for k in shortened:
        if k.startswith("cull_") or k.startswith("reach_out") or k == "parallel_along_back":
            assert shortened[k] == 0, (k, shortened)
    named_set = set(named.values())
    far = np.array([[(e, n) not in named_set and n < sc.CRAFT_N - sc.CRAFT_KEEP for n in range(sc.CRAFT_N)] for e in range(sc.CRAFT_E)])
    assert np.array_equal(vis[far], hid[far]) and (vis[far] == 1.0).all()                 # (e): far from everything
    # the minimum in both orders: behind the blocker some beams return the vehicle (hidden run already short, unchanged) and some the
    # building; before the building every beam towards the vehicle behind it returns the building first
    e, n = named["behind_vehicle"]
    assert ((hid[e, n] < 1.0) & (vis[e, n] == hid[e, n])).any() and ((hid[e, n] == 1.0) & (vis[e, n] < 1.0)).any()
    e, n = named["before_building"]
    assert (hid[e, n] < 1.0).any() and (vis[e, n][hid[e, n] < 1.0] < hid[e, n][hid[e, n] < 1.0]).all()
    fl = outs[1]["flags"]
    assert fl[named["touching"]] & 8 and not fl[named["clear"]] & 8                      # COPO_F_CRASH through the building loop
