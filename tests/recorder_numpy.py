"""The rules of the device evaluation recorder (include/copo_hip.h `copo_recorder_*`) restated in plain float64
numpy: a python loop over scenes and steps, numpy over the slots.  All 29 columns of `copo_amd.eval.device_recorder.COLUMNS` -- the 25
of `VecRecorder` by its own rules, then the SVO estimate of the reference's RecorderEnv (copo/eval/recoder.py:49-70, 326-347) -- from
the five tensors of a fragment; the state of every scene and slot is carried across calls.  No torch.

Sums over slots take the device's fixed tree (csrc/recorder_common.h): lane l adds its slots l, l + 64, ... in ascending order onto
+0.0, then six butterfly stages at lane distances 32 ... 1."""
import numpy as np

F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = (1 << i for i in range(8))
I_VELOCITY, I_COST, I_EPISODE_LENGTH, I_EPISODE_REWARD = 0, 4, 5, 6

COLUMNS = ("velocity_step_mean_episode_min", "velocity_step_mean_episode_mean", "velocity_step_mean_episode_max",
           "num_neighbours_mean_episode_mean", "num_neighbours_mean_episode_max", "num_agents_total",
           "num_agents_total_per_300_steps", "success_rate", "num_agents_success", "num_agents_success_per_300_steps",
           "num_agents_failed_per_300_steps", "episode_reward_mean", "episode_reward_min", "episode_reward_max",
           "episode_cost_mean", "episode_cost_min", "episode_cost_max", "episode_cost_sum", "crash_rate", "num_agents_crash",
           "out_rate", "num_agents_out", "episode_length_mean", "success_episode_length_mean", "env_episode_steps",
           "svo_estimate_deg_mean", "svo_estimate_deg_min", "svo_estimate_deg_max", "svo_reward")
NCOL = len(COLUMNS) + 2          # + scene, + episode index of the scene
EXACT = ("velocity_step_mean_episode_min", "velocity_step_mean_episode_max", "num_neighbours_mean_episode_max", "num_agents_total",
         "num_agents_success", "episode_reward_min", "episode_reward_max", "episode_cost_min", "episode_cost_max", "num_agents_crash",
         "num_agents_out", "env_episode_steps", "svo_estimate_deg_min", "svo_estimate_deg_max")
_LANES = np.arange(64)


def tree_sum(x):
    """Sum of float64 [N] in the device's order."""
    x = np.asarray(x, np.float64)
    k = -(-len(x) // 64)
    pad = np.zeros(64 * k)
    pad[:len(x)] = x
    v = np.zeros(64)
    for row in pad.reshape(k, 64):
        v = v + row
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ d]
    return float(v[0])


def _armed():
    a = dict.fromkeys(("steps", "vsteps", "vsum", "nsteps", "nsum", "agents", "succ", "crash", "out", "rsum", "csum", "lsum", "slsum",
                       "svo_n", "svo_sum", "svo_rew"), 0.0)
    a.update(vmin=np.inf, rmin=np.inf, cmin=np.inf, svo_min=np.inf, vmax=-np.inf, nmax=-np.inf, rmax=-np.inf, cmax=-np.inf, svo_max=-np.inf)
    return a


def _row(a, scene, episode):
    n, steps = a["agents"], max(a["steps"], 1.0)
    return np.array([
        a["vmin"], a["vsum"] / max(a["vsteps"], 1.0), a["vmax"], a["nsum"] / max(a["nsteps"], 1.0), a["nmax"], n, n / steps * 300.0,
        a["succ"] / n, a["succ"], a["succ"] / steps * 300.0, a["crash"] / steps * 300.0, a["rsum"] / n, a["rmin"], a["rmax"],
        a["csum"] / n, a["cmin"], a["cmax"], a["csum"], a["crash"] / n, a["crash"], a["out"] / n, a["out"], a["lsum"] / n,
        a["slsum"] / a["succ"] if a["succ"] > 0 else 0.0, a["steps"],
        a["svo_sum"] / a["svo_n"], a["svo_min"], a["svo_max"], a["svo_rew"] / n, float(scene), float(episode)], np.float64)


class RecorderNumpy:
    """`add(flags, infos, rewards, nei_rewards, nbr_cnt)` per fragment; `rows` float64 [n, NCOL] in (fragment, scene, step) order, at
    most `max_rows` of them, `dropped` the rest; `episodes` int64 [E]."""

    def __init__(self, E, N, max_rows=1 << 30, limit=0):
        self.E, self.N, self.max_rows, self.limit = int(E), int(N), int(max_rows), int(limit)
        self.reset()

    def clear(self):
        self._rows, self.dropped = [], 0

    def reset(self):
        self.clear()
        self.acc = [_armed() for _ in range(self.E)]
        self.cost, self.own, self.nei = (np.zeros((self.E, self.N)) for _ in range(3))
        self.episodes = np.zeros(self.E, np.int64)

    @property
    def rows(self):
        return np.array(self._rows, np.float64).reshape(-1, NCOL)

    def add(self, flags, infos, rewards, nei_rewards, nbr_cnt):
        flags, nbr_cnt = np.asarray(flags).astype(np.int64), np.asarray(nbr_cnt).astype(np.int64)
        infos, rewards, nei_rewards = (np.asarray(x).astype(np.float64) for x in (infos, rewards, nei_rewards))
        T = flags.shape[0]
        assert flags.shape == (T, self.E, self.N) and infos.shape == (T, self.E, self.N, 8)
        for e in range(self.E):
            cost, own, nei = self.cost[e], self.own[e], self.nei[e]
            for t in range(T):
                if self.limit > 0 and self.episodes[e] >= self.limit:
                    break
                a, f = self.acc[e], flags[t, e]
                resetting = bool(((f & F_ENV_RESET) > 0).any())
                acted = (f & F_ACTED) > 0
                present = acted | (((f & F_SPAWNED) > 0) & (not resetting))
                done = acted & ((f & F_DONE) > 0)
                a["steps"] += 1.0
                if acted.any():
                    vel = tree_sum(np.where(acted, infos[t, e, :, I_VELOCITY], 0.0)) / float(acted.sum())
                    a["vsteps"] += 1.0
                    a["vsum"] += vel
                    a["vmin"], a["vmax"] = min(a["vmin"], vel), max(a["vmax"], vel)
                if present.any():
                    nn = float(nbr_cnt[t, e][present].sum()) / float(present.sum())
                    a["nsteps"] += 1.0
                    a["nsum"] += nn
                    a["nmax"] = max(a["nmax"], nn)
                cost[acted] += infos[t, e, :, I_COST][acted]
                own[present] += rewards[t, e][present]
                nei[present] += np.where(nbr_cnt[t, e] > 0, nei_rewards[t, e], rewards[t, e])[present]
                if done.any():
                    won = done & ((f & F_ARRIVE) > 0)
                    er, el = infos[t, e, :, I_EPISODE_REWARD], infos[t, e, :, I_EPISODE_LENGTH]
                    alpha = np.degrees(np.arctan2(nei, own))
                    svo = np.clip(alpha, 0.0, 90.0)
                    w = np.hypot(nei, own) * np.cos(np.radians(svo - alpha))
                    a["agents"] += float(done.sum())
                    a["succ"] += float(won.sum())
                    a["crash"] += float((done & ((f & F_CRASH) > 0)).sum())
                    a["out"] += float((done & ((f & F_OUT) > 0)).sum())
                    a["rsum"] += tree_sum(np.where(done, er, 0.0))
                    a["csum"] += tree_sum(np.where(done, cost, 0.0))
                    a["lsum"] += tree_sum(np.where(done, el, 0.0))
                    a["slsum"] += tree_sum(np.where(won, el, 0.0))
                    a["rmin"], a["rmax"] = min(a["rmin"], er[done].min()), max(a["rmax"], er[done].max())
                    a["cmin"], a["cmax"] = min(a["cmin"], cost[done].min()), max(a["cmax"], cost[done].max())
                    a["svo_n"] += float(done.sum())
                    a["svo_sum"] += tree_sum(np.where(done, svo, 0.0))
                    a["svo_rew"] += tree_sum(np.where(done, w, 0.0))
                    a["svo_min"], a["svo_max"] = min(a["svo_min"], svo[done].min()), max(a["svo_max"], svo[done].max())
                    cost[done] = own[done] = nei[done] = 0.0
                if resetting:
                    if a["agents"] > 0:
                        if len(self._rows) < self.max_rows:
                            self._rows.append(_row(a, e, self.episodes[e]))
                        else:
                            self.dropped += 1
                    self.episodes[e] += 1
                    self.acc[e] = _armed()
