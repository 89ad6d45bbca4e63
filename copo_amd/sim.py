"""Vectorised multi-agent driving simulator handle (host side of `copo_sim_*`).

`VecSim` owns one `copo_sim` handle on one GPU and the output tensors of a step.  It is the
array-level interface; `copo_amd.torch_copo.utils.env_wrappers` layers the reference's dict-style
`MultiAgentEnv` surface on top of it.
"""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import maps as _maps
from ._handle import Handle

STATE_DIM, NAVI_DIM = 6, 10

# per-map observation options of MetaDrive 0.2.5's multi-agent environments (first-layer shapes of the reference's
# best_checkpoints: Intersection / Roundabout / ParkingLot 91, Bottleneck 96, Tollgate 156; +1 LCF column for CoPO)
MAP_OBS_DEFAULTS = dict(
    bottleneck=dict(side_lasers=4, side_range=50.0, lane_line_lasers=4, lane_line_range=20.0),
    # (MATollConfig: side detector 72 / 20 m, lane-line detector 4 / 20 m, LiDAR 72 / 20 m -- the LiDAR's 20 m were in the spec since round 3 and
    #  missing HERE until round 6: the scene ran with the other maps' 40 m, and the shipped populations read every obstacle at half its distance)
    tollgate=dict(side_lasers=72, side_range=20.0, lane_line_lasers=4, lane_line_range=20.0, navi_dim=0, toll_dim=2, lidar_range=20.0),
)


# per-map reward / termination rules that differ from MULTI_AGENT_METADRIVE_DEFAULT_CONFIG (MetaDrive 0.2.5 marl_tollgate.py: MATollConfig
# speed_reward 0.0, overspeed_penalty 0.5, TollGate.SPEED_LIMIT 3 km/h, an early exit is done_info["out_of_road"]).  Filled in after the
# round-6 experiments (profiles/r06_fidelity.txt); TOLLGATE_METADRIVE_RULES is the restated rule set either way.
TOLLGATE_METADRIVE_RULES = dict(speed_reward=0.0, toll_speed_limit=3.0 / 3.6, overspeed_penalty=0.5, toll_early_exit=1, toll_buildings=2)
# Round 6: ON for the Tollgate, with buildings that end an agent on touch and that the LiDAR does NOT see (toll_buildings = 2).  That is the one variant
# both of the reference's Tollgate records agree with (profiles/r06_fidelity.txt): the shipped IPPO population scores 0.00 in it -- IPPO's training
# success on 0.2.5 is 4.41 +- 2.56 %, so a file of such a run CANNOT score the 0.25 it reaches when it sees the buildings -- the CoPO population 0.28
# (table 27.19), and from scratch at the reference's batch structure CoPO trains to 24.1 +- 24.5 % (27.19 +- 25.63) where every visible-building or
# no-building variant trains to 80-96 %.  toll_buildings = 1: the LiDAR sees them; TOLLGATE_ROUND5_SCENE: rounds 2-5's scene.
MAP_RULE_DEFAULTS = dict(tollgate=TOLLGATE_METADRIVE_RULES)
TOLLGATE_ROUND5_SCENE = dict(speed_reward=0.1, toll_speed_limit=0.0, overspeed_penalty=0.0, toll_early_exit=0, toll_buildings=0, lidar_range=40.0)


@dataclass
class SimConfig:
    """Python mirror of `copo_sim_cfg` with the build's defaults."""
    map: str = "intersection"
    map_kwargs: dict = field(default_factory=dict)
    num_envs: int = 1
    num_agents: int = None            # default: the map's population (Inter 30, Round 40, ...)
    num_lasers: int = 72
    nbr_k: int = 8
    enable_lcf: bool = True
    horizon: int = 1000
    delay_done: int = 25
    respawn_cooldown: int = 0
    substeps: int = 5
    lidar_range: float = None          # None = the map's default: 40 m (MULTI_AGENT_METADRIVE_DEFAULT_CONFIG), 20 m on the Tollgate
    neighbours_distance: float = 40.0  # env_wrappers.py:168
    mf_distance: float = 10.0          # algo_ccppo.py:43
    dt: float = 0.1
    veh_half_len: float = 2.2575       # MetaDrive DefaultVehicle 4.515 x 1.852 m
    veh_half_wid: float = 0.926
    wheelbase: float = 2.4686          # front 1.05234 + rear 1.4166
    max_steer: float = math.radians(40.0)
    max_speed: float = 80.0 / 3.6
    acc_max: float = 2.9               # 4 wheels x max_engine_force 800 N / 1100 kg
    brake_gain: float = 27.0           # 4 wheels x max_brake_force 150 N s per 0.02 s physics step / 1100 kg ...
    brake_max: float = 8.8             # ... limited by tyre friction 0.9 g
    lat_acc_max: float = 0.0           # friction limit on v x yaw rate (0: none)
    reverse_acc: float = None          # reverse gear (MetaDrive enable_reverse): m/s^2 at full negative throttle; None / 0 = none
    spawn_region_len: float = 8.0      # SpawnManager.RESPAWN_REGION_LONGITUDE / LATERAL
    spawn_region_wid: float = 3.0
    driving_reward: float = 1.0
    speed_reward: float = None         # None = the map's default: 0.1 (MULTI_AGENT_METADRIVE_DEFAULT_CONFIG), MAP_RULE_DEFAULTS otherwise
    success_reward: float = 10.0
    crash_penalty: float = 10.0
    out_penalty: float = 10.0
    arrive_margin: float = 5.0
    body_margin: float = 0.75         # pinned by the reference populations: 0 = centre rule, 1 = whole body
    lane_width: float = 3.5
    lcf_mean: float = 0.0
    lcf_std: float = 0.1               # env_wrappers.py:176
    start_seed: int = 5000
    lidar_clockwise: bool = True       # beam k is turned k * 360 / n degrees clockwise of the heading (MetaDrive 0.2.5)
    # observation / action extensions of CCEnv / LCFEnv (env_wrappers.py:44-46); off by default like the reference
    add_traffic_light: bool = False
    traffic_light_interval: int = 30
    comm_size: int = 0                 # > 0 = communication on (comm_method != "none"): actions carry 2 + comm_size floats
    comm_neighbours: int = 4
    add_pos_in_comm: bool = False
    # MetaDrive's optional detectors; None = the map's default (MAP_OBS_DEFAULTS)
    side_lasers: int = None
    lane_line_lasers: int = None
    side_range: float = None
    lane_line_range: float = None
    navi_dim: int = None
    toll_dim: int = None
    toll_min_steps: int = 30
    # MultiAgentTollgateEnv's booth rules (copo_sim_cfg ABI 8; MetaDrive 0.2.5 marl_tollgate.py): speed limit on the booth road in m/s
    # (TollGate.SPEED_LIMIT = 3 km/h; 0 = no rule), its penalty factor, and what leaving the booth early is (0 crash, 1 out-of-road flag
    # with the ordinary step reward).  None = the map's default (MAP_RULE_DEFAULTS)
    toll_speed_limit: float = None
    overspeed_penalty: float = None
    toll_early_exit: int = None
    toll_buildings: int = None         # 2: as 1, but the LiDAR does not see them (experiment); 1: the map's static boxes are in the scene (Tollgate: booth buildings in every second booth lane,
                                       # TollGate._add_building_and_speed_limit): crash on touch, seen by the LiDAR

    def __post_init__(self):
        d = MAP_OBS_DEFAULTS.get(self.map, {})
        for k, dflt in (("side_lasers", 0), ("lane_line_lasers", 0), ("side_range", 20.0), ("lane_line_range", 20.0),
                        ("navi_dim", NAVI_DIM), ("toll_dim", 0), ("lidar_range", 40.0)):
            if getattr(self, k) is None:
                setattr(self, k, d.get(k, dflt))
        r = MAP_RULE_DEFAULTS.get(self.map, {})
        for k, dflt in (("speed_reward", 0.1), ("toll_speed_limit", 0.0), ("overspeed_penalty", 0.0), ("toll_early_exit", 0), ("toll_buildings", 0)):
            if getattr(self, k) is None:
                setattr(self, k, r.get(k, dflt))
        if self.reverse_acc is None:
            # no reverse gear anywhere by default.  (Later MetaDrive versions set vehicle_config["enable_reverse"] for the ParkingLot;
            # the population the reference ships for it drives the rebuilt scene better WITHOUT a reverse gear -- success 0.18 vs
            # 0.11, the reference's table has 0.17 -- so 0.2.5's env is taken to have none.  `reverse_acc = acc_max` switches it on.)
            self.reverse_acc = 0.0

    def tables(self):
        return _maps.MAP_BUILDERS[self.map](**self.map_kwargs)

    def resolved(self):
        t = self.tables()
        n = self.num_agents if self.num_agents is not None else t.default_num_agents
        return t, int(n)

    @property
    def comm_dim(self):
        return (self.comm_size + (3 if self.add_pos_in_comm else 0)) if self.comm_size > 0 else 0

    @property
    def ego_dim(self):
        return (self.side_lasers or 2) + STATE_DIM + (self.lane_line_lasers or 1)

    @property
    def obs_dim(self):
        """[side | 6 state | lane | navigation | lasers | toll | 3 traffic light | 1 lcf | comm] (COPO_OBS_DIM)."""
        return (self.ego_dim + self.navi_dim + self.num_lasers + self.toll_dim + (3 if self.add_traffic_light else 0)
                + (1 if self.enable_lcf else 0) + (self.comm_neighbours * self.comm_dim if self.comm_size > 0 else 0))

    @property
    def lcf_col(self):
        """Column of the (lcf + 1) / 2 entry (-1 without LCF)."""
        if not self.enable_lcf:
            return -1
        return self.ego_dim + self.navi_dim + self.num_lasers + self.toll_dim + (3 if self.add_traffic_light else 0)

    @property
    def act_dim(self):
        return 2 + max(0, self.comm_size)


def line_table(lines):
    """[n][8] = x0, y0, theta0, length, kappa, kind -> [n][COPO_LINE_STRIDE] records of the detectors."""
    out = np.zeros((len(lines), 12), np.float64)
    for i, (x0, y0, th, ln, kap, kind, _, _) in enumerate(np.asarray(lines, np.float64)):
        out[i, :7] = [kind, x0, y0, math.cos(th), math.sin(th), ln, kap]
        if kap != 0.0:
            sg, r, ang = (1.0 if kap > 0 else -1.0), 1.0 / abs(kap), abs(kap) * ln
            cx, cy = x0 - sg * r * math.sin(th), y0 + sg * r * math.cos(th)
            ux, uy = sg * math.sin(th), -sg * math.cos(th)
            c, s = math.cos(sg * ang / 2.0), math.sin(sg * ang / 2.0)
            out[i, 7:] = [cx, cy, c * ux - s * uy, s * ux + c * uy, math.cos(ang / 2.0)]
    return out.astype(np.float32)


def fill_cfg_struct(cfg: SimConfig, struct_cls):
    """Build the C struct (works for both the HIP library and the test oracle, which share the layout).
    Returns (struct, keepalive) -- keepalive holds the numpy tables the struct points into."""
    t, n = cfg.resolved()
    c = struct_cls()
    c.num_envs, c.num_agents, c.num_lasers, c.obs_dim = cfg.num_envs, n, cfg.num_lasers, cfg.obs_dim
    c.nbr_k = min(cfg.nbr_k, 64)
    c.enable_lcf = 1 if cfg.enable_lcf else 0
    c.horizon, c.delay_done, c.respawn_cooldown, c.substeps = cfg.horizon, cfg.delay_done, cfg.respawn_cooldown, cfg.substeps
    for k in ("lidar_range", "neighbours_distance", "mf_distance", "dt", "veh_half_len", "veh_half_wid", "wheelbase",
              "max_steer", "max_speed", "acc_max", "brake_gain", "brake_max", "lat_acc_max", "reverse_acc", "spawn_region_len", "spawn_region_wid",
              "driving_reward", "speed_reward", "success_reward", "crash_penalty", "out_penalty", "arrive_margin", "body_margin",
              "lane_width", "side_range", "lane_line_range", "toll_speed_limit", "overspeed_penalty"):
        setattr(c, k, float(getattr(cfg, k)))
    c.lcf_mean, c.lcf_std = float(cfg.lcf_mean), float(cfg.lcf_std)
    c.add_traffic_light, c.traffic_light_interval = int(bool(cfg.add_traffic_light)), int(cfg.traffic_light_interval)
    c.comm_size, c.comm_neighbours = max(0, int(cfg.comm_size)), int(cfg.comm_neighbours)
    c.add_pos_in_comm = int(bool(cfg.add_pos_in_comm))
    c.side_lasers, c.lane_line_lasers = int(cfg.side_lasers), int(cfg.lane_line_lasers)
    c.navi_dim, c.toll_dim, c.toll_min_steps = int(cfg.navi_dim), int(cfg.toll_dim), int(cfg.toll_min_steps)
    c.toll_early_exit = int(cfg.toll_early_exit)
    for k, v in enumerate(_maps.bounding_box(t)):
        c.map_bbox[k] = float(v)
    assert abs(t.lane_width - cfg.lane_width) < 1e-6, "the map was built for another lane width"
    keep = dict(
        route_segs=np.ascontiguousarray(t.route_segs, np.float32), route_meta=np.ascontiguousarray(t.route_meta, np.float32),
        spawn_tab=np.ascontiguousarray(t.spawn_tab, np.int32), spawn_s=np.ascontiguousarray(t.spawn_s, np.float32),
        ray_cs=_maps.ray_table(cfg.num_lasers, clockwise=cfg.lidar_clockwise),
        lines=line_table(t.lines),
        boxes=np.ascontiguousarray(t.boxes if (cfg.toll_buildings and t.boxes is not None) else np.zeros((0, 6)), np.float32),
        side_cs=_maps.ray_table(max(1, cfg.side_lasers), offset_deg=90.0),
        lane_line_cs=_maps.ray_table(max(1, cfg.lane_line_lasers), offset_deg=90.0))
    c.n_routes, c.n_spawns, c.n_lines, c.n_boxes = t.n_routes, t.n_spawns, len(keep["lines"]), len(keep["boxes"])
    c.boxes_hidden = 1 if int(cfg.toll_buildings) == 2 else 0
    for k, v in keep.items():
        setattr(c, k, v.ctypes.data)
    return c, keep


def lcf_table_array(table, num_envs):
    """float32 [num_envs, 2] of per-scene (mean, std), checked as `copo_sim_set_lcf_table` checks it."""
    table = np.ascontiguousarray(np.asarray(table, np.float32))
    if table.shape != (int(num_envs), 2):
        raise ValueError("lcf table: shape %s, need (%d, 2) = (mean, std) per scene" % (table.shape, num_envs))
    bad = ~((table[:, 1] > 0.0) & (table[:, 0] >= -1.0) & (table[:, 0] <= 1.0))
    if bad.any():
        e = int(np.argmax(bad))
        raise ValueError("lcf table scene %d (mean=%g, std=%g): need -1 <= mean <= 1, std > 0" % (e, table[e, 0], table[e, 1]))
    return table


class VecSim(Handle):
    """E independent scenes x N agent slots on one GPU; every call is asynchronous on torch's current stream."""

    OUT_FIELDS = ("obs", "rew", "nei_rew", "glob_rew", "flags", "nbr_idx", "nbr_cnt", "mf_cnt", "nbr_dist", "lcf",
                  "info", "agent_id")
    _prefix = "copo_sim_"

    def __init__(self, cfg: SimConfig, device=0, with_info=True):
        import torch
        from . import _capi
        self._capi, self._torch = _capi, torch
        self.cfg = cfg
        self.tables, self.N = cfg.resolved()
        self.E, self.O, self.K = cfg.num_envs, cfg.obs_dim, min(cfg.nbr_k, 64)
        self.A = cfg.act_dim
        self.device = torch.device("cuda", device)
        struct, self._keep = fill_cfg_struct(cfg, _capi.SimCfg)
        self._create(_capi.lib.copo_sim_create, C.byref(struct), device)
        self.on_shape_change = []        # weak references to callables (VecSampler registers the reset of its captured rollout)
        E, N, O, K, dev = self.E, self.N, self.O, self.K, self.device
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        self.out = dict(
            obs=torch.zeros(E, N, O, dtype=f32, device=dev), rew=torch.zeros(E, N, dtype=f32, device=dev),
            nei_rew=torch.zeros(E, N, dtype=f32, device=dev), glob_rew=torch.zeros(E, dtype=f32, device=dev),
            flags=torch.zeros(E, N, dtype=u8, device=dev), nbr_idx=torch.zeros(E, N, K, dtype=i32, device=dev),
            nbr_cnt=torch.zeros(E, N, dtype=i32, device=dev), mf_cnt=torch.zeros(E, N, dtype=i32, device=dev),
            nbr_dist=torch.zeros(E, N, K, dtype=f32, device=dev), lcf=torch.zeros(E, N, dtype=f32, device=dev),
            info=torch.zeros(E, N, _capi.INFO_DIM, dtype=f32, device=dev) if with_info else None,
            agent_id=torch.zeros(E, N, dtype=i32, device=dev),
        )
        self._step_out = self.make_step_out(self.out)

    def make_step_out(self, tensors):
        so = self._capi.StepOut()
        for k in self.OUT_FIELDS:
            t = tensors.get(k)
            setattr(so, k, t.data_ptr() if t is not None else None)
        return so

    def reset(self, seeds=None, out=None):
        if seeds is None:
            seeds = np.arange(self.E, dtype=np.uint64) + np.uint64(self.cfg.start_seed)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.shape == (self.E,)
        so = self._step_out if out is None else self.make_step_out(out)
        self._capi.check(self._capi.lib.copo_sim_reset(self._h, seeds.ctypes.data, C.byref(so), self._stream()))
        self._torch.cuda.current_stream(self.device).synchronize()   # seeds is a host buffer
        return self.out if out is None else out

    def step(self, act, out=None):
        """act: [E, N, 2 (+ comm_size)] fp32 cuda tensor.  Returns the dict of output tensors (overwritten every step)."""
        assert act.is_cuda and act.dtype == self._torch.float32 and act.is_contiguous() and act.numel() == self.E * self.N * self.A
        so = self._step_out if out is None else self.make_step_out(out)
        self._capi.check(self._capi.lib.copo_sim_step(self._h, act.data_ptr(), C.byref(so), self._stream()))
        return self.out if out is None else out

    def set_lcf_dist(self, mean, std):
        self._capi.check(self._capi.lib.copo_sim_set_lcf_dist(self._h, float(mean), float(std)))

    def set_lcf_table(self, table):
        """One LCF distribution per scene for agents spawned from now on: `table` [E, 2] = (mean, std) of scene e, or None to
        return to the single distribution of `set_lcf_dist`.  `set_force_lcf` still overrides every scene."""
        if table is None:
            self._capi.check(self._capi.lib.copo_sim_set_lcf_table(self._h, None))
            return
        table = lcf_table_array(table, self.E)
        self._capi.check(self._capi.lib.copo_sim_set_lcf_table(self._h, table.ctypes.data))      # (copied by the library)

    def set_force_lcf(self, v):
        self._capi.check(self._capi.lib.copo_sim_set_force_lcf(self._h, float(v)))

    def set_capacity(self, capacity):
        """Active agent slots (curriculum): takes effect for respawns from the next step, for everything after a reset."""
        self._capi.check(self._capi.lib.copo_sim_set_capacity(self._h, int(capacity)))

    def flush(self):
        """Push pending set_lcf_dist/set_force_lcf values to the device (needed before replaying a captured graph)."""
        self._capi.check(self._capi.lib.copo_sim_flush(self._h, self._stream()))

    def set_block(self, threads):
        """Launch shape of the step / reset kernels.  The shape parameters live in the device parameter block, so a hipGraph
        captured before this call would replay its OLD block size against the NEW chunking: every holder of a captured
        rollout registers a callback in `on_shape_change` (VecSampler does) and is reset here."""
        self._capi.check(self._capi.lib.copo_sim_set_block(self._h, int(threads)))
        self._shape_changed()

    def _shape_changed(self):
        live = []
        for ref in self.on_shape_change:
            cb = ref()
            if cb is not None:        # (its owner is gone otherwise: drop the entry)
                cb()
                live.append(ref)
        self.on_shape_change = live

    def set_chunk(self, fans):
        """LiDAR fans held in LDS at a time in the one-wave-per-scene shape (tuning knob; 0 = default)."""
        self._capi.check(self._capi.lib.copo_sim_set_chunk(self._h, int(fans)))
        self._shape_changed()

    def get_state(self):
        torch = self._torch
        st = torch.empty(self._capi.STATE_FIELDS, self.E, self.N, dtype=torch.float32, device=self.device)
        env = torch.empty(self.E, 4, dtype=torch.int32, device=self.device)
        self._capi.check(self._capi.lib.copo_sim_get_state(self._h, st.data_ptr(), env.data_ptr(), self._stream()))
        return st, env

    def set_state(self, st, env):
        assert st.is_cuda and env.is_cuda and st.is_contiguous() and env.is_contiguous()
        self._capi.check(self._capi.lib.copo_sim_set_state(self._h, st.data_ptr(), env.data_ptr(), self._stream()))
