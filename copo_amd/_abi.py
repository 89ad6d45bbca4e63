"""Struct layouts of include/copo_hip.h shared by the ctypes binding of libcopo_hip.so (`_capi`) and by the test
oracle's loader (tests/oracle_lib.py).  Importing this module loads no native code."""
import ctypes as C

ABI_VERSION = 8
MAX_AGENTS = 64
MAX_SEGS = 16
SEG_STRIDE = 16
MAX_LASERS = 256
MAX_SPAWNS = 256
MAX_SAFE = 32
MAX_ROUTES = 128
MAX_LINES = 128
LINE_STRIDE = 12
STATE_DIM = 6
NAVI_DIM = 10
INFO_DIM = 8
STATE_FIELDS = 16

SIM_CFG_FIELDS = [
    ("num_envs", C.c_int32), ("num_agents", C.c_int32), ("num_lasers", C.c_int32), ("obs_dim", C.c_int32),
    ("nbr_k", C.c_int32), ("enable_lcf", C.c_int32), ("horizon", C.c_int32), ("delay_done", C.c_int32),
    ("respawn_cooldown", C.c_int32), ("substeps", C.c_int32),
    ("lidar_range", C.c_float), ("neighbours_distance", C.c_float), ("mf_distance", C.c_float),
    ("dt", C.c_float), ("veh_half_len", C.c_float), ("veh_half_wid", C.c_float), ("wheelbase", C.c_float),
    ("max_steer", C.c_float), ("max_speed", C.c_float), ("acc_max", C.c_float), ("brake_gain", C.c_float),
    ("brake_max", C.c_float), ("lat_acc_max", C.c_float), ("reverse_acc", C.c_float), ("spawn_region_len", C.c_float), ("spawn_region_wid", C.c_float),
    ("driving_reward", C.c_float), ("speed_reward", C.c_float), ("success_reward", C.c_float),
    ("crash_penalty", C.c_float), ("out_penalty", C.c_float), ("arrive_margin", C.c_float), ("body_margin", C.c_float),
    ("lane_width", C.c_float),
    ("lcf_mean", C.c_double), ("lcf_std", C.c_double),
    ("n_routes", C.c_int32), ("n_spawns", C.c_int32),
    ("route_segs", C.c_void_p), ("route_meta", C.c_void_p), ("spawn_tab", C.c_void_p), ("spawn_s", C.c_void_p),
    ("ray_cs", C.c_void_p),
    ("add_traffic_light", C.c_int32), ("traffic_light_interval", C.c_int32), ("comm_size", C.c_int32),
    ("comm_neighbours", C.c_int32), ("add_pos_in_comm", C.c_int32), ("map_bbox", C.c_float * 4),
    ("side_lasers", C.c_int32), ("lane_line_lasers", C.c_int32), ("side_range", C.c_float),
    ("lane_line_range", C.c_float), ("navi_dim", C.c_int32), ("toll_dim", C.c_int32), ("toll_min_steps", C.c_int32),
    ("n_lines", C.c_int32), ("lines", C.c_void_p), ("side_cs", C.c_void_p), ("lane_line_cs", C.c_void_p),
    ("toll_speed_limit", C.c_float), ("overspeed_penalty", C.c_float), ("toll_early_exit", C.c_int32),
    ("n_boxes", C.c_int32), ("boxes", C.c_void_p), ("boxes_hidden", C.c_int32),
]

STEP_OUT_FIELDS = ("obs", "rew", "nei_rew", "glob_rew", "flags", "nbr_idx", "nbr_cnt", "mf_cnt", "nbr_dist", "lcf",
                   "info", "agent_id")


class SimCfg(C.Structure):
    """Mirror of `copo_sim_cfg`."""
    _fields_ = SIM_CFG_FIELDS


class StepOut(C.Structure):
    """Mirror of `copo_step_out` (pointers, 0 = skip)."""
    _fields_ = [(n, C.c_void_p) for n in STEP_OUT_FIELDS]


class InteractCfg(C.Structure):
    """Mirror of `copo_interact_cfg`."""
    _fields_ = [("horizon_s", C.c_float), ("ttc_crit_s", C.c_float), ("gap_near_m", C.c_float), ("brake_mps2", C.c_float)]


class ClipCfg(C.Structure):
    """Mirror of `copo_clip_cfg`."""
    _fields_ = [("pre", C.c_int32), ("post", C.c_int32), ("max_clips", C.c_int32), ("flag_mask", C.c_uint32), ("ttc_below", C.c_float),
                ("gap_below", C.c_float)]


CLIP_MAX_CAP, CLIP_WORDS, CLIP_HEADER = 256, 6, 8


class RewindCfg(C.Structure):
    """Mirror of `copo_rewind_cfg`."""
    _fields_ = [("depth", C.c_int32), ("stride", C.c_int32)]


REWIND_MAX_DEPTH, REWIND_TALLY = 64, 8


class FieldCfg(C.Structure):
    """Mirror of `copo_field_cfg`."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("cell", C.c_float), ("W", C.c_int32), ("H", C.c_int32), ("G", C.c_int32),
                ("ttc_below", C.c_float)]


FIELD_LAYERS, FIELD_MAX_SIDE, FIELD_MAX_GROUPS = 10, 1024, 64


class GateCfg(C.Structure):
    """Mirror of `copo_gate_cfg`."""
    _fields_ = [("L", C.c_int32), ("S", C.c_int32), ("G", C.c_int32), ("T", C.c_int32), ("bin_records", C.c_int32), ("HB", C.c_int32),
                ("TB", C.c_int32), ("tt_bin", C.c_int32)]


GATE_MAX_GATES, GATE_MAX_SECTIONS, GATE_MAX_GROUPS, GATE_MAX_BINS, GATE_MAX_HIST = 32, 64, 64, 256, 64


class TripCfg(C.Structure):
    """Mirror of `copo_trip_cfg`."""
    _fields_ = [("max_rows", C.c_int32), ("stop_speed", C.c_float)]


TRIP_WORDS, TRIP_DONE, TRIP_VANISHED, TRIP_FLUSHED = 16, 1, 2, 3


class ConflictCfg(C.Structure):
    """Mirror of `copo_conflict_cfg`."""
    _fields_ = [("max_rows", C.c_int32), ("radius", C.c_float), ("leave_radius", C.c_float)]


CONFLICT_WORDS, CONFLICT_DONE, CONFLICT_VANISHED, CONFLICT_PARTED, CONFLICT_FLUSHED = 16, 1, 2, 3, 4


class PetCfg(C.Structure):
    """Mirror of `copo_pet_cfg`."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("cell", C.c_float), ("W", C.c_int32), ("H", C.c_int32), ("G", C.c_int32),
                ("window", C.c_int32), ("critical_records", C.c_int32), ("max_rows", C.c_int32)]


PET_WORDS, PET_MAX_WINDOW, PET_TYPES = 16, 4096, 3
RECORDER_NCOL, RECORDER_MAX_SLOTS = 31, 256


class AuditCfg(C.Structure):
    """Mirror of `copo_audit_cfg`."""
    _fields_ = [("E", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("G", C.c_int32), ("heads", C.c_int32), ("bins", C.c_int32),
                ("count_truncated", C.c_int32), ("reserved0", C.c_int32), ("gamma", C.c_double * 3), ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


AUDIT_WORDS, AUDIT_MAX_BINS, AUDIT_BIN_COUNT, AUDIT_BIN_VALUE, AUDIT_BIN_RETURN = 56, 16, 8, 24, 40
