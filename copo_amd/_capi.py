"""ctypes binding of libcopo_hip.so (include/copo_hip.h).

This is the thin host layer the north star asks for: Python hosts the loop, the simulator and the
custom learn-side ops are HIP kernels behind a C ABI.  There is NO fallback: if the shared library
is missing or a symbol is absent, importing this module raises, and every op raises on a non-zero
return code with the library's own error string.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcopo_hip.so")
# Profiling scripts (scripts/sim_valu_split.py) load a differently compiled copy -- phases of the step kernel compiled out,
# `make prof SKIP=<mask>` -- by setting `copo_amd._libsel.PATH` BEFORE importing this module.  There is no environment
# variable and no runtime knob: the shipped library always does all the work.
try:
    from . import _libsel as _sel
    if getattr(_sel, "PATH", None):
        LIB_PATH = _sel.PATH
except ImportError:
    pass

from ._abi import *  # noqa: F401,F403  (re-exported: the struct mirrors and limits live where no native code is loaded)

LCF_STATS_DOUBLES = 8 + 6 * 2048

F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = (1 << i for i in range(8))
I_VELOCITY, I_STEERING, I_ACCELERATION, I_STEP_REWARD, I_COST, I_EPISODE_LENGTH, I_EPISODE_REWARD, \
    I_ROUTE_COMPLETION = range(8)

ERR_NAMES = {0: "COPO_OK", -1: "COPO_ERR_NULL", -2: "COPO_ERR_DIM", -3: "COPO_ERR_DEVICE", -4: "COPO_ERR_STATE",
             -5: "COPO_ERR_CONFIG"}


class CopoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


class NetLayout(C.Structure):
    """Mirror of `copo_net_layout`."""
    _fields_ = [("w1", C.c_int64), ("b1", C.c_int64), ("w2", C.c_int64), ("b2", C.c_int64), ("w3", C.c_int64),
                ("b3", C.c_int64), ("in_dim", C.c_int32), ("out_dim", C.c_int32)]


class PpoCfg(C.Structure):
    """Mirror of `copo_ppo_cfg`."""
    _fields_ = [
        ("mb", C.c_int32), ("hidden", C.c_int32), ("act_dim", C.c_int32), ("n_value_heads", C.c_int32),
        ("pack_width", C.c_int32), ("col_actions", C.c_int32), ("col_logp", C.c_int32), ("col_dist", C.c_int32),
        ("col_adv", C.c_int32), ("col_meta_adv", C.c_int32), ("col_vpred", C.c_int32 * 3), ("col_vtarget", C.c_int32 * 3),
        ("use_kl", C.c_int32), ("old_value_loss", C.c_int32), ("operand_dtype", C.c_int32), ("reserved0", C.c_int32),
        ("clip_param", C.c_float), ("vf_clip_param", C.c_float), ("vf_loss_coeff", C.c_float), ("entropy_coeff", C.c_float),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("pol", NetLayout), ("val", NetLayout * 3), ("n_params", C.c_int64),
    ]


HEAD_PPO, HEAD_META_NEW, HEAD_META_OLD = 0, 1, 2
OPERAND_F32, OPERAND_BF16 = 0, 1
LOWP_BF16, LOWP_E4M3 = 1, 2
PPO_STATS = 8
META_DOT_PARTIALS = 8192

_SIGS = {
    "copo_ppo_workspace_floats": (C.c_int64, [C.POINTER(PpoCfg)]),
    "copo_ppo_fused_step_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 14 + [C.c_int32, C.c_int32, C.c_void_p,
                                                                                   C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_gather_rows_f32": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                       C.c_int64, C.c_void_p]),
    "copo_pack_columns_f32": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "copo_dp_workspace_bytes": (C.c_int64, [C.POINTER(PpoCfg), C.c_int32]),
    "copo_ppo_fused_step_dp_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 13 + [C.c_void_p, C.c_int32, C.c_void_p,
                                                                                      C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p]),
    "copo_dp_status": (C.c_int, [C.c_void_p, C.POINTER(PpoCfg), C.c_int32, C.c_void_p]),
    "copo_transpose_weights_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_mlp_forward_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32] +
                             [C.c_void_p] * 7),
    "copo_mlp_forward_bank_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64] +
                                  [C.c_void_p] * 7),
    "copo_mlp_forward_rows_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32] +
                                  [C.c_void_p] * 2),
    "copo_mlp_forward_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_int64] + [C.c_void_p] * 7),
    "copo_adv_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_pgd_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64] + [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_cert_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_int64] + [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "copo_lin_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "copo_jury_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_int64] + [C.c_void_p] * 3),
    "copo_hidden_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_int64] + [C.c_void_p] * 3),
    "copo_cka_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 +
                            [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "copo_cka_finish": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p] * 5),
    "copo_probe_targets": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_int32] * 3 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p]),
    "copo_probe_accumulate": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 3 + [C.c_int64] +
                              [C.c_void_p] * 3 + [C.c_int64] + [C.c_int32] * 3 + [C.c_void_p] * 4),
    "copo_ig_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_attrib_tally": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p] * 3),
    "copo_jury_tally": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_float] * 2 + [C.c_void_p, C.c_void_p]),
    "copo_lowp_pack": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "copo_lowp_forward_seats": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int64] + [C.c_void_p] * 7),
    "copo_value_obs_seats_f32": (C.c_int, [C.POINTER(PpoCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "copo_audit_create": (C.c_int, [C.POINTER(AuditCfg), C.POINTER(C.c_void_p)]),
    "copo_audit_record": (C.c_int, [C.c_void_p] * 9),
    "copo_audit_read": (C.c_int, [C.c_void_p] * 3),
    "copo_audit_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_audit_destroy": (C.c_int, [C.c_void_p]),
    "copo_debug_lowp_round": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "copo_debug_lowp_scale": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "copo_influence_heading": (C.c_int, [C.c_void_p] * 4),
    "copo_influence_obs": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 7),
    "copo_influence_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 3),
    "copo_influence_tally": (C.c_int, [C.c_void_p] * 8 + [C.c_int32] * 5 + [C.c_float] * 2 + [C.c_void_p] * 3),
    "copo_seat_tally": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "copo_certify_tally": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "copo_fault_obs": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_int32, C.c_void_p,
                                 C.c_uint64, C.c_void_p]),
    "copo_fault_act": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_int32, C.c_void_p,
                                 C.c_uint64, C.c_void_p]),
    "copo_adam_step_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 5),
    "copo_meta_grads_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 15),
    "copo_meta_lcf_f64": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] +
                          [C.c_void_p] * 5),
    "copo_meta_finish_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_meta_step_f64": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 13 + [C.c_int32, C.c_int32] + [C.c_void_p] * 5 +
                           [C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_episode_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "copo_plan_epoch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] +
                        [C.c_void_p] * 5),
    "copo_meta_fold_len": (C.c_int64, [C.POINTER(PpoCfg)]),
    "copo_meta_batch_workspace_floats": (C.c_int64, [C.POINTER(PpoCfg), C.c_int32]),
    "copo_meta_batch_grads_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 8 + [C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 4),
    "copo_meta_batch_dot_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_meta_rows_workspace_floats": (C.c_int64, [C.POINTER(PpoCfg), C.c_int64]),
    "copo_meta_rows_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3),
    "copo_meta_batch_wgrads_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 2 +
                                   [C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 4),
    "copo_meta_rowstat_f32": (C.c_int, [C.POINTER(PpoCfg)] + [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_meta_batch_lcf_f64": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] +
                                [C.c_void_p] * 3 + [C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_version": (C.c_int, []),
    "copo_build_info": (C.c_char_p, []),
    "copo_last_error": (C.c_char_p, []),
    "copo_sim_create": (C.c_int, [C.POINTER(SimCfg), C.c_int, C.POINTER(C.c_void_p)]),
    "copo_sim_destroy": (C.c_int, [C.c_void_p]),
    "copo_sim_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StepOut), C.c_void_p]),
    "copo_sim_set_lcf_dist": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "copo_sim_set_lcf_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_sim_set_force_lcf": (C.c_int, [C.c_void_p, C.c_double]),
    "copo_sim_set_capacity": (C.c_int, [C.c_void_p, C.c_int32]),
    "copo_sim_set_block": (C.c_int, [C.c_void_p, C.c_int32]),
    "copo_sim_set_chunk": (C.c_int, [C.c_void_p, C.c_int32]),
    "copo_sim_flush": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_sim_set_debug": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_sim_step": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StepOut), C.c_void_p]),
    "copo_sim_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_sim_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_render_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "copo_render_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_render_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_render_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_render_destroy": (C.c_int, [C.c_void_p]),
    "copo_interact_create": (C.c_int, [C.c_void_p, C.POINTER(InteractCfg), C.POINTER(C.c_void_p)]),
    "copo_interact_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_interact_totals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_interact_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_interact_destroy": (C.c_int, [C.c_void_p]),
    "copo_clip_create": (C.c_int, [C.c_void_p, C.POINTER(ClipCfg), C.POINTER(C.c_void_p)]),
    "copo_clip_record": (C.c_int, [C.c_void_p] * 5),
    "copo_clip_flush": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_clip_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "copo_clip_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_clip_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_clip_destroy": (C.c_int, [C.c_void_p]),
    "copo_clip_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_rewind_create": (C.c_int, [C.c_void_p, C.POINTER(RewindCfg), C.POINTER(C.c_void_p)]),
    "copo_rewind_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_rewind_reset": (C.c_int, [C.c_void_p]),
    "copo_rewind_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "copo_rewind_fork": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8),
    "copo_rewind_tally": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "copo_rewind_destroy": (C.c_int, [C.c_void_p]),
    "copo_field_create": (C.c_int, [C.c_void_p, C.POINTER(FieldCfg), C.POINTER(C.c_void_p)]),
    "copo_field_set_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_field_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "copo_field_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_field_forget": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_field_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_field_destroy": (C.c_int, [C.c_void_p]),
    "copo_gate_create": (C.c_int, [C.c_void_p, C.POINTER(GateCfg), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "copo_gate_set_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_gate_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_gate_words": (C.c_int64, [C.POINTER(GateCfg)]),
    "copo_gate_read": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "copo_gate_forget": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_gate_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_gate_destroy": (C.c_int, [C.c_void_p]),
    "copo_trip_create": (C.c_int, [C.c_void_p, C.POINTER(TripCfg), C.POINTER(C.c_void_p)]),
    "copo_trip_record": (C.c_int, [C.c_void_p] * 6),
    "copo_trip_flush": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_trip_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "copo_trip_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_trip_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_trip_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_trip_destroy": (C.c_int, [C.c_void_p]),
    "copo_conflict_create": (C.c_int, [C.c_void_p, C.POINTER(ConflictCfg), C.POINTER(C.c_void_p)]),
    "copo_conflict_record": (C.c_int, [C.c_void_p] * 3),
    "copo_conflict_flush": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_conflict_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "copo_conflict_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_conflict_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_conflict_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_conflict_destroy": (C.c_int, [C.c_void_p]),
    "copo_pet_create": (C.c_int, [C.c_void_p, C.POINTER(PetCfg), C.POINTER(C.c_void_p)]),
    "copo_pet_set_groups": (C.c_int, [C.c_void_p] * 3),
    "copo_pet_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_pet_forget": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_pet_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "copo_pet_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_pet_aggregates": (C.c_int, [C.c_void_p] * 4),
    "copo_pet_memory": (C.c_int, [C.c_void_p] * 4),
    "copo_pet_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_pet_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_pet_destroy": (C.c_int, [C.c_void_p]),
    "copo_recorder_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "copo_recorder_add": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_void_p]),
    "copo_recorder_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "copo_recorder_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "copo_recorder_episodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_recorder_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_recorder_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "copo_recorder_destroy": (C.c_int, [C.c_void_p]),
    "copo_neighbours_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "copo_gae3_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_cc_fuse_mf_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "copo_cc_fuse_concat_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 7 + [C.c_void_p, C.c_void_p]),
    "copo_lcf_mix_partial_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_lcf_mix_apply_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "copo_peer_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "copo_peer_alloc": (C.c_int, [C.c_int64, C.POINTER(C.c_void_p)]),
    "copo_peer_free": (C.c_int, [C.c_void_p]),
    "copo_ipc_export": (C.c_int, [C.c_void_p, C.c_char_p]),
    "copo_ipc_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "copo_ipc_close": (C.c_int, [C.c_void_p]),
    "copo_peer_allreduce_sum_f32": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "copo_peer_status": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "copo_debug_peer_allreduce_all_ranks": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, C.c_int32, C.c_void_p]),
    "copo_debug_rowpass_stamps": (C.c_int, [C.c_void_p]),
    "copo_debug_wg_times": (C.c_int, [C.c_void_p]),
    "copo_debug_learner_plan": (C.c_int, [C.POINTER(PpoCfg), C.c_int32, C.c_int32, C.c_int64] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32]),
    "copo_debug_learner_kernel": (C.c_char_p, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libcopo_hip.so not found at %s -- build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64.so.7; load it first so that this library binds to the SAME HIP
    # runtime (one runtime per process -- two would not share devices, streams or allocations).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    v = lib.copo_version()
    if v != ABI_VERSION:
        raise ImportError("libcopo_hip.so ABI %d != binding ABI %d" % (v, ABI_VERSION))
    return lib


lib = _load()


def check(rc):
    if rc != 0:
        raise CopoError(rc, lib.copo_last_error().decode("utf-8", "replace"))


def ptr(t):
    """Device/host address of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream
