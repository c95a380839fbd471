"""ctypes binding of libf110.so (the C ABI in include/f110.h).

Loads the in-tree library; there is no CPU fallback: if the library or a
gfx950 device is missing, the calls fail loudly with the library's error.
"""
from __future__ import annotations

import ctypes
import os

from . import _build

_P = ctypes.c_void_p
_D = ctypes.POINTER(ctypes.c_double)


class F110Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in
                ("mu", "C_Sf", "C_Sr", "lf", "lr", "h", "m", "I", "s_min", "s_max", "sv_min", "sv_max",
                 "v_switch", "a_max", "v_min", "v_max", "width", "length", "lidar_max")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class F110Config(ctypes.Structure):
    _fields_ = [("n_envs", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("n_beams", ctypes.c_int32),
                ("theta_dis", ctypes.c_int32), ("integrator", ctypes.c_int32), ("ego_idx", ctypes.c_int32),
                ("autoreset", ctypes.c_int32), ("_pad", ctypes.c_int32), ("fov", ctypes.c_double),
                ("eps", ctypes.c_double), ("max_range", ctypes.c_double), ("time_step", ctypes.c_double),
                ("lidar_dist", ctypes.c_double), ("ttc_thresh", ctypes.c_double),
                ("noise_std", ctypes.c_double), ("env_offset", ctypes.c_int64), ("seed", ctypes.c_uint64)]


class F110Outputs(ctypes.Structure):
    _fields_ = [("obs", _P), ("scans", _P), ("scans_f64", _P), ("collisions", _P), ("terminated", _P),
                ("was_reset", _P), ("lap_times", _P), ("lap_counts", _P), ("sim_time", _P),
                ("obs_stride", ctypes.c_int64)]


class F110RewardParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in
                ("dt", "w_prog", "forward_sign", "alive_bonus", "w_rel_lead", "lead_clip", "w_lat", "lat_cap",
                 "default_half_width", "lidar_max", "near_wall_dist", "w_wall", "wall_quantile", "opp_safe_dist",
                 "w_opp", "ego_crash_penalty", "opp_crash_bonus", "beta")] + \
               [(n, ctypes.c_int32) for n in ("grace_steps_wall", "grace_steps_opp", "auto_flip_steps",
                                             "use_progress")]


class F110PursuitParams(ctypes.Structure):  # f110_pursuit_params
    _fields_ = [(n, ctypes.c_double) for n in ("lookahead", "wheelbase", "speed", "a_lat", "v_floor", "steer_limit")] + \
               [("direction", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class F110GemmOp(ctypes.Structure):  # f110_gemm_op
    _fields_ = [(n, _P) for n in ("A", "B", "bias", "amask", "omask", "x2", "w2", "C")] + \
               [(n, ctypes.c_int32) for n in ("N", "K", "lda", "ldb", "ldc", "ldx2", "ldw2", "nx2", "relu", "nn")]


class F110WgradOp(ctypes.Structure):  # f110_wgrad_op
    _fields_ = [(n, _P) for n in ("G", "gmask", "X", "dW", "db")] + \
               [(n, ctypes.c_int32) for n in ("N", "KX", "ldg", "ldx", "ldw")]


class F110EpisodeState(ctypes.Structure):  # f110_episode_state (zero bytes = fresh)
    _fields_ = [("ret", ctypes.c_double), ("len", ctypes.c_int32), ("closed", ctypes.c_int32)]


class F110EpisodeTotals(ctypes.Structure):  # f110_episode_totals (zero bytes = fresh)
    _fields_ = [(n, ctypes.c_int64) for n in ("episodes", "terminated", "truncated", "length_sum")] + \
               [(n, ctypes.c_double) for n in ("return_sum", "return_min", "return_max")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class F110RaceParams(ctypes.Structure):  # f110_race_params
    _fields_ = [("pass_margin", ctypes.c_double), ("direction", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class F110RaceState(ctypes.Structure):  # f110_race_state (zero bytes = fresh)
    _fields_ = [("s_prev", ctypes.c_double * 2), ("prog", ctypes.c_double * 2), ("lead0", ctypes.c_double),
                ("t_max", ctypes.c_double)] + \
               [(n, ctypes.c_int32) for n in ("len", "passes", "passed", "flags")]


class F110RaceTotals(ctypes.Structure):  # f110_race_totals (zero bytes = fresh)
    _fields_ = [(n, ctypes.c_int64) for n in ("episodes", "ego_crashes", "completed", "truncated", "opp_crashes",
                                             "ahead_at_end", "passes", "passed", "length_sum")] + \
               [(n, ctypes.c_double) for n in ("progress_sum", "progress_min", "progress_max", "lead_sum", "t_max")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class F110TrackObsParams(ctypes.Structure):  # f110_track_obs_params
    _fields_ = [(n, ctypes.c_double) for n in ("v_scale", "steer_scale", "yaw_rate_scale", "slip_scale", "lat_scale",
                                              "gap_scale")] + \
               [("preview", ctypes.c_double * 8), ("n_preview", ctypes.c_int32), ("direction", ctypes.c_int32)]


class F110ScanObsParams(ctypes.Structure):  # f110_scan_obs_params
    _fields_ = [(n, ctypes.c_int32) for n in ("n_bins", "n_frames", "stride", "reduce", "keep_mid")]


class F110SpawnRange(ctypes.Structure):  # f110_spawn_range (zero bytes = the agent's base pose at rest)
    _fields_ = [("lateral", ctypes.c_double * 2), ("heading", ctypes.c_double * 2), ("speed", ctypes.c_double * 2),
                ("gap", ctypes.c_int32 * 2), ("behind", ctypes.c_double), ("clearance", ctypes.c_double)]


class F110SensorParams(ctypes.Structure):  # f110_sensor_params: (lo, hi) each; the defaults are the identity
    _fields_ = [(n, ctypes.c_float * 2) for n in ("scale", "noise_abs", "noise_rel", "dropout", "blackout", "quant",
                                                 "pose_xy", "pose_theta")]


class F110RayKnobs(ctypes.Structure):  # f110_ray_knobs (include/f110_debug.h)
    _fields_ = [(n, ctypes.c_int32) for n in
                ("kernel", "lanes", "refill", "fxs_lds", "count_slots", "wtrace", "heavy_list", "heavy_on",
                 "heavy_use", "heavy_cap", "has_rm", "has_rmp", "fxs_ok", "rotated", "E", "A", "B", "theta_dis",
                 "ray_wpb", "has_geo")]


class F110RayPlan(ctypes.Structure):  # f110_ray_plan
    _fields_ = [(n, ctypes.c_int32) for n in ("family", "rot", "mask", "handoff", "lds", "count", "trace")] + \
               [("grid", ctypes.c_uint32), ("block", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("wpb", "nch", "G4", "HB", "geo_blocks", "table", "wcost", "geo_ready")]


RAY_FAMILIES = ("tiled_flat", "tiled_chunked", "fx", "fxn_clamped", "fxn_padded", "fxs")  # F110_RAY_*
RAY_TABLES = ("tiled", "rowmajor", "padded")  # F110_TABLE_*

REWARD_STATE_BYTES = 8 * 12 + 4 * 4   # f110_reward_state
EPISODE_STATE_BYTES = 16              # f110_episode_state
EPISODE_TOTALS_BYTES = 56             # f110_episode_totals
RACE_STATE_BYTES = 64                 # f110_race_state
RACE_TOTALS_BYTES = 112               # f110_race_totals
RACE_FLAGS = dict(STARTED=1, CLOSED=2, S0=4, S1=8, AHEAD=16, OPP_CRASHED=32)  # f110_race_state.flags
RACE_RESULT = dict(finished=1, ego_crash=2, completed=4, truncated=8, opp_crashed=16, ahead_at_end=32)  # result bits

SPAWN_RANGE_BYTES = 72                # f110_spawn_range
SPAWN_FIELDS = tuple(n for n, _ in F110SpawnRange._fields_)  # lateral, heading, speed, gap: (lo, hi); behind, clearance

PARAM_FIELDS = tuple(n for n, _ in F110Params._fields_)
DYN_FIELDS = PARAM_FIELDS[:16]  # the fields a context may hold per env (f110_set_env_params)

ABI_VERSION = 3  # include/f110.h F110_ABI_VERSION
F32 = 0
F64 = 1
INTEGRATOR_RK4 = 1
INTEGRATOR_EULER = 2

_i, _i32, _i64, _u64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
_f32, _f64 = ctypes.c_float, ctypes.c_double
_PP = ctypes.POINTER(F110Params)
_SR = ctypes.POINTER(F110SpawnRange)
_SP = ctypes.POINTER(F110SensorParams)
_OUT = ctypes.POINTER(F110Outputs)
_PTRS6 = [ctypes.POINTER(_P)] * 6
_EXPLORE = [_P] * 5 + [_i32] * 3 + [_P, _P, _f64, _f64, _P, _P, _u64, _P, _i64]  # f110_ddpg_actor_explore less its stream

# The C ABI, one line per entry point of include/f110.h and include/f110_debug.h:
# name -> (restype, argtypes); restype None is void.  tests/test_host_lib.py checks every line
# against the headers' prototypes.
_API = {
    "f110_abi_version": (_i, []),
    "f110_last_error": (ctypes.c_char_p, []),
    "f110_default_params": (None, [_PP]),
    "f110_default_config": (None, [ctypes.POINTER(F110Config)]),
    "f110_edt_k": (_i, [_P, _i32, _i32, _P]),
    "f110_create": (_i, [ctypes.POINTER(_P), _i32, ctypes.POINTER(F110Config), _PP, _P, _i32, _i32, _f64, _D, _P,
                         _i32]),
    "f110_destroy": (_i, [_P]),
    "f110_reset": (_i, [_P, _P, _P, _OUT, _P]),
    "f110_step": (_i, [_P, _P, _i32, _OUT, _P]),
    "f110_get_state": (_i, [_P, _P, _P, _P, _P]),
    "f110_set_state": (_i, [_P, _P, _P, _P, _P]),
    "f110_scan_batch": (_i, [_P, _P, _i64, _P, _P, _P, _P]),
    "f110_dynamics_batch": (_i, [_P, _P, _P, _P, _i64, _P]),
    "f110_read_counters": (_i, [_P, ctypes.POINTER(_u64), ctypes.POINTER(_u64), _P]),
    "f110_reset_counters": (_i, [_P, _P]),
    "f110_debug_read_simt": (_i, [_P, ctypes.POINTER(_u64), ctypes.POINTER(_u64), _P]),
    "f110_debug_set_simt": (_i, [_P, _i32]),
    "f110_debug_set_handoff_check": (_i, [_P, _i32]),
    "f110_debug_profile_stamps": (_i, [_P, _P, _P, _i32, ctypes.POINTER(_i32)]),
    "f110_host_beam_runs_agree": (_i, [_f64, _f64, _i32, _i32]),
    "f110_host_sincos_fast": (None, [_P, _i64, _P, _P, _P]),
    "f110_host_tan_cos_fast": (None, [_P, _i64, _P, _P, _P, _P]),
    "f110_profile_begin": (_i, [_P, _i32]),
    "f110_profile_end": (_i, [_P, _D, ctypes.POINTER(_i32)]),
    "f110_host_tables": (None, [_i32, _i32, _f64, _PP, _P, _P, _P, _P, _P]),
    "f110_host_beam_indices": (_i, [_f64, _f64, _i32, _i32, _P]),
    "f110_set_scan_noise": (_i, [_P, _P]),
    "f110_set_params": (_i, [_P, _PP, _i32, _P]),
    "f110_host_cell_index": (_i, [_i32, _i32, _f64, _D, _P, _i64, _P]),
    "f110_gap_follow": (_i, [_P, _i64, _i64, _i32, _f64, _f64, _P, _i64, _P, _P]),
    "f110_host_window_ranges": (None, [_f64, _f64, _i32, _f64, _f64, _P]),
    "f110_track_create": (_i, [ctypes.POINTER(_P), _i32, _P, _P, _P, _i32, _i32]),
    "f110_track_destroy": (_i, [_P]),
    "f110_track_arrays": (_f64, [_P, _P, _P, _P, _P]),
    "f110_default_reward_params": (None, [ctypes.POINTER(F110RewardParams)]),
    "f110_reward": (_i, [_P, ctypes.POINTER(F110RewardParams), _P, _i64, _i32, _i32, _P, _P, _P, _P]),
    "f110_replay_create": (_i, [ctypes.POINTER(_P), _i32, _i64, _i32, _i32, _i32, _i64, _f64, _f64, _u64]),
    "f110_replay_destroy": (_i, [_P]),
    "f110_replay_add": (_i, [_P, _P, _i64, _P, _i64, _P, _P, _i64, _P, _P, _P, _i64, _P]),
    "f110_replay_add_env": (_i, [_P, _P, _i64, _P, _i64, _P, _P, _i64, _P, _P, _i64, _P]),
    "f110_replay_sample": (_i, [_P, _i32, _f64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f110_replay_update_priorities": (_i, [_P, _P, _P, _i64, _i32, _f32, _P]),
    "f110_replay_length": (_i, [_P, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _P]),
    "f110_replay_arrays": (_i, [_P] + _PTRS6),
    "f110_replay_select_keys": (_i, [_P, _P, _i64, _i32, _f64, _P, _P, _P]),
    "f110_replay_select_state": (_i, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P)] +
                                 [ctypes.POINTER(ctypes.c_uint32)] * 3 + [_D, ctypes.POINTER(ctypes.c_uint32), _P]),
    "f110_debug_wave_trace": (_i, [_P, _i32, _P, _i64, ctypes.POINTER(_i64), _P]),
    "f110_debug_set_ray_gate": (_i, [_P, _P, _P]),
    "f110_debug_disable_heavy_first": (_i, [_P]),
    "f110_debug_ray_kernel": (_i, [_P]),
    "f110_debug_ray_lanes": (_i, [_P]),
    "f110_debug_ray_refill": (_i, [_P]),
    "f110_debug_set_ray_refill": (_i, [_P, _i32]),
    "f110_debug_read_counter": (_i, [_P, _i32, ctypes.POINTER(_u64), _P]),
    "f110_step_n": (_i, [_P, _P, _i32, _i32, _i64, _P, _P]),
    "f110_debug_set_ray_lanes": (_i, [_P, _i32]),
    "f110_set_reset_dtype": (_i, [_P, _i32]),
    "f110_set_device_share": (_i, [_P, _i64, _i32]),
    "f110_host_np_sincosf": (None, [_P, _i64, _i32, _P]),
    "f110_host_sincos": (None, [_P, _i64, _P, _P]),
    "f110_host_sincos_series": (None, [_P, _i64, _P, _P]),
    "f110_host_map_table": (_i64, [_P, _i32, _i32, _f64, _i32, _i32, _P, _i64, _P]),
    "f110_get_lap_state": (_i, [_P, _P, _P, _P]),
    "f110_host_ray_plan": (_i, [ctypes.POINTER(F110RayKnobs), _i32, ctypes.POINTER(F110RayPlan)]),
    "f110_host_ray_rules": (_i, [_i64, _i64, _i32, _i32, _i32, ctypes.POINTER(_i32)]),
    "f110_set_env_params": (_i, [_P, _PP, _P]),
    "f110_get_env_params": (_i, [_P, _PP, _P]),
    "f110_set_param_randomization": (_i, [_P, _PP, _PP, _u64, _P]),
    "f110_host_check_param_ranges": (_i, [_PP, _PP, _PP, _i32]),
    "f110_host_param_draw": (_i, [_u64, _i64, _i32, _u64, _PP, _PP, _PP]),
    "f110_set_spawn_randomization": (_i, [_P, _SR, _u64, _P]),
    "f110_get_spawn_state": (_i, [_P, _P, _P]),
    "f110_host_check_spawn_ranges": (_i, [_SR, _i32, _i32]),
    "f110_host_spawn_rows": (_i, [_SR, _i32, _u64, _u64, _P, _i32, _i32, _f64, _D, _P, _i32, _P, _P, _P, _P, _i64, _i32,
                                  _P, _P]),
    "f110_set_episode_limits": (_i, [_P, _i64, _f64, _i32, _P, _P]),
    "f110_host_check_episode_limits": (_i, [_i64, _f64, _i32]),
    "f110_episode_scratch_bytes": (_i64, [_i64]),
    "f110_episode_stats": (_i, [_P, _P, _P, _P, _i64, _P, _P, _P, _P, _P, _P, _P]),
    "f110_host_episode_stats": (_i, [_P, _P, _P, _P, _i64, _P, _P, _P, _P, _P]),
    "f110_dynamics_ks_batch": (_i, [_P, _P, _P, _P, _i64, _P]),
    "f110_collision_batch": (_i, [_P, _P, _i64, _P, _P]),
    "f110_collision_multiple": (_i, [_P, _i64, _i32, _P, _P, _P]),
    "f110_adam_step": (_i, [_P, _P, _P, _P, _i64, _f64, _f64, _f64, _f64, _P, _P, _f64, _P]),
    "f110_ddpg_scratch_floats": (_i64, [_i32, _i32, _i32]),
    "f110_ddpg_actor_head": (_i, [_P] * 5 + [_i32] * 3 + [_P] * 3),
    "f110_ddpg_actor_explore": (_i, _EXPLORE + [_P]),
    "f110_ddpg_actor_head_bwd": (_i, [_P] * 5 + [_i32] * 3 + [_P] * 6),
    "f110_ddpg_td_target": (_i, [_P] * 5 + [_f32, _i32, _i32, _P, _P]),
    "f110_ddpg_critic_loss": (_i, [_P] * 5 + [_i32] * 2 + [_P] * 4),
    "f110_ddpg_critic_loss_bwd": (_i, [_P] * 5 + [_i32] * 2 + [_P] * 6),
    "f110_ddpg_q_mean": (_i, [_P] * 3 + [_f32, _i32, _i32] + [_P] * 3),
    "f110_ddpg_q_mean_bwd": (_i, [_P] * 3 + [_f32, _i32, _i32] + [_P] * 6),
    "f110_ddpg_relu_bwd_scratch_floats": (_i64, [_i32, _i32]),
    "f110_ddpg_relu_bwd": (_i, [_P, _P, _i32, _i32, _P, _P, _P, _P]),
    "f110_learner_gemm": (_i, [ctypes.POINTER(F110GemmOp), _i32, _i32, _P]),
    "f110_learner_wgrad_scratch_floats": (_i64, [ctypes.POINTER(F110WgradOp), _i32, _i32]),
    "f110_learner_wgrad": (_i, [ctypes.POINTER(F110WgradOp), _i32, _i32, _P, _P]),
    "f110_learner_wgrad_loss": (_i, [ctypes.POINTER(F110WgradOp), _i32, _i32, _P, _P, _i32, _f32, _P, _P]),
    "f110_ddpg_critic_step": (_i, [_P] * 5 + [_f32] + [_P] * 5 + [_i32, _i32] + [_P] * 6),
    "f110_ddpg_q_mean_step": (_i, [_P] * 4 + [_f32, _i32, _i32] + [_P] * 4),
    "f110_ddpg_row_blocks": (_i32, [_i32]),
    "f110_ddpg_actor_explore_env": (_i, _EXPLORE + [_i32, _P, _f64, _f64, _f64, _P, _P, _P, _P]),
    "f110_host_explore_rows": (_i, [_P, _P, _i64, _i32, _i32, _P, _f64, _f64, _f64, _P, _P, _P, _P, _f64, _f64, _P,
                                    _P, _P]),
    "f110_td3_target_action": (_i, [_P] * 5 + [_i32] * 3 + [_f32, _f32, _P, _P, _u64, _P, _P, _P, _P]),
    "f110_td3_critic_step": (_i, [_P] * 8 + [_f32] + [_P] * 8 + [_i32, _i32] + [_P] * 9),
    "f110_host_td3_smooth_rows": (_i, [_P, _P, _i64, _i32, _f32, _f32, _P, _P, _P, _P]),
    "f110_host_td3_rows": (_i, [_P, _P, _f32] + [_P] * 5 + [_f32, _i64] + [_P] * 6),
    "f110_nstep_create": (_i, [ctypes.POINTER(_P), _i32, _i64, _i32, _f64, _i32, _i32]),
    "f110_nstep_destroy": (_i, [_P]),
    "f110_nstep_push": (_i, [_P, _P, _P, _i64, _P, _i64, _P, _P, _i64, _P, _P, _P, _P]),
    "f110_nstep_reset": (_i, [_P, _P, _P]),
    "f110_nstep_arrays": (_i, [_P] + _PTRS6),
    "f110_host_nstep": (_i, [_i64, _i32, _f64, _i32, _i32, _i64] + [_P] * 18 + [ctypes.POINTER(_i64)]),
    "f110_repeat_create": (_i, [ctypes.POINTER(_P), _i32, _i64, _i32, _f64, _i32, _i32]),
    "f110_repeat_destroy": (_i, [_P]),
    "f110_repeat_hold": (_i, [_P, _P, _i64, _P, _i64, _P, _P]),
    "f110_repeat_push": (_i, [_P, _P, _P, _P, _i64, _P, _P, _P, _P]),
    "f110_repeat_reset": (_i, [_P, _P, _P]),
    "f110_repeat_arrays": (_i, [_P] + [ctypes.POINTER(_P)] * 4),
    "f110_host_repeat_hold": (_i, [_i64, _i32, _i32] + [_P] * 6),
    "f110_host_repeat_push": (_i, [_i64, _i32, _f64, _i32, _i32, _i64] + [_P] * 14 + [ctypes.POINTER(_i64)]),
    "f110_agent_obs": (_i, [_P, _i64, _P, _i64, _i64, _i32, _i32, _i32, _f32, _P, _i64, _P]),
    "f110_policy_head_rows": (_i, [_P] * 5 + [_i64, _i32, _i32, _P, _P, _i64, _P]),
    "f110_host_agent_obs": (_i, [_P, _i64, _P, _i64, _i64, _i32, _i32, _i32, _f32, _P, _i64]),
    "f110_default_pursuit_params": (None, [ctypes.POINTER(F110PursuitParams)]),
    "f110_pure_pursuit": (_i, [_P, ctypes.POINTER(F110PursuitParams), _P, _i64, _i64, _P, _P, _P, _i64, _P, _P]),
    "f110_host_pure_pursuit": (_i, [_P, ctypes.POINTER(F110PursuitParams), _P, _i64, _i64, _P, _P, _P, _i64, _P]),
    "f110_default_race_params": (None, [ctypes.POINTER(F110RaceParams)]),
    "f110_race_scratch_bytes": (_i64, [_i64]),
    "f110_race_stats": (_i, [_P, ctypes.POINTER(F110RaceParams), _P, _P, _i64, _P, _P, _P, _i64] + [_P] * 9),
    "f110_host_race_stats": (_i, [_P, ctypes.POINTER(F110RaceParams), _P, _P, _i64, _P, _P, _P, _i64] + [_P] * 7),
    "f110_default_track_obs_params": (None, [ctypes.POINTER(F110TrackObsParams)]),
    "f110_track_obs_width": (_i32, [_i32, _i32]),
    "f110_track_obs": (_i, [_P, ctypes.POINTER(F110TrackObsParams), _P, _i64, _i32, _i32, _i32, _P, _i64, _P]),
    "f110_ctx_track_obs": (_i, [_P, _P, ctypes.POINTER(F110TrackObsParams), _i32, _i32, _P, _i64, _P]),
    "f110_host_track_obs": (_i, [_P, ctypes.POINTER(F110TrackObsParams), _P, _i64, _i32, _i32, _i32, _P, _i64]),
    "f110_default_scan_obs_params": (None, [ctypes.POINTER(F110ScanObsParams)]),
    "f110_scan_obs_width": (_i32, [ctypes.POINTER(F110ScanObsParams), _i32, _i32, _i32]),
    "f110_scan_obs_create": (_i, [ctypes.POINTER(_P), _i32, _i64, _i32, _i32, _i32, ctypes.POINTER(F110ScanObsParams)]),
    "f110_scan_obs_destroy": (_i, [_P]),
    "f110_scan_obs_push": (_i, [_P, _P, _i64, _P, _P, _i64, _P]),
    "f110_scan_obs_reset": (_i, [_P, _P, _P]),
    "f110_scan_obs_arrays": (_i, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    "f110_host_scan_obs_push": (_i, [ctypes.POINTER(F110ScanObsParams), _i64, _i32, _i32, _i32, _P, _i64, _P, _P, _P, _P,
                                     _i64]),
    "f110_default_sensor_params": (None, [_SP]),
    "f110_sensor_create": (_i, [ctypes.POINTER(_P), _i32, _i64, _i32, _i32, _i32, _f32, _u64, _i64, _P, _SP]),
    "f110_sensor_destroy": (_i, [_P]),
    "f110_sensor_apply": (_i, [_P, _P, _i64, _P, _P, _i64, _P]),
    "f110_sensor_reset": (_i, [_P, _P, _P]),
    "f110_sensor_arrays": (_i, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    "f110_host_check_sensor_params": (_i, [_SP, _i32]),
    "f110_host_sensor_apply": (_i, [_SP, _i64, _i32, _i32, _i32, _f32, _u64, _i64, _P, _P, _i64, _P, _P, _P, _P, _P,
                                    _i64]),
}
EXPORTS = list(_API)

_lib = None


class F110Error(RuntimeError):
    pass


class _Missing:
    """An entry point an older A/B build (F110_LIB) does not export."""

    def __init__(self, name):
        self.name, self.argtypes, self.restype = name, None, None

    def __call__(self, *a):
        raise F110Error(f"{self.name}: not exported by this (alternate) build")


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load libf110.so (building it with hipcc if it is missing/stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("F110_LIB") or _build.LIB  # F110_LIB: an alternate build (A/B runs)
    if build_if_missing and path == _build.LIB:
        try:
            _build.build()
        except Exception as exc:  # pragma: no cover - toolchain missing
            if not os.path.exists(path):
                raise F110Error(f"libf110.so is missing and could not be built: {exc}") from exc
    if not os.path.exists(path):
        raise F110Error(f"libf110.so not found at {path}; run f110_gymnasium_ros2_jazzy_amd._build.build()")
    try:  # share torch's HIP runtime (same SONAME) when torch is present
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(path)
    alternate = path != _build.LIB
    for name, (restype, argtypes) in _API.items():
        fn = getattr(L, name, None) if alternate else getattr(L, name)
        if fn is None and name.startswith("f110_debug_"):
            # an older build for A/B (ABI 2): its diagnostics under their pre-f110_debug_ names
            fn = getattr(L, name.replace("f110_debug_", "f110_"), None)
        if fn is None:  # newer than that build: fails when called
            fn = _Missing(name)
        setattr(L, name, fn)
        fn.restype, fn.argtypes = restype, argtypes
    if L.f110_abi_version() != ABI_VERSION and not (alternate and L.f110_abi_version() == 2):
        raise F110Error(f"libf110.so ABI version mismatch ({L.f110_abi_version()} != {ABI_VERSION})")
    _lib = L
    return L


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = load().f110_last_error()
        raise F110Error(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc


def default_params() -> F110Params:
    p = F110Params()
    load().f110_default_params(ctypes.byref(p))
    return p


def default_config() -> F110Config:
    c = F110Config()
    load().f110_default_config(ctypes.byref(c))
    return c
