"""mantis_amd — MI355X-native mantis3 hot path.

Python is only a thin ctypes view of the C-ABI in include/mantis.h, used by
tests/, bench.py and __graft_entry__.py; the product is libmantis_amd.so
(HIP kernels for gfx950 + C++ host orchestration). There is no CPU fallback:
loading fails loudly when the library is missing, and mantis_create fails
when no GPU is present.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MANTIS_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                             "libmantis_amd.so")

MANTIS_OK = 0
REASONS = {0: "published", 1: "no_quads", 2: "no_hyps", 3: "yaw_ambiguous", 4: "no_yaw"}


class MantisConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("max_cams", C.c_int32),
                ("max_width", C.c_int32), ("max_height", C.c_int32), ("rng_seed", C.c_uint64),
                ("canny_low", C.c_int32), ("polygon_epsilon", C.c_int32),
                ("search_radius_multiplier", C.c_double), ("grid_spacing", C.c_double),
                ("particles", C.c_int32), ("iterations", C.c_int32), ("gn_enable", C.c_int32),
                ("gn_iterations", C.c_int32), ("max_quads", C.c_int32), ("max_contour_points", C.c_int32),
                ("quad_gn_iterations", C.c_int32), ("rig_weighting", C.c_int32)]


class MantisImage(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("step_bytes", C.c_int32), ("mem_kind", C.c_int32),
                ("bgr", C.c_void_p), ("K", C.c_double * 9), ("D", C.c_double * 4),
                ("T_base_cam", C.c_double * 16), ("stamp_ns", C.c_int64), ("frame_id", C.c_char_p)]


class MantisMotion(C.Structure):
    _fields_ = [("delta_pos", C.c_double * 3), ("delta_quat_xyzw", C.c_double * 4)]


class MantisCamResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("publish", C.c_int32), ("n_quads", C.c_int32),
                ("n_hyps", C.c_int32), ("n_scored", C.c_int32), ("position", C.c_double * 3),
                ("orientation_xyzw", C.c_double * 4), ("covariance", C.c_double * 36), ("error", C.c_double),
                ("min_yaw_diff", C.c_double), ("pf_error", C.c_double), ("c2w", C.c_double * 12)]


class MantisResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("publish", C.c_int32), ("n_cams_published", C.c_int32),
                ("num_particles", C.c_int32), ("position", C.c_double * 3), ("orientation_xyzw", C.c_double * 4),
                ("covariance", C.c_double * 36), ("weight", C.c_double), ("min_yaw_diff", C.c_double),
                ("n_quads", C.c_int32), ("gn_iterations", C.c_int32), ("gn_cost", C.c_double),
                ("rng_state_after", C.c_uint64)]


class MantisRigGnInfo(C.Structure):
    _fields_ = [("T_init", C.c_double * 16), ("T_final", C.c_double * 16), ("cost0", C.c_double),
                ("cost", C.c_double), ("valid", C.c_int32), ("iterations", C.c_int32), ("n_obs", C.c_int32),
                ("n_obs_local", C.c_int32)]


class MantisTrackParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("particles", C.c_int32), ("iterations", C.c_int32),
                ("sigma_rot", C.c_double), ("sigma_t", C.c_double), ("min_projections", C.c_int32),
                ("record", C.c_int32), ("max_error", C.c_double)]


class MantisTrackResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("tracked", C.c_int32), ("n_proj", C.c_int32), ("n_scored", C.c_int32),
                ("T_w_b", C.c_double * 16), ("error", C.c_double), ("seed_error", C.c_double),
                ("iter_err", C.c_double * 11), ("iter_pick", C.c_int32 * 10), ("rng_state_after", C.c_uint64)]


class MantisMclParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_particles", C.c_int32), ("sigma_rot", C.c_double),
                ("sigma_t", C.c_double), ("tau", C.c_double), ("resample_frac", C.c_double),
                ("min_projections", C.c_int32), ("record", C.c_int32)]


class MantisMclResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("lost", C.c_int32), ("resampled", C.c_int32), ("n_particles", C.c_int32),
                ("n_valid", C.c_int32), ("best", C.c_int32), ("ess", C.c_double), ("best_error", C.c_double),
                ("T_w_b", C.c_double * 16), ("covariance", C.c_double * 36), ("weight_sum", C.c_uint64),
                ("U", C.c_uint32), ("pad", C.c_uint32), ("rng_state_after", C.c_uint64)]


class MantisMclMode(C.Structure):
    _fields_ = [("ix", C.c_int32), ("iy", C.c_int32), ("yaw_quadrant", C.c_int32), ("n", C.c_int32),
                ("best", C.c_int32), ("pad", C.c_int32), ("weight", C.c_uint64), ("share", C.c_double),
                ("best_error", C.c_double), ("T_w_b", C.c_double * 16), ("covariance", C.c_double * 36)]


class MantisMclModes(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_modes", C.c_int32), ("n_cells", C.c_int32), ("n_outside", C.c_int32),
                ("weight_sum", C.c_uint64), ("outside_weight", C.c_uint64), ("anchor_T_w_b", C.c_double * 16),
                ("mode", MantisMclMode * 8)]


class MantisMclColorParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("enable", C.c_int32), ("color_tau", C.c_double),
                ("color_miss", C.c_double), ("min_color_projections", C.c_int32), ("pad", C.c_int32)]


class MantisRefineParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("iterations", C.c_int32), ("half_window", C.c_int32),
                ("white_thresh", C.c_int32), ("min_weight", C.c_int32), ("min_obs", C.c_int32),
                ("lambda_", C.c_double), ("landmark_pitch", C.c_double), ("max_rms", C.c_double),
                ("record", C.c_int32), ("pad", C.c_int32)]


class MantisRefineResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("refined", C.c_int32), ("iterations_run", C.c_int32), ("n_cand", C.c_int32),
                ("T_w_b", C.c_double * 16), ("n_obs", C.c_int32 * 11), ("pad", C.c_int32), ("rms", C.c_double * 11),
                ("delta", (C.c_double * 6) * 10), ("covariance", C.c_double * 36)]


class MantisSmoothParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("iterations", C.c_int32), ("half_window", C.c_int32),
                ("white_thresh", C.c_int32), ("min_weight", C.c_int32), ("min_obs", C.c_int32),
                ("lambda_", C.c_double), ("landmark_pitch", C.c_double), ("max_rms", C.c_double),
                ("sigma_row", C.c_double), ("sigma_t", C.c_double), ("sigma_rot", C.c_double),
                ("record", C.c_int32), ("pad", C.c_int32)]


class MantisSmoothResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("smoothed", C.c_int32), ("iterations_run", C.c_int32), ("n_cand", C.c_int32),
                ("n_views", C.c_int32), ("n_factors", C.c_int32), ("has_prior", C.c_int32), ("dof", C.c_int32),
                ("n_obs", C.c_int32 * 11), ("pad", C.c_int32), ("rms", C.c_double * 11),
                ("motion_rms", C.c_double * 11), ("cost", C.c_double * 11), ("sigma2", C.c_double)]


class MantisSmoothView(C.Structure):
    _fields_ = [("n_obs", C.c_int32), ("pad", C.c_int32), ("rms", C.c_double), ("T_w_b", C.c_double * 16),
                ("covariance", C.c_double * 36)]


class MantisLagParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("capacity", C.c_int32), ("cams_per_rig", C.c_int32), ("pad", C.c_int32),
                ("smooth", MantisSmoothParams)]


class MantisLagInfo(C.Structure):
    _fields_ = [("pushes", C.c_int64), ("oldest_stamp_ns", C.c_int64), ("n_views", C.c_int32),
                ("has_prior", C.c_int32), ("drop_reason", C.c_int32), ("slid", C.c_int32)]


class MantisRefineRobustParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("loss", C.c_int32), ("tuning", C.c_double), ("scale_floor", C.c_double)]


class MantisRefineRobustStats(C.Structure):
    _fields_ = [("loss", C.c_int32), ("pad", C.c_int32), ("median_key", C.c_uint32 * 11), ("n_down", C.c_int32 * 11),
                ("n_zero", C.c_int32 * 11), ("scale", C.c_double * 11), ("sum_w", C.c_double * 11)]


class MantisCalibRobustStats(C.Structure):
    _fields_ = [("loss", C.c_int32), ("kind", C.c_int32), ("n_rigs", C.c_int32), ("n_cams", C.c_int32),
                ("median_key", C.c_uint32 * 11), ("n_down", C.c_int32 * 11), ("n_zero", C.c_int32 * 11),
                ("pad", C.c_int32), ("scale", C.c_double * 11), ("sum_w", C.c_double * 11),
                ("n_obs_view", C.c_int32 * 256), ("n_zero_view", C.c_int32 * 256), ("sum_w_view", C.c_double * 256),
                ("n_zero_cam", C.c_int32 * 8), ("sum_w_cam", C.c_double * 8)]


class MantisMclModeRefined(C.Structure):
    _fields_ = [("applied", C.c_int32), ("key_kept", C.c_int32), ("n_moved", C.c_int32), ("pad", C.c_int32),
                ("refine", MantisRefineResult)]


class MantisMclRefined(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_modes", C.c_int32), ("apply", C.c_int32), ("n_moved", C.c_int32),
                ("modes", MantisMclModes), ("mode", MantisMclModeRefined * 8)]


class MantisCalibParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("free_cams", C.c_int32), ("min_obs_cam", C.c_int32), ("pad", C.c_int32)]


class MantisCalibResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("calibrated", C.c_int32), ("iterations_run", C.c_int32), ("n_cand", C.c_int32),
                ("n_rigs", C.c_int32), ("n_cams", C.c_int32), ("free_cams", C.c_int32), ("pad", C.c_int32),
                ("T_base_cam", (C.c_double * 16) * 8), ("n_obs", C.c_int32 * 11), ("pad2", C.c_int32),
                ("n_obs_cam", (C.c_int32 * 8) * 11), ("rms", C.c_double * 11), ("rms_cam", C.c_double * 8),
                ("delta_cam", ((C.c_double * 6) * 8) * 10), ("covariance", (C.c_double * 36) * 8)]


class MantisIcalibParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("free_cams", C.c_int32), ("param_mask", C.c_int32),
                ("min_obs_cam", C.c_int32)]


class MantisIcalibResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("calibrated", C.c_int32), ("iterations_run", C.c_int32), ("n_cand", C.c_int32),
                ("n_rigs", C.c_int32), ("n_cams", C.c_int32), ("free_cams", C.c_int32), ("param_mask", C.c_int32),
                ("K", (C.c_double * 4) * 8), ("D", (C.c_double * 4) * 8), ("n_obs", C.c_int32 * 11), ("pad", C.c_int32),
                ("n_obs_cam", (C.c_int32 * 8) * 11), ("rms", C.c_double * 11), ("rms_cam", C.c_double * 8),
                ("delta_cam", ((C.c_double * 8) * 8) * 10), ("covariance", (C.c_double * 64) * 8)]


class MantisRcalibParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("free_ext", C.c_int32), ("free_int", C.c_int32),
                ("param_mask", C.c_int32), ("min_obs_cam", C.c_int32), ("pad", C.c_int32)]


class MantisRcalibResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("calibrated", C.c_int32), ("iterations_run", C.c_int32), ("n_cand", C.c_int32),
                ("n_rigs", C.c_int32), ("n_cams", C.c_int32), ("free_ext", C.c_int32), ("free_int", C.c_int32),
                ("param_mask", C.c_int32), ("pad", C.c_int32),
                ("T_base_cam", (C.c_double * 16) * 8), ("K", (C.c_double * 4) * 8), ("D", (C.c_double * 4) * 8),
                ("n_obs", C.c_int32 * 11), ("pad2", C.c_int32), ("n_obs_cam", (C.c_int32 * 8) * 11),
                ("rms", C.c_double * 11), ("rms_cam", C.c_double * 8),
                ("delta_ext", ((C.c_double * 6) * 8) * 10), ("delta_int", ((C.c_double * 8) * 8) * 10),
                ("cov_ext", (C.c_double * 36) * 8), ("cov_int", (C.c_double * 64) * 8)]


class SynthCamC(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k", C.c_double * 4), ("R_wc", C.c_double * 9), ("pos", C.c_double * 3),
                ("w", C.c_int32), ("h", C.c_int32), ("pad", C.c_int32 * 2)]


class FrameDebug(C.Structure):
    """Layout of mk::FrameDebug == oracle orc_frame_debug."""
    _fields_ = [
        ("reason", C.c_int32), ("publish", C.c_int32), ("n_raw_quads", C.c_int32), ("n_quads", C.c_int32),
        ("quads", (C.c_int32 * 8) * 256), ("test_pts", (C.c_double * 8) * 256),
        ("n_gen", C.c_int32), ("n_hyps", C.c_int32),
        ("hyp_c2w", (C.c_double * 12) * 1024), ("hyp_err", C.c_double * 1024), ("hyp_n", C.c_int32 * 1024),
        ("best1_c2w", C.c_double * 12), ("best1_err", C.c_double),
        ("pf_c2w", C.c_double * 12), ("pf_err", C.c_double), ("pf_iter_err", C.c_double * 11),
        ("shift_err", C.c_double * 81), ("top20_err", C.c_double * 20), ("yaw_err", C.c_double * 4),
        ("yaw_best", C.c_int32), ("min_yaw_diff", C.c_double), ("pub_c2w", C.c_double * 12),
        ("pub_error", C.c_double), ("position", C.c_double * 3), ("orientation_xyzw", C.c_double * 4),
        ("covariance", C.c_double * 36), ("rng_state_after", C.c_uint64), ("n_scored", C.c_int32),
    ]


_lib = None

_SIGS = {
    "mantis_abi_version": (C.c_int32, []),
    "mantis_default_config": (None, [C.POINTER(MantisConfig)]),
    "mantis_create": (C.c_int, [C.POINTER(MantisConfig), C.POINTER(C.c_void_p)]),
    "mantis_destroy": (C.c_int, [C.c_void_p]),
    "mantis_last_error": (C.c_char_p, [C.c_void_p]),
    "mantis_set_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mantis_parse_coordinates": (C.c_int32, [C.c_char_p, C.c_void_p, C.c_int32]),
    "mantis_rng_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mantis_rng_set": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mantis_process": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.POINTER(MantisMotion),
                                 C.POINTER(MantisResult), C.POINTER(MantisCamResult)]),
    "mantis_process_batch": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32,
                                       C.POINTER(MantisResult), C.POINTER(MantisCamResult)]),
    "mantis_canny": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_void_p]),
    "mantis_hysteresis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "mantis_masks": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_void_p, C.c_void_p]),
    "mantis_detect_quads": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_void_p, C.c_int32,
                                      C.POINTER(C.c_int32)]),
    "mantis_score_hypotheses": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_rpp_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mantis_small_batch_frames": (C.c_int32, [C.c_void_p]),
    "mantis_rpp_solve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mantis_quad_gn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p]),
    "mantis_get_rig_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int32)]),
    "mantis_markov_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mantis_markov_sense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mantis_markov_convolve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mantis_markov_weight": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mantis_markov_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mantis_set_prior_pose": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mantis_get_prior_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "mantis_synth_render": (C.c_int, [C.c_void_p, C.POINTER(SynthCamC), C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mantis_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mantis_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mantis_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mantis_synchronize": (C.c_int, [C.c_void_p]),
    "mantis_kernel_times": (C.c_int32, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int32]),
    "mantis_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "mantis_frame_debug_size": (C.c_size_t, []),
    "mantis_get_frame_debug": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "mantis_get_contours": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p]),
    "mantis_frame_counters": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mantis_gn_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    "mantis_gn_solve": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "mantis_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mantis_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "mantis_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_process_rig_sharded": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_int32, C.POINTER(MantisResult), C.POINTER(MantisCamResult)]),
    "mantis_get_rig_gn": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MantisRigGnInfo), C.c_void_p, C.c_int32]),
    "mantis_gn_allreduce": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mantis_score_argmin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                      C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_score_argmin_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                      C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_argmin_pick": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_score_argmin_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_get_rig_weights_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_shard_gauss_offsets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "mantis_default_track_params": (None, [C.c_void_p, C.POINTER(MantisTrackParams)]),
    "mantis_track_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_track_batch": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                     C.POINTER(MantisTrackParams), C.POINTER(MantisTrackResult)]),
    "mantis_track": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.POINTER(MantisMotion),
                               C.POINTER(MantisTrackParams), C.POINTER(MantisResult),
                               C.POINTER(MantisTrackResult)]),
    "mantis_get_track_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_int32)]),
    "mantis_default_mcl_params": (None, [C.POINTER(MantisMclParams)]),
    "mantis_mcl_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_mcl_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.POINTER(MantisMclParams)]),
    "mantis_mcl_init_particles": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MantisMclParams)]),
    "mantis_mcl_step": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.POINTER(MantisMotion),
                                  C.POINTER(MantisResult), C.POINTER(MantisMclResult)]),
    "mantis_mcl_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "mantis_mcl_get_record": (C.c_int, [C.c_void_p] + [C.c_void_p] * 9 + [C.POINTER(C.c_int32)] * 2),
    "mantis_mcl_reset": (C.c_int, [C.c_void_p]),
    "mantis_mcl_modes_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_mcl_init_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                          C.POINTER(MantisMclParams)]),
    "mantis_mcl_modes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MantisMclModes)]),
    "mantis_mcl_select_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "mantis_default_mcl_color_params": (None, [C.POINTER(MantisMclColorParams)]),
    "mantis_mcl_color_sizes": (None, [C.POINTER(C.c_int32)]),
    "mantis_mcl_set_color": (C.c_int, [C.c_void_p, C.POINTER(MantisMclColorParams)]),
    "mantis_mcl_get_color_record": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.POINTER(C.c_int32)] * 2),
    "mantis_mcl_modes_color": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mantis_default_refine_params": (None, [C.POINTER(MantisRefineParams)]),
    "mantis_refine_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_refine_line_flags": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_int32]),
    "mantis_refine_batch": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                      C.POINTER(MantisRefineParams), C.POINTER(MantisRefineResult)]),
    "mantis_refine": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.POINTER(MantisMotion),
                                C.POINTER(MantisRefineParams), C.POINTER(MantisResult),
                                C.POINTER(MantisRefineResult)]),
    "mantis_get_refine_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "mantis_default_smooth_params": (None, [C.POINTER(MantisSmoothParams)]),
    "mantis_smooth_sizes": (None, [C.POINTER(C.c_int32)] * 3),
    "mantis_smooth_batch": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MantisSmoothParams),
                                      C.POINTER(MantisSmoothResult), C.POINTER(MantisSmoothView)]),
    "mantis_get_smooth_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "mantis_get_smooth_pass": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5),
    "mantis_default_lag_params": (None, [C.POINTER(MantisLagParams)]),
    "mantis_lag_sizes": (None, [C.POINTER(C.c_int32)] * 2),
    "mantis_lag_reset": (C.c_int, [C.c_void_p, C.POINTER(MantisLagParams), C.c_void_p, C.c_void_p]),
    "mantis_lag_push": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_void_p, C.c_void_p,
                                  C.POINTER(MantisSmoothResult), C.POINTER(MantisSmoothView), C.POINTER(MantisLagInfo)]),
    "mantis_lag_get_prior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_lag_get_views": (C.c_int, [C.c_void_p, C.POINTER(MantisSmoothView), C.POINTER(C.c_int32)]),
    "mantis_default_refine_robust_params": (None, [C.c_int32, C.POINTER(MantisRefineRobustParams)]),
    "mantis_refine_robust_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_refine_set_robust": (C.c_int, [C.c_void_p, C.POINTER(MantisRefineRobustParams)]),
    "mantis_get_refine_robust": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MantisRefineRobustStats)]),
    "mantis_get_refine_robust_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mantis_default_calib_params": (None, [C.POINTER(MantisCalibParams)]),
    "mantis_calib_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_calibrate_extrinsics": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                              C.POINTER(MantisRefineParams), C.POINTER(MantisCalibParams), C.c_void_p,
                                              C.POINTER(MantisCalibResult)]),
    "mantis_get_calib_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "mantis_default_icalib_params": (None, [C.POINTER(MantisIcalibParams)]),
    "mantis_icalib_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_calibrate_intrinsics": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                              C.POINTER(MantisRefineParams), C.POINTER(MantisIcalibParams), C.c_void_p,
                                              C.POINTER(MantisIcalibResult)]),
    "mantis_get_icalib_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "mantis_default_rcalib_params": (None, [C.POINTER(MantisRcalibParams)]),
    "mantis_rcalib_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_calibrate_rig": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32, C.c_void_p,
                                       C.POINTER(MantisRefineParams), C.POINTER(MantisRcalibParams), C.c_void_p,
                                       C.POINTER(MantisRcalibResult)]),
    "mantis_get_rcalib_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8),
    "mantis_calib_robust_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_calib_set_robust": (C.c_int, [C.c_void_p, C.POINTER(MantisRefineRobustParams)]),
    "mantis_get_calib_robust": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MantisCalibRobustStats)]),
    "mantis_get_calib_robust_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_void_p]),
    "mantis_mcl_refine_sizes": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mantis_mcl_refine_modes": (C.c_int, [C.c_void_p, C.POINTER(MantisImage), C.c_int32, C.c_int32,
                                          C.POINTER(MantisRefineParams), C.c_int32, C.POINTER(MantisMclRefined)]),
}


# include/mantis_ros.h (ROS side of the drop-in; mirrored in mantis_amd/ros.py)
class RosHeader(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_void_p), ("frame_id_len", C.c_uint32)]


class RosImage(C.Structure):
    _fields_ = [("header", RosHeader), ("height", C.c_uint32), ("width", C.c_uint32), ("encoding", C.c_void_p),
                ("encoding_len", C.c_uint32), ("is_bigendian", C.c_uint8), ("step", C.c_uint32),
                ("data", C.c_void_p), ("data_len", C.c_uint32)]


class RosCameraInfo(C.Structure):
    _fields_ = [("header", RosHeader), ("height", C.c_uint32), ("width", C.c_uint32),
                ("distortion_model", C.c_void_p), ("distortion_model_len", C.c_uint32), ("D_len", C.c_uint32),
                ("D", C.c_double * 16), ("K", C.c_double * 9), ("R", C.c_double * 9), ("P", C.c_double * 12),
                ("binning_x", C.c_uint32), ("binning_y", C.c_uint32), ("roi_x_offset", C.c_uint32),
                ("roi_y_offset", C.c_uint32), ("roi_height", C.c_uint32), ("roi_width", C.c_uint32),
                ("roi_do_rectify", C.c_uint8)]


class RosPoseStamped(C.Structure):
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_char * 32), ("position", C.c_double * 3), ("orientation_xyzw", C.c_double * 4),
                ("covariance", C.c_double * 36)]


class RosServiceResponse(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("orientation_xyzw", C.c_double * 4), ("weight", C.c_double),
                ("num_particles", C.c_int32)]


_SIGS.update({
    "mantis_ros_parse_image": (C.c_int64, [C.c_void_p, C.c_size_t, C.POINTER(RosImage)]),
    "mantis_ros_parse_camera_info": (C.c_int64, [C.c_void_p, C.c_size_t, C.POINTER(RosCameraInfo)]),
    "mantis_ros_parse_service_request": (C.c_int64, [C.c_void_p, C.c_size_t, C.POINTER(RosImage),
                                                     C.POINTER(C.c_int32), C.POINTER(RosCameraInfo),
                                                     C.POINTER(C.c_int32), C.c_int32, C.POINTER(MantisMotion)]),
    "mantis_ros_write_pose": (C.c_int64, [C.POINTER(RosPoseStamped), C.c_void_p, C.c_size_t]),
    "mantis_ros_write_service_response": (C.c_int64, [C.POINTER(RosServiceResponse), C.c_void_p, C.c_size_t]),
    "mantis_ros_to_image": (C.c_int, [C.POINTER(RosImage), C.POINTER(RosCameraInfo), C.POINTER(MantisImage)]),
    "mantis_ros_pose_from_result": (C.c_int32, [C.POINTER(MantisCamResult), C.POINTER(RosHeader), C.c_int32,
                                                C.POINTER(RosPoseStamped)]),
    "mantis_ros_service_response_from_result": (C.c_int, [C.POINTER(MantisResult),
                                                           C.POINTER(RosServiceResponse)]),
    "mantis_ros_image_callback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32,
                                            C.c_void_p, C.c_size_t, C.POINTER(C.c_int64),
                                            C.POINTER(MantisCamResult)]),
    "mantis_ros_service_call": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_int64), C.POINTER(MantisResult)]),
})


def lib():
    """Load libmantis_amd.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with __graft_entry__.build() (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            if not hasattr(L, name) and os.environ.get("MANTIS_AMD_LIB"):
                continue  # an older library under A/B (MANTIS_AMD_LIB): entry points it lacks stay unbound
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class MantisError(RuntimeError):
    pass


def default_config(**kw):
    cfg = MantisConfig()
    lib().mantis_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def make_image(bgr, K, D, T_base_cam=None, device_ptr=None, width=None, height=None):
    """mantis_image for a host numpy BGR8 array or a device pointer."""
    im = MantisImage()
    if device_ptr is not None:
        im.width, im.height = width, height
        im.step_bytes = 3 * width
        im.mem_kind = 1
        im.bgr = device_ptr
    else:
        assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
        bgr = np.ascontiguousarray(bgr)
        im.height, im.width = bgr.shape[:2]
        im.step_bytes = bgr.strides[0]
        im.mem_kind = 0
        im.bgr = bgr.ctypes.data
        im._keep = bgr
    Kf = np.asarray(K, np.float64).reshape(9)
    for i in range(9):
        im.K[i] = Kf[i]
    Df = np.asarray(D, np.float64).reshape(4)
    for i in range(4):
        im.D[i] = Df[i]
    T = np.eye(4) if T_base_cam is None else np.asarray(T_base_cam, np.float64)
    for i in range(16):
        im.T_base_cam[i] = T.reshape(16)[i]
    return im


class Batch:
    """mantis_process_batch arguments built once (the bench's throughput path:
    no per-call Python conversion of thousands of ctypes records). run() is
    one C call (ctypes releases the GIL); results stay in .out / .cam_out."""

    def __init__(self, ctx, images, rigs):
        self.ctx, self.n, self.rigs = ctx, len(images), rigs
        self.cams = (MantisImage * self.n)(*images)
        self.out = (MantisResult * rigs)()
        self.cam_out = (MantisCamResult * self.n)()

    def run(self):
        st = lib().mantis_process_batch(self.ctx.h, self.cams, self.rigs, self.n // self.rigs, self.out, self.cam_out)
        self.ctx._chk(st, "process_batch")


class Mantis:
    """One mantis_amd context (one GPU, one HIP stream, one cv::RNG stream)."""

    def __init__(self, cfg=None, **kw):
        L = lib()
        self.cfg = cfg if cfg is not None else default_config(**kw)
        h = C.c_void_p()
        st = L.mantis_create(C.byref(self.cfg), C.byref(h))
        if st != MANTIS_OK:
            raise MantisError(f"mantis_create failed ({st}): {L.mantis_last_error(None).decode()}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().mantis_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, what):
        if st != MANTIS_OK:
            raise MantisError(f"{what} failed ({st}): {lib().mantis_last_error(self.h).decode()}")

    def set_map(self, white, red, green):
        self._map = [np.ascontiguousarray(a, np.float64) for a in (white, red, green)]
        w, r, g = self._map
        self._chk(lib().mantis_set_map(self.h, w.ctypes.data, len(w), r.ctypes.data, len(r), g.ctypes.data, len(g)),
                  "set_map")

    @property
    def rng_state(self):
        v = C.c_uint64()
        self._chk(lib().mantis_rng_get(self.h, C.byref(v)), "rng_get")
        return v.value

    @rng_state.setter
    def rng_state(self, s):
        self._chk(lib().mantis_rng_set(self.h, C.c_uint64(s)), "rng_set")

    def process(self, images, rigs=1):
        n = len(images)
        cams = (MantisImage * n)(*images)
        out = (MantisResult * rigs)()
        cam_out = (MantisCamResult * n)()
        st = lib().mantis_process_batch(self.h, cams, rigs, n // rigs, out, cam_out)
        self._chk(st, "process_batch")
        return list(out), list(cam_out)

    def process_motion(self, images, delta_pos=None, delta_quat_xyzw=None):
        """mantis_process (one rig) with an optional mantisService motion."""
        n = len(images)
        cams = (MantisImage * n)(*images)
        out = MantisResult()
        cam_out = (MantisCamResult * n)()
        mo = None
        if delta_pos is not None:
            mo = MantisMotion()
            for i in range(3):
                mo.delta_pos[i] = delta_pos[i]
            for i in range(4):
                mo.delta_quat_xyzw[i] = delta_quat_xyzw[i]
        st = lib().mantis_process(self.h, cams, n, None if mo is None else C.byref(mo), C.byref(out), cam_out)
        self._chk(st, "process")
        return out, list(cam_out)

    @property
    def prior_pose(self):
        T = np.zeros((4, 4))
        h = C.c_int32()
        self._chk(lib().mantis_get_prior_pose(self.h, T.ctypes.data, C.byref(h)), "get_prior_pose")
        return T if h.value else None

    @prior_pose.setter
    def prior_pose(self, T):
        if T is None:
            self._chk(lib().mantis_set_prior_pose(self.h, None), "set_prior_pose")
        else:
            T = np.ascontiguousarray(T, np.float64)
            self._chk(lib().mantis_set_prior_pose(self.h, T.ctypes.data), "set_prior_pose")

    # rig tracking (mantis_track*, include/mantis.h) -------------------------
    def track_params(self, **params):
        """mantis_default_track_params for this context, then the overrides."""
        p = MantisTrackParams()
        lib().mantis_default_track_params(self.h, C.byref(p))
        for k, v in params.items():
            if k not in dict(MantisTrackParams._fields_) or k == "struct_size":
                raise TypeError(f"track: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def track_batch(self, images, rigs, T_pred, **params):
        """mantis_track_batch: `rigs` rigs (images rig-major) refined from the
        predicted base poses T_pred (rigs x 4 x 4); returns the rigs'
        MantisTrackResult records."""
        n = len(images)
        assert rigs > 0 and n % rigs == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_pred, np.float64).reshape(-1)
        assert T.size == 16 * rigs
        p = self.track_params(**params)
        out = (MantisTrackResult * rigs)()
        self._track_cams = n // rigs
        st = lib().mantis_track_batch(self.h, cams, rigs, n // rigs, T.ctypes.data, C.byref(p), out)
        self._chk(st, "track_batch")
        return list(out)

    def track(self, images, delta_pos=None, delta_quat_xyzw=None, **params):
        """mantis_track: one rig from the context's prior pose and an optional
        mantisService motion; returns (MantisResult, MantisTrackResult).
        result.publish == 0: not tracked, fall back to process_motion()."""
        n = len(images)
        cams = (MantisImage * n)(*images)
        mo = None
        if delta_pos is not None:
            mo = MantisMotion()
            for i in range(3):
                mo.delta_pos[i] = delta_pos[i]
            for i in range(4):
                mo.delta_quat_xyzw[i] = delta_quat_xyzw[i]
        p = self.track_params(**params)
        out = MantisResult()
        tout = MantisTrackResult()
        self._track_cams = n
        st = lib().mantis_track(self.h, cams, n, None if mo is None else C.byref(mo), C.byref(p), C.byref(out),
                                C.byref(tout))
        self._chk(st, "track")
        return out, tout

    def track_record(self, rig, iteration):
        """Record of rig `rig` of the last track call made with record=1
        (mantis_get_track_record), iteration 1 .. iterations or -1 = the seed:
        (T_w_b [P, 4, 4], c2w [P, C, 12], sums [P, C] int64, counts [P, C] int32)."""
        Cn = getattr(self, "_track_cams", None)
        if Cn is None:
            raise MantisError("track_record: no track call on this context")
        T = np.zeros((96, 16))  # the record's particle count is at most 96
        c2w = np.zeros(96 * Cn * 12)
        sums = np.zeros(96 * Cn, np.int64)
        cnt = np.zeros(96 * Cn, np.int32)
        npart = C.c_int32()
        self._chk(lib().mantis_get_track_record(self.h, rig, iteration, T.ctypes.data, c2w.ctypes.data,
                                                sums.ctypes.data, cnt.ctypes.data, C.byref(npart)), "get_track_record")
        P = npart.value
        return (T[:P].reshape(P, 4, 4).copy(), c2w[: P * Cn * 12].reshape(P, Cn, 12).copy(),
                sums[: P * Cn].reshape(P, Cn).copy(), cnt[: P * Cn].reshape(P, Cn).copy())

    # line refinement (mantis_refine*, include/mantis.h) ----------------------
    def refine_params(self, **params):
        """mantis_default_refine_params, then the overrides (`lambda_` is the C field `lambda`)."""
        p = MantisRefineParams()
        lib().mantis_default_refine_params(C.byref(p))
        for k, v in params.items():
            if k not in dict(MantisRefineParams._fields_) or k == "struct_size":
                raise TypeError(f"refine: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def refine_batch(self, images, rigs, T_in, **params):
        """mantis_refine_batch: `rigs` rigs (images rig-major) refined on the
        grid lines from the base poses T_in (rigs x 4 x 4); returns the rigs'
        MantisRefineResult records."""
        n = len(images)
        assert rigs > 0 and n % rigs == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_in, np.float64).reshape(-1)
        assert T.size == 16 * rigs
        p = self.refine_params(**params)
        out = (MantisRefineResult * rigs)()
        self._chk(lib().mantis_refine_batch(self.h, cams, rigs, n // rigs, T.ctypes.data, C.byref(p), out),
                  "refine_batch")
        self._refine_slots = (n // rigs) * out[0].n_cand
        return list(out)

    def refine(self, images, delta_pos=None, delta_quat_xyzw=None, **params):
        """mantis_refine: one rig from the context's prior pose and an optional
        mantisService motion; returns (MantisResult, MantisRefineResult).
        result.publish == 0: not refined, fall back to process_motion()."""
        n = len(images)
        cams = (MantisImage * n)(*images)
        mo = None
        if delta_pos is not None:
            mo = MantisMotion()
            for i in range(3):
                mo.delta_pos[i] = delta_pos[i]
            for i in range(4):
                mo.delta_quat_xyzw[i] = delta_quat_xyzw[i]
        p = self.refine_params(**params)
        out = MantisResult()
        rout = MantisRefineResult()
        st = lib().mantis_refine(self.h, cams, n, None if mo is None else C.byref(mo), C.byref(p), C.byref(out),
                                 C.byref(rout))
        self._chk(st, "refine")
        self._refine_slots = n * rout.n_cand
        return out, rout

    def refine_record(self, rig, pass_):
        """Pass `pass_` (0 .. the rig's iterations_run) of rig `rig` of the last
        refine call made with record=1 (mantis_get_refine_record): (T_w_b
        [4, 4], codes, Sw, Skw [slots] int32, rows [slots, 7], acc28 [28]);
        slot = camera x n_cand + candidate."""
        ns = getattr(self, "_refine_slots", None)
        if ns is None:
            raise MantisError("refine_record: no refine call on this context")
        T = np.zeros((4, 4))
        codes = np.zeros(ns, np.int32)
        Sw = np.zeros(ns, np.int32)
        Skw = np.zeros(ns, np.int32)
        rows = np.zeros((ns, 7))
        acc = np.zeros(28)
        self._chk(lib().mantis_get_refine_record(self.h, rig, pass_, T.ctypes.data, codes.ctypes.data, Sw.ctypes.data,
                                                 Skw.ctypes.data, rows.ctypes.data, acc.ctypes.data),
                  "get_refine_record")
        return T, codes, Sw, Skw, rows, acc

    # window smoothing (mantis_smooth*, include/mantis.h) ---------------------
    def smooth_params(self, **params):
        """mantis_default_smooth_params, then the overrides (`lambda_` is the C field `lambda`)."""
        p = MantisSmoothParams()
        lib().mantis_default_smooth_params(C.byref(p))
        for k, v in params.items():
            if k not in dict(MantisSmoothParams._fields_) or k == "struct_size":
                raise TypeError(f"smooth: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def smooth_batch(self, images, windows, views, T_in, motions=None, prior_T=None, prior_cov=None, **params):
        """mantis_smooth_batch: `windows` windows of `views` views (images
        window-major, then view, then camera) from the base poses T_in
        (windows x views x 4 x 4). motions: windows x (views - 1) x 7 =
        delta_pos | delta_quat_xyzw (a zero quaternion: no factor on that
        step). prior_T (windows x 4 x 4) with prior_cov (windows x 6 x 6):
        the optional prior on view 0. Returns (results [windows],
        views [windows][views])."""
        n = len(images)
        assert windows > 0 and views > 0 and n % (windows * views) == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_in, np.float64).reshape(-1)
        assert T.size == 16 * windows * views
        mo = None
        if motions is not None:
            mo = np.ascontiguousarray(motions, np.float64).reshape(-1)
            assert mo.size == 7 * windows * (views - 1)
        pT = pC = None
        if prior_T is not None:
            pT = np.ascontiguousarray(prior_T, np.float64).reshape(-1)
            assert pT.size == 16 * windows
        if prior_cov is not None:
            pC = np.ascontiguousarray(prior_cov, np.float64).reshape(-1)
            assert pC.size == 36 * windows
        p = self.smooth_params(**params)
        out = (MantisSmoothResult * windows)()
        vw = (MantisSmoothView * (windows * views))()
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        self._chk(lib().mantis_smooth_batch(self.h, cams, windows, views, n // (windows * views), T.ctypes.data, ptr(mo),
                                            ptr(pT), ptr(pC), C.byref(p), out, vw), "smooth_batch")
        self._smooth_shape = (views, (n // (windows * views)) * out[0].n_cand)
        return list(out), [[vw[w * views + k] for k in range(views)] for w in range(windows)]

    def smooth_record(self, window, view, pass_):
        """mantis_get_smooth_record: refine_record's tuple for view `view` of
        window `window`, pass `pass_` (0 .. the window's iterations_run) of
        the last smooth call made with record=1."""
        shape = getattr(self, "_smooth_shape", None)
        if shape is None:
            raise MantisError("smooth_record: no smooth call on this context")
        ns = shape[1]
        T = np.zeros((4, 4))
        codes = np.zeros(ns, np.int32)
        Sw = np.zeros(ns, np.int32)
        Skw = np.zeros(ns, np.int32)
        rows = np.zeros((ns, 7))
        acc = np.zeros(28)
        self._chk(lib().mantis_get_smooth_record(self.h, window, view, pass_, T.ctypes.data, codes.ctypes.data,
                                                 Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data, acc.ctypes.data),
                  "get_smooth_record")
        return T, codes, Sw, Skw, rows, acc

    def smooth_pass_record(self, window, pass_):
        """mantis_get_smooth_pass: (e [N - 1, 6], J [N - 1, 2, 6, 6] = Ja | Jb,
        prior_e [6], prior_J [6, 6], delta [N, 6]) of pass `pass_` of window
        `window` of the last smooth call made with record=1."""
        shape = getattr(self, "_smooth_shape", None)
        if shape is None:
            raise MantisError("smooth_pass_record: no smooth call on this context")
        N = shape[0]
        e = np.zeros((max(N - 1, 0), 6))
        J = np.zeros((max(N - 1, 0), 2, 6, 6))
        pe = np.zeros(6)
        pJ = np.zeros((6, 6))
        delta = np.zeros((N, 6))
        self._chk(lib().mantis_get_smooth_pass(self.h, window, pass_, e.ctypes.data if e.size else None,
                                               J.ctypes.data if J.size else None, pe.ctypes.data, pJ.ctypes.data,
                                               delta.ctypes.data), "get_smooth_pass")
        return e, J, pe, pJ, delta

    # fixed-lag smoothing (mantis_lag_*, include/mantis.h) ----------------------
    LAG_DROPS = {0: "kept", 1: "no_factor", 2: "not_ok", 3: "h00", 4: "lambda", 5: "cov"}

    def lag_params(self, capacity=None, cams_per_rig=None, **smooth):
        """mantis_default_lag_params, then the overrides (`smooth`: fields of the embedded MantisSmoothParams)."""
        p = MantisLagParams()
        lib().mantis_default_lag_params(C.byref(p))
        if capacity is not None:
            p.capacity = capacity
        if cams_per_rig is not None:
            p.cams_per_rig = cams_per_rig
        for k, v in smooth.items():
            if k not in dict(MantisSmoothParams._fields_) or k == "struct_size":
                raise TypeError(f"lag: unknown parameter {k!r}")
            setattr(p.smooth, k, v)
        return p

    def lag_reset(self, capacity=None, cams_per_rig=None, prior_T=None, prior_cov=None, **smooth):
        """mantis_lag_reset: empty the window and fix its shape; prior_T (4 x 4) with prior_cov (6 x 6): the
        optional prior on the first view."""
        p = self.lag_params(capacity, cams_per_rig, **smooth)
        pT = None if prior_T is None else np.ascontiguousarray(prior_T, np.float64).reshape(16)
        pC = None if prior_cov is None else np.ascontiguousarray(prior_cov, np.float64).reshape(36)
        self._chk(lib().mantis_lag_reset(self.h, C.byref(p), None if pT is None else pT.ctypes.data,
                                         None if pC is None else pC.ctypes.data), "lag_reset")
        self._lag = p

    def lag_push(self, images, motion=None, T_start=None):
        """mantis_lag_push: one view of cams_per_rig images. motion: delta_pos | delta_quat_xyzw (7), the step
        from the newest held view (None only on the first push; a zero quaternion: no factor). T_start (4 x 4):
        None lets the device form T_newest Delta. Returns (result, views held [newest last], info)."""
        p = getattr(self, "_lag", None)
        if p is None:
            raise MantisError("lag_push: no lag_reset on this context")
        cams = (MantisImage * len(images))(*images)
        mo = None if motion is None else np.ascontiguousarray(motion, np.float64).reshape(7)
        T = None if T_start is None else np.ascontiguousarray(T_start, np.float64).reshape(16)
        out, info = MantisSmoothResult(), MantisLagInfo()
        vw = (MantisSmoothView * p.capacity)()
        self._chk(lib().mantis_lag_push(self.h, cams, None if mo is None else mo.ctypes.data,
                                        None if T is None else T.ctypes.data, C.byref(out), vw, C.byref(info)), "lag_push")
        self._smooth_shape = (out.n_views, p.cams_per_rig * out.n_cand)
        return out, [vw[k] for k in range(out.n_views)], info

    def lag_prior(self):
        """mantis_lag_get_prior: (has, T [4, 4], cov [6, 6], drop_reason) of the prior the next push's solve will use."""
        T, cov = np.zeros((4, 4)), np.zeros((6, 6))
        has, why = C.c_int32(0), C.c_int32(0)
        self._chk(lib().mantis_lag_get_prior(self.h, T.ctypes.data, cov.ctypes.data, C.byref(has), C.byref(why)),
                  "lag_get_prior")
        return bool(has.value), T, cov, why.value

    def lag_views(self):
        """mantis_lag_get_views: the last push's views again."""
        p = getattr(self, "_lag", None)
        if p is None:
            raise MantisError("lag_views: no lag_reset on this context")
        vw = (MantisSmoothView * p.capacity)()
        n = C.c_int32(p.capacity)
        self._chk(lib().mantis_lag_get_views(self.h, vw, C.byref(n)), "lag_get_views")
        return [vw[k] for k in range(n.value)]

    REFINE_LOSSES = {None: 0, "none": 0, "huber": 1, "tukey": 2}

    def set_refine_robust(self, loss=None, **params):
        """mantis_refine_set_robust: the robust rows of every later refine call
        on this context (refine, refine_batch, mcl_refine_modes). loss: None
        (NULL: off), 0 / "none", 1 / "huber", 2 / "tukey"; `tuning` and
        `scale_floor` override mantis_default_refine_robust_params."""
        if loss is None and not params:
            self._chk(lib().mantis_refine_set_robust(self.h, None), "refine_set_robust")
            return
        p = MantisRefineRobustParams()
        lib().mantis_default_refine_robust_params(self.REFINE_LOSSES.get(loss, loss), C.byref(p))
        for k, v in params.items():
            if k not in ("tuning", "scale_floor"):
                raise TypeError(f"refine robust: unknown parameter {k!r}")
            setattr(p, k, v)
        self._chk(lib().mantis_refine_set_robust(self.h, C.byref(p)), "refine_set_robust")

    def refine_robust_stats(self, rig=0):
        """mantis_get_refine_robust: the MantisRefineRobustStats of rig `rig` of
        the last refine call (made with the robust rows on)."""
        st = MantisRefineRobustStats()
        self._chk(lib().mantis_get_refine_robust(self.h, rig, C.byref(st)), "get_refine_robust")
        return st

    def refine_robust_record(self, rig, pass_):
        """mantis_get_refine_robust_record: (keys uint32 [slots], weights
        [slots]) of pass `pass_` of rig `rig` of the last refine call, made
        with the robust rows on and record=1; 0 in rejected slots."""
        ns = getattr(self, "_refine_slots", None)
        if ns is None:
            raise MantisError("refine_robust_record: no refine call on this context")
        keys = np.zeros(ns, np.uint32)
        w = np.zeros(ns)
        self._chk(lib().mantis_get_refine_robust_record(self.h, rig, pass_, keys.ctypes.data, w.ctypes.data),
                  "get_refine_robust_record")
        return keys, w

    def line_flags(self, pitch=0.08):
        """mantis_refine_line_flags: one byte per landmark of the current map
        (bit 0: a neighbour at +- pitch along x, bit 1: along y)."""
        n = sum(len(a) for a in self._map)
        f = np.zeros(n, np.uint8)
        self._chk(lib().mantis_refine_line_flags(self.h, float(pitch), f.ctypes.data, n), "refine_line_flags")
        return f

    # extrinsic calibration (mantis_calibrate_extrinsics, include/mantis.h) ----
    def calib_params(self, free_cams, **params):
        """mantis_default_calib_params with `free_cams` (a bit mask or an iterable of camera indices)."""
        p = MantisCalibParams()
        lib().mantis_default_calib_params(C.byref(p))
        if not isinstance(free_cams, int):
            free_cams = sum(1 << int(c) for c in free_cams)
        p.free_cams = free_cams
        for k, v in params.items():
            if k != "min_obs_cam":
                raise TypeError(f"calib: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def calibrate_extrinsics(self, images, views, T_in, free_cams, min_obs_cam=None, **refine_params):
        """mantis_calibrate_extrinsics: `views` views of one rig (images
        view-major, every view with the rig's nominal T_base_cam) from the base
        poses T_in (views x 4 x 4); `free_cams` names the cameras whose
        extrinsics are unknown. Returns (T_w_b [views, 4, 4], MantisCalibResult)."""
        n = len(images)
        assert views > 0 and n % views == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_in, np.float64).reshape(-1)
        assert T.size == 16 * views
        p = self.refine_params(**refine_params)
        cp = self.calib_params(free_cams, **({} if min_obs_cam is None else {"min_obs_cam": min_obs_cam}))
        T_out = np.zeros((views, 4, 4))
        out = MantisCalibResult()
        self._chk(lib().mantis_calibrate_extrinsics(self.h, cams, views, n // views, T.ctypes.data, C.byref(p),
                                                    C.byref(cp), T_out.ctypes.data, C.byref(out)),
                  "calibrate_extrinsics")
        self._calib_shape = (n // views, out.n_cand)
        return T_out, out

    def calib_record(self, rig, pass_):
        """Pass `pass_` (0 .. iterations_run) of view `rig` of the last
        calibration made with record=1 (mantis_get_calib_record): (T_w_b
        [4, 4], T_base_cam [C, 4, 4], codes, Sw, Skw [slots] int32, rows
        [slots, 13], acc91 [C, 91]); slot = camera x n_cand + candidate."""
        shape = getattr(self, "_calib_shape", None)
        if shape is None:
            raise MantisError("calib_record: no calibration on this context")
        Cn, nc = shape
        ns = Cn * nc
        T = np.zeros((4, 4))
        E = np.zeros((Cn, 4, 4))
        codes = np.zeros(ns, np.int32)
        Sw = np.zeros(ns, np.int32)
        Skw = np.zeros(ns, np.int32)
        rows = np.zeros((ns, 13))
        acc = np.zeros((Cn, 91))
        self._chk(lib().mantis_get_calib_record(self.h, rig, pass_, T.ctypes.data, E.ctypes.data, codes.ctypes.data,
                                                Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data, acc.ctypes.data),
                  "get_calib_record")
        return T, E, codes, Sw, Skw, rows, acc

    # intrinsic calibration (mantis_calibrate_intrinsics, include/mantis.h) ----
    def icalib_params(self, free_cams, **params):
        """mantis_default_icalib_params with `free_cams` (a bit mask or an iterable of camera indices)."""
        p = MantisIcalibParams()
        lib().mantis_default_icalib_params(C.byref(p))
        if not isinstance(free_cams, int):
            free_cams = sum(1 << int(c) for c in free_cams)
        p.free_cams = free_cams
        for k, v in params.items():
            if k not in ("param_mask", "min_obs_cam"):
                raise TypeError(f"icalib: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def calibrate_intrinsics(self, images, views, T_in, free_cams, param_mask=None, min_obs_cam=None, **refine_params):
        """mantis_calibrate_intrinsics: `views` views of one rig (images
        view-major, every view with the rig's nominal K, D and T_base_cam) from
        the base poses T_in (views x 4 x 4); `free_cams` names the cameras
        whose intrinsics are unknown, `param_mask` which of (fx, fy, cx, cy,
        k1..k4) are. Returns (T_w_b [views, 4, 4], MantisIcalibResult); a K
        fed back through make_image is rounded to float there."""
        n = len(images)
        assert views > 0 and n % views == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_in, np.float64).reshape(-1)
        assert T.size == 16 * views
        p = self.refine_params(**refine_params)
        kw = {k: v for k, v in (("param_mask", param_mask), ("min_obs_cam", min_obs_cam)) if v is not None}
        ip = self.icalib_params(free_cams, **kw)
        T_out = np.zeros((views, 4, 4))
        out = MantisIcalibResult()
        self._chk(lib().mantis_calibrate_intrinsics(self.h, cams, views, n // views, T.ctypes.data, C.byref(p),
                                                    C.byref(ip), T_out.ctypes.data, C.byref(out)),
                  "calibrate_intrinsics")
        self._icalib_shape = (n // views, out.n_cand)
        return T_out, out

    def icalib_record(self, rig, pass_):
        """Pass `pass_` (0 .. iterations_run) of view `rig` of the last
        intrinsic calibration made with record=1 (mantis_get_icalib_record):
        (T_w_b [4, 4], KD [C, 8] = fx, fy, cx, cy, k1..k4, codes, Sw, Skw
        [slots] int32, rows [slots, 15], acc120 [C, 120]); slot = camera x
        n_cand + candidate."""
        shape = getattr(self, "_icalib_shape", None)
        if shape is None:
            raise MantisError("icalib_record: no intrinsic calibration on this context")
        Cn, nc = shape
        ns = Cn * nc
        T = np.zeros((4, 4))
        KD = np.zeros((Cn, 8))
        codes = np.zeros(ns, np.int32)
        Sw = np.zeros(ns, np.int32)
        Skw = np.zeros(ns, np.int32)
        rows = np.zeros((ns, 15))
        acc = np.zeros((Cn, 120))
        self._chk(lib().mantis_get_icalib_record(self.h, rig, pass_, T.ctypes.data, KD.ctypes.data, codes.ctypes.data,
                                                 Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data, acc.ctypes.data),
                  "get_icalib_record")
        return T, KD, codes, Sw, Skw, rows, acc

    # rig calibration (mantis_calibrate_rig, include/mantis.h) ----------------
    def rcalib_params(self, free_ext, free_int, **params):
        """mantis_default_rcalib_params with `free_ext` and `free_int` (bit masks or iterables of camera indices)."""
        p = MantisRcalibParams()
        lib().mantis_default_rcalib_params(C.byref(p))
        mask = lambda m: m if isinstance(m, int) else sum(1 << int(c) for c in m)
        p.free_ext = mask(free_ext)
        p.free_int = mask(free_int)
        for k, v in params.items():
            if k not in ("param_mask", "min_obs_cam"):
                raise TypeError(f"rcalib: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def calibrate_rig(self, images, views, T_in, free_ext, free_int, param_mask=None, min_obs_cam=None,
                      **refine_params):
        """mantis_calibrate_rig: `views` views of one rig (images view-major,
        every view with the rig's nominal K, D and T_base_cam) from the base
        poses T_in (views x 4 x 4); `free_ext` names the cameras whose
        extrinsics are unknown (one at least stays held), `free_int` those
        whose intrinsics are, `param_mask` which of (fx, fy, cx, cy, k1..k4).
        Returns (T_w_b [views, 4, 4], MantisRcalibResult)."""
        n = len(images)
        assert views > 0 and n % views == 0
        cams = (MantisImage * n)(*images)
        T = np.ascontiguousarray(T_in, np.float64).reshape(-1)
        assert T.size == 16 * views
        p = self.refine_params(**refine_params)
        kw = {k: v for k, v in (("param_mask", param_mask), ("min_obs_cam", min_obs_cam)) if v is not None}
        rp = self.rcalib_params(free_ext, free_int, **kw)
        T_out = np.zeros((views, 4, 4))
        out = MantisRcalibResult()
        self._chk(lib().mantis_calibrate_rig(self.h, cams, views, n // views, T.ctypes.data, C.byref(p), C.byref(rp),
                                             T_out.ctypes.data, C.byref(out)),
                  "calibrate_rig")
        self._rcalib_shape = (n // views, out.n_cand)
        return T_out, out

    def rcalib_record(self, rig, pass_):
        """Pass `pass_` (0 .. iterations_run) of view `rig` of the last rig
        calibration made with record=1 (mantis_get_rcalib_record): (T_w_b
        [4, 4], T_base_cam [C, 4, 4], KD [C, 8] = fx, fy, cx, cy, k1..k4,
        codes, Sw, Skw [slots] int32, rows [slots, 21], acc231 [C, 231]);
        slot = camera x n_cand + candidate."""
        shape = getattr(self, "_rcalib_shape", None)
        if shape is None:
            raise MantisError("rcalib_record: no rig calibration on this context")
        Cn, nc = shape
        ns = Cn * nc
        T = np.zeros((4, 4))
        E = np.zeros((Cn, 4, 4))
        KD = np.zeros((Cn, 8))
        codes = np.zeros(ns, np.int32)
        Sw = np.zeros(ns, np.int32)
        Skw = np.zeros(ns, np.int32)
        rows = np.zeros((ns, 21))
        acc = np.zeros((Cn, 231))
        self._chk(lib().mantis_get_rcalib_record(self.h, rig, pass_, T.ctypes.data, E.ctypes.data, KD.ctypes.data,
                                                 codes.ctypes.data, Sw.ctypes.data, Skw.ctypes.data, rows.ctypes.data,
                                                 acc.ctypes.data),
                  "get_rcalib_record")
        return T, E, KD, codes, Sw, Skw, rows, acc

    # the calibrations' robust rows (mantis_calib_set_robust, include/mantis.h) ----
    CALIB_KINDS = {"ext": 0, "int": 1, "rig": 2}

    def set_calib_robust(self, loss=None, **params):
        """mantis_calib_set_robust: the robust rows of every later calibration
        on this context (all three kinds). loss: None (NULL: off), 0 / "none",
        1 / "huber", 2 / "tukey"; `tuning` and `scale_floor` override
        mantis_default_refine_robust_params."""
        if loss is None and not params:
            self._chk(lib().mantis_calib_set_robust(self.h, None), "calib_set_robust")
            return
        p = MantisRefineRobustParams()
        lib().mantis_default_refine_robust_params(self.REFINE_LOSSES.get(loss, loss), C.byref(p))
        for k, v in params.items():
            if k not in ("tuning", "scale_floor"):
                raise TypeError(f"calib robust: unknown parameter {k!r}")
            setattr(p, k, v)
        self._chk(lib().mantis_calib_set_robust(self.h, C.byref(p)), "calib_set_robust")

    def calib_robust_stats(self, kind):
        """mantis_get_calib_robust: the MantisCalibRobustStats of the last
        calibration of `kind` (0 / "ext", 1 / "int", 2 / "rig"), made with the
        robust rows on."""
        st = MantisCalibRobustStats()
        self._chk(lib().mantis_get_calib_robust(self.h, self.CALIB_KINDS.get(kind, kind), C.byref(st)),
                  "get_calib_robust")
        return st

    def calib_robust_record(self, kind, rig, pass_):
        """mantis_get_calib_robust_record: (keys uint32 [slots], weights
        [slots]) of pass `pass_` of view `rig` of the last calibration of
        `kind`, made with the robust rows on and record=1; 0 in rejected slots."""
        kind = self.CALIB_KINDS.get(kind, kind)
        names = ("_calib_shape", "_icalib_shape", "_rcalib_shape")
        shape = getattr(self, names[kind], None) if kind in (0, 1, 2) else (0, 0)  # a wrong kind: the library's error
        if shape is None:
            raise MantisError("calib_robust_record: no calibration of that kind on this context")
        ns = shape[0] * shape[1]
        keys = np.zeros(ns, np.uint32)
        w = np.zeros(ns)
        self._chk(lib().mantis_get_calib_robust_record(self.h, kind, rig, pass_, keys.ctypes.data, w.ctypes.data),
                  "get_calib_robust_record")
        return keys, w

    # Monte Carlo localization (mantis_mcl_*, include/mantis.h) ---------------
    def mcl_params(self, **params):
        """mantis_default_mcl_params, then the overrides."""
        p = MantisMclParams()
        lib().mantis_default_mcl_params(C.byref(p))
        for k, v in params.items():
            if k not in dict(MantisMclParams._fields_) or k == "struct_size":
                raise TypeError(f"mcl: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def mcl_init(self, T_mean, sigma_rot0, sigma_t0, **params):
        """mantis_mcl_init: n_particles draws around the base pose T_mean."""
        T = np.ascontiguousarray(T_mean, np.float64).reshape(16)
        p = self.mcl_params(**params)
        self._chk(lib().mantis_mcl_init(self.h, T.ctypes.data, sigma_rot0, sigma_t0, C.byref(p)), "mcl_init")

    def mcl_init_particles(self, T_w_b, **params):
        """mantis_mcl_init_particles: the set from given base poses (N x 4 x 4)."""
        T = np.ascontiguousarray(T_w_b, np.float64).reshape(-1, 16)
        p = self.mcl_params(n_particles=len(T), **params)
        self._chk(lib().mantis_mcl_init_particles(self.h, T.ctypes.data, C.byref(p)), "mcl_init_particles")

    def mcl_step(self, images, delta_pos=None, delta_quat_xyzw=None):
        """mantis_mcl_step: one step on the rig's frames with an optional
        mantisService motion; returns (MantisResult, MantisMclResult)."""
        n = len(images)
        cams = (MantisImage * n)(*images)
        mo = None
        if delta_pos is not None:
            mo = MantisMotion()
            for i in range(3):
                mo.delta_pos[i] = delta_pos[i]
            for i in range(4):
                mo.delta_quat_xyzw[i] = delta_quat_xyzw[i]
        out = MantisResult()
        mout = MantisMclResult()
        st = lib().mantis_mcl_step(self.h, cams, n, None if mo is None else C.byref(mo), C.byref(out), C.byref(mout))
        self._chk(st, "mcl_step")
        return out, mout

    def mcl_particles(self):
        """mantis_mcl_get: (T_w_b [N, 4, 4], log-weights [N])."""
        n = C.c_int32()
        self._chk(lib().mantis_mcl_get(self.h, None, None, C.byref(n)), "mcl_get")
        T = np.zeros((n.value, 4, 4))
        L = np.zeros(n.value)
        self._chk(lib().mantis_mcl_get(self.h, T.ctypes.data, L.ctypes.data, C.byref(n)), "mcl_get")
        return T, L

    def mcl_record(self):
        """mantis_mcl_get_record: the last step's record (record=1) as a dict:
        T_pred [N, 4, 4], c2w [N, C, 12], sums / counts [N, C], L_before /
        L_after [N], q / cum [N] uint64, ancestors [N] int32."""
        n, cn = C.c_int32(), C.c_int32()
        none = [None] * 9
        self._chk(lib().mantis_mcl_get_record(self.h, *none, C.byref(n), C.byref(cn)), "mcl_get_record")
        N, Cn = n.value, cn.value
        r = {"T_pred": np.zeros((N, 4, 4)), "c2w": np.zeros((N, Cn, 12)), "sums": np.zeros((N, Cn), np.int64),
             "counts": np.zeros((N, Cn), np.int32), "L_before": np.zeros(N), "L_after": np.zeros(N),
             "q": np.zeros(N, np.uint64), "cum": np.zeros(N, np.uint64), "ancestors": np.zeros(N, np.int32)}
        self._chk(lib().mantis_mcl_get_record(self.h, *[a.ctypes.data for a in r.values()], C.byref(n), C.byref(cn)),
                  "mcl_get_record")
        return r

    def mcl_reset(self):
        self._chk(lib().mantis_mcl_reset(self.h), "mcl_reset")

    def mcl_init_lattice(self, T_mean, sigma_rot0, sigma_t0, cells_x, cells_y, **params):
        """mantis_mcl_init_lattice: mcl_init's draws spread over the (2 cells_x
        + 1) x (2 cells_y + 1) lattice of the floor grid around T_mean."""
        T = np.ascontiguousarray(T_mean, np.float64).reshape(16)
        p = self.mcl_params(**params)
        self._chk(lib().mantis_mcl_init_lattice(self.h, T.ctypes.data, sigma_rot0, sigma_t0, cells_x, cells_y,
                                                C.byref(p)), "mcl_init_lattice")

    def mcl_modes(self, max_modes=8):
        """mantis_mcl_modes: the last step's set as one estimate per lattice
        cell and yaw quadrant, heaviest first (MantisMclModes)."""
        out = MantisMclModes()
        self._chk(lib().mantis_mcl_modes(self.h, max_modes, C.byref(out)), "mcl_modes")
        return out

    def mcl_select_mode(self, k):
        """mantis_mcl_select_mode: keep mode k of the last mcl_modes call."""
        self._chk(lib().mantis_mcl_select_mode(self.h, k), "mcl_select_mode")

    def mcl_color_params(self, **params):
        """mantis_default_mcl_color_params, then the overrides."""
        p = MantisMclColorParams()
        lib().mantis_default_mcl_color_params(C.byref(p))
        for k, v in params.items():
            if k not in dict(MantisMclColorParams._fields_) or k == "struct_size":
                raise TypeError(f"mcl colour: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def mcl_set_color(self, enable, **params):
        """mantis_mcl_set_color: 0 = off, 1 = score and record the green
        border's COLOR evidence, 2 = also fold it into the log-weights."""
        p = self.mcl_color_params(enable=enable, **params)
        self._chk(lib().mantis_mcl_set_color(self.h, C.byref(p)), "mcl_set_color")

    def mcl_color_record(self):
        """mantis_mcl_get_color_record: the last step's colour record as a
        dict: csums [N, C] int64, ccounts [N, C] int32, Ec / charge [N]."""
        n, cn = C.c_int32(), C.c_int32()
        self._chk(lib().mantis_mcl_get_color_record(self.h, None, None, None, None, C.byref(n), C.byref(cn)),
                  "mcl_get_color_record")
        N, Cn = n.value, cn.value
        r = {"csums": np.zeros((N, Cn), np.int64), "ccounts": np.zeros((N, Cn), np.int32), "Ec": np.zeros(N),
             "charge": np.zeros(N)}
        self._chk(lib().mantis_mcl_get_color_record(self.h, *[a.ctypes.data for a in r.values()], C.byref(n),
                                                    C.byref(cn)), "mcl_get_color_record")
        return r

    def mcl_modes_color(self):
        """mantis_mcl_modes_color: (Ec [8], pooled green count [8]) of the
        heaviest particle of each mode of the last mcl_modes call."""
        e, n = np.zeros(8), np.zeros(8, np.int32)
        self._chk(lib().mantis_mcl_modes_color(self.h, e.ctypes.data, n.ctypes.data), "mcl_modes_color")
        return e, n

    def mcl_refine_modes(self, images, max_modes=8, apply=False, **refine_params):
        """mantis_mcl_refine_modes: every mode of the last step refined on the
        grid lines of that step's frames `images`; apply=True also moves each
        refined mode's particles rigidly onto its refined pose (once per
        step). Returns the MantisMclRefined record (its `modes` is
        mcl_modes(max_modes)'s answer); with record=1 refine_record(k, pass)
        reads mode k's passes."""
        n = len(images)
        cams = (MantisImage * n)(*images)
        p = self.refine_params(**refine_params)
        out = MantisMclRefined()
        self._chk(lib().mantis_mcl_refine_modes(self.h, cams, n, max_modes, C.byref(p), 1 if apply else 0,
                                                C.byref(out)), "mcl_refine_modes")
        if out.n_modes > 0:
            self._refine_slots = n * out.mode[0].refine.n_cand
        return out

    def process_sharded(self, images, rigs, cam_index, cams_per_rig):
        """Camera-sharded rig call (mantis_process_rig_sharded): images are this
        rank's cameras cam_index of each rig, rig-major. Returns (rig results,
        every camera's result in global order)."""
        n = len(images)
        n_local = len(cam_index)
        assert n == rigs * n_local
        cams = (MantisImage * n)(*images)
        idx = np.ascontiguousarray(cam_index, np.int32)
        out = (MantisResult * rigs)()
        cam_out = (MantisCamResult * (rigs * cams_per_rig))()
        st = lib().mantis_process_rig_sharded(self.h, cams, rigs, n_local, idx.ctypes.data, cams_per_rig, out, cam_out)
        self._chk(st, "process_rig_sharded")
        return list(out), list(cam_out)

    def shard_gauss_offsets(self, pairs, n_global, gidx, per_frame):
        """k_gauss_offsets_global on gathered (global index, PF flag) pairs
        (mantis_shard_gauss_offsets): (offsets of the local frames gidx, total)."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        gidx = np.ascontiguousarray(gidx, np.int32)
        off = np.zeros(len(gidx), np.int32)
        tot = C.c_int32()
        self._chk(lib().mantis_shard_gauss_offsets(self.h, pairs.ctypes.data, len(pairs), n_global, gidx.ctypes.data,
                                                   len(gidx), per_frame, off.ctypes.data, C.byref(tot)),
                  "shard_gauss_offsets")
        return off, tot.value

    def comm_info(self):
        nr, rk = C.c_int32(), C.c_int32()
        self._chk(lib().mantis_comm_info(self.h, C.byref(nr), C.byref(rk)), "comm_info")
        return nr.value, rk.value

    def rig_gn(self, rig, cap=4096):
        """(mantis_rig_gn_info, this rank's correspondences [cam, u, v, X, Y, Z])."""
        info = MantisRigGnInfo()
        obs = np.zeros((cap, 6))
        self._chk(lib().mantis_get_rig_gn(self.h, rig, C.byref(info), obs.ctypes.data, cap), "get_rig_gn")
        return info, obs[: min(cap, info.n_obs_local if info.valid else 0)].copy()

    def contours(self, i, max_borders=8192, max_points=1 << 20):
        """Border-following output of frame i of the last batch: a list of
        (points (n, 2) int32, hole) in the library's border order."""
        cnt = np.zeros(max_borders, np.int32)
        hol = np.zeros(max_borders, np.int32)
        pts = np.zeros(2 * max_points, np.int32)
        nb = C.c_int32(0)
        self._chk(lib().mantis_get_contours(self.h, i, cnt.ctypes.data, hol.ctypes.data, max_borders,
                                            pts.ctypes.data, max_points, C.byref(nb)), "get_contours")
        out, k = [], 0
        for b in range(nb.value):
            out.append((pts[2 * k: 2 * (k + cnt[b])].reshape(-1, 2).copy(), int(hol[b])))
            k += int(cnt[b])
        return out

    def frame_counters(self, i):
        out = np.zeros(32, np.int32)
        k = lib().mantis_frame_counters(self.h, i, out.ctypes.data, 32)
        if k < 0:
            raise MantisError("frame_counters: bad frame index")
        return out[:k]

    def frame_debug(self, i):
        d = FrameDebug()
        assert C.sizeof(d) == lib().mantis_frame_debug_size(), "FrameDebug layout mismatch"
        self._chk(lib().mantis_get_frame_debug(self.h, i, C.byref(d), C.sizeof(d)), "get_frame_debug")
        return d

    def canny(self, img):
        out = np.zeros((img.height, img.width), np.uint8)
        self._chk(lib().mantis_canny(self.h, C.byref(img), out.ctypes.data), "canny")
        return out

    def hysteresis(self, cls):
        """cv::Canny's hysteresis on a class plane (0 none, 1 weak candidate, 2 strong)."""
        cls = np.ascontiguousarray(cls, np.uint8)
        h, w = cls.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(lib().mantis_hysteresis(self.h, cls.ctypes.data, w, h, out.ctypes.data), "hysteresis")
        return out

    def masks(self, img):
        det = np.zeros((img.height, img.width), np.uint8)
        mask = np.zeros((img.height, img.width), np.uint8)
        self._chk(lib().mantis_masks(self.h, C.byref(img), det.ctypes.data, mask.ctypes.data), "masks")
        return det, mask

    def detect_quads(self, img, max_quads=256):
        corners = np.zeros((max_quads, 8), np.int32)
        n = C.c_int32()
        self._chk(lib().mantis_detect_quads(self.h, C.byref(img), corners.ctypes.data, max_quads, C.byref(n)),
                  "detect_quads")
        return corners[: n.value].copy()

    def score(self, img, c2w, fast=True, mask=None):
        c2w = np.ascontiguousarray(c2w, np.float64).reshape(-1, 12)
        n = len(c2w)
        err = np.zeros(n)
        npj = np.zeros(n, np.int32)
        mptr = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            mptr = mask.ctypes.data
        self._chk(lib().mantis_score_hypotheses(self.h, C.byref(img), mptr, c2w.ctypes.data, n, int(fast),
                                                err.ctypes.data, npj.ctypes.data), "score_hypotheses")
        return err, npj

    def comm_init(self, rank, world, dist=None):
        """RCCL communicator for this context: rank 0 creates the unique id and
        torch.distributed (any backend) broadcasts it."""
        uid = (C.c_uint8 * 128)()
        if rank == 0:
            self._chk(lib().mantis_comm_unique_id(uid), "comm_unique_id")
        if dist is not None and world > 1:
            box = [bytes(uid)]
            dist.broadcast_object_list(box, src=0)
            C.memmove(uid, box[0], 128)
        self._chk(lib().mantis_comm_init(self.h, uid, world, rank), "comm_init")

    def score_argmin(self, img, c2w, index_base=0, use_comm=False, mask=None):
        """Dense scoring + first-minimum argmin (config 5); returns (err, global index)."""
        c2w = np.ascontiguousarray(c2w, np.float64).reshape(-1, 12)
        e = C.c_double()
        i = C.c_int64()
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._chk(lib().mantis_score_argmin(self.h, C.byref(img), None if mk is None else mk.ctypes.data,
                                            c2w.ctypes.data, len(c2w), index_base, int(use_comm), C.byref(e),
                                            C.byref(i)), "score_argmin")
        return e.value, i.value

    def score_argmin_dev(self, img, c2w_dev, n, index_base=0, use_comm=False, mask_dev=None):
        """score_argmin on device-resident inputs (mantis_score_argmin_dev): c2w_dev = device
        pointer to n x 12 doubles, mask_dev = device pointer to W*H bytes or None."""
        e = C.c_double()
        i = C.c_int64()
        self._chk(lib().mantis_score_argmin_dev(self.h, C.byref(img), None if mask_dev is None else C.c_void_p(mask_dev),
                                                C.c_void_p(c2w_dev), int(n), index_base, int(use_comm), C.byref(e),
                                                C.byref(i)), "score_argmin_dev")
        return e.value, i.value

    def score_argmin_batch(self, imgs, c2w_devs, ns, index_bases=None, use_comm=False, mask_devs=None):
        """mantis_score_argmin_batch: per-frame device hypothesis blocks (and
        masks) scored in one launch; returns [(err, global index)] per frame."""
        nf = len(imgs)
        arr = (MantisImage * nf)(*imgs)
        cp = (C.c_void_p * nf)(*[C.c_void_p(p) for p in c2w_devs])
        mp = None if mask_devs is None else (C.c_void_p * nf)(*[C.c_void_p(p) for p in mask_devs])
        n = np.ascontiguousarray(ns, np.int32)
        ib = np.ascontiguousarray(index_bases if index_bases is not None else np.zeros(nf), np.int64)
        e = np.zeros(nf)
        i = np.zeros(nf, np.int64)
        self._chk(lib().mantis_score_argmin_batch(self.h, arr, nf, mp, cp, n.ctypes.data, ib.ctypes.data,
                                                  int(use_comm), e.ctypes.data, i.ctypes.data), "score_argmin_batch")
        return list(zip(e.tolist(), i.tolist()))

    def rpp(self, img_pts, obj_pts):
        img_pts = np.ascontiguousarray(img_pts, np.float64).reshape(-1, 4, 2)
        obj_pts = np.ascontiguousarray(obj_pts, np.float64).reshape(-1, 4, 3)
        n = len(img_pts)
        R = np.zeros((n, 9))
        t = np.zeros((n, 3))
        e = np.zeros((n, 2))
        s = np.zeros(n, np.int32)
        self._chk(lib().mantis_rpp_batch(self.h, img_pts.ctypes.data, obj_pts.ctypes.data, n, R.ctypes.data,
                                         t.ctypes.data, e.ctypes.data, s.ctypes.data), "rpp_batch")
        return R.reshape(n, 3, 3), t, e, s

    def rpp_solve(self, model, iprts):
        """RPP::Rpp(model, iprts) (RPP.cpp:13-64) on the device for any point
        count 4..12 (mantis_rpp_solve): model 3 x n (or k x 3 x n), iprts 3 x n
        homogeneous with a unit third row (demo.cpp:41-53's layout). Returns
        (R [k,3,3], t [k,3], errs [k,2] = obj_err, img_err, status [k], iterations [k])."""
        m = np.asarray(model, np.float64)
        q = np.asarray(iprts, np.float64)
        if m.ndim == 2:
            m, q = m[None], q[None]
        k, _, npts = m.shape
        if not np.all(q[:, 2, :] == 1.0):
            raise ValueError("rpp_solve: image points must be homogeneous with z = 1")
        obj = np.ascontiguousarray(np.transpose(m, (0, 2, 1)))      # k x n x 3
        img = np.ascontiguousarray(np.transpose(q[:, :2, :], (0, 2, 1)))  # k x n x 2
        R = np.zeros((k, 9))
        t = np.zeros((k, 3))
        e = np.zeros((k, 2))
        s = np.zeros(k, np.int32)
        it = np.zeros(k, np.int32)
        self._chk(lib().mantis_rpp_solve(self.h, img.ctypes.data, obj.ctypes.data, int(npts), int(k), R.ctypes.data,
                                         t.ctypes.data, e.ctypes.data, s.ctypes.data, it.ctypes.data), "rpp_solve")
        return R.reshape(k, 3, 3), t, e, s, it

    def rig_weights(self, rig, cams_per_rig=None):
        """Legacy rig weighting record of rig `rig` (mantis_get_rig_weights):
        (weights[C+1], c2w[C+1, C, 12], sums[C+1, C, 2], chosen slot or -1);
        slot C = the mantisService motion prediction. The buffers are sized from
        the record's own camera count (mantis_get_rig_weights_info); a
        cams_per_rig that disagrees with it is an error."""
        rigs, Cn = C.c_int32(), C.c_int32()
        self._chk(lib().mantis_get_rig_weights_info(self.h, C.byref(rigs), C.byref(Cn)), "get_rig_weights_info")
        Cn = Cn.value
        if cams_per_rig is not None and cams_per_rig != Cn:
            raise MantisError(f"rig_weights: the last batch had {Cn} cameras per rig, not {cams_per_rig}")
        w = np.zeros(Cn + 1)
        c2w = np.zeros((Cn + 1, Cn, 12))
        sums = np.zeros((Cn + 1, Cn, 2))
        ch = C.c_int32()
        self._chk(lib().mantis_get_rig_weights(self.h, rig, w.ctypes.data, c2w.ctypes.data, sums.ctypes.data,
                                               C.byref(ch)), "get_rig_weights")
        return w, c2w, sums, ch.value

    # Markov yaw filter (include/mantis3/Markov.cpp) ----------------------
    def markov_init(self, w2c_R):
        R = np.ascontiguousarray(w2c_R, np.float64).reshape(-1, 9)
        self._markov_n = len(R)
        self._chk(lib().mantis_markov_init(self.h, len(R), R.ctypes.data), "markov_init")

    def _markov_len(self, arr, what):
        n = getattr(self, "_markov_n", None)
        if n is None:
            raise MantisError("markov: no filters (markov_init first)")
        if len(arr) != n:  # the C API reads markov_n entries of each array
            raise MantisError(f"markov: {what} has {len(arr)} entries, the context holds {n} filters")

    def markov_sense(self, w2c_R, active=None):
        R = np.ascontiguousarray(w2c_R, np.float64).reshape(-1, 9)
        a = None if active is None else np.ascontiguousarray(active, np.int32)
        self._markov_len(R, "w2c_R")
        if a is not None:
            self._markov_len(a, "active")
        self._chk(lib().mantis_markov_sense(self.h, R.ctypes.data, None if a is None else a.ctypes.data),
                  "markov_sense")

    def markov_convolve(self, dtheta, dt, active=None):
        th = np.ascontiguousarray(dtheta, np.float64)
        d = np.ascontiguousarray(dt, np.float64)
        a = None if active is None else np.ascontiguousarray(active, np.int32)
        self._markov_len(th, "dtheta")
        self._markov_len(d, "dt")
        if a is not None:
            self._markov_len(a, "active")
        self._chk(lib().mantis_markov_convolve(self.h, th.ctypes.data, d.ctypes.data,
                                               None if a is None else a.ctypes.data), "markov_convolve")

    def markov_weight(self, f, w2c_R, error):
        R = np.ascontiguousarray(w2c_R, np.float64).reshape(-1, 9)
        e = np.ascontiguousarray(error, np.float64).copy()
        self._chk(lib().mantis_markov_weight(self.h, f, R.ctypes.data, len(R), e.ctypes.data), "markov_weight")
        return e

    def markov_get(self):
        n = self._markov_n
        planes = np.zeros((n, 360))
        yaw = np.zeros(n)
        am = np.zeros(n, np.int32)
        self._chk(lib().mantis_markov_get(self.h, planes.ctypes.data, yaw.ctypes.data, am.ctypes.data), "markov_get")
        return planes, yaw, am

    def quad_gn(self, img_pts, obj_pts, R, t, iterations):
        """Per-quad GN after RPP (mantis_quad_gn): (R, t, steps, costs)."""
        img_pts = np.ascontiguousarray(img_pts, np.float64).reshape(-1, 4, 2)
        obj_pts = np.ascontiguousarray(obj_pts, np.float64).reshape(-1, 4, 3)
        n = len(img_pts)
        R = np.ascontiguousarray(R, np.float64).reshape(n, 9).copy()
        t = np.ascontiguousarray(t, np.float64).reshape(n, 3).copy()
        steps = np.zeros(n, np.int32)
        costs = np.zeros((n, 2))
        self._chk(lib().mantis_quad_gn(self.h, img_pts.ctypes.data, obj_pts.ctypes.data, n, R.ctypes.data,
                                       t.ctypes.data, iterations, steps.ctypes.data, costs.ctypes.data), "quad_gn")
        return R.reshape(n, 3, 3), t, steps, costs

    # device buffers -------------------------------------------------------
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(lib().mantis_device_alloc(self.h, nbytes, C.byref(p)), "device_alloc")
        return p.value

    def device_free(self, p):
        self._chk(lib().mantis_device_free(self.h, C.c_void_p(p)), "device_free")

    def h2d(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(lib().mantis_memcpy_h2d(self.h, C.c_void_p(dst), arr.ctypes.data, arr.nbytes), "h2d")

    def d2h(self, arr, src):
        self._chk(lib().mantis_memcpy_d2h(self.h, arr.ctypes.data, C.c_void_p(src), arr.nbytes), "d2h")
        return arr

    def synth_render(self, cams, seeds, out_dev):
        n = len(cams)
        arr = (SynthCamC * n)()
        for i, c in enumerate(cams):
            C.memmove(C.byref(arr[i]), C.byref(c), C.sizeof(SynthCamC))
        s = np.ascontiguousarray(seeds, np.uint64)
        self._chk(lib().mantis_synth_render(self.h, arr, n, s.ctypes.data, C.c_void_p(out_dev)), "synth_render")

    def synchronize(self):
        self._chk(lib().mantis_synchronize(self.h), "synchronize")

    def set_profiling(self, on):
        self._chk(lib().mantis_set_profiling(self.h, int(on)), "set_profiling")

    def kernel_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = lib().mantis_kernel_times(self.h, names, ms, 64)
        return [(names[i].decode(), ms[i]) for i in range(n)]

    def stage_times(self):
        """kernel_times() summed per stage: a mark named "stage/kernel" (the
        hot stages are marked per kernel) counts toward "stage"."""
        out = {}
        for name, ms in self.kernel_times():
            st = name.split("/", 1)[0]
            out[st] = out.get(st, 0.0) + ms
        return list(out.items())


def argmin_pick(pairs):
    """The cross-shard first-minimum rule of mantis_score_argmin (host only):
    pairs = ranks x (err, global index), index -1 for an empty shard."""
    pairs = np.ascontiguousarray(pairs, np.float64).reshape(-1, 2)
    e = C.c_double()
    i = C.c_int64()
    st = lib().mantis_argmin_pick(pairs.ctypes.data, len(pairs), C.byref(e), C.byref(i))
    if st != MANTIS_OK:
        raise MantisError(f"argmin_pick failed ({st})")
    return e.value, i.value
