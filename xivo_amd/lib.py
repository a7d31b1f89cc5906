"""ctypes binding of include/xivo_hip.h (test / bench plumbing only)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OOS_MAX_OBS = 16

FLAG_FIX_GROUP_BLOCK = 1
FLAG_PROFILE = 2
FLAG_DENSE_H = 64
FLAG_SYMMETRIC_FORM = 256
FLAG_STANDALONE_TAIL = 512
FLAG_NO_LDLT_FALLBACK = 4096
FLAG_FP32_WHITENED = 16384  # N > 256 / M > 176: V^T, Y^T as float, P - V^T Y on the fp32 MFMA
FLAG_THROUGHPUT_ROUTE = 8192    # every batch size on the kernels sized for thousands of filters (default: <= 64 filters take the latency route)
FLAG_INVDEPTH = 32768           # USE_INVDEPTH build: features are (X/Z, Y/Z, 1/Z) (src/feature.cpp:98-105)
OOS_WHOLE_BUFFER = 1             # xivo_hip_oos_project_ex options
FLAG_MULTI_KERNEL = 65536       # keep shapes the one-kernel update holds (fused_update.hip) on the multi-kernel pipeline
CAM_PINHOLE, CAM_ATAN, CAM_RADTAN, CAM_EQUI = 0, 1, 2, 3


class XivoHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"xivo_hip status {status}: {msg}")
        self.status = status


class Layout(C.Structure):
    _fields_ = [("N", C.c_int), ("group_begin", C.c_int), ("n_groups", C.c_int),
                ("feature_begin", C.c_int), ("n_features", C.c_int)]


class Cam(C.Structure):
    _fields_ = [("model", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("d", C.c_double * 5)]


def make_cam(cam):
    """a camera dict (model, fx, fy, cx, cy; rows / cols default 480 / 640; d: the model's coefficients) -> Cam"""
    c = Cam()
    c.model, c.rows, c.cols = cam["model"], cam.get("rows", 480), cam.get("cols", 640)
    c.fx, c.fy, c.cx, c.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    d = list(cam.get("d", [])) + [0.0] * 5
    for i in range(5):
        c.d[i] = d[i]
    return c


# numpy dtypes mirroring the C structs (all naturally aligned, no padding surprises:
# sizes are asserted against ctypes below)
pose_dtype = np.dtype([("Rsb", "f8", 9), ("Tsb", "f8", 3), ("Rbc", "f8", 9), ("Tbc", "f8", 3),
                       ("Vsb", "f8", 3), ("bg", "f8", 3), ("ba", "f8", 3), ("Rsg", "f8", 9)])
group_dtype = np.dtype([("Rsb", "f8", 9), ("Tsb", "f8", 3)])
feat_dtype = np.dtype([("x", "f8", 3), ("xp", "f8", 2), ("ref_sind", "i4"), ("sind", "i4")])
oos_dtype = np.dtype([("Xs", "f8", 3), ("n_obs", "i4"), ("group_sind", "i4", OOS_MAX_OBS),
                      ("_pad", "i4"), ("xp", "f8", (OOS_MAX_OBS, 2))])


class _OosC(C.Structure):
    _fields_ = [("Xs", C.c_double * 3), ("n_obs", C.c_int), ("group_sind", C.c_int * OOS_MAX_OBS),
                ("xp", (C.c_double * 2) * OOS_MAX_OBS)]


assert oos_dtype.itemsize == C.sizeof(_OosC), (oos_dtype.itemsize, C.sizeof(_OosC))
lc_dtype = np.dtype([("feat", "i4"), ("group_sind", "i4"), ("xp", "f8", 2)])      # xivo_lc_match
assert lc_dtype.itemsize == 24
imu_dtype = np.dtype([("gyro", "f8", 3), ("accel", "f8", 3), ("slope_gyro", "f8", 3), ("slope_accel", "f8", 3), ("dt", "f8")])
prop_opts_dtype = np.dtype([("Qimu", "f8", 144), ("Qmodel", "f8", 529), ("g", "f8", 3), ("method", "i4"), ("_pad", "i4"),
                            ("stepsize", "f8"), ("control_stepsize", "i4"), ("attempts", "i4"), ("tolerance", "f8"),
                            ("min_scale_factor", "f8"), ("max_scale_factor", "f8")])
assert imu_dtype.itemsize == 104 and prop_opts_dtype.itemsize == (144 + 529 + 3) * 8 + 16 + 32
subfilter_dtype = np.dtype([("x", "f8", 3), ("P", "f8", 9), ("xp", "f8", 2), ("outlier_counter", "f8"), ("score", "f8"),
                            ("ref_sind", "i4"), ("status", "i4"), ("init_counter", "i4"), ("candidate", "i4")])
subfilter_opts_dtype = np.dtype([("Rtri", "f8"), ("MH_thresh", "f8"), ("ready_steps", "i4"), ("_pad", "i4"),
                                 ("min_depth", "f8"), ("max_depth", "f8"), ("max_subfilter_outlier", "f8")])
# xivo_edit_op (include/xivo_hip.h): one resident-state edit of one filter
edit_dtype = np.dtype([("b", "i4"), ("kind", "i4"), ("i0", "i4"), ("i1", "i4"), ("i2", "i4"), ("reserved", "i4"),
                       ("v", "f8", 14)])
assert edit_dtype.itemsize == 136
EDIT_P_ZERO_RC, EDIT_P_COPY_RC, EDIT_P_SET_BLOCK3, EDIT_ADD_GROUP, EDIT_REMOVE_GROUP, EDIT_ADD_FEATURE, \
    EDIT_REMOVE_FEATURE, EDIT_SET_XP, EDIT_ADD_GROUP_ANCHOR, EDIT_ADMIT_POOL = range(10)
# xivo_pool_new (include/xivo_hip.h): one new track for the out-of-state feature pool
pool_new_dtype = np.dtype([("b", "i4"), ("entry", "i4"), ("anchor", "i4"), ("reserved", "i4"), ("xp", "f8", 2), ("z0", "f8"),
                           ("std_xyz", "f8", 3)])
assert pool_new_dtype.itemsize == 64
POOL_MAX_ENTRIES = 512
# depth initialisation of new tracks (include/xivo_hip.h): triangulation and AdaptInitialDepth
TRI_OFF, TRI_DLT_SVD, TRI_DLT_AVG, TRI_L1, TRI_L2, TRI_LINF = range(6)
TRI_METHODS = {"direct_linear_transform_svd": TRI_DLT_SVD, "direct_linear_transform_avg": TRI_DLT_AVG,
               "l1_angular": TRI_L1, "l2_angular": TRI_L2, "linf_angular": TRI_LINF}
tri_opts_dtype = np.dtype([("struct_size", "i4"), ("method", "i4"), ("zmin", "f8"), ("zmax", "f8"),
                           ("max_theta_thresh", "f8"), ("beta_thresh", "f8")])
tri_in_dtype = np.dtype([("R12", "f8", 9), ("t12", "f8", 3), ("xc1", "f8", 2), ("xc2", "f8", 2)])
tri_out_dtype = np.dtype([("X", "f8", 3), ("ret", "i4"), ("good", "i4")])
adapt_opts_dtype = np.dtype([("struct_size", "i4"), ("min_feature_lifetime", "i4"), ("initial_z", "f8"),
                             ("median_weight", "f8"), ("min_z", "f8"), ("max_z", "f8")])
assert tri_opts_dtype.itemsize == 40 and tri_in_dtype.itemsize == 128 and tri_out_dtype.itemsize == 32
assert adapt_opts_dtype.itemsize == 40
POOL_ADD_ADAPTIVE_Z = 1
assert subfilter_dtype.itemsize == 144 and subfilter_opts_dtype.itemsize == 48
assert feat_dtype.itemsize == 48 and pose_dtype.itemsize == 336 and group_dtype.itemsize == 96
# trajectory log (include/xivo_hip.h): xivo_traj_opts, xivo_traj_rec
TRAJ_MAX_COLS = 32
ERR_FULL = -6
traj_opts_dtype = np.dtype([("T_max", "i4"), ("n_cols", "i4"), ("cols", "i4", TRAJ_MAX_COLS)])
traj_dtype = np.dtype([("Rsb", "f8", 9), ("Tsb", "f8", 3), ("Vsb", "f8", 3), ("bg", "f8", 3), ("ba", "f8", 3),
                       ("status", "i4"), ("reserved", "i4")])
assert traj_dtype.itemsize == 176 and traj_opts_dtype.itemsize == 136
# trajectory score (include/xivo_hip.h): xivo_traj_score_opts, xivo_traj_score
TRAJ_SCORE_UNDETERMINED = 1
traj_score_opts_dtype = np.dtype([("align", "i4"), ("rpe_lag", "i4")])
traj_score_dtype = np.dtype([("ate", "f8"), ("ate_raw", "f8"), ("rpe_pos", "f8"), ("rpe_rot", "f8"), ("R", "f8", 9), ("T", "f8", 3),
                             ("sv", "f8", 3), ("n_used", "i4"), ("n_pairs", "i4"), ("flags", "i4"), ("reserved", "i4")])
assert traj_score_dtype.itemsize == 168 and traj_score_opts_dtype.itemsize == 8
# landmark log (include/xivo_hip.h): xivo_map_opts, xivo_map_pt
MAP_MAX_OUT = 128
MAP_WORLD_COV = 1
map_opts_dtype = np.dtype([("T_max", "i4"), ("n_out", "i4"), ("flags", "u4")])
map_pt_dtype = np.dtype([("Xs", "f8", 3), ("cov_local", "f8", 6), ("cov_world", "f8", 6), ("xp", "f8", 2), ("score", "f8"),
                         ("pos", "i4"), ("sind", "i4"), ("ref_sind", "i4"), ("reserved", "i4")])
assert map_pt_dtype.itemsize == 160 and map_opts_dtype.itemsize == 12
# innovation log (include/xivo_hip.h): xivo_innov_opts, xivo_innov_rec
INNOV_FAILED, INNOV_LDLT = 1, 2
innov_opts_dtype = np.dtype([("T_max", "i4")])
innov_rec_dtype = np.dtype([("nis", "f8"), ("prefit", "f8"), ("postfit", "f8"), ("inn_max", "f8"), ("dx_max", "f8"),
                            ("dof", "i4"), ("rows", "i4"), ("flags", "i4"), ("reserved", "i4"), ("reserved2", "f8")])
assert innov_rec_dtype.itemsize == 64 and innov_opts_dtype.itemsize == 4
# device life cycle (include/xivo_hip.h): xivo_life_opts, xivo_life_stats
LIFE_MAX_TRACKS, LIFE_MAX_SLOTS = 2048, 256
life_opts_dtype = np.dtype([("tracks_max", "i4"), ("min_new_features", "i4"), ("min_depth", "f8"), ("max_depth", "f8"),
                            ("var_xyz", "f8", 3)])
life_stats_dtype = np.dtype([("updates", "i8"), ("rejected", "i8"), ("dropped", "i8"), ("admitted", "i8"), ("groups_added", "i8"),
                             ("not_spd", "i8")])
assert life_opts_dtype.itemsize == 48 and life_stats_dtype.itemsize == 48
# tuning table (include/xivo_hip.h): xivo_tune_in, one filter's R, MH_thresh, var_xyz, Qimu 12 x 12 and Qmodel 23 x 23 (the two
# matrices column-major, as prop_opts_dtype holds them)
tune_dtype = np.dtype([("R", "f8"), ("mh_thresh", "f8"), ("var_xyz", "f8", 3), ("Qimu", "f8", 144), ("Qmodel", "f8", 529)])
assert tune_dtype.itemsize == 5424
# device pool life cycle (include/xivo_hip.h): xivo_pool_life_opts, xivo_pool_life_stats
pool_life_opts_dtype = np.dtype([("struct_size", "i4"), ("tracks_max", "i4"), ("max_group_lifetime", "i4"), ("adaptive_z", "i4"),
                                 ("initial_z", "f8"), ("std_xyz", "f8", 3)])
pool_life_stats_dtype = np.dtype([(k, "i8") for k in ("updates", "rejected", "dropped", "admitted", "groups_added", "not_spd",
                                                       "pool_added", "pool_dropped", "pool_outliers", "anchors_created",
                                                       "anchors_freed", "admit_steps")])
assert pool_life_opts_dtype.itemsize == 48 and pool_life_stats_dtype.itemsize == 96
POOL_LIFE_MAX_ANCHORS = 256
# MSCKF update from dropped pool entries (include/xivo_hip.h): xivo_pool_oos_opts, xivo_pool_oos_cand, xivo_pool_oos_stats
pool_oos_opts_dtype = np.dtype([("struct_size", "i4"), ("oos_max", "i4"), ("max_obs", "i4"), ("min_obs", "i4"), ("Roos", "f8"),
                                ("chi2", "f8", 32)])
pool_oos_cand_dtype = np.dtype([("b", "i4"), ("entry", "i4"), ("n_obs", "i4"), ("reserved", "i4"),
                                ("group_sind", "i4", OOS_MAX_OBS), ("xp", "f8", (OOS_MAX_OBS, 2))])
pool_oos_stats_dtype = np.dtype([(k, "i8") for k in ("oos_used", "oos_gated", "oos_surplus", "oos_short")])
assert pool_oos_opts_dtype.itemsize == 280 and pool_oos_cand_dtype.itemsize == 336 and pool_oos_stats_dtype.itemsize == 32
# chi-square 0.95 quantiles for 1 .. 29 degrees of freedom (index = dof; 0 and 30, 31 unused): the gate of an OOS feature's
# the resident landmark map (include/xivo_hip.h): xivo_lcmap_opts, _entry, _add_rec, _query, _match, _stats
lcmap_opts_dtype = np.dtype([("struct_size", "i4"), ("map_max", "i4"), ("lc_max", "i4"), ("min_matches", "i4"), ("Rlc", "f8"),
                             ("chi2", "f8"), ("max_depth_var", "f8")])
lcmap_entry_dtype = np.dtype([("key", "i8"), ("Xs", "f8", 3)])
lcmap_add_dtype = np.dtype([("b", "i4"), ("feat", "i4"), ("key", "i8")])
lcmap_query_dtype = np.dtype([("b", "i4"), ("group_sind", "i4"), ("key", "i8"), ("xp", "f8", 2)])
lcmap_match_dtype = np.dtype([("entry", "i4"), ("group_sind", "i4"), ("xp", "f8", 2), ("gamma", "f8"), ("kept", "i4"), ("reserved", "i4")])
LCMAP_STATS_FIELDS = ("added", "dup", "full", "poor", "skipped", "queries", "matched", "surplus", "gated", "short_frames", "closed_frames")
lcmap_stats_dtype = np.dtype([(k, "i8") for k in LCMAP_STATS_FIELDS])
assert (lcmap_opts_dtype.itemsize, lcmap_entry_dtype.itemsize, lcmap_add_dtype.itemsize, lcmap_query_dtype.itemsize,
        lcmap_match_dtype.itemsize, lcmap_stats_dtype.itemsize) == (40, 32, 16, 32, 40, 88)
# its options on top (xivo_hip_lcmap_cov_config): xivo_lcmap_cov_opts, _cov_stats
lcmap_cov_opts_dtype = np.dtype([("struct_size", "i4"), ("point_cov", "i4"), ("revisit_gap", "i4"), ("reserved", "i4")])
LCMAP_COV_STATS_FIELDS = ("resting", "rested_frames", "bad_cov")
lcmap_cov_stats_dtype = np.dtype([(k, "i8") for k in LCMAP_COV_STATS_FIELDS])
assert (lcmap_cov_opts_dtype.itemsize, lcmap_cov_stats_dtype.itemsize) == (16, 24)
LCMAP_MAX_ENTRIES, LCMAP_MAX_MATCHES = 4096, 64
CHI2_2DOF_95 = 5.991464547107979   # -2 ln 0.05: the 95 % point of chi-square with 2 degrees of freedom
# 2k - 3 projected rows (tests/test_pool_oos_cpu.py holds the table against scipy.stats.chi2.ppf)
CHI2_95 = (0.0, 3.841458820694124, 5.991464547107979, 7.814727903251179, 9.487729036781154, 11.070497693516351,
           12.591587243743977, 14.067140449340169, 15.50731305586545, 16.918977604620448, 18.307038053275146,
           19.67513757268249, 21.02606981748307, 22.362032494826934, 23.684791304840576, 24.995790139728616,
           26.29622760486423, 27.587111638275324, 28.869299430392623, 30.14352720564616, 31.410432844230918,
           32.670573340917315, 33.92443847144381, 35.17246162690806, 36.41502850180731, 37.65248413348277,
           38.885138659830055, 40.11327206941361, 41.33713815142739, 42.55696780429269, 0.0, 0.0)
# point-cloud world (include/xivo_hip.h): xivo_pcw_opts
pcw_opts_dtype = np.dtype([("struct_size", "i4"), ("npts", "i4"), ("fx", "f8"), ("fy", "f8"), ("cx", "f8"), ("cy", "f8"),
                           ("imw", "f8"), ("imh", "f8")])
assert pcw_opts_dtype.itemsize == 56
# track faults of the producer (include/xivo_hip.h): xivo_pcw_fault_opts, xivo_pcw_fault_stats
pcw_fault_opts_dtype = np.dtype([("struct_size", "i4"), ("sticky", "i4"), ("p_drop", "f8"), ("p_outlier", "f8"), ("p_tail", "f8"),
                                 ("outlier_min_px", "f8"), ("outlier_max_px", "f8"), ("tail_scale", "f8")])
assert pcw_fault_opts_dtype.itemsize == 56
pcw_fault_stats_dtype = np.dtype([(k, "i8") for k in ("tracks", "dropped", "outlier_events", "tail_events", "biased",
                                                      "outlier_rejected", "outlier_kept", "nominal_rejected", "nominal_kept")])
assert pcw_fault_stats_dtype.itemsize == 72
# trajectory producer (include/xivo_hip.h): xivo_trajsim_opts
trajsim_opts_dtype = np.dtype([("struct_size", "i4"), ("n_max", "i4"), ("T_max", "i4"), ("reserved", "i4"), ("imu_dt", "f8"),
                               ("rot_amp", "f8"), ("rot_w", "f8", 3), ("noise_accel", "f8"), ("noise_gyro", "f8"),
                               ("grav_s", "f8", 3), ("Rbc", "f8", 9), ("Tbc", "f8", 3), ("seed", "u8")])
assert trajsim_opts_dtype.itemsize == 200
TRAJSIM_MOTIONS = {"lissajous": 0, "trefoil": 1}


def lib_path():
    # XIVO_HIP_LIBRARY: A/B timing of experimental builds in one process pool (scripts only)
    return os.environ.get("XIVO_HIP_LIBRARY") or os.path.join(_HERE, "libxivo_hip.so")


_LIB = None

_SIGS = {
    "xivo_hip_create": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint],
    "xivo_hip_sync": [C.c_void_p],
    "xivo_hip_set_flags": [C.c_void_p, C.c_uint],
    "xivo_hip_upload_P": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int],
    "xivo_hip_download_P": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int],
    "xivo_hip_snapshot_P": [C.c_void_p],
    "xivo_hip_restore_P": [C.c_void_p],
    "xivo_hip_p_zero_rc": [C.c_void_p, C.c_int, C.c_int, C.c_int],
    "xivo_hip_p_copy_rc": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
    "xivo_hip_p_set_block3": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_p_diag": [C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_set_measurements": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int,
                                  C.c_void_p, C.c_long, C.c_void_p, C.c_long],
    "xivo_hip_set_measurements_device": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int,
                                         C.c_void_p, C.c_long, C.c_void_p, C.c_long],
    "xivo_hip_update_joseph": [C.c_void_p, C.c_int],
    "xivo_hip_get_err": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long],
    "xivo_hip_get_status": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_mh_gate_dense": [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                               C.c_void_p, C.c_void_p],
    "xivo_hip_update_dense_gated": [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int],
    "xivo_hip_get_gate": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_set_layout": [C.c_void_p, C.POINTER(Layout), C.POINTER(Cam)],
    "xivo_hip_set_scene": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_jacobians_instate": [C.c_void_p, C.c_int],
    "xivo_hip_get_jacobians": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_mh_gate": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p,
                         C.c_void_p],
    "xivo_hip_stack": [C.c_void_p, C.c_int, C.c_double],
    "xivo_hip_oos_project": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p],
    "xivo_hip_oos_project_ex": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_uint],
    "xivo_hip_close_loop_stack": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double],
    "xivo_hip_compress_oos": [C.c_void_p, C.c_int, C.c_double, C.c_void_p],
    "xivo_hip_one_point_ransac": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p],
    "xivo_hip_filter_update": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int],
    "xivo_hip_last_path": [C.c_void_p],
    "xivo_hip_last_route": [C.c_void_p],
    "xivo_hip_stage_kernel": [C.c_void_p, C.c_int],
    "xivo_hip_stage_bytes": [C.c_void_p, C.c_int],
    "xivo_hip_absorb_error": [C.c_void_p, C.c_int],
    "xivo_hip_propagate": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_givens": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                        C.c_void_p],
    "xivo_hip_qr": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_subfilter_update": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_candidate_order": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_pool_config": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double],
    "xivo_hip_pool_anchor": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pool_add": [C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_pool_step": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_pool_get": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_triangulate": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_pool_triangulation": [C.c_void_p, C.c_void_p],
    "xivo_hip_pool_tri_counts": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_pool_adapt_depth_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_pool_adapt_depth": [C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_pool_add_ex": [C.c_void_p, C.c_int, C.c_void_p, C.c_uint],
    "xivo_hip_pool_get_init_z": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_edit_batch": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_set_pixels": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_get_scene": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_get_H": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_propagate_cov": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_dev_alloc": [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)],
    "xivo_hip_dev_free": [C.c_void_p, C.c_void_p],
    "xivo_hip_dev_upload": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t],
    "xivo_hip_timer_begin": [C.c_void_p],
    "xivo_hip_timer_end": [C.c_void_p, C.POINTER(C.c_float)],
    "xivo_hip_profile_reset": [C.c_void_p],
    "xivo_hip_profile_get": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_float),
                             C.POINTER(C.c_int), C.POINTER(C.c_double)],
    "xivo_hip_bench_mfma_peak": [C.c_void_p, C.POINTER(C.c_double)],
    "xivo_hip_get_ldlt_used": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_update_joseph_host": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_uint],
    "xivo_hip_set_calib": [C.c_void_p, C.c_void_p],
    "xivo_hip_set_calib_state": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_get_jacobians_calib": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_get_calib_state": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_set_calib_gyro": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_propagate_calib": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_selftest_fused_tiles": [C.c_int, C.c_void_p],
    "xivo_hip_selftest_fused_shape": [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int],
    "xivo_hip_selftest_host_compress": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_selftest_glevel_launch": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int],
    "xivo_hip_selftest_ctx_allocs": [C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_traj_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_traj_record": [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p],
    "xivo_hip_traj_count": [C.c_void_p],
    "xivo_hip_traj_reset": [C.c_void_p],
    "xivo_hip_traj_read": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_traj_nees": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p],
    "xivo_hip_traj_score": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_map_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_map_record": [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p],
    "xivo_hip_map_count": [C.c_void_p],
    "xivo_hip_map_reset": [C.c_void_p],
    "xivo_hip_map_read": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_map_nees": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p],
    "xivo_hip_innov_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_innov_record": [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p],
    "xivo_hip_innov_count": [C.c_void_p],
    "xivo_hip_innov_reset": [C.c_void_p],
    "xivo_hip_innov_read": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_innov_stats": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p],
    "xivo_hip_life_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_life_set_book": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_life_get_book": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_life_begin": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_life_end": [C.c_void_p, C.c_int],
    "xivo_hip_life_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_life_begin_tracks": [C.c_void_p, C.c_int, C.c_int],
    "xivo_hip_pool_life_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_pool_life_set_book": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pool_life_get_book": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7,
    "xivo_hip_pool_life_begin": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "xivo_hip_pool_life_begin_tracks": [C.c_void_p, C.c_int, C.c_int, C.c_int],
    "xivo_hip_pcw_camera": [C.c_void_p, C.c_void_p, C.c_double],
    "xivo_hip_pool_life_end": [C.c_void_p, C.c_int],
    "xivo_hip_pool_life_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pool_oos_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_pool_oos_rows": [C.c_void_p],
    "xivo_hip_pool_oos_collect": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pool_oos_project": [C.c_void_p, C.c_int],
    "xivo_hip_pool_oos_gate": [C.c_void_p, C.c_int],
    "xivo_hip_pool_oos_get": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_pool_oos_get_rings": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5,
    "xivo_hip_pool_oos_get_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_add": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_close": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_set": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_get": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_get_matches": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_get_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_cov_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_set_cov": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_get_cov": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_get_cov_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_life_config": [C.c_void_p, C.c_int],
    "xivo_hip_life_begin_keys": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_add_resident": [C.c_void_p, C.c_int],
    "xivo_hip_lcmap_close_resident": [C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_lcmap_life_get_keys": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_lcmap_life_get_track_keys": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pcw_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_pcw_set_world": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_pcw_get_world": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_pcw_tracks": [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_ulonglong, C.c_ulonglong],
    "xivo_hip_pcw_get_tracks": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_pcw_tracks_resident": [C.c_void_p, C.c_int, C.c_double, C.c_ulonglong, C.c_ulonglong],
    "xivo_hip_pcw_fault_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_pcw_stream_share": [C.c_void_p, C.c_int],
    "xivo_hip_pcw_fault_score": [C.c_void_p, C.c_int],
    "xivo_hip_pcw_fault_get_stats": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_pcw_fault_get_flags": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_trajsim_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_trajsim_set": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "xivo_hip_trajsim_frame": [C.c_void_p, C.c_int, C.c_ulonglong, C.c_int],
    "xivo_hip_propagate_resident": [C.c_void_p, C.c_int, C.c_void_p],
    "xivo_hip_trajsim_get": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "xivo_hip_trajsim_get_gt": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_trajsim_count": [C.c_void_p],
    "xivo_hip_trajsim_reset": [C.c_void_p],
    "xivo_hip_tune_config": [C.c_void_p, C.c_void_p],
    "xivo_hip_tune_set": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "xivo_hip_tune_get": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
}
HOST_P_RESIDENT, HOST_KEEP_P = 1, 2


def tri_options(method, zmin=0.05, zmax=5.0, max_theta_thresh=0.1 * np.pi / 180, beta_thresh=0.25 * np.pi / 180):
    """xivo_triangulate_opts; method = TRI_* or the cfg's name ("l1_angular", ...); thresholds in radians"""
    o = np.zeros(1, dtype=tri_opts_dtype)
    o["struct_size"] = tri_opts_dtype.itemsize
    o["method"] = TRI_METHODS[method] if isinstance(method, str) else int(method)
    o["zmin"], o["zmax"], o["max_theta_thresh"], o["beta_thresh"] = zmin, zmax, max_theta_thresh, beta_thresh
    return o


class CalibLayout(C.Structure):
    _fields_ = [("td", C.c_int), ("Cg", C.c_int), ("cam_begin", C.c_int), ("cam_dim", C.c_int)]


calib_dtype = np.dtype([("gyro", "f8", 3), ("Cg", "f8", 9), ("td", "f8"), ("Ca", "f8", 9), ("intr", "f8", 9)])
assert calib_dtype.itemsize == 248


def cam_intr(cam):
    """xivo_calib_in::intr of a camera dict: fx fy cx cy, then the distortion parameters in xivo_cam.d's order"""
    d = list(cam.get("d", [])) + [0.0] * 5
    return np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]] + d[:5], dtype=np.float64)
# every symbol include/xivo_hip.h declares (tests check the library exports them all)
ALL_SYMBOLS = sorted(list(_SIGS) + ["xivo_hip_destroy", "xivo_hip_strerror", "xivo_hip_gemm_tile", "xivo_hip_device_count",
                                        "xivo_hip_device_numa_node", "xivo_hip_route_name"])


def load_library():
    """Load libxivo_hip.so; raises (no fallback) if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not built - run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP extension is the product; there is no CPU fallback)")
    lib = C.CDLL(path)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.xivo_hip_device_count.argtypes = []
    lib.xivo_hip_device_count.restype = C.c_int
    lib.xivo_hip_device_numa_node.argtypes = [C.c_int]
    lib.xivo_hip_device_numa_node.restype = C.c_int
    lib.xivo_hip_destroy.argtypes = [C.c_void_p]
    lib.xivo_hip_destroy.restype = None
    lib.xivo_hip_strerror.argtypes = [C.c_int]
    lib.xivo_hip_strerror.restype = C.c_char_p
    lib.xivo_hip_route_name.argtypes = [C.c_int]
    lib.xivo_hip_route_name.restype = C.c_char_p
    lib.xivo_hip_gemm_tile.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.xivo_hip_gemm_tile.restype = None
    lib.xivo_hip_stage_kernel.restype = C.c_char_p
    lib.xivo_hip_stage_bytes.restype = C.c_double
    _LIB = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def candidate_order(feats, strict=False, score_type=0):
    """Criteria::CandidateComparison order (src/options.cpp:34-61) of a [nb, n] subfilter_dtype array: returns
    (order [nb, n] padded with -1, count [nb], score [nb, n] of `score_type`). Host arithmetic, no GPU needed."""
    lib = load_library()
    feats = np.ascontiguousarray(feats, dtype=subfilter_dtype)
    nb, n = feats.shape
    order = np.full((nb, n), -1, dtype=np.int32); cnt = np.zeros(nb, dtype=np.int32); score = np.zeros((nb, n))
    rc = lib.xivo_hip_candidate_order(_ptr(feats), nb, n, int(strict), int(score_type), _ptr(order), _ptr(cnt), _ptr(score))
    if rc != 0:
        raise XivoHipError(rc, lib.xivo_hip_strerror(rc).decode())
    return order, cnt, score


def prop_options(Qimu, Qmodel, g, method="RK4", stepsize=0.002, pd_control=None):
    """xivo_prop_opts: Qimu 12x12, Qmodel 23x23 (numpy row-major); pd_control: dict(tolerance, attempts, min_scale_factor,
    max_scale_factor) switches on the step-size-controlled branch of Estimator::PrinceDormand"""
    o = np.zeros(1, dtype=prop_opts_dtype)
    o["Qimu"] = np.asarray(Qimu, dtype=np.float64).T.reshape(-1)
    o["Qmodel"] = np.asarray(Qmodel, dtype=np.float64).T.reshape(-1)
    o["g"] = g; o["method"] = 0 if method == "RK4" else 1; o["stepsize"] = stepsize
    if pd_control is not None:
        o["control_stepsize"] = 1
        o["tolerance"] = pd_control.get("tolerance", 1e-3); o["attempts"] = pd_control.get("attempts", 12)
        o["min_scale_factor"] = pd_control.get("min_scale_factor", 0.125); o["max_scale_factor"] = pd_control.get("max_scale_factor", 4.0)
    return o


def tune_entry(R, mh_thresh, var_xyz, Qimu, Qmodel):
    """one xivo_tune_in record: Qimu 12x12, Qmodel 23x23 (numpy row-major, as prop_options takes them)"""
    e = np.zeros((), dtype=tune_dtype)
    e["R"], e["mh_thresh"], e["var_xyz"] = R, mh_thresh, np.asarray(var_xyz, dtype=np.float64)
    e["Qimu"] = np.asarray(Qimu, dtype=np.float64).T.reshape(-1)
    e["Qmodel"] = np.asarray(Qmodel, dtype=np.float64).T.reshape(-1)
    return e


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """A batch of `batch` independent filters with state dim N on one GPU.

    Matrices cross this boundary as numpy arrays shaped [batch, cols, rows]
    C-contiguous == column-major [rows x cols] per filter (Eigen's layout); the
    helpers below take/return [batch, rows, cols] arrays and do the transposes.
    """

    pcw_npts = 0     # points per resident world (pcw_config; a borrowed context: set it to the owner's)

    def __init__(self, N, M_max, batch, device=0, flags=0):
        self.lib = load_library()
        self.N, self.M_max, self.batch = int(N), int(M_max), int(batch)
        h = C.c_void_p()
        self._check(self.lib.xivo_hip_create(C.byref(h), device, N, M_max, batch, flags))
        self.h = h
        self.flags = flags

    @classmethod
    def borrow(cls, handle, N, M_max, batch):
        """View of a context that someone else owns and destroys (xivo_batch_ctx of the C++ BatchEstimator): close() leaves
        the handle alone."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.N, self.M_max, self.batch = int(N), int(M_max), int(batch)
        self.h, self.flags, self._borrowed = C.c_void_p(handle), 0, True
        return self

    def _check(self, rc):
        if rc != 0:
            raise XivoHipError(rc, self.lib.xivo_hip_strerror(rc).decode())

    def close(self):
        if getattr(self, "_borrowed", False):
            self.h = None
        if getattr(self, "h", None):
            for p in getattr(self, "_dev_bufs", []):
                self.lib.xivo_hip_dev_free(self.h, p)
            self._dev_bufs = []
            self.lib.xivo_hip_destroy(self.h)
            self.h = None

    def ctx_allocs(self):
        """(live, bytes): number and total size of the device blocks the context owns right now (test hook)"""
        live, nbytes = C.c_int(0), C.c_ulonglong(0)
        self._check(self.lib.xivo_hip_selftest_ctx_allocs(self.h, C.byref(live), C.byref(nbytes)))
        return live.value, nbytes.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._check(self.lib.xivo_hip_sync(self.h))

    def set_flags(self, flags):
        self._check(self.lib.xivo_hip_set_flags(self.h, flags))
        self.flags = flags

    # ---- P ---------------------------------------------------------------
    def upload_P(self, P, b0=0):
        P = np.asarray(P, dtype=np.float64)
        nb = P.shape[0]
        Pc = _f64(np.transpose(P, (0, 2, 1)))  # column-major per filter
        self._check(self.lib.xivo_hip_upload_P(self.h, b0, nb, _ptr(Pc), self.N * self.N, self.N))

    def download_P(self, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        out = np.empty((nb, self.N, self.N), dtype=np.float64)
        self._check(self.lib.xivo_hip_download_P(self.h, b0, nb, _ptr(out), self.N * self.N, self.N))
        return np.transpose(out, (0, 2, 1)).copy()

    def snapshot_P(self):
        self._check(self.lib.xivo_hip_snapshot_P(self.h))

    def restore_P(self):
        self._check(self.lib.xivo_hip_restore_P(self.h))

    def p_zero_rc(self, b, off, length):
        self._check(self.lib.xivo_hip_p_zero_rc(self.h, b, off, length))

    def p_copy_rc(self, b, dst, src, length):
        self._check(self.lib.xivo_hip_p_copy_rc(self.h, b, dst, src, length))

    def p_set_block3(self, b, off, P3):
        P3c = _f64(np.asarray(P3).T)
        self._check(self.lib.xivo_hip_p_set_block3(self.h, b, off, _ptr(P3c)))

    def p_diag(self, b):
        out = np.empty(self.N)
        self._check(self.lib.xivo_hip_p_diag(self.h, b, _ptr(out)))
        return out

    # ---- S-level ------------------------------------------------------------
    def set_measurements(self, H, inn, diagR, b0=0):
        H = np.asarray(H, dtype=np.float64)
        nb, M, N = H.shape
        assert N == self.N
        Hc = _f64(np.transpose(H, (0, 2, 1)))
        inn = _f64(inn)
        dR = _f64(diagR)
        self._check(self.lib.xivo_hip_set_measurements(self.h, b0, nb, M, _ptr(Hc), M * N, M, _ptr(inn), M,
                                                       _ptr(dR), M))

    def set_measurements_device(self, dH, dinn, dR, M, nb, b0=0, strideH=None, ldh=None):
        """Hand-over of measurements that already live in device memory: dH / dinn / dR are device addresses
        (ints, e.g. torch tensor .data_ptr()) of nb column-major M x N matrices and M-vectors."""
        ldh = M if ldh is None else ldh
        strideH = ldh * self.N if strideH is None else strideH
        self._check(self.lib.xivo_hip_set_measurements_device(self.h, b0, nb, M, C.c_void_p(dH), strideH, ldh,
                                                              C.c_void_p(dinn), M, C.c_void_p(dR), M))

    def device_array(self, a, total=None):
        """Device copy of the numpy array `a` on this context's GPU (bench / tests: inputs that are already resident);
        total = number of leading-axis entries the buffer holds, `a` is repeated to fill it. Returns the address."""
        a = np.ascontiguousarray(a)
        total = a.shape[0] if total is None else total
        per = a.nbytes // a.shape[0]
        p = C.c_void_p()
        self._check(self.lib.xivo_hip_dev_alloc(self.h, per * total, C.byref(p)))
        self._dev_bufs = getattr(self, "_dev_bufs", []) + [p]
        n0 = min(a.shape[0], total)
        self._check(self.lib.xivo_hip_dev_upload(self.h, p, _ptr(a), per * n0, per * total))
        return p.value

    def update_joseph(self, B=None):
        self._check(self.lib.xivo_hip_update_joseph(self.h, self.batch if B is None else B))

    # ---- online-calibration builds (measurement side) ----------------------------
    def set_calib(self, td=-1, Cg=-1, cam_begin=0, cam_dim=0):
        """switch the td / Cg / bg / intrinsics Jacobian blocks on (td = Cg = -1 and cam_dim = 0: off)"""
        if td < 0 and Cg < 0 and cam_dim == 0:
            self._check(self.lib.xivo_hip_set_calib(self.h, None))
        else:
            cl = CalibLayout(td, Cg, cam_begin, cam_dim)
            self._check(self.lib.xivo_hip_set_calib(self.h, C.byref(cl)))

    def set_calib_state(self, calib, b0=0):
        calib = np.ascontiguousarray(calib, dtype=calib_dtype)
        self._check(self.lib.xivo_hip_set_calib_state(self.h, b0, calib.shape[0], _ptr(calib)))

    def set_calib_gyro(self, gyro, b0=0):
        gyro = np.ascontiguousarray(gyro, dtype=np.float64).reshape(-1, 3)
        self._check(self.lib.xivo_hip_set_calib_gyro(self.h, b0, gyro.shape[0], _ptr(gyro)))

    def get_calib_state(self, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        out = np.zeros(nb, dtype=calib_dtype)
        self._check(self.lib.xivo_hip_get_calib_state(self.h, b0, nb, _ptr(out)))
        return out

    def get_jacobians_calib(self, b0=0, nb=None, F=None):
        nb = self.batch - b0 if nb is None else nb
        out = np.empty((nb, F, 2, 22))
        self._check(self.lib.xivo_hip_get_jacobians_calib(self.h, b0, nb, _ptr(out)))
        return out

    def update_joseph_host(self, H, inn, diagR, P_cm, b=0, mode=0, check=True):
        """The one-call plumbing entry (xivo_hip_update_joseph_host): H [M, N] row-major here (transposed to Eigen's
        column-major), P_cm a column-major N x N float64 array updated IN PLACE. Returns (err, rc)."""
        H = np.asarray(H, dtype=np.float64)
        M, N = H.shape
        assert N == self.N, (N, self.N)
        assert P_cm is None or (P_cm.dtype == np.float64 and P_cm.flags["F_CONTIGUOUS"] and P_cm.shape == (N, N))
        Hc = _f64(H.T)
        inn = _f64(inn); dR = _f64(diagR)
        err = np.empty(self.N)
        rc = self.lib.xivo_hip_update_joseph_host(self.h, b, M, _ptr(Hc), M, _ptr(inn), _ptr(dR),
                                                  None if P_cm is None else _ptr(P_cm), self.N, _ptr(err), mode)
        if check:
            self._check(rc)
        return err, rc

    def get_err(self, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        out = np.empty((nb, self.N))
        self._check(self.lib.xivo_hip_get_err(self.h, b0, nb, _ptr(out), self.N))
        return out

    def get_status(self, b0=0, nb=None, check=True):
        nb = self.batch - b0 if nb is None else nb
        out = np.zeros(nb, dtype=np.int32)
        rc = self.lib.xivo_hip_get_status(self.h, b0, nb, _ptr(out))
        if check:
            self._check(rc)
        return out

    def get_ldlt_used(self, b0=0, nb=None):
        """1 for every filter whose last update ran the pivoted L D L^T fallback (S not positive definite)"""
        nb = self.batch - b0 if nb is None else nb
        out = np.zeros(nb, dtype=np.int32)
        self._check(self.lib.xivo_hip_get_ldlt_used(self.h, b0, nb, _ptr(out)))
        return out

    def mh_gate_dense(self, F, R, thresh, mult, min_inliers, B=None):
        B = self.batch if B is None else B
        mask = np.zeros((B, F), dtype=np.uint8)
        dist = np.zeros((B, F))
        self._check(self.lib.xivo_hip_mh_gate_dense(self.h, B, F, R, thresh, mult, min_inliers, _ptr(mask),
                                                    _ptr(dist)))
        return mask.astype(bool), dist

    def update_dense_gated(self, F, R, thresh, mult, min_inliers, B=None):
        self._check(self.lib.xivo_hip_update_dense_gated(self.h, self.batch if B is None else B, F, R, thresh, mult,
                                                         min_inliers))

    def get_gate(self, F, B=None):
        B = self.batch if B is None else B
        mask = np.zeros((B, F), dtype=np.uint8)
        dist = np.zeros((B, F))
        self._check(self.lib.xivo_hip_get_gate(self.h, B, F, _ptr(mask), _ptr(dist)))
        return mask.astype(bool), dist

    # ---- G-level ------------------------------------------------------------
    def set_layout(self, N, group_begin, n_groups, feature_begin, n_features, cam):
        lay = Layout(N, group_begin, n_groups, feature_begin, n_features)
        self.layout = lay
        c = make_cam(cam)
        self._check(self.lib.xivo_hip_set_layout(self.h, C.byref(lay), C.byref(c)))

    def set_scene(self, poses, groups, feats, b0=0):
        poses = np.ascontiguousarray(poses, dtype=pose_dtype)
        groups = np.ascontiguousarray(groups, dtype=group_dtype)
        feats = np.ascontiguousarray(feats, dtype=feat_dtype)
        nb, F = feats.shape
        self.F = F
        self._check(self.lib.xivo_hip_set_scene(self.h, b0, nb, F, _ptr(poses), _ptr(groups), _ptr(feats)))

    def jacobians_instate(self, B=None):
        self._check(self.lib.xivo_hip_jacobians_instate(self.h, self.batch if B is None else B))

    def get_jacobians(self, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        J = np.empty((nb, self.F, 2, 21))
        inn = np.empty((nb, self.F, 2))
        self._check(self.lib.xivo_hip_get_jacobians(self.h, b0, nb, _ptr(J), _ptr(inn)))
        return J, inn

    def mh_gate(self, R, thresh, mult, min_inliers, B=None, want=True):
        B = self.batch if B is None else B
        if not want:      # mask / distances stay on the device (read them with get_gate)
            self._check(self.lib.xivo_hip_mh_gate(self.h, B, R, thresh, mult, min_inliers, None, None))
            return None
        mask = np.zeros((B, self.F), dtype=np.uint8)
        dist = np.zeros((B, self.F))
        self._check(self.lib.xivo_hip_mh_gate(self.h, B, R, thresh, mult, min_inliers, _ptr(mask), _ptr(dist)))
        return mask.astype(bool), dist

    def stack(self, R, B=None):
        self._check(self.lib.xivo_hip_stack(self.h, self.batch if B is None else B, R))

    def oos_project(self, feats, Roos, want_rows=True, whole_buffer=False):
        """feats: [nb, n_oos] oos_dtype, or a (nb, n_oos) tuple to project the resident list of the last call again.
        whole_buffer: XIVO_HIP_OOS_WHOLE_BUFFER - 2 * n_groups - 3 rows per feature, as src/oos.cpp:28 is coded"""
        if isinstance(feats, tuple):
            nb, n_oos = feats
            ptr = None
        else:
            feats = np.ascontiguousarray(feats, dtype=oos_dtype)
            nb, n_oos = feats.shape
            ptr = _ptr(feats)
        rows = np.zeros(nb, dtype=np.int32) if want_rows else None
        self._check(self.lib.xivo_hip_oos_project_ex(self.h, 0, nb, n_oos, ptr, Roos, _ptr(rows) if want_rows else None,
                                                     OOS_WHOLE_BUFFER if whole_buffer else 0))
        return rows

    def close_loop_stack(self, matches, Rlc, b0=0):
        """matches: [nb, n] lc_dtype - Feature::ComputeLCJacobian rows of Estimator::CloseLoopInternal become the staged measurement"""
        matches = np.ascontiguousarray(matches, dtype=lc_dtype)
        nb, n = matches.shape
        self._check(self.lib.xivo_hip_close_loop_stack(self.h, b0, nb, n, _ptr(matches), Rlc))

    def compress_oos(self, trigger_ratio=1.5, B=None, want_rows=True):
        """QR measurement compression of the OOS rows appended by oos_project (estimator.h:399-402)."""
        B = self.batch if B is None else B
        rows = np.zeros(B, dtype=np.int32)
        self._check(self.lib.xivo_hip_compress_oos(self.h, B, trigger_ratio, _ptr(rows) if want_rows else None))
        return rows

    def one_point_ransac(self, R, ransac_thresh, ransac_chi2, gauge=None, absorb_groups=None, B=None, want=True):
        """Estimator::OnePointRANSAC on the resident state (after jacobians_instate + mh_gate). gauge: [B] group slots
        (-1 none); absorb_groups: [B] uint64 masks of instate_groups_ (None: every slot).
        Returns (inlier mask [B, F], chi-square of the rescue test [B, F], rejected per filter [B])."""
        B = self.batch if B is None else B
        F = self.F
        g = None if gauge is None else np.ascontiguousarray(gauge, dtype=np.int32)
        ag = None if absorb_groups is None else np.ascontiguousarray(absorb_groups, dtype=np.uint64)
        if not want:      # results stay on the device (the inlier mask is read by the following stack / absorb)
            self._check(self.lib.xivo_hip_one_point_ransac(self.h, B, R, ransac_thresh, ransac_chi2, None if g is None else _ptr(g),
                                                           None if ag is None else _ptr(ag), None, None, None))
            return None
        mask = np.zeros((B, F), dtype=np.uint8); chi = np.zeros((B, F)); nrej = np.zeros(B, dtype=np.int32)
        self._check(self.lib.xivo_hip_one_point_ransac(self.h, B, R, ransac_thresh, ransac_chi2, None if g is None else _ptr(g),
                                                       None if ag is None else _ptr(ag), _ptr(mask), _ptr(chi), _ptr(nrej)))
        return mask.astype(bool), chi, nrej

    def filter_update(self, R, thresh, mult, min_inliers, use_gating=True, B=None):
        self._check(self.lib.xivo_hip_filter_update(self.h, self.batch if B is None else B, R, thresh, mult,
                                                    min_inliers, int(use_gating)))

    def last_path(self):
        """0: dense rows, 1: sparse-H (row-pair compressed) rows."""
        return int(self.lib.xivo_hip_last_path(self.h))

    def last_route(self):
        """Name of the route the last update pass took (the table of plan_update in capi_update.hip): fused, sparse_in_solve,
        sparse_whitened, sparse_symmetric, sparse_tail, dense_ascoded, dense_whitened, dense_symmetric."""
        return self.lib.xivo_hip_route_name(int(self.lib.xivo_hip_last_route(self.h))).decode()

    def subfilter_update(self, feats, Rtri=3.5, MH_thresh=5.991, ready_steps=5, min_depth=0.05, max_depth=5.0,
                         max_subfilter_outlier=0.01, b0=0):
        """feats: [nb, n] array of subfilter_dtype (P column-major); returns the updated copy."""
        feats = np.ascontiguousarray(feats, dtype=subfilter_dtype).copy()
        nb, n = feats.shape
        o = np.zeros(1, dtype=subfilter_opts_dtype)
        o["Rtri"], o["MH_thresh"], o["ready_steps"] = Rtri, MH_thresh, ready_steps
        o["min_depth"], o["max_depth"], o["max_subfilter_outlier"] = min_depth, max_depth, max_subfilter_outlier
        self._check(self.lib.xivo_hip_subfilter_update(self.h, b0, nb, n, _ptr(feats), _ptr(o)))
        return feats

    # ---- out-of-state feature pool (xivo_hip_pool_*)
    def pool_config(self, pool_max, anchor_max, Rtri=3.5, MH_thresh=5.991, ready_steps=5, min_depth=0.05, max_depth=5.0,
                    max_subfilter_outlier=0.01, remove_outlier_counter=10.0):
        o = np.zeros(1, dtype=subfilter_opts_dtype)
        o["Rtri"], o["MH_thresh"], o["ready_steps"] = Rtri, MH_thresh, ready_steps
        o["min_depth"], o["max_depth"], o["max_subfilter_outlier"] = min_depth, max_depth, max_subfilter_outlier
        self._check(self.lib.xivo_hip_pool_config(self.h, int(pool_max), int(anchor_max), _ptr(o), float(remove_outlier_counter)))
        self.pool_max, self.anchor_max = int(pool_max), int(anchor_max)

    def pool_anchor(self, slot, b0=0):
        """slot [nb]: anchor of each filter that takes the filter's current pose (-1: none)"""
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        self._check(self.lib.xivo_hip_pool_anchor(self.h, b0, int(slot.size), _ptr(slot)))

    def pool_add(self, recs):
        """recs: array of pool_new_dtype"""
        recs = np.ascontiguousarray(recs, dtype=pool_new_dtype)
        self._check(self.lib.xivo_hip_pool_add(self.h, int(recs.size), _ptr(recs) if recs.size else None))

    def pool_step(self, xp, strict=False):
        """xp [B, pool_max, 2] (NaN = dropped) -> (order [B, pool_max], n [B], live [B, pool_max] bool)"""
        xp = np.ascontiguousarray(xp, dtype=np.float64)
        B = xp.shape[0]
        order = np.empty((B, self.pool_max), dtype=np.int32); n = np.empty(B, dtype=np.int32)
        live = np.empty((B, self.pool_max), dtype=np.uint8)
        self._check(self.lib.xivo_hip_pool_step(self.h, B, _ptr(xp), int(bool(strict)), _ptr(order), _ptr(n), _ptr(live)))
        return order, n, live.astype(bool)

    def pool_get(self, b0=0, nb=None):
        """-> (entries [nb, pool_max] subfilter_dtype with ref_sind = anchor (-1: free), anchor poses [nb, anchor_max]
        group_dtype, anchor slots [nb, anchor_max] (-1: unlinked))"""
        nb = self.batch - b0 if nb is None else nb
        ent = np.zeros((nb, self.pool_max), dtype=subfilter_dtype)
        ap = np.zeros((nb, self.anchor_max), dtype=group_dtype); sl = np.zeros((nb, self.anchor_max), dtype=np.int32)
        self._check(self.lib.xivo_hip_pool_get(self.h, b0, nb, _ptr(ent), _ptr(ap), _ptr(sl)))
        return ent, ap, sl

    # ---- depth initialisation of new tracks: triangulation, AdaptInitialDepth
    def triangulate(self, R12, t12, xc1, xc2, method, zmin=0.05, zmax=5.0, max_theta_thresh=0.1 * np.pi / 180,
                    beta_thresh=0.25 * np.pi / 180):
        """n two-view problems (R12 [n, 3, 3], t12 [n, 3], xc1 / xc2 [n, 2]; thresholds in radians) -> (X [n, 3], ret [n] bool,
        good [n] bool) from xivo_hip_triangulate"""
        R12 = np.asarray(R12, dtype=np.float64).reshape(-1, 3, 3)
        n = R12.shape[0]
        pin = np.zeros(n, dtype=tri_in_dtype)
        pin["R12"] = np.transpose(R12, (0, 2, 1)).reshape(n, 9)   # column-major
        pin["t12"] = np.asarray(t12, dtype=np.float64).reshape(n, 3)
        pin["xc1"] = np.asarray(xc1, dtype=np.float64).reshape(n, 2)
        pin["xc2"] = np.asarray(xc2, dtype=np.float64).reshape(n, 2)
        out = np.zeros(n, dtype=tri_out_dtype)
        o = tri_options(method, zmin, zmax, max_theta_thresh, beta_thresh)
        self._check(self.lib.xivo_hip_triangulate(self.h, n, _ptr(pin), _ptr(out), _ptr(o)))
        return out["X"].copy(), out["ret"].astype(bool), out["good"].astype(bool)

    def pool_triangulation(self, method=None, zmin=0.05, zmax=5.0, max_theta_thresh=0.1 * np.pi / 180,
                           beta_thresh=0.25 * np.pi / 180):
        """triangulate_pre_subfilter on the pool's first steps; method None / TRI_OFF / "off" disables it"""
        if method is None:
            self._check(self.lib.xivo_hip_pool_triangulation(self.h, None))
            return
        o = tri_options(method, zmin, zmax, max_theta_thresh, beta_thresh)
        self._check(self.lib.xivo_hip_pool_triangulation(self.h, _ptr(o)))

    def pool_tri_counts(self, b0=0, nb=None):
        """-> (good [nb], bad [nb]) triangulations since pool_config"""
        nb = self.batch - b0 if nb is None else nb
        g = np.zeros(nb, dtype=np.int32); b = np.zeros(nb, dtype=np.int32)
        self._check(self.lib.xivo_hip_pool_tri_counts(self.h, b0, nb, _ptr(g), _ptr(b)))
        return g, b

    def pool_adapt_depth_config(self, initial_z, median_weight=0.99, min_feature_lifetime=5, min_z=0.05, max_z=5.0):
        o = np.zeros(1, dtype=adapt_opts_dtype)
        o["struct_size"] = adapt_opts_dtype.itemsize
        o["initial_z"], o["median_weight"], o["min_feature_lifetime"] = initial_z, median_weight, min_feature_lifetime
        o["min_z"], o["max_z"] = min_z, max_z
        self._check(self.lib.xivo_hip_pool_adapt_depth_config(self.h, _ptr(o)))

    def pool_adapt_depth(self, B=None):
        """AdaptInitialDepth on filters [0, B) -> init_z [B] afterwards"""
        B = self.batch if B is None else int(B)
        z = np.zeros(B, dtype=np.float64)
        self._check(self.lib.xivo_hip_pool_adapt_depth(self.h, B, _ptr(z)))
        return z

    def pool_get_init_z(self, b0=0, nb=None):
        """-> [nb] the resident init_z as it is (no AdaptInitialDepth step); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        z = np.zeros(nb)
        self._check(self.lib.xivo_hip_pool_get_init_z(self.h, int(b0), nb, _ptr(z)))
        return z

    def pool_add_ex(self, recs, options=0):
        """recs: array of pool_new_dtype; options POOL_ADD_ADAPTIVE_Z: z0 from the filter's resident init_z"""
        recs = np.ascontiguousarray(recs, dtype=pool_new_dtype)
        self._check(self.lib.xivo_hip_pool_add_ex(self.h, int(recs.size), _ptr(recs) if recs.size else None, int(options)))

    def givens(self, x, Hx, Hf, effective_rows=-1):
        """Batched xivo::Givens. x [nb, rows], Hx [nb, rows, nx], Hf [nb, rows, nf] (row-major numpy views of the
        matrices); returns (rows_out, x, Hx, Hf)."""
        nb, rows, nx = Hx.shape
        nf = Hf.shape[2]
        xd = np.ascontiguousarray(x, dtype=np.float64).copy()
        Hxd = np.ascontiguousarray(np.transpose(Hx, (0, 2, 1)), dtype=np.float64).copy()   # column-major per problem
        Hfd = np.ascontiguousarray(np.transpose(Hf, (0, 2, 1)), dtype=np.float64).copy()
        ro = np.zeros(nb, dtype=np.int32)
        self._check(self.lib.xivo_hip_givens(self.h, nb, rows, nx, nf, _ptr(xd), _ptr(Hxd), _ptr(Hfd), effective_rows, _ptr(ro)))
        return ro, xd, np.transpose(Hxd, (0, 2, 1)).copy(), np.transpose(Hfd, (0, 2, 1)).copy()

    def qr(self, x, Hx, effective_rows=-1):
        nb, rows, nx = Hx.shape
        xd = np.ascontiguousarray(x, dtype=np.float64).copy()
        Hxd = np.ascontiguousarray(np.transpose(Hx, (0, 2, 1)), dtype=np.float64).copy()
        ro = np.zeros(nb, dtype=np.int32)
        self._check(self.lib.xivo_hip_qr(self.h, nb, rows, nx, _ptr(xd), _ptr(Hxd), effective_rows, _ptr(ro)))
        return ro, xd, np.transpose(Hxd, (0, 2, 1)).copy()

    def propagate(self, imu, Qimu, Qmodel, g, method="RK4", stepsize=0.002, b0=0, pd_control=None):
        """imu: [nb] or [nb, n_imu] array of imu_dtype (the samples since the last call, in order); Qimu 12x12,
        Qmodel 23x23 (numpy row-major). pd_control: dict(tolerance, attempts, min_scale_factor, max_scale_factor) switches on the
        step-size-controlled branch of Estimator::PrinceDormand (src/princedormand.cpp:26-60, as coded)."""
        imu = np.ascontiguousarray(imu, dtype=imu_dtype)
        if imu.ndim == 1:
            imu = imu[:, None]
        imu = np.ascontiguousarray(imu)
        o = prop_options(Qimu, Qmodel, g, method, stepsize, pd_control)
        self._check(self.lib.xivo_hip_propagate(self.h, b0, imu.shape[0], imu.shape[1], _ptr(imu), _ptr(o)))

    def propagate_calib(self, imu, Qimu, Qmodel, g, method="RK4", stepsize=0.002, b0=0, pd_control=None):
        """Estimator::Propagate of an online-calibration build (set_calib with td >= 0 or Cg >= 0): Qmodel is
        kMotionSize x kMotionSize (numpy row-major); the resident calibration state supplies Cg / Ca."""
        imu = np.ascontiguousarray(imu, dtype=imu_dtype)
        if imu.ndim == 1:
            imu = imu[:, None]
        imu = np.ascontiguousarray(imu)
        o = np.zeros(1, dtype=prop_opts_dtype)
        o["Qimu"] = np.asarray(Qimu, dtype=np.float64).T.reshape(-1)
        o["g"] = g; o["method"] = 0 if method == "RK4" else 1; o["stepsize"] = stepsize
        if pd_control is not None:
            o["control_stepsize"] = 1
            o["tolerance"] = pd_control.get("tolerance", 1e-3); o["attempts"] = pd_control.get("attempts", 12)
            o["min_scale_factor"] = pd_control.get("min_scale_factor", 0.125); o["max_scale_factor"] = pd_control.get("max_scale_factor", 4.0)
        Qm = np.ascontiguousarray(np.asarray(Qmodel, dtype=np.float64).T)
        self._check(self.lib.xivo_hip_propagate_calib(self.h, b0, imu.shape[0], imu.shape[1], _ptr(imu), _ptr(o), _ptr(Qm)))

    def absorb_error(self, B=None):
        self._check(self.lib.xivo_hip_absorb_error(self.h, self.batch if B is None else B))

    def edit_batch(self, F, ops):
        """ops: array of edit_dtype; sorted by filter here (stable, so the per-filter order is kept)."""
        ops = np.ascontiguousarray(ops, dtype=edit_dtype)
        if ops.size:
            ops = np.ascontiguousarray(ops[np.argsort(ops["b"], kind="stable")])
        self.F = F
        self._check(self.lib.xivo_hip_edit_batch(self.h, F, int(ops.size), _ptr(ops) if ops.size else None))

    def set_pixels(self, xp, b0=0):
        """xp: [nb, F, 2], NaN = leave the entry's pixel as it is"""
        xp = np.ascontiguousarray(xp, dtype=np.float64)
        nb, F = xp.shape[:2]
        self.F = F
        self._check(self.lib.xivo_hip_set_pixels(self.h, b0, nb, F, _ptr(xp)))

    def get_scene(self, b0=0, nb=None):
        nb = self.batch - b0 if nb is None else nb
        poses = np.zeros(nb, dtype=pose_dtype)
        groups = np.zeros((nb, self.layout.n_groups), dtype=group_dtype)
        feats = np.zeros((nb, self.F), dtype=feat_dtype)
        self._check(self.lib.xivo_hip_get_scene(self.h, b0, nb, _ptr(poses), _ptr(groups), _ptr(feats)))
        return poses, groups, feats

    def get_H(self, b):
        M = C.c_int()
        self._check(self.lib.xivo_hip_get_H(self.h, b, C.byref(M), None, 0, None, None))
        M = M.value
        H = np.empty((self.N, M))
        inn = np.empty(M)
        dR = np.empty(M)
        self._check(self.lib.xivo_hip_get_H(self.h, b, None, _ptr(H), M, _ptr(inn), _ptr(dR)))
        return H.T.copy(), inn, dR

    # ---- what the per-frame logs share: `log` is "traj", "map" or "innov" (xivo_hip_<log>_record / _count / _reset; _log_span
    # also takes "trajsim", whose count is 0 where the others' is an error)
    def _log_record(self, log, ts_ns, B):
        k = C.c_int(-1)
        self._check(getattr(self.lib, "xivo_hip_%s_record" % log)(self.h, self.batch if B is None else int(B), int(ts_ns), C.byref(k)))
        return k.value

    def _log_count(self, log):
        n = getattr(self.lib, "xivo_hip_%s_count" % log)(self.h)
        if n < 0:
            self._check(n)
        return n

    def _log_reset(self, log):
        self._check(getattr(self.lib, "xivo_hip_%s_reset" % log)(self.h))

    def _log_span(self, log, b0, nb, t0, nt):
        """(nb, nt) of a slice: by default the filters from b0 on and the recorded frames from t0 on"""
        return (self.batch - b0 if nb is None else int(nb)), (self._log_count(log) - t0 if nt is None else int(nt))

    # ---- trajectory log (xivo_hip_traj_*)
    def traj_config(self, T_max, cols=()):
        """a device log of T_max frames: per frame and filter the motion state and the packed lower triangle of
        P[cols, cols]; T_max = 0 releases it"""
        cols = np.asarray(cols, dtype=np.int64).reshape(-1)
        o = np.zeros(1, dtype=traj_opts_dtype)
        o["T_max"], o["n_cols"] = int(T_max), cols.size
        if cols.size <= TRAJ_MAX_COLS:
            o["cols"][0, :cols.size] = np.clip(cols, -1, 2 ** 31 - 1)
        self._check(self.lib.xivo_hip_traj_config(self.h, _ptr(o)))
        self.traj_cols = cols.astype(np.int32) if T_max > 0 else None

    def traj_record(self, ts_ns=0, B=None):
        """append one frame (asynchronous) -> its index"""
        return self._log_record("traj", ts_ns, B)

    def traj_count(self):
        return self._log_count("traj")

    def traj_reset(self):
        self._log_reset("traj")

    def traj_read(self, b0=0, nb=None, t0=0, nt=None):
        """-> (recs [nt, nb] traj_dtype, cov [nt, nb, n, n] symmetric (from the packed lower triangle), ts [nt] ns)"""
        nb, nt = self._log_span("traj", b0, nb, t0, nt)
        n = int(self.traj_cols.size)
        recs = np.zeros((nt, nb), dtype=traj_dtype)
        packed = np.zeros((nt, nb, n * (n + 1) // 2))
        ts = np.zeros(nt, dtype=np.int64)
        self._check(self.lib.xivo_hip_traj_read(self.h, b0, nb, t0, nt, _ptr(recs), _ptr(packed), _ptr(ts)))
        cov = np.zeros((nt, nb, n, n))
        i, j = np.tril_indices(n)      # row by row: (i, j) at i (i + 1) / 2 + j
        cov[:, :, i, j] = packed
        cov[:, :, j, i] = packed
        return recs, cov, ts

    def traj_nees(self, gt_Rsb, gt_Tsb, b0=0, t0=0):
        """gt_Rsb [nt, nb, 3, 3], gt_Tsb [nt, nb, 3]: the true poses of the slice -> (err6 [nt, nb, 6] = (log(R_est^T R_gt),
        T_gt - T_est), nees [nt, nb] (NaN: block not positive definite), anees [nt], n_used [nt])"""
        R = np.asarray(gt_Rsb, dtype=np.float64)
        nt, nb = R.shape[:2]
        gt = np.empty((nt, nb, 12))
        gt[:, :, :9] = np.transpose(R, (0, 1, 3, 2)).reshape(nt, nb, 9)      # column-major
        gt[:, :, 9:] = np.asarray(gt_Tsb, dtype=np.float64).reshape(nt, nb, 3)
        err6 = np.zeros((nt, nb, 6)); nees = np.zeros((nt, nb)); anees = np.zeros(nt); used = np.zeros(nt, dtype=np.int32)
        self._check(self.lib.xivo_hip_traj_nees(self.h, b0, nb, t0, nt, _ptr(gt), _ptr(err6), _ptr(nees), _ptr(anees), _ptr(used)))
        return err6, nees, anees, used

    def traj_score(self, gt, b0=0, nb=None, t0=0, nt=None, align=True, rpe_lag=0):
        """ATE / RPE of the logged poses of the slice against ground truth, on the device (xivo_hip_traj_score).
        gt: (gt_Rsb [nt, nb, 3, 3], gt_Tsb [nt, nb, 3]) or the packed [nt, nb, 12] (Rsb column-major, then Tsb)
        -> traj_score_dtype [nb]; R as stored (column-major): rec["R"].reshape(3, 3).T is the matrix, gt -> est"""
        if isinstance(gt, (tuple, list)):
            R = np.asarray(gt[0], dtype=np.float64)
            g = np.empty(R.shape[:2] + (12,))
            g[:, :, :9] = np.transpose(R, (0, 1, 3, 2)).reshape(R.shape[:2] + (9,))
            g[:, :, 9:] = np.asarray(gt[1], dtype=np.float64).reshape(R.shape[:2] + (3,))
        else:
            g = _f64(gt)
        nb, nt = self._log_span("traj", b0, nb, t0, nt)
        if g.shape != (nt, nb, 12):
            raise ValueError("gt must be [nt = %d, nb = %d, 12], got %s" % (nt, nb, g.shape))
        o = np.zeros(1, dtype=traj_score_opts_dtype)
        o["align"], o["rpe_lag"] = int(bool(align)), int(rpe_lag)
        out = np.zeros(nb, dtype=traj_score_dtype)
        self._check(self.lib.xivo_hip_traj_score(self.h, int(b0), nb, int(t0), nt, _ptr(g), _ptr(o), _ptr(out)))
        return out

    # ---- landmark log (xivo_hip_map_*)
    def map_config(self, T_max, n_out=0, world_cov=True):
        """a device log of T_max frames: per frame and filter the best n_out in-state features (ascending norm of the local
        covariance block, ties by list position) with world position, local block, pixel and - world_cov - the covariance
        of the world position; T_max = 0 releases it"""
        o = np.zeros(1, dtype=map_opts_dtype)
        o["T_max"], o["n_out"], o["flags"] = int(T_max), int(n_out), MAP_WORLD_COV if world_cov else 0
        self._check(self.lib.xivo_hip_map_config(self.h, _ptr(o)))
        self.map_n_out = int(n_out) if T_max > 0 else None

    def map_record(self, ts_ns=0, B=None):
        """append one frame (asynchronous) -> its index"""
        return self._log_record("map", ts_ns, B)

    def map_count(self):
        return self._log_count("map")

    def map_reset(self):
        self._log_reset("map")

    def map_read(self, b0=0, nb=None, t0=0, nt=None):
        """-> (pts [nt, nb, n_out] map_pt_dtype, n_pts [nt, nb], ts [nt] ns); slots behind n_pts are zeros with pos = sind = -1"""
        nb, nt = self._log_span("map", b0, nb, t0, nt)
        pts = np.zeros((nt, nb, self.map_n_out), dtype=map_pt_dtype)
        n_pts = np.zeros((nt, nb), dtype=np.int32)
        ts = np.zeros(nt, dtype=np.int64)
        self._check(self.lib.xivo_hip_map_read(self.h, b0, nb, t0, nt, _ptr(pts), _ptr(n_pts), _ptr(ts)))
        return pts, n_pts, ts

    def map_nees(self, gt, b0=0, t0=0):
        """gt [nt, nb, n_out, 3]: the true world point of every slot of the slice (NaN: none) -> (err3 [nt, nb, n_out, 3] =
        gt - Xs, nees [nt, nb, n_out] (NaN: no entry, no truth, covariance not positive definite), anees [nt], n_used [nt])"""
        gt = _f64(gt)
        nt, nb, n_out = gt.shape[:3]
        if n_out != self.map_n_out or gt.shape[3:] != (3,):
            raise ValueError("gt must be [nt, nb, n_out, 3]")
        err3 = np.zeros((nt, nb, n_out, 3)); nees = np.zeros((nt, nb, n_out)); anees = np.zeros(nt)
        used = np.zeros(nt, dtype=np.int32)
        self._check(self.lib.xivo_hip_map_nees(self.h, b0, nb, t0, nt, _ptr(gt), _ptr(err3), _ptr(nees), _ptr(anees), _ptr(used)))
        return err3, nees, anees, used

    # ---- innovation log (xivo_hip_innov_*)
    def innov_config(self, T_max):
        """a device log of T_max frames: per frame and filter the normalised innovation squared of the update, its pre- and
        post-fit sums, the counted rows and the update's flags; T_max = 0 releases it"""
        o = np.zeros(1, dtype=innov_opts_dtype)
        o["T_max"] = int(T_max)
        self._check(self.lib.xivo_hip_innov_config(self.h, _ptr(o)))

    def innov_record(self, ts_ns=0, B=None):
        """append one frame (asynchronous; after the update, before absorb_error) -> its index"""
        return self._log_record("innov", ts_ns, B)

    def innov_count(self):
        return self._log_count("innov")

    def innov_reset(self):
        self._log_reset("innov")

    def innov_read(self, b0=0, nb=None, t0=0, nt=None):
        """-> (recs [nt, nb] innov_rec_dtype, ts [nt] ns)"""
        nb, nt = self._log_span("innov", b0, nb, t0, nt)
        recs = np.zeros((nt, nb), dtype=innov_rec_dtype)
        ts = np.zeros(nt, dtype=np.int64)
        self._check(self.lib.xivo_hip_innov_read(self.h, int(b0), nb, int(t0), nt, _ptr(recs), _ptr(ts)))
        return recs, ts

    def innov_stats(self, b0=0, nb=None, t0=0, nt=None):
        """sums over the records with flags = 0 and a finite nis -> dict: frame_nis / frame_dof / frame_used [nt] over the
        slice's filters, filt_nis / filt_dof / filt_used [nb] over its frames; frame_nis / frame_dof is the figure to hold
        against 1"""
        nb, nt = self._log_span("innov", b0, nb, t0, nt)
        out = {"frame_nis": np.zeros(nt), "frame_dof": np.zeros(nt, dtype=np.int64), "frame_used": np.zeros(nt, dtype=np.int32),
               "filt_nis": np.zeros(nb), "filt_dof": np.zeros(nb, dtype=np.int64), "filt_used": np.zeros(nb, dtype=np.int32)}
        self._check(self.lib.xivo_hip_innov_stats(self.h, int(b0), nb, int(t0), nt, _ptr(out["frame_nis"]), _ptr(out["frame_dof"]),
                                                  _ptr(out["frame_used"]), _ptr(out["filt_nis"]), _ptr(out["filt_dof"]),
                                                  _ptr(out["filt_used"])))
        return out

    # ---- device life cycle (xivo_hip_life_*)
    def life_config(self, tracks_max, min_depth=0.05, max_depth=10.0, min_new_features=3, var_xyz=(1.0, 1.0, 1.0)):
        """the device-resident slot book and the track staging of the "immediate" life cycle: at most tracks_max tracks per
        filter and frame (<= LIFE_MAX_TRACKS); var_xyz: diagonal of a new feature's covariance; tracks_max = 0 releases it"""
        o = np.zeros(1, dtype=life_opts_dtype)
        o["tracks_max"], o["min_new_features"], o["min_depth"], o["max_depth"] = int(tracks_max), int(min_new_features), min_depth, max_depth
        o["var_xyz"] = np.asarray(var_xyz, dtype=np.float64)
        self._check(self.lib.xivo_hip_life_config(self.h, _ptr(o)))

    def life_set_book(self, feat_id, b0=0):
        """feat_id [nb, F]: the track ids of the scene placed with set_scene (-1: absent entry)"""
        feat_id = np.ascontiguousarray(feat_id, dtype=np.int64)
        self._check(self.lib.xivo_hip_life_set_book(self.h, int(b0), feat_id.shape[0], _ptr(feat_id)))

    def life_get_book(self, b0=0, nb=None):
        """-> (feat_id [nb, F] int64, feat_ref [nb, F], group_refs [nb, n_groups]); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        feat_id = np.full((nb, self.F), -1, dtype=np.int64)
        feat_ref = np.full((nb, self.F), -1, dtype=np.int32)
        group_refs = np.full((nb, self.layout.n_groups), -1, dtype=np.int32)
        self._check(self.lib.xivo_hip_life_get_book(self.h, int(b0), nb, _ptr(feat_id), _ptr(feat_ref), _ptr(group_refs)))
        return feat_id, feat_ref, group_refs

    def life_begin(self, F, off, ids, meas, B=None):
        """before the update (asynchronous): the frame's tracks as off [B + 1] int32, ids [n] int64, meas [n, 3] (u, v, depth)"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        meas = np.ascontiguousarray(meas, dtype=np.float64)
        B = off.size - 1 if B is None else int(B)
        if off.size != B + 1 or ids.size != int(off[-1]) or meas.size != 3 * ids.size:
            raise ValueError("off [B + 1], ids [off[B]], meas [off[B], 3]")
        self._check(self.lib.xivo_hip_life_begin(self.h, B, int(F), _ptr(off), _ptr(ids), _ptr(meas)))
        self.F = int(F)

    def life_begin_keys(self, F, off, ids, meas, keys, B=None):
        """life_begin plus keys [n] int64, parallel to ids (after lcmap_life_config(True))"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        meas = np.ascontiguousarray(meas, dtype=np.float64)
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        B = off.size - 1 if B is None else int(B)
        if off.size != B + 1 or ids.size != int(off[-1]) or meas.size != 3 * ids.size or keys.size != ids.size:
            raise ValueError("off [B + 1], ids [off[B]], meas [off[B], 3], keys [off[B]]")
        self._check(self.lib.xivo_hip_life_begin_keys(self.h, B, int(F), _ptr(off), _ptr(ids), _ptr(meas), _ptr(keys)))
        self.F = int(F)

    def life_begin_tracks(self, F, B=None):
        """life_begin on the tracks the last pcw_tracks(B) left on the device (asynchronous, no upload)"""
        self._check(self.lib.xivo_hip_life_begin_tracks(self.h, self.batch if B is None else int(B), int(F)))
        self.F = int(F)

    # ---- tuning table (xivo_hip_tune_*)
    def tune_config(self, entry=None):
        """every filter's R, MH_thresh, var_xyz, Qimu and Qmodel from a resident table whose rows all start as `entry` (one
        tune_dtype record; tune_entry builds one); None releases the table and brings the calls' scalar arguments back"""
        if entry is None:
            self._check(self.lib.xivo_hip_tune_config(self.h, None))
            return
        e = np.ascontiguousarray(entry, dtype=tune_dtype).reshape(1)
        self._check(self.lib.xivo_hip_tune_config(self.h, _ptr(e)))

    def tune_set(self, table, b0=0):
        """rows [b0, b0 + len(table)) <- table (tune_dtype); staged and enqueued, all rows or none"""
        t = np.ascontiguousarray(table, dtype=tune_dtype).reshape(-1)
        self._check(self.lib.xivo_hip_tune_set(self.h, int(b0), t.shape[0], _ptr(t)))

    def tune_get(self, b0=0, nb=None):
        """-> rows [b0, b0 + nb) as a tune_dtype array; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        t = np.zeros(nb, dtype=tune_dtype)
        self._check(self.lib.xivo_hip_tune_get(self.h, int(b0), nb, _ptr(t)))
        return t

    # ---- point-cloud world on the device (xivo_hip_pcw_*)
    def pcw_config(self, npts, fx=0.0, fy=0.0, cx=0.0, cy=0.0, imw=0.0, imh=0.0):
        """the resident worlds of every filter, npts points each (<= the life cycle's tracks_max; 0 releases them), seen by
        one pinhole camera; needs life_config or pool_life_config first, and either releases them"""
        o = np.zeros(1, dtype=pcw_opts_dtype)
        o["struct_size"], o["npts"] = pcw_opts_dtype.itemsize, int(npts)
        o["fx"], o["fy"], o["cx"], o["cy"], o["imw"], o["imh"] = fx, fy, cx, cy, imw, imh
        self._check(self.lib.xivo_hip_pcw_config(self.h, _ptr(o)))
        self.pcw_npts = int(npts)

    def pcw_camera(self, cam=None, max_radius=float("inf")):
        """the camera the producer projects through, after pcw_config: a camera dict as set_layout takes it (any model; the image
        is cols x rows); a point whose normalised radius exceeds max_radius is not visible. None: the pinhole of pcw_config"""
        if cam is None:
            self._check(self.lib.xivo_hip_pcw_camera(self.h, None, 0.0))
        else:
            self._check(self.lib.xivo_hip_pcw_camera(self.h, C.byref(make_cam(cam)), float(max_radius)))

    def pcw_set_world(self, Xs, ids=None, next_id=None, b0=0):
        """Xs [nb, npts, 3]; ids [nb, npts] int64 (None: no point is tracked); next_id [nb] (None: 10000)"""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 3 or Xs.shape[1:] != (self.pcw_npts, 3):
            raise ValueError("Xs [nb, npts, 3]")
        nb = Xs.shape[0]
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        next_id = None if next_id is None else np.ascontiguousarray(next_id, dtype=np.int64)
        if (ids is not None and ids.shape != (nb, self.pcw_npts)) or (next_id is not None and next_id.shape != (nb,)):
            raise ValueError("ids [nb, npts], next_id [nb]")
        self._check(self.lib.xivo_hip_pcw_set_world(self.h, int(b0), nb, _ptr(Xs), None if ids is None else _ptr(ids),
                                                    None if next_id is None else _ptr(next_id)))

    def pcw_get_world(self, b0=0, nb=None):
        """-> (ids [nb, npts] int64, next_id [nb] int64); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        ids = np.full((nb, self.pcw_npts), -1, dtype=np.int64)
        next_id = np.zeros(nb, dtype=np.int64)
        self._check(self.lib.xivo_hip_pcw_get_world(self.h, int(b0), nb, _ptr(ids), _ptr(next_id)))
        return ids, next_id

    def pcw_tracks(self, gsc, noise_px_std, seed, frame, B=None):
        """one frame's tracks of filters [0, B) from the resident worlds (asynchronous): gsc [B, 12] = Rsc row-major, Tsc"""
        gsc = np.ascontiguousarray(gsc, dtype=np.float64)
        B = gsc.shape[0] if B is None else int(B)
        if gsc.shape != (B, 12):
            raise ValueError("gsc [B, 12]")
        self._check(self.lib.xivo_hip_pcw_tracks(self.h, B, _ptr(gsc), float(noise_px_std), int(seed), int(frame)))

    def pcw_get_tracks(self, tracks_max, b0=0, nb=None):
        """what the last pcw_tracks left -> (cnt [nb] int32, ids [nb, tracks_max] int64, meas [nb, tracks_max, 3]); entries
        behind cnt read -1 / 0; tracks_max: the life cycle's; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        cnt = np.zeros(nb, dtype=np.int32)
        ids = np.full((nb, int(tracks_max)), -1, dtype=np.int64)
        meas = np.zeros((nb, int(tracks_max), 3))
        self._check(self.lib.xivo_hip_pcw_get_tracks(self.h, int(b0), nb, _ptr(cnt), _ptr(ids), _ptr(meas)))
        return cnt, ids, meas

    def pcw_tracks_resident(self, noise_px_std, seed, frame, B=None):
        """pcw_tracks on the camera poses the last trajsim_frame(B) left on the device (asynchronous, no upload)"""
        self._check(self.lib.xivo_hip_pcw_tracks_resident(self.h, self.batch if B is None else int(B), float(noise_px_std),
                                                          int(seed), int(frame)))

    # ---- track faults of the producer (xivo_hip_pcw_fault_*)
    def pcw_fault_config(self, faults=None):
        """faults: a dict of xivo_pcw_fault_opts' fields (pcw.fault_opts fills the defaults) - on; None - off, releases"""
        if faults is None:
            self._check(self.lib.xivo_hip_pcw_fault_config(self.h, None))
            return
        o = np.zeros(1, dtype=pcw_fault_opts_dtype)
        o["struct_size"] = pcw_fault_opts_dtype.itemsize
        for k, v in faults.items():
            o[k] = v
        self._check(self.lib.xivo_hip_pcw_fault_config(self.h, _ptr(o)))

    def pcw_stream_share(self, W):
        """filters w, w + W, ... draw the same pixel-noise and fault words from the next frame call on (0: each its own)"""
        self._check(self.lib.xivo_hip_pcw_stream_share(self.h, int(W)))

    def pcw_fault_score(self, B=None):
        """the gate's decisions of the open frame against the tracks' fault flags, added to the counters (asynchronous)"""
        self._check(self.lib.xivo_hip_pcw_fault_score(self.h, self.batch if B is None else int(B)))

    def pcw_fault_stats(self, b0=0, nb=None):
        """-> [nb] pcw_fault_stats_dtype; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=pcw_fault_stats_dtype)
        self._check(self.lib.xivo_hip_pcw_fault_get_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    def pcw_fault_flags(self, tracks_max, b0=0, nb=None):
        """the flag byte of every track the last pcw_tracks left -> [nb, tracks_max] uint8, parallel to pcw_get_tracks' ids"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros((nb, int(tracks_max)), dtype=np.uint8)
        self._check(self.lib.xivo_hip_pcw_fault_get_flags(self.h, int(b0), nb, _ptr(out)))
        return out

    # ---- trajectory producer on the device (xivo_hip_trajsim_*)
    def trajsim_config(self, n_max, T_max=0, imu_dt=0.0025, rot_amp=0.2, rot_w=None, noise_accel=1e-4, noise_gyro=1e-5,
                       grav_s=(0, 0, -9.8), Rbc=None, Tbc=(0, 0, 0), seed=1):
        """the simulated IMU and ground truth of every filter on the device: at most n_max samples per frame, a ground-truth
        log of T_max frames (n_max = 0 releases it); Rbc [3, 3], Tbc [3]: body to camera; the rest as BatchTrajectorySim"""
        o = np.zeros(1, dtype=trajsim_opts_dtype)
        o["struct_size"], o["n_max"], o["T_max"], o["imu_dt"] = trajsim_opts_dtype.itemsize, int(n_max), int(T_max), imu_dt
        # (the default profile is BatchTrajectorySim's, to the bit: 0.3 * 3.0 is not 0.9)
        o["rot_amp"], o["rot_w"] = rot_amp, np.array([0.3, 0.4, 0.1]) * 3.0 if rot_w is None else rot_w
        o["noise_accel"], o["noise_gyro"], o["grav_s"] = noise_accel, noise_gyro, grav_s
        o["Rbc"] = (np.eye(3) if Rbc is None else np.asarray(Rbc, dtype=np.float64)).reshape(-1)
        o["Tbc"], o["seed"] = Tbc, int(seed) & (2 ** 64 - 1)
        self._check(self.lib.xivo_hip_trajsim_config(self.h, _ptr(o)))

    def trajsim_set(self, motion, rate, b0=0):
        """curve ("lissajous" / "trefoil" or 0 / 1) and rate of filters [b0, b0 + len(rate))"""
        m = np.ascontiguousarray([TRAJSIM_MOTIONS[x] if isinstance(x, str) else int(x) for x in motion], dtype=np.int32)
        r = np.ascontiguousarray(rate, dtype=np.float64)
        if m.shape != r.shape or r.ndim != 1:
            raise ValueError("motion [nb], rate [nb]")
        self._check(self.lib.xivo_hip_trajsim_set(self.h, int(b0), r.shape[0], _ptr(m), _ptr(r)))

    def trajsim_frame(self, k0, n, B=None):
        """records k0 + 1 .. k0 + n and the poses at sample k0 + n of filters [0, B) (asynchronous)"""
        self._check(self.lib.xivo_hip_trajsim_frame(self.h, self.batch if B is None else int(B), int(k0), int(n)))

    def propagate_resident(self, Qimu=None, Qmodel=None, g=None, method="RK4", stepsize=0.002, pd_control=None, B=None, opts=None):
        """propagate over the records the last trajsim_frame(B) left (asynchronous); opts: a prop_options() record kept by the
        caller, instead of building one per call"""
        o = prop_options(Qimu, Qmodel, g, method, stepsize, pd_control) if opts is None else opts
        self._check(self.lib.xivo_hip_propagate_resident(self.h, self.batch if B is None else int(B), _ptr(o)))

    def trajsim_get(self, b0=0, nb=None):
        """what the last trajsim_frame left -> (recs [nb, n] imu_dtype, gsc [nb, 12]); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        n = C.c_int(0)
        self._check(self.lib.xivo_hip_trajsim_get(self.h, int(b0), 0, None, None, C.byref(n)))
        recs = np.zeros((nb, n.value), dtype=imu_dtype)
        gsc = np.zeros((nb, 12))
        self._check(self.lib.xivo_hip_trajsim_get(self.h, int(b0), nb, _ptr(recs), _ptr(gsc), None))
        return recs, gsc

    def trajsim_count(self):
        return int(self.lib.xivo_hip_trajsim_count(self.h))

    def trajsim_get_gt(self, b0=0, nb=None, t0=0, nt=None):
        """the ground-truth log -> gt [nt, nb, 12] (Rsb column-major, Tsb): what traj_score / traj_nees take packed"""
        nb, nt = self._log_span("trajsim", b0, nb, t0, nt)
        gt = np.zeros((nt, nb, 12))
        self._check(self.lib.xivo_hip_trajsim_get_gt(self.h, int(b0), nb, int(t0), nt, _ptr(gt)))
        return gt

    def trajsim_reset(self):
        self._check(self.lib.xivo_hip_trajsim_reset(self.h))

    def life_end(self, B=None):
        """after the update and absorb_error (asynchronous)"""
        self._check(self.lib.xivo_hip_life_end(self.h, self.batch if B is None else int(B)))

    def life_stats(self, b0=0, nb=None):
        """-> [nb] life_stats_dtype: the per-filter counters; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=life_stats_dtype)
        self._check(self.lib.xivo_hip_life_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    # ---- device pool life cycle (xivo_hip_pool_life_*)
    def pool_life_config(self, tracks_max, max_group_lifetime=1, initial_z=2.5, std_xyz=(1.0, 1.0, 1.0), adaptive_z=False):
        """the device-resident books, the step's device buffers and the track staging of the "subfilter" life cycle, after
        pool_config on an empty pool: at most tracks_max tracks per filter and frame (<= LIFE_MAX_TRACKS); initial_z / std_xyz:
        a new entry's depth and stds; adaptive_z: the depth is the resident init_z (after pool_adapt_depth_config);
        tracks_max = 0 releases it and hands the pool back to the host calls"""
        o = np.zeros(1, dtype=pool_life_opts_dtype)
        o["struct_size"], o["tracks_max"], o["max_group_lifetime"] = pool_life_opts_dtype.itemsize, int(tracks_max), int(max_group_lifetime)
        o["adaptive_z"], o["initial_z"], o["std_xyz"] = int(bool(adaptive_z)), float(initial_z), np.asarray(std_xyz, dtype=np.float64)
        self._check(self.lib.xivo_hip_pool_life_config(self.h, _ptr(o)))

    def pool_life_set_book(self, feat_id, b0=0):
        """feat_id [nb, F]: the track ids of the scene placed with set_scene (-1: absent entry)"""
        feat_id = np.ascontiguousarray(feat_id, dtype=np.int64)
        self._check(self.lib.xivo_hip_pool_life_set_book(self.h, int(b0), feat_id.shape[0], _ptr(feat_id)))

    def pool_life_get_book(self, b0=0, nb=None):
        """-> dict(feat_id [nb, F] int64, feat_ref [nb, F], group_refs [nb, n_groups], ent_id [nb, pool_max] int64, ent_born
        [nb, pool_max], anc_used / anc_life [nb, anchor_max]); one synchronising read. The entries' anchors and the anchors'
        links are the resident ones: pool_get."""
        nb = self.batch - b0 if nb is None else int(nb)
        out = dict(feat_id=np.full((nb, self.F), -1, dtype=np.int64), feat_ref=np.full((nb, self.F), -1, dtype=np.int32),
                   group_refs=np.full((nb, self.layout.n_groups), -1, dtype=np.int32),
                   ent_id=np.full((nb, self.pool_max), -1, dtype=np.int64), ent_born=np.zeros((nb, self.pool_max), dtype=np.int32),
                   anc_used=np.zeros((nb, self.anchor_max), dtype=np.int32), anc_life=np.zeros((nb, self.anchor_max), dtype=np.int32))
        self._check(self.lib.xivo_hip_pool_life_get_book(self.h, int(b0), nb, *[_ptr(out[k]) for k in (
            "feat_id", "feat_ref", "group_refs", "ent_id", "ent_born", "anc_used", "anc_life")]))
        return out

    def pool_life_begin(self, F, off, ids, meas, strict=False, B=None):
        """before the update (asynchronous): the frame's tracks as off [B + 1] int32, ids [n] int64, meas [n, 3] (u, v, depth);
        begin kernel, pool step, admit kernel"""
        off = np.ascontiguousarray(off, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        meas = np.ascontiguousarray(meas, dtype=np.float64)
        B = off.size - 1 if B is None else int(B)
        if off.size != B + 1 or ids.size != int(off[-1]) or meas.size != 3 * ids.size:
            raise ValueError("off [B + 1], ids [off[B]], meas [off[B], 3]")
        self._check(self.lib.xivo_hip_pool_life_begin(self.h, B, int(F), _ptr(off), _ptr(ids), _ptr(meas), int(bool(strict))))
        self.F = int(F)

    def pool_life_begin_tracks(self, F, strict=False, B=None):
        """pool_life_begin on the tracks the last pcw_tracks(B) / pcw_tracks_resident(B) left on the device (asynchronous, no
        upload)"""
        self._check(self.lib.xivo_hip_pool_life_begin_tracks(self.h, self.batch if B is None else int(B), int(F), int(bool(strict))))
        self.F = int(F)

    def pool_life_end(self, B=None):
        """after the update and absorb_error (asynchronous)"""
        self._check(self.lib.xivo_hip_pool_life_end(self.h, self.batch if B is None else int(B)))

    def pool_life_stats(self, b0=0, nb=None):
        """-> [nb] pool_life_stats_dtype: the per-filter counters; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=pool_life_stats_dtype)
        self._check(self.lib.xivo_hip_pool_life_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    def pool_oos_config(self, oos_max, max_obs=6, min_obs=5, Roos=3.5 ** 2, chi2=CHI2_95):
        """MSCKF update from dropped pool entries (xivo_hip_pool_oos_config; after pool_config): oos_max features of at most
        max_obs observations per filter and frame, used from min_obs valid observations on; chi2[dof] gates a feature's
        2k - 3 rows (0: no gate; None: none at all). oos_max = 0 switches it off. -> the rows every frame appends"""
        o = np.zeros(1, dtype=pool_oos_opts_dtype)
        o["struct_size"] = pool_oos_opts_dtype.itemsize
        o["oos_max"], o["max_obs"], o["min_obs"], o["Roos"] = oos_max, max_obs, min_obs, Roos
        if chi2 is not None:
            o["chi2"][0, :len(chi2)] = chi2
        self._check(self.lib.xivo_hip_pool_oos_config(self.h, _ptr(o)))
        self.oos_max, self.oos_max_obs = int(oos_max), int(max_obs)
        return int(self.lib.xivo_hip_pool_oos_rows(self.h))

    def pool_oos_collect(self, cands, B=None):
        """the frame's OOS list from the dropped entries cands [n] pool_oos_cand_dtype, ordered by (b, entry), before the frame's
        pool step"""
        cands = np.ascontiguousarray(cands, dtype=pool_oos_cand_dtype)
        self._check(self.lib.xivo_hip_pool_oos_collect(self.h, self.batch if B is None else int(B), len(cands),
                                                       _ptr(cands) if len(cands) else None))

    def pool_oos_project(self, B=None):
        """after stack: the list's rows into the fixed block behind the in-state rows (asynchronous)"""
        self._check(self.lib.xivo_hip_pool_oos_project(self.h, self.batch if B is None else int(B)))

    def pool_oos_gate(self, B=None):
        """after pool_oos_project: the chi-square gate of every feature's rows (asynchronous)"""
        self._check(self.lib.xivo_hip_pool_oos_gate(self.h, self.batch if B is None else int(B)))

    def pool_oos_get(self, b0=0, nb=None):
        """-> (list [nb, oos_max] oos_dtype, gamma [nb, oos_max]); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        lst = np.zeros((nb, self.oos_max), dtype=oos_dtype); gamma = np.zeros((nb, self.oos_max))
        self._check(self.lib.xivo_hip_pool_oos_get(self.h, int(b0), nb, _ptr(lst), _ptr(gamma)))
        return lst, gamma

    def pool_oos_get_rings(self, b0=0, nb=None):
        """device pool life cycle: dict(anc_born [nb, anchor_max], hist_cnt [nb, pool_max], hist_anchor / hist_born
        [nb, pool_max, max_obs], hist_xp [nb, pool_max, max_obs, 2]); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        pm, am, mo = self.pool_max, self.anchor_max, self.oos_max_obs
        r = dict(anc_born=np.zeros((nb, am), dtype=np.int32), hist_cnt=np.zeros((nb, pm), dtype=np.int32),
                 hist_anchor=np.zeros((nb, pm, mo), dtype=np.int32), hist_born=np.zeros((nb, pm, mo), dtype=np.int32),
                 hist_xp=np.zeros((nb, pm, mo, 2)))
        self._check(self.lib.xivo_hip_pool_oos_get_rings(self.h, int(b0), nb, _ptr(r["anc_born"]), _ptr(r["hist_cnt"]),
                                                         _ptr(r["hist_anchor"]), _ptr(r["hist_born"]), _ptr(r["hist_xp"])))
        return r

    def pool_oos_stats(self, b0=0, nb=None):
        """-> [nb] pool_oos_stats_dtype: the per-filter counters; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=pool_oos_stats_dtype)
        self._check(self.lib.xivo_hip_pool_oos_get_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    # ---- loop closure: the resident landmark map --------------------------------
    def lcmap_config(self, map_max, lc_max=8, min_matches=5, Rlc=1.5 ** 2, chi2=CHI2_2DOF_95, max_depth_var=0.0):
        """the resident landmark map (xivo_hip_lcmap_config): map_max entries per filter, at most lc_max matches a frame (2 lc_max
        staged rows), a filter closes with at least min_matches matches kept by the chi2 gate (0: no gate); map_max = 0 releases"""
        o = np.zeros(1, dtype=lcmap_opts_dtype)
        o["struct_size"] = lcmap_opts_dtype.itemsize
        o["map_max"] = map_max; o["lc_max"] = lc_max; o["min_matches"] = min_matches
        o["Rlc"] = Rlc; o["chi2"] = chi2; o["max_depth_var"] = max_depth_var
        self._check(self.lib.xivo_hip_lcmap_config(self.h, _ptr(o)))
        self.lcmap_max, self.lc_max = int(map_max), int(lc_max)

    def lcmap_add(self, recs, B=None):
        """the in-state features that leave, recs [n] lcmap_add_dtype ordered by b, before the edit that removes them
        (asynchronous)"""
        recs = np.ascontiguousarray(recs, dtype=lcmap_add_dtype)
        self._check(self.lib.xivo_hip_lcmap_add(self.h, self.batch if B is None else int(B), len(recs), _ptr(recs) if len(recs) else None))

    def lcmap_close(self, queries, B=None, wait=True):
        """match queries [n] lcmap_query_dtype (ordered by b) against the maps, verify, stage the 2 lc_max loop-closure rows.
        wait: -> the number of closing filters, and nothing is staged when that is 0; else always stages, returns None"""
        queries = np.ascontiguousarray(queries, dtype=lcmap_query_dtype)
        k = C.c_int(0)
        self._check(self.lib.xivo_hip_lcmap_close(self.h, self.batch if B is None else int(B), len(queries),
                                                  _ptr(queries) if len(queries) else None, C.byref(k) if wait else None))
        return k.value if wait else None

    # ---- loop closure inside the device life cycle (xivo_hip_lcmap_life_config)
    def lcmap_life_config(self, on=True):
        """keys beside the track block and the in-state book, the device's own add records and queries (after life_config and
        lcmap_config); False releases them"""
        self._check(self.lib.xivo_hip_lcmap_life_config(self.h, 1 if on else 0))

    def lcmap_add_resident(self, B=None):
        """lcmap_add on the records the frame's begin call left on the device, then the removals it decided (asynchronous)"""
        self._check(self.lib.xivo_hip_lcmap_add_resident(self.h, self.batch if B is None else int(B)))

    def lcmap_close_resident(self, B=None, wait=True):
        """lcmap_close on queries the device makes from the book, the inlier mask and the frame's pixels. wait: -> the number of
        closing filters, nothing staged when it is 0; else asynchronous, always stages, -> None"""
        n = C.c_int(0)
        self._check(self.lib.xivo_hip_lcmap_close_resident(self.h, self.batch if B is None else int(B), C.byref(n) if wait else None))
        return n.value if wait else None

    def lcmap_life_get_keys(self, b0=0, nb=None):
        """-> feat_key [nb, F] int64 (-1: free slot); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.full((nb, self.F), -1, dtype=np.int64)
        self._check(self.lib.xivo_hip_lcmap_life_get_keys(self.h, int(b0), nb, _ptr(out), None))
        return out

    def lcmap_life_get_track_keys(self, tracks_max, b0=0, nb=None):
        """the keys the last pcw_tracks left -> [nb, tracks_max] int64 (-1 behind the filter's count); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.full((nb, int(tracks_max)), -1, dtype=np.int64)
        self._check(self.lib.xivo_hip_lcmap_life_get_track_keys(self.h, int(b0), nb, _ptr(out)))
        return out

    def lcmap_set(self, entries, count, b0=0):
        """load whole maps: entries [nb, map_max] lcmap_entry_dtype, count [nb]"""
        entries = np.ascontiguousarray(entries, dtype=lcmap_entry_dtype); count = np.ascontiguousarray(count, dtype=np.int32)
        assert entries.shape == (len(count), self.lcmap_max)
        self._check(self.lib.xivo_hip_lcmap_set(self.h, int(b0), len(count), _ptr(entries), _ptr(count)))

    def lcmap_get(self, b0=0, nb=None):
        """-> (entries [nb, map_max] lcmap_entry_dtype, count [nb]); one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        ent = np.zeros((nb, self.lcmap_max), dtype=lcmap_entry_dtype); cnt = np.zeros(nb, dtype=np.int32)
        self._check(self.lib.xivo_hip_lcmap_get(self.h, int(b0), nb, _ptr(ent), _ptr(cnt)))
        return ent, cnt

    def lcmap_matches(self, b0=0, nb=None):
        """-> [nb, lc_max] lcmap_match_dtype: the match lists of the last lcmap_close (entry = -1: empty position)"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros((nb, self.lc_max), dtype=lcmap_match_dtype)
        self._check(self.lib.xivo_hip_lcmap_get_matches(self.h, int(b0), nb, _ptr(out)))
        return out

    def lcmap_stats(self, b0=0, nb=None):
        """-> [nb] lcmap_stats_dtype: the per-filter counters; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=lcmap_stats_dtype)
        self._check(self.lib.xivo_hip_lcmap_get_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    def lcmap_cov_config(self, point_cov=False, revisit_gap=0):
        """the map's two options (xivo_hip_lcmap_cov_config, after lcmap_config): point_cov - every entry carries the covariance
        of its point, which weighs its matches; revisit_gap > 0 - an entry closes the loop once per visit, a visit ending after
        that many close calls without a match of it. Both off: releases, the map behaves as without this call"""
        o = np.zeros(1, dtype=lcmap_cov_opts_dtype)
        o["struct_size"] = lcmap_cov_opts_dtype.itemsize
        o["point_cov"] = int(point_cov); o["revisit_gap"] = int(revisit_gap)
        self._check(self.lib.xivo_hip_lcmap_cov_config(self.h, _ptr(o)))

    def lcmap_set_cov(self, cov, b0=0):
        """the points' covariances of whole maps: cov [nb, map_max, 6], packed (0,0),(0,1),(0,2),(1,1),(1,2),(2,2)"""
        cov = _f64(cov)
        assert cov.ndim == 3 and cov.shape[1:] == (self.lcmap_max, 6)
        self._check(self.lib.xivo_hip_lcmap_set_cov(self.h, int(b0), len(cov), _ptr(cov)))

    def lcmap_get_cov(self, b0=0, nb=None):
        """-> [nb, map_max, 6]; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros((nb, self.lcmap_max, 6))
        self._check(self.lib.xivo_hip_lcmap_get_cov(self.h, int(b0), nb, _ptr(out)))
        return out

    def lcmap_cov_stats(self, b0=0, nb=None):
        """-> [nb] lcmap_cov_stats_dtype: the counters of the two options; one synchronising read"""
        nb = self.batch - b0 if nb is None else int(nb)
        out = np.zeros(nb, dtype=lcmap_cov_stats_dtype)
        self._check(self.lib.xivo_hip_lcmap_get_cov_stats(self.h, int(b0), nb, _ptr(out)))
        return out

    def propagate_cov(self, Phi, Pmm, b0=0):
        Phi = np.asarray(Phi, dtype=np.float64)
        nb, nm, _ = Phi.shape
        Phic = _f64(np.transpose(Phi, (0, 2, 1)))
        Pmmc = _f64(np.transpose(np.asarray(Pmm, dtype=np.float64), (0, 2, 1)))
        self._check(self.lib.xivo_hip_propagate_cov(self.h, b0, nb, nm, _ptr(Phic), _ptr(Pmmc)))

    # ---- timing ---------------------------------------------------------------
    def timer_begin(self):
        self._check(self.lib.xivo_hip_timer_begin(self.h))

    def timer_end(self):
        ms = C.c_float()
        self._check(self.lib.xivo_hip_timer_end(self.h, C.byref(ms)))
        return ms.value

    def profile_reset(self):
        self._check(self.lib.xivo_hip_profile_reset(self.h))

    def profile_get(self):
        n = C.c_int()
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        launches = (C.c_int * 16)()
        flops = (C.c_double * 16)()
        self._check(self.lib.xivo_hip_profile_get(self.h, C.byref(n), names, ms, launches, flops))
        return {names[i].decode(): {"ms": ms[i], "launches": launches[i], "flops_per_launch": flops[i],
                                    "kernel": self.lib.xivo_hip_stage_kernel(self.h, i).decode(),
                                    "bytes_per_launch": self.lib.xivo_hip_stage_bytes(self.h, i)}
                for i in range(n.value)}

    def bench_mfma_peak(self):
        t = (C.c_double * 4)()
        self._check(self.lib.xivo_hip_bench_mfma_peak(self.h, t))
        return {"tflops_full_chip": t[0], "cycles_per_mfma_1wave_per_simd": t[1],
                "clock_ghz_lower_bound_full_chip": t[2], "tflops_1wave_per_simd": t[3]}
