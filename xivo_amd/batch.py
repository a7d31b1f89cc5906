"""ctypes view of xivo::hip::BatchEstimator (xivo_amd/host/batch_estimator.h): the C++ host side of the sequence loop -
Estimator::InertialMeas / VisualMeasPointCloud semantics for B filters resident on one GPU context."""
import ctypes as C
import os

import numpy as np

from . import lib as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_HOST = None

# struct xivo_batch_cfg (xivo_amd/host/batch_estimator.cpp)
batch_cfg_dtype = np.dtype([
    ("n_groups", "i4"), ("n_features", "i4"),
    ("cam_model", "i4"), ("cam_rows", "i4"), ("cam_cols", "i4"), ("_pad0", "i4"),
    ("fx", "f8"), ("fy", "f8"), ("cx", "f8"), ("cy", "f8"), ("d", "f8", 5),
    ("visual_meas_std", "f8"), ("MH_thresh", "f8"), ("MH_adjust_factor", "f8"),
    ("min_inliers", "i4"), ("min_new_features", "i4"), ("fix_group_block", "i4"), ("disable_MH_gating", "i4"),
    ("initial_std_x", "f8"), ("initial_std_y", "f8"), ("initial_std_z", "f8"), ("min_depth", "f8"), ("max_depth", "f8"),
    ("prop", L.prop_opts_dtype),
    ("use_1pt_RANSAC", "i4"), ("use_invdepth", "i4"), ("ransac_thresh", "f8"), ("ransac_Chi2", "f8")])


# struct xivo_batch_subfilter_cfg (xivo_amd/host/batch_estimator.cpp): the "subfilter" life cycle
batch_subfilter_cfg_dtype = np.dtype([("initial_z", "f8"), ("remove_outlier_counter", "f8"), ("strict_criteria_timesteps", "i4"),
                                      ("max_group_lifetime", "i4"), ("opts", L.subfilter_opts_dtype), ("pool_max", "i4"),
                                      ("anchor_max", "i4")])


# struct xivo_batch_depth_init_cfg (xivo_amd/host/batch_estimator.cpp): triangulation / AdaptInitialDepth of new tracks
batch_depth_init_cfg_dtype = np.dtype([("triangulate", "i4"), ("adaptive", "i4"), ("tri", L.tri_opts_dtype),
                                       ("std_badtri", "f8", 3), ("adapt", L.adapt_opts_dtype)])


def load_host_library():
    """libxivo_host.so (C++ adapter + batch estimator); raises if it has not been built - there is no fallback."""
    global _HOST
    if _HOST is None:
        L.load_library()      # the C ABI first (the host library links against it)
        path = os.path.join(_HERE, "libxivo_host.so")
        if not os.path.exists(path):
            raise FileNotFoundError(path + " not built: python -c 'import __graft_entry__ as g; g.build()'")
        _HOST = C.CDLL(path)
        _HOST.xivo_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        _HOST.xivo_batch_create_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        _HOST.xivo_batch_enable_oos.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_destroy.argtypes = [C.c_void_p]; _HOST.xivo_batch_destroy.restype = None
        _HOST.xivo_batch_imu.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_visual.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_poses.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_book.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_double)]
        _HOST.xivo_batch_stats.restype = None
        _HOST.xivo_batch_ctx.argtypes = [C.c_void_p]; _HOST.xivo_batch_ctx.restype = C.c_void_p
        _HOST.xivo_batch_enable_subfilter.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_pool_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        _HOST.xivo_batch_pool_stats.restype = None
        _HOST.xivo_batch_enable_depth_init.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_init_z.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_innov_log.argtypes = [C.c_void_p, C.c_int]
        _HOST.xivo_batch_enable_device_lifecycle.argtypes = [C.c_void_p, C.c_int]
        _HOST.xivo_batch_enable_device_pool_lifecycle.argtypes = [C.c_void_p, C.c_int]
        _HOST.xivo_batch_enable_device_world.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double]
        _HOST.xivo_batch_set_track_faults.argtypes = [C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_visual_world.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_ulonglong, C.c_void_p]
        _HOST.xivo_batch_enable_device_imu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _HOST.xivo_batch_frame_resident.argtypes = [C.c_void_p, C.c_ulonglong, C.c_int, C.c_double, C.c_ulonglong, C.c_void_p]
    return _HOST


class BatchEstimator:
    def __init__(self, cfg, B, poses0, P0, device=0):
        """cfg: xivo_amd.sequence.SequenceConfig; poses0: [B] pose_dtype; P0: [N, N] shared initial covariance"""
        from .sequence import check_lifecycle
        check_lifecycle(cfg)                     # (before anything is allocated)
        self.host = load_host_library()
        self.cfg, self.B, self.F = cfg, B, cfg.n_features
        c = np.zeros(1, dtype=batch_cfg_dtype)
        c["n_groups"], c["n_features"] = cfg.n_groups, cfg.n_features
        cam = cfg.cam
        c["cam_model"], c["cam_rows"], c["cam_cols"] = cam["model"], cam["rows"], cam["cols"]
        c["fx"], c["fy"], c["cx"], c["cy"] = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        c["d"][0, :len(cam.get("d", []))] = cam.get("d", [])
        c["visual_meas_std"], c["MH_thresh"], c["MH_adjust_factor"] = cfg.visual_meas_std, cfg.MH_thresh, cfg.MH_adjust_factor
        c["min_inliers"], c["min_new_features"], c["fix_group_block"] = cfg.min_inliers, cfg.min_new_features, int(cfg.fix_group_block)
        c["disable_MH_gating"] = 0 if getattr(cfg, "use_MH_gating", True) else 1
        c["use_1pt_RANSAC"] = 1 if getattr(cfg, "use_1pt_RANSAC", False) else 0
        c["use_invdepth"] = 1 if getattr(cfg, "use_invdepth", False) else 0
        c["ransac_thresh"], c["ransac_Chi2"] = getattr(cfg, "ransac_thresh", 5.0), getattr(cfg, "ransac_Chi2", 5.89)
        c["initial_std_x"], c["initial_std_y"], c["initial_std_z"] = cfg.initial_std_x, cfg.initial_std_y, cfg.initial_std_z
        c["min_depth"], c["max_depth"] = cfg.min_depth, cfg.max_depth
        c["prop"]["Qimu"] = cfg.Qimu_matrix().T.reshape(-1); c["prop"]["Qmodel"] = cfg.Qmodel_matrix().T.reshape(-1)
        c["prop"]["g"] = cfg.gravity; c["prop"]["method"] = 0 if cfg.integration_method == "RK4" else 1
        c["prop"]["stepsize"] = cfg.stepsize
        poses0 = np.ascontiguousarray(poses0, dtype=L.pose_dtype)
        P0 = np.asfortranarray(np.asarray(P0, dtype=np.float64))
        h = C.c_void_p()
        use_oos = bool(getattr(cfg, "use_oos", False))
        if use_oos and getattr(cfg, "pool_lifecycle", "host") != "device":
            raise ValueError("BatchEstimator: use_oos needs pool_lifecycle='device' (its host life cycle keeps no observation history)")
        if self.host.xivo_batch_create_rows(c.ctypes.data, B, device, poses0.ctypes.data, P0.ctypes.data,
                                            cfg.M_max() - 2 * cfg.n_features if use_oos else 0, C.byref(h)) != 0:
            raise RuntimeError("xivo_batch_create failed")
        self.h = h
        self.device_lifecycle = getattr(cfg, "lifecycle", "host") == "device"
        self.device_pool_lifecycle = getattr(cfg, "pool_lifecycle", "host") == "device"
        # device life cycles: no mask download unless asked for
        self.want_mask = not (self.device_lifecycle or self.device_pool_lifecycle)
        if self.device_lifecycle:
            if getattr(cfg, "feature_init", "immediate") != "immediate":
                raise ValueError("lifecycle='device' runs the 'immediate' life cycle only")
            self.enable_device_lifecycle(cfg.tracks_max)
        if getattr(cfg, "feature_init", "immediate") == "subfilter":
            sc = np.zeros(1, dtype=batch_subfilter_cfg_dtype)
            sc["initial_z"], sc["remove_outlier_counter"] = cfg.initial_z, cfg.remove_outlier_counter
            sc["strict_criteria_timesteps"], sc["max_group_lifetime"] = cfg.strict_criteria_timesteps, cfg.max_group_lifetime
            o = sc["opts"]
            o["Rtri"], o["MH_thresh"] = float(cfg.subfilter["visual_meas_std"]) ** 2, cfg.subfilter["MH_thresh"]
            o["ready_steps"], o["min_depth"], o["max_depth"] = cfg.subfilter["ready_steps"], cfg.min_depth, cfg.max_depth
            o["max_subfilter_outlier"] = cfg.max_subfilter_outlier
            sc["opts"] = o
            sc["pool_max"], sc["anchor_max"] = cfg.pool_max, cfg.anchor_max
            if self.host.xivo_batch_enable_subfilter(self.h, sc.ctypes.data) != 0:
                raise RuntimeError("xivo_batch_enable_subfilter failed")
            tri_on, adapt_on = bool(getattr(cfg, "triangulate_pre_subfilter", False)), bool(getattr(cfg, "adaptive_initial_depth", False))
            if tri_on or adapt_on:
                dc = np.zeros(1, dtype=batch_depth_init_cfg_dtype)
                dc["triangulate"], dc["adaptive"] = int(tri_on), int(adapt_on)
                t = cfg.triangulation
                dc["tri"] = L.tri_options(t["method"], t["zmin"], t["zmax"], t["max_theta_thresh"], t["beta_thresh"])
                dc["std_badtri"] = [cfg.initial_std_x_badtri, cfg.initial_std_y_badtri, cfg.initial_std_z_badtri]
                a = dc["adapt"]
                a["struct_size"] = L.adapt_opts_dtype.itemsize
                a["initial_z"], a["median_weight"] = cfg.initial_z, cfg.adaptive_depth["median_weight"]
                a["min_feature_lifetime"] = cfg.adaptive_depth["minimum_feature_lifetime"]
                a["min_z"], a["max_z"] = cfg.min_depth, cfg.max_depth
                dc["adapt"] = a
                if self.host.xivo_batch_enable_depth_init(self.h, dc.ctypes.data) != 0:
                    raise RuntimeError("xivo_batch_enable_depth_init failed")
            if self.device_pool_lifecycle:
                self.enable_device_pool_lifecycle(cfg.tracks_max)
                if use_oos:
                    self.enable_oos(cfg)

    def init_z(self):
        """AdaptInitialDepth's init_z [B] after the last frame (None while adaptive_initial_depth is off)"""
        z = np.zeros(self.B)
        return z if self.host.xivo_batch_init_z(self.h, z.ctypes.data) == 0 else None

    def enable_innovation_log(self, T_max):
        """BatchEstimator::EnableInnovationLog: every camera frame records the update's NIS on the estimator's context between
        the update and AbsorbError (read it through a borrowed Context: innov_read / innov_stats); 0 releases the log"""
        if self.host.xivo_batch_innov_log(self.h, int(T_max)) != 0:
            raise RuntimeError("xivo_batch_innov_log failed")

    def enable_device_lifecycle(self, tracks_max):
        """BatchEstimator::EnableDeviceLifecycle: the slot book moves to the device (xivo_hip_life_*); VisualMeasPointCloud then
        downloads nothing unless a mask is asked for, book() and stats() read the device"""
        if self.host.xivo_batch_enable_device_lifecycle(self.h, int(tracks_max)) != 0:
            raise RuntimeError("xivo_batch_enable_device_lifecycle failed")

    def enable_device_pool_lifecycle(self, tracks_max):
        """BatchEstimator::EnableDevicePoolLifecycle: after the sub-filter life cycle (and its depth initialisation) is set up,
        its decisions move to the device (xivo_hip_pool_life_*); VisualMeasPointCloud then downloads nothing unless a mask is
        asked for, book() and stats() read the device"""
        if self.host.xivo_batch_enable_device_pool_lifecycle(self.h, int(tracks_max)) != 0:
            raise RuntimeError("xivo_batch_enable_device_pool_lifecycle failed")

    def enable_oos(self, cfg):
        """BatchEstimator::EnableOosUpdates with cfg's oos_* options and the 0.95 chi-square table"""
        o = np.zeros(1, dtype=L.pool_oos_opts_dtype)
        o["struct_size"] = L.pool_oos_opts_dtype.itemsize
        o["oos_max"], o["max_obs"], o["min_obs"] = cfg.oos_max, cfg.oos_max_obs, cfg.oos_min_observations
        o["Roos"] = float(cfg.oos_meas_std) ** 2
        o["chi2"][0, :] = L.CHI2_95
        if self.host.xivo_batch_enable_oos(self.h, o.ctypes.data) != 0:
            raise RuntimeError("xivo_batch_enable_oos failed")

    def oos_stats(self):
        """[B] pool_oos_stats_dtype read from the estimator's context"""
        return L.Context.borrow(self.host.xivo_batch_ctx(self.h), self.cfg.N, self.cfg.M_max(), self.B).pool_oos_stats(0, self.B)

    def set_track_faults(self, faults=None):
        """BatchEstimator::SetTrackFaults: the producer's track faults (a dict of xivo_pcw_fault_opts' fields; None: off) that the
        next enable_device_world turns on with the worlds"""
        from .pcw import fault_opts
        if faults is None:
            self.host.xivo_batch_set_track_faults(self.h, None)
            return
        o = np.zeros(1, dtype=L.pcw_fault_opts_dtype)
        o["struct_size"] = L.pcw_fault_opts_dtype.itemsize
        for k, v in fault_opts(faults).items():
            o[k] = v
        self.host.xivo_batch_set_track_faults(self.h, o.ctypes.data)

    def fault_stats(self):
        """[B] pcw_fault_stats_dtype read from the estimator's context (track faults on)"""
        return L.Context.borrow(self.host.xivo_batch_ctx(self.h), self.cfg.N, self.cfg.M_max(), self.B).pcw_fault_stats(0, self.B)

    def enable_device_world(self, Xs, max_radius=None, faults=None):
        """BatchEstimator::EnableDeviceWorld: the worlds' points Xs [B, npts, 3] go to the device once (camera: cfg.cam, whatever
        its model; max_radius, default cfg.pcw_max_radius: a distorted camera's guard against the fold-back far off axis); the
        frames are then VisualMeasDeviceWorld. Needs one of the device life cycles and npts <= tracks_max. faults (default
        cfg.track_faults): the producer's track faults, scored after every update"""
        self.set_track_faults(getattr(self.cfg, "track_faults", None) if faults is None else faults)
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 3 or Xs.shape[0] != self.B or Xs.shape[2] != 3:
            raise ValueError("Xs [B, npts, 3]")
        cam = self.cfg.cam
        o = np.zeros(1, dtype=L.pcw_opts_dtype)
        o["fx"], o["fy"], o["cx"], o["cy"], o["imw"], o["imh"] = cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["cols"], cam["rows"]
        if max_radius is None:
            max_radius = getattr(self.cfg, "pcw_max_radius", float("inf"))
        if self.host.xivo_batch_enable_device_world(self.h, Xs.shape[1], o.ctypes.data, Xs.ctypes.data, float(max_radius)) != 0:
            raise RuntimeError("xivo_batch_enable_device_world failed")

    def VisualMeasDeviceWorld(self, t, gsc, noise_px_std, seed, mask=None):
        """the camera frame on tracks the device produces: gsc [B, 12] ground-truth camera poses (Rsc row-major, Tsc); mask:
        a [B, F] uint8 array to receive the inlier mask, or None (nothing is downloaded)"""
        gsc = np.ascontiguousarray(gsc, dtype=np.float64)
        if gsc.shape != (self.B, 12):
            raise ValueError("gsc [B, 12]")
        if self.host.xivo_batch_visual_world(self.h, float(t), gsc.ctypes.data, float(noise_px_std), int(seed),
                                             mask.ctypes.data if mask is not None else None) != 0:
            raise RuntimeError("VisualMeasDeviceWorld failed")

    def enable_device_imu(self, motion, rate, n_max, T_max, imu_dt, rot_amp=0.2, rot_w=None, noise_accel=1e-4,
                          noise_gyro=1e-5, grav_s=(0, 0, -9.8), seed=1):
        """BatchEstimator::EnableDeviceImu: the simulated IMU and the ground-truth poses come from the device
        (xivo_hip_trajsim_*); motion [B] ("lissajous" / "trefoil"), rate [B], the rest as BatchTrajectorySim; the camera is
        cfg.Wbc / cfg.Tbc. Needs the device world. The frames are then FrameResident."""
        from .pcw import so3_exp
        o = np.zeros(1, dtype=L.trajsim_opts_dtype)
        o["n_max"], o["T_max"], o["imu_dt"] = int(n_max), int(T_max), imu_dt
        # (the default profile is BatchTrajectorySim's, to the bit: 0.3 * 3.0 is not 0.9)
        o["rot_amp"], o["rot_w"] = rot_amp, np.array([0.3, 0.4, 0.1]) * 3.0 if rot_w is None else rot_w
        o["noise_accel"], o["noise_gyro"], o["grav_s"] = noise_accel, noise_gyro, grav_s
        o["Rbc"], o["Tbc"], o["seed"] = so3_exp(self.cfg.Wbc).reshape(-1), self.cfg.Tbc, int(seed) & (2 ** 64 - 1)
        m = np.ascontiguousarray([L.TRAJSIM_MOTIONS[x] if isinstance(x, str) else int(x) for x in motion], dtype=np.int32)
        r = np.ascontiguousarray(rate, dtype=np.float64)
        if m.shape != (self.B,) or r.shape != (self.B,):
            raise ValueError("motion [B], rate [B]")
        if self.host.xivo_batch_enable_device_imu(self.h, o.ctypes.data, m.ctypes.data, r.ctypes.data) != 0:
            raise RuntimeError("xivo_batch_enable_device_imu failed")

    def FrameResident(self, k0, n, noise_px_std, seed, mask=None):
        """a whole camera frame at sample k0 + n from device-resident data: the IMU records k0 + 1 .. k0 + n, the ground-truth
        poses, the tracks, the life cycle and the update are enqueued; nothing goes down, and nothing comes back unless mask
        (a [B, F] uint8 array) is given"""
        if self.host.xivo_batch_frame_resident(self.h, int(k0), int(n), float(noise_px_std), int(seed),
                                               mask.ctypes.data if mask is not None else None) != 0:
            raise RuntimeError("FrameResident failed")

    def sync(self):
        """wait for the estimator's stream (the device life cycle leaves a frame enqueued)"""
        lib = L.load_library()
        rc = lib.xivo_hip_sync(self.host.xivo_batch_ctx(self.h))
        if rc != 0:
            raise L.XivoHipError(rc, lib.xivo_hip_strerror(rc).decode())

    def close(self):
        if self.h:
            self.host.xivo_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def InertialMeas(self, t, gyro, accel):
        gyro = np.ascontiguousarray(gyro, dtype=np.float64).reshape(self.B, 3)
        accel = np.ascontiguousarray(accel, dtype=np.float64).reshape(self.B, 3)
        if self.host.xivo_batch_imu(self.h, float(t), gyro.ctypes.data, accel.ctypes.data) != 0:
            raise RuntimeError("InertialMeas failed")

    def VisualMeasPointCloud(self, t, tracks):
        """tracks: per filter (ids [n], xp_and_depths [n x 3]) -> inlier mask [B x F] (None with the device life cycle unless
        want_mask is set)"""
        off = np.zeros(self.B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(tr[0]) for tr in tracks])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(tr[0], dtype=np.int64) for tr in tracks])) if off[-1] else np.zeros(1, dtype=np.int64)
        meas = np.ascontiguousarray(np.concatenate([np.asarray(tr[1], dtype=np.float64).reshape(-1, 3) for tr in tracks])) if off[-1] else np.zeros((1, 3))
        mask = np.zeros((self.B, self.F), dtype=np.uint8) if self.want_mask else None
        if self.host.xivo_batch_visual(self.h, float(t), off.ctypes.data, ids.ctypes.data, meas.ctypes.data,
                                       mask.ctypes.data if mask is not None else None) != 0:
            raise RuntimeError("VisualMeasPointCloud failed")
        return mask.astype(bool) if mask is not None else None

    def poses(self):
        p = np.zeros(self.B, dtype=L.pose_dtype)
        if self.host.xivo_batch_poses(self.h, p.ctypes.data) != 0:
            raise RuntimeError("poses failed")
        return p

    def gsb(self):
        p = self.poses()
        return p["Rsb"].reshape(-1, 3, 3).transpose(0, 2, 1).copy(), p["Tsb"].copy()

    def book(self, b):
        fid = np.zeros(self.F, dtype=np.int64); fref = np.zeros(self.F, dtype=np.int32)
        gref = np.zeros(self.cfg.n_groups, dtype=np.int32)
        self.host.xivo_batch_book(self.h, b, fid.ctypes.data, fref.ctypes.data, gref.ctypes.data)
        return fid, fref, gref

    def stats(self):
        nu, nr, hs = C.c_long(), C.c_long(), C.c_double()
        self.host.xivo_batch_stats(self.h, C.byref(nu), C.byref(nr), C.byref(hs))
        na, nd = C.c_long(), C.c_long()
        self.host.xivo_batch_pool_stats(self.h, C.byref(na), C.byref(nd))
        return dict(updates=nu.value, mh_rejected=nr.value, host_seconds=hs.value, admitted=na.value, pool_dropped=nd.value)
