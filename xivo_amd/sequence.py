"""Image-free sequence driver over the resident C-ABI path (BASELINE configs 1 / 5 surrogate).

Runs B independent visual-inertial sequences at once on one GPU context: for every camera frame the IMU samples since the
last frame go down in one `xivo_hip_propagate` call, the frame's state edits of all filters in one `xivo_hip_edit_batch`
call and its pixels in one `xivo_hip_set_pixels` call, then `xivo_hip_filter_update` (Jacobians -> MH gating -> stacking -> Joseph update) and `xivo_hip_absorb_error`.
State, covariance, groups and features never leave the device; the host keeps only the slot book-keeping
(`gsel_` / `fsel_` of src/estimator.h:496-503) and decides who enters and leaves the state.

What is mirrored from the reference and what is simplified:
  * IMU bookkeeping (`ImuFeeder`): Estimator::Propagate's last/curr/slope handling, src/estimator.cpp:548-575.
  * message order: IMU before camera at equal timestamps (scripts/pyxivo_pcw.py:121-129).
  * per frame (Estimator::UpdateStep order, src/manager.cpp:30-110): tracker-dropped in-state features are removed
    (ProcessTracks, :152-169), the filter update runs on the tracked in-state features, MH-rejected features are
    removed (src/update.cpp:105-113), groups that lost all their features are discarded (DiscardAffectedGroups),
    then new features enter (SelectAndAddNewFeatures).
  * new features, two life cycles (`SequenceConfig.feature_init`):
    - "immediate" (default, SIMPLIFIED): a new feature enters the state in the frame it is first seen, with the
      simulator's depth (`InitWithSimDepths`, scripts/pyxivo_pcw.py:139-140, src/manager.cpp:588) and the configured
      initial std (src/estimator.cpp:349-353) - no depth sub-filter warm-up; its anchor is a group created from the
      current pose (AddGroupToState).
    - "subfilter": the reference's life cycle of a new track on the device-resident feature pool (xivo_hip_pool_*). A
      new track starts from `initial_z` (Feature::Initialize, src/feature.cpp:144-160) anchored to an anchor made from
      the frame's post-update pose (src/manager.cpp:121-126), runs Feature::SubfilterUpdate in every frame it stays out
      of the state (ProcessTracks, :171-250; dropped tracks and outliers leave the pool) and enters the state before the
      update once Criteria::Candidate - CandidateStrict from `strict_criteria_timesteps` frames on - passes, best first
      (ZeroGaugeXYAddFeatures, :408-450): its anchor's group enters a free group slot with the anchor's own pose
      (AddGroupToState, src/estimator.cpp:801-816) unless it is in the state already; without a free slot the candidate
      waits. An anchor whose group left the state keeps the group's last pose; unlinked anchors without live entries are
      freed after `max_group_lifetime` frames (EnforceMaxGroupLifetime, :282-304). New tracks that find no free pool
      entry or anchor are dropped and counted (`SequenceRunner.n_pool_dropped`).
      Two opt-in parts of the depth initialisation, both on the device: `triangulate_pre_subfilter` triangulates every
      pool entry at its second observation before its sub-filter step (Feature::Triangulate, src/feature.cpp:686-751;
      new tracks then start with the `initial_std_*_badtri` stds, :585-586), and `adaptive_initial_depth` runs
      AdaptInitialDepth (:255-278) after the new tracks are added, whose init_z the next frame's new tracks start from.
  * who runs the "immediate" life cycle (`SequenceConfig.lifecycle`): "host" (default) - this file decides filter by filter and
    sends op lists; "device" - the slot book lives on the device and the frame is xivo_hip_life_begin -> update ->
    xivo_hip_life_end (lifecycle_kernels.hip): the tracks of all filters go down in one array, nothing is downloaded during
    a frame, `books` / `n_updates` / `n_rejected` are read from the device on demand. Same decisions, same results.
  * where the tracks come from (`SequenceConfig.track_source`): "host" (default) - the numpy worlds of xivo_amd/pcw.py, uploaded
    by the frame call; "device" (needs lifecycle="device" or pool_lifecycle="device") - the worlds are resident and xivo_hip_pcw_tracks (pcw_kernels.hip)
    produces each frame's tracks from the ground-truth camera poses straight into the block the life cycle reads
    (`SequenceRunner.frame_world`): 96 bytes per filter go down instead of the tracks. Its pixel noise is the counter-based
    stream pcw.philox_normal restates.
  * what goes wrong with the tracks (`SequenceConfig.track_faults`, needs track_source="device"; None by default): a dict of
    xivo_pcw_fault_opts' fields - random track loss, gross outliers (one frame or sticky) and heavy-tailed noise drawn by the
    producer (xivo_hip_pcw_fault_config), a ground-truth flag byte beside every track, and after every update
    xivo_hip_pcw_fault_score adds the gate's decisions against the flags to `HipBackend.fault_stats()`. BatchPCW(noise="philox",
    faults=...) restates the producer bit for bit.
  * where the IMU records come from (`SequenceConfig.imu_source`): "host" (default) - the numpy simulator and `ImuFeeder`, uploaded
    by xivo_hip_propagate; "device" (needs track_source="device") - xivo_hip_trajsim_frame (trajsim_kernels.hip) produces the
    feeder's records and the ground-truth camera and body poses on the device, xivo_hip_propagate_resident consumes the records
    there (`SequenceRunner.frame_resident`): a frame takes no host data and no host wait. Its IMU noise is the counter-based
    stream pcw.trajsim_normals restates.
  * tracks that end outside the state (`SequenceConfig.use_oos`, needs feature_init="subfilter"; both pool life cycles): the
    step the reference only announces (use_OOS parses, then "MSCKF not implemented", src/estimator.cpp:113-122). Every pool
    entry keeps a ring of its last `oos_max_obs` observations (anchor, pixel), one per frame that created an anchor; an entry
    whose track ends while it is READY with at least `oos_min_observations` observations from anchors whose groups are in the
    state constrains those groups once, through the null-space rows (xivo_hip_pool_oos_*): at most `oos_max` per filter and
    frame, chi-square gated, in a fixed block of oos_max * (2 * oos_max_obs - 3) rows behind the in-state rows. The rules are
    pool_lifecycle_device.h's plife_hist_* / plife_oos_*; the device decides with the entry's status and depth. With
    pool_lifecycle="device" the rings are resident too and xivo_hip_pool_life_begin / _end select and record themselves.
  * loop closure (`SequenceConfig.loop_closure`; both host life cycles, and the device "immediate" life cycle with
    `lc_lifecycle="device"`): Estimator::CloseLoop on a device-resident landmark map
    (xivo_hip_lcmap_*). `frame(imu, tracks, keys)` takes one key per track - the stand-in for the mapper's descriptor match
    (src/mapper.cpp:158-222, :335-418): equal non-negative keys are one world point; the point-cloud worlds supply the point's
    index (`last_point_index`). The in-state features the tracker dropped go to the map before they are removed
    (DiscardFeatures -> Mapper::AddFeature; gate-rejected ones never do, DestroyFeatures); right after the frame's update and
    AbsorbError every tracked, gate-kept in-state feature queries the map with this frame's pixel, observed by the body pose,
    and the filters with at least `lc_min_matches` chi-square-kept matches take a second update on the loop-closure rows
    (CloseLoopInternal, src/update.cpp:171-212). The stored point is treated as exact, as the reference does.
    `lc_lifecycle`: "host" (default) - this file keeps the keys in its slot book, makes the add records and the queries filter
    by filter and downloads the inlier mask every frame; refused with the device life cycles. "device" (needs
    lifecycle="device") - the keys go down beside the tracks (`frame(imu, tracks, keys)`; with track_source="device" the
    producer writes each track's world-point index), the resident book keeps one per slot, and the frame is life_begin ->
    lcmap_add_resident -> update -> lcmap_close_resident -> [second update] -> life_end (xivo_hip_lcmap_life_config): no
    per-filter Python, and no download but the close call's count of closing filters - which `frame_resident` does not wait
    for either: there every filter takes the second update, the ones that do not close on neutral rows. Same decisions, same
    results. Refused with use_oos and the innovation log whoever runs it; with pool_lifecycle="device" the pool book carries
    no keys yet (not there: ent_key and its hand-over at admission), so loop closure stays refused there.
  * NOT IN EITHER: RefineDepth (`use_depth_opt`), gauge XY features and SwitchRefGroup, ownership transfer, feature merging and
    map eviction, the g2o pose graph.
The numerics of every step are the device path; this file holds no arithmetic of the filter itself.
"""
import numpy as np

from . import lib as L
from .pcw import so3_exp, so3_log


class ImuFeeder:
    """last_/curr_/slope_ bookkeeping of Estimator::Propagate (src/estimator.cpp:548-575) for B filters: turns raw
    (t, gyro, accel) messages and camera timestamps into the xivo_imu_in records of xivo_hip_propagate."""

    def __init__(self, B, t0, gyro0, accel0):
        self.t = np.full(B, float(t0))
        self.last_gyro = np.array(gyro0, dtype=float).reshape(B, 3).copy()
        self.last_accel = np.array(accel0, dtype=float).reshape(B, 3).copy()
        self.slope_gyro = np.zeros((B, 3)); self.slope_accel = np.zeros((B, 3))
        self.pending = []

    def imu(self, t, gyro, accel):
        """one IMU message per filter at time t (visual_meas == false branch, :558-567)"""
        dt = t - self.t
        if np.all(dt <= 0):
            # Estimator::Propagate returns early on dt == 0 and leaves last_ / slope_ untouched (src/estimator.cpp:550-555);
            # a message from the past (dt < 0) is skipped the same way, with a warning
            if np.any(dt < 0):
                import warnings
                warnings.warn("IMU message older than the filter time: skipped")
            return
        # per-filter clocks: a filter whose dt <= 0 returns early like the reference's estimator (its last_ / slope_ / time
        # stay untouched and its record is a zero-length step, which xivo_hip_propagate integrates as the identity)
        go = dt > 0
        rec = np.zeros(self.t.shape[0], dtype=L.imu_dtype)
        gyro = np.broadcast_to(np.asarray(gyro, dtype=float), self.last_gyro.shape)
        accel = np.broadcast_to(np.asarray(accel, dtype=float), self.last_accel.shape)
        safe = np.where(go, dt, 1.0)[:, None]
        self.slope_gyro = np.where(go[:, None], (gyro - self.last_gyro) / safe, self.slope_gyro)
        self.slope_accel = np.where(go[:, None], (accel - self.last_accel) / safe, self.slope_accel)
        rec["gyro"], rec["accel"] = self.last_gyro, self.last_accel
        rec["slope_gyro"], rec["slope_accel"], rec["dt"] = self.slope_gyro, self.slope_accel, np.where(go, dt, 0.0)
        self.last_gyro = np.where(go[:, None], gyro, self.last_gyro)
        self.last_accel = np.where(go[:, None], accel, self.last_accel)
        self.t = np.where(go, t, self.t)
        self.pending.append(rec)

    def visual(self, t):
        """camera message at time t (visual_meas == true branch, :568-575); dt == 0 propagates nothing (:550-555)"""
        dt = np.maximum(t - self.t, 0.0)      # (a filter already at or past t propagates nothing: zero-length record)
        if np.all(dt == 0):
            return
        rec = np.zeros(self.t.shape[0], dtype=L.imu_dtype)
        rec["gyro"], rec["accel"] = self.last_gyro, self.last_accel
        rec["slope_gyro"], rec["slope_accel"], rec["dt"] = self.slope_gyro, self.slope_accel, dt
        self.last_gyro = self.last_gyro + self.slope_gyro * dt[:, None]
        self.last_accel = self.last_accel + self.slope_accel * dt[:, None]
        self.t = np.maximum(self.t, t)
        self.pending.append(rec)

    def take(self):
        """-> [B x K] records since the last take (None if there are none)"""
        if not self.pending:
            return None
        out = np.stack(self.pending, axis=1)
        self.pending = []
        return out


class SequenceConfig:
    """The numbers of cfg/pcw.json the path reads (reference defaults), sizes of the TUM-VI build (src/core.h:95-105)."""

    def __init__(self, **kw):
        self.n_groups, self.n_features = 15, 30
        self.cam = dict(model=L_CAM_PINHOLE, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[])
        self.Wbc, self.Tbc = np.array([-1.57079633, 0.0, 0.0]), np.zeros(3)
        self.gravity = np.array([0.0, 0.0, -9.8])
        self.X0 = None                  # cfg "X" (initial nominal state) when the filter does not start from ground truth
        self.P0 = dict(Wsb=0.001, Tsb=0.001, Vsb=0.5, bg=1e-10, ba=1e-10, Wbc=1e-10, Tbc=1e-10, Wsg=1e-10)
        self.Qmodel = dict(Wsb=0.01, Wbc=0.0, Wsg=0.0)
        self.Qimu = dict(gyro=5e-3, accel=5e-2, gyro_bias=0.0, accel_bias=0.0)
        self.integration_method, self.stepsize = "PrinceDormand", 0.002
        self.visual_meas_std = 1.0
        self.MH_thresh, self.MH_adjust_factor, self.min_inliers = 5.991, 1.1, 5
        self.use_MH_gating = True       # cfg use_MH_gating (src/estimator.cpp:364)
        self.use_1pt_RANSAC = False     # cfg use_1pt_RANSAC (off in cfg/pcw.json, cfg/tumvi_cam0.json)
        self.ransac_thresh, self.ransac_Chi2 = 5.0, 5.89       # 1pt_RANSAC_thresh / 1pt_RANSAC_Chi2 defaults (estimator.cpp:132-134)
        self.initial_std_x = self.initial_std_y = 1.0      # pixels, divided by the focal length (estimator.cpp:351-352)
        self.initial_std_z = 0.10
        self.min_depth, self.max_depth = 0.05, 10.0
        # Feature::FillJacobianBlock as coded drops the group-rotation block (src/feature.cpp:675-676); a
        # sequence tracks markedly worse with it, so the driver asks for the evidently intended row.
        # False = bit-faithful to the reference's stacking.
        self.fix_group_block = True
        self.min_new_features = 3       # open a new group only when at least this many feature slots are free
        # the reference's USE_INVDEPTH build (src/CMakeLists.txt:10): features are (X/Z, Y/Z, 1/Z); initial_std_z is then an
        # inverse-depth standard deviation
        self.use_invdepth = False
        # life cycle of a new feature: "immediate" (enters the state at once with the simulator's depth) or "subfilter"
        # (the reference's: depth sub-filter in the device-resident feature pool first). Reference cfg keys / defaults:
        self.feature_init = "immediate"
        self.initial_z = 2.5                    # initial_z (cfg/tumvi_cam0.json:115)
        self.remove_outlier_counter = 10.0      # remove_outlier_counter (src/estimator.cpp:171)
        self.strict_criteria_timesteps = 5      # strict_criteria_timesteps (src/estimator.cpp:374)
        self.max_group_lifetime = 1             # max_group_lifetime (src/manager.cpp:285)
        self.max_subfilter_outlier = 0.01       # max_subfilter_outlier (src/options.cpp:10-33)
        self.subfilter = dict(visual_meas_std=3.5, MH_thresh=5.991, ready_steps=5)   # cfg "subfilter" (src/estimator.cpp:137-142)
        self.pool_max, self.anchor_max = 200, 64   # feature pool / anchor table per filter (device resident)
        # depth initialisation of new tracks in the "subfilter" life cycle (both off by default, as the reference's
        # triangulate_pre_subfilter is, src/estimator.cpp:157-158). Thresholds in radians (the cfg's degrees * pi / 180,
        # :163-164); the badtri stds replace initial_std_* for every new track while triangulation is on (manager.cpp:585-586)
        self.triangulate_pre_subfilter = False
        self.triangulation = dict(method="l1_angular", zmin=0.05, zmax=5.0, max_theta_thresh=0.1 * np.pi / 180,
                                  beta_thresh=0.25 * np.pi / 180)
        self.initial_std_x_badtri = self.initial_std_y_badtri = 1.0
        self.initial_std_z_badtri = 0.10
        # AdaptInitialDepth (src/manager.cpp:255-278): the init_z of new tracks follows the median feature depth
        self.adaptive_initial_depth = False
        self.adaptive_depth = dict(median_weight=0.99, minimum_feature_lifetime=5)   # cfg "adaptive_initial_depth"
        # who runs the per-frame life cycle of the "immediate" mode: "host" (SequenceRunner.frame decides filter by filter and
        # sends op lists) or "device" (xivo_hip_life_begin / _end: the slot book is device resident, nothing is downloaded
        # during a frame). tracks_max: the most tracks one filter may bring in a frame on the device path.
        self.lifecycle = "host"
        self.tracks_max = 1024
        # who runs the per-frame life cycle of the "subfilter" mode: "host" (SequenceRunner._frame_subfilter decides filter by
        # filter around pool_step and sends op lists, pixels, anchor slots and new-track records) or "device"
        # (xivo_hip_pool_life_begin / _end: both books are device resident, nothing is downloaded during a frame; tracks_max as
        # above). A name of its own: lifecycle="device" stays the "immediate" mode's switch.
        self.pool_lifecycle = "host"
        # where a frame's tracks come from: "host" (the simulator's arrays, uploaded) or "device" (xivo_hip_pcw_tracks on the
        # resident worlds of npts points each; needs lifecycle or pool_lifecycle = "device" and npts <= tracks_max)
        self.track_source = "host"
        self.npts = 1000
        # track faults of the device producer (xivo_hip_pcw_fault_config): None, or a dict of xivo_pcw_fault_opts' fields
        # (sticky, p_drop, p_outlier, p_tail, outlier_min_px, outlier_max_px, tail_scale; pcw.fault_opts fills the rest)
        self.track_faults = None
        # the simulated camera is `cam`, whatever its model; a distorted one sees no point whose normalised radius hypot(x, y)
        # exceeds this (the guard against a polynomial distortion's fold-back far off axis; inf: no guard)
        self.pcw_max_radius = float("inf")
        # where the simulated IMU records and the ground-truth poses come from: "host" (the numpy simulator and ImuFeeder, the
        # records uploaded by xivo_hip_propagate) or "device" (xivo_hip_trajsim_frame / xivo_hip_propagate_resident; needs
        # track_source = "device": a frame then takes no host data at all)
        self.imu_source = "host"
        # MSCKF update from pool entries whose track ends (cfg/pcw.json: use_OOS, OOS_update_min_observations, oos_meas_std);
        # oos_max features per filter and frame of at most oos_max_obs observations each
        self.use_oos = False
        self.oos_min_observations = 5
        self.oos_meas_std = 3.5
        self.oos_max, self.oos_max_obs = 4, 6
        # loop closure on the resident landmark map (xivo_hip_lcmap_*; off by default): lc_map_max entries per filter, at most
        # lc_max matches a frame, a filter closes with lc_min_matches kept ones (the mapper's default, src/mapper.cpp:411-415);
        # lc_meas_std: cfg loop_closure_meas_std (cfg/pcw.json); lc_chi2: the gate of one match, the 95 % point of chi-square
        # with 2 degrees of freedom, -2 ln 0.05 (0: no gate); lc_max_depth_var: a feature whose depth variance is above this
        # when it leaves is not stored (0: no test)
        self.loop_closure = False
        self.lc_map_max, self.lc_max, self.lc_min_matches = 1024, 16, 5
        self.lc_meas_std, self.lc_chi2, self.lc_max_depth_var = 4.0, 5.99, 0.0
        # lc_point_cov: a stored point carries the covariance it had when it left the state and its matches are weighed with
        # it; lc_revisit_gap > 0: a stored point closes the loop once per visit, a visit ending after that many frames without
        # a match of it (xivo_hip_lcmap_cov_config; both off: the stored point is exact and closes in every frame it is seen)
        self.lc_point_cov, self.lc_revisit_gap = False, 0
        # who feeds and queries the map: "host" (the runner's slot book keeps the keys; host life cycles only) or "device" (the
        # keys ride in the track block and the resident book, xivo_hip_lcmap_life_config; needs lifecycle = "device")
        self.lc_lifecycle = "host"
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option " + k)
            setattr(self, k, v)

    @property
    def N(self):
        return 23 + 6 * self.n_groups + 3 * self.n_features

    def oos_rows(self):
        """rows the OOS block adds to every frame's update (0: use_oos off)"""
        return self.oos_max * (2 * self.oos_max_obs - 3) if getattr(self, "use_oos", False) else 0

    def M_max(self):
        """rows a context of this configuration stages at most: the in-state rows, and with use_oos the fixed OOS block plus the
        16 rows the mixed stacking pads it with (and the round-up of the block itself)"""
        r = self.oos_rows()
        m = 2 * self.n_features + (((r + 16 + 15) // 16) * 16 if r else 0)
        # (loop_closure: its 2 lc_max rows replace the frame's rows for the second update)
        return max(m, 2 * self.lc_max) if getattr(self, "loop_closure", False) else m

    def P_init(self):
        """Estimator ctor, src/estimator.cpp:257-304: P_ = identity (kFullSize - unused group / feature slots keep a
        unit diagonal until a remove op zeroes them), the motion blocks scaled by cfg "P" - which are STANDARD
        DEVIATIONS: the whole matrix is then squared (`P_ *= P_`, :304). "Tbc" may be a scalar or a 3-vector (:266-271)."""
        P = np.eye(self.N)
        d = np.ones(23)
        p = self.P0
        d[0:3], d[3:6], d[6:9], d[9:12], d[12:15] = p["Wsb"], p["Tsb"], p["Vsb"], p["bg"], p["ba"]
        d[15:18], d[18:21], d[21:23] = p["Wbc"], np.asarray(p["Tbc"], dtype=float).reshape(-1)[:3], p["Wsg"]
        P[:23, :23] = np.diag(d * d)
        return P

    def focal_length(self):
        """Camera::GetFocalLength() = 0.5 sqrt(fx^2 + fy^2) (src/camera_manager.cpp:56) - what the initial feature
        std in pixels is divided by (src/estimator.cpp:351-352); NOT fx: 0.707 fx for a square pixel."""
        return 0.5 * float(np.hypot(self.cam["fx"], self.cam["fy"]))

    def Qmodel_matrix(self):
        """src/estimator.cpp:313-318: only the Wsb, Wbc and Wsg blocks are read from cfg "Qmodel", then squared"""
        q = self.Qmodel
        d = np.zeros(23)
        d[0:3], d[15:18], d[21:23] = q["Wsb"], q["Wbc"], q["Wsg"]
        return np.diag(d * d)

    def Qimu_matrix(self):
        """src/estimator.cpp:325-330 (std -> variance)"""
        q = self.Qimu
        d = np.concatenate([np.full(3, q["gyro"]), np.full(3, q["accel"]), np.full(3, q["gyro_bias"]),
                            np.full(3, q["accel_bias"])])
        return np.diag(d * d)


L_CAM_PINHOLE = 0
TRAJ_LOG_COLS = tuple(range(15))      # trajectory_log=True: the covariance block of Wsb, Tsb, Vsb, bg, ba


def _trajectory(ctx):
    recs, cov, ts = ctx.traj_read()
    n, B = recs.shape
    return dict(ts=ts, Rsb=recs["Rsb"].reshape(n, B, 3, 3).transpose(0, 1, 3, 2).copy(), Tsb=recs["Tsb"].copy(),
                Vsb=recs["Vsb"].copy(), bg=recs["bg"].copy(), ba=recs["ba"].copy(), status=recs["status"].copy(), cov=cov,
                cols=ctx.traj_cols.copy())


def _traj_cols(trajectory_log):
    return TRAJ_LOG_COLS if trajectory_log is True else tuple(int(c) for c in trajectory_log)


def _score(ctx, traj, gt_R, gt_T, out, rpe_lag=0):
    """NEES of the logged poses against the simulator's ground truth (xivo_hip_traj_nees), when the pose block is logged, and
    the accuracy score of every sequence (xivo_hip_traj_score): aligned / unaligned ATE, RPE at rpe_lag frames"""
    out["trajectory"] = traj
    if set(range(6)) <= set(int(c) for c in traj["cols"]):
        out["err6"], out["nees"], out["anees"], out["nees_used"] = ctx.traj_nees(gt_R, gt_T)
    sc = ctx.traj_score((gt_R, gt_T), align=True, rpe_lag=rpe_lag)
    out["ate_aligned"], out["ate_raw"], out["rpe_pos"], out["rpe_rot"] = sc["ate"], sc["ate_raw"], sc["rpe_pos"], sc["rpe_rot"]


def rpe_lag_frames(rpe_dt, vision_dt):
    """the RPE interval in camera frames (xivo_hip_traj_score takes frames; time association is the driver's): the nearest
    whole number of frames and at least one; rpe_dt <= 0 is lag 0, no RPE (rpe_pos = rpe_rot = -1)"""
    return max(1, int(round(rpe_dt / vision_dt))) if rpe_dt > 0 else 0


def truth_by_track(world_ids, world_Xs, fid):
    """world points of the tracks in fid [B, F] (-1: none) -> [B, F, 3], NaN where the track is not a currently visible point.
    world_ids [B, npts] (-1: not tracked) / world_Xs [B, npts, 3] as RandomPCW / BatchPCW keep them: a visible point holds its
    track id, ids start at 10000 and count up per world."""
    world_ids = np.asarray(world_ids); fid = np.asarray(fid)
    B = fid.shape[0]
    base = 10000
    top = int(max(world_ids.max(initial=base - 1), fid.max(initial=base - 1))) - base + 1
    lut = np.full((B, max(top, 1)), -1, dtype=np.int64)
    bi, pi = np.nonzero(world_ids >= base)
    lut[bi, world_ids[bi, pi] - base] = pi
    have = fid >= base
    pt = np.where(have, lut[np.arange(B)[:, None], np.where(have, fid - base, 0)], -1)
    out = np.full(fid.shape + (3,), np.nan)
    ok = pt >= 0
    out[ok] = np.asarray(world_Xs)[np.nonzero(ok)[0], pt[ok]]
    return out


class _MapLog:
    """Host side of the landmark log of a run: per frame the slot book (track id by list position) and the simulator's world
    point of each; at the end one read of the device log, ids and truth translated through (pos), and the landmark NEES."""

    def __init__(self, ctx, T_max, n_out, B):
        self.ctx, self.B = ctx, B
        ctx.map_config(T_max, n_out, world_cov=True)
        self.fid, self.gt = [], []

    def record(self, ts, fid, world_ids, world_Xs):
        """fid [B, F]: the slot book after the frame (position in the resident feature list -> track id, -1: free)"""
        self.ctx.map_record(ts, self.B)
        fid = np.asarray(fid, dtype=np.int64)
        self.fid.append(fid); self.gt.append(truth_by_track(world_ids, world_Xs, fid))

    def finish(self, out):
        pts, n_pts, ts = self.ctx.map_read()
        fid, gtp = np.array(self.fid), np.array(self.gt)                  # [n, B, F], [n, B, F, 3]
        pos = pts["pos"]
        t, b = np.arange(pos.shape[0])[:, None, None], np.arange(pos.shape[1])[None, :, None]
        ids = np.where(pos >= 0, fid[t, b, np.maximum(pos, 0)], -1)
        gt = np.where((pos >= 0)[..., None], gtp[t, b, np.maximum(pos, 0)], np.nan)
        err3, nees, anees, used = self.ctx.map_nees(gt)
        out["map"] = dict(ts=ts, pts=pts, n_pts=n_pts, ids=ids, gt=gt)
        out["landmark_err3"], out["landmark_nees"], out["landmark_anees"], out["landmarks_used"] = err3, nees, anees, used
        scored = used > 0
        # mean over the frames that scored any landmark of the frame's ensemble mean (3 for a consistent map); landmarks
        # scored per sequence and frame
        out["anees_landmark"] = float(np.mean(anees[scored])) if scored.any() else float("nan")
        out["landmarks_scored_mean"] = float(used.mean() / self.B) if used.size else 0.0


def _innovation(ctx, out):
    """the innovation log of a run in one read (xivo_hip_innov_read / _stats): `innovation` (recs [n, B] innov_rec_dtype, ts),
    nis_per_dof [n] - per frame the ensemble's sum of nis over its sum of counted rows, the figure to hold against 1 (NaN for
    a frame no record entered) -, nis_per_dof_seq [B] the same per sequence over its frames, nis_used [n] the records that
    entered and nis_records_left_out (flagged updates, non-finite sums)"""
    recs, ts = ctx.innov_read()
    st = ctx.innov_stats()
    with np.errstate(invalid="ignore", divide="ignore"):
        out["nis_per_dof"] = np.where(st["frame_dof"] > 0, st["frame_nis"] / st["frame_dof"], np.nan)
        out["nis_per_dof_seq"] = np.where(st["filt_dof"] > 0, st["filt_nis"] / st["filt_dof"], np.nan)
    out["innovation"] = dict(recs=recs, ts=ts, stats=st)
    out["nis_used"] = st["frame_used"]
    out["nis_records_left_out"] = int(recs.size - st["frame_used"].sum())


class HipBackend:
    """The product path: every numeric step is a C-ABI call on the resident state (fails loudly without the
    library / a GPU - there is no host fallback)."""

    def __init__(self, cfg, B, poses0, P0, device=0, flags=0):
        self.cfg, self.B, self.F = cfg, B, cfg.n_features
        if cfg.fix_group_block:
            flags |= L.FLAG_FIX_GROUP_BLOCK
        if getattr(cfg, "use_invdepth", False):
            flags |= L.FLAG_INVDEPTH
        check_lifecycle(cfg)
        self.ctx = L.Context(cfg.N, cfg.M_max(), B, device=device, flags=flags)
        self.ctx.set_layout(cfg.N, 23, cfg.n_groups, 23 + 6 * cfg.n_groups, cfg.n_features, cfg.cam)
        self.ctx.upload_P(P0)
        groups = np.zeros((B, cfg.n_groups), dtype=L.group_dtype)
        groups["Rsb"][:] = np.eye(3).reshape(-1)
        feats = np.zeros((B, self.F), dtype=L.feat_dtype)
        feats["sind"] = -1
        self.ctx.set_scene(poses0, groups, feats)
        self.Qimu, self.Qmodel = cfg.Qimu_matrix(), cfg.Qmodel_matrix()
        self.pool_on = False
        self.innov_on, self.frame_ts = False, 0   # innovation log: on / the stamp (ns) of the frame update() records under
        if cfg.feature_init == "subfilter":
            self.enable_pool()
        if cfg.lifecycle == "device":
            self.enable_device_lifecycle()
        if cfg.pool_lifecycle == "device":
            self.enable_device_pool_lifecycle()
        self.faults_on = False
        if cfg.track_source == "device":
            self.enable_device_world(faults=getattr(cfg, "track_faults", None))
        self.oos_on = False
        if getattr(cfg, "use_oos", False):
            self.enable_oos()
        self.lc_on = False
        if getattr(cfg, "loop_closure", False):
            self.enable_loop_closure()

    def enable_loop_closure(self):
        """allocate the resident landmark map, its match lists and counters (xivo_hip_lcmap_config)"""
        c = self.cfg
        if self.innov_on:
            raise ValueError("loop_closure with the innovation log is not supported: the log holds one update per frame")
        self.ctx.lcmap_config(c.lc_map_max, lc_max=c.lc_max, min_matches=c.lc_min_matches, Rlc=float(c.lc_meas_std) ** 2,
                              chi2=c.lc_chi2, max_depth_var=c.lc_max_depth_var)
        self.lc_cov_on = bool(getattr(c, "lc_point_cov", False)) or int(getattr(c, "lc_revisit_gap", 0)) > 0
        if self.lc_cov_on:
            self.ctx.lcmap_cov_config(point_cov=bool(c.lc_point_cov), revisit_gap=int(c.lc_revisit_gap))
        if getattr(c, "lc_lifecycle", "host") == "device":      # after the life cycle and the map: keys beside tracks and book
            self.ctx.lcmap_life_config(True)
        self.lc_on = True

    def lcmap_add(self, recs):
        """the in-state features about to leave -> map entries (asynchronous); before the edit that removes them"""
        self.ctx.lcmap_add(recs, B=self.B)

    def lcmap_close(self, queries):
        """match, verify and stage the loop-closure rows; if any filter closes, the second update and AbsorbError
        (CloseLoopInternal, src/update.cpp:207-208) -> the number of closing filters"""
        n = self.ctx.lcmap_close(queries, B=self.B, wait=True)
        if n > 0:
            self.ctx.update_joseph()
            self.ctx.absorb_error()
        return n

    def life_begin_keys(self, off, ids, meas, keys):
        self.ctx.life_begin_keys(self.F, off, ids, meas, keys, B=self.B)

    def lcmap_add_resident(self):
        """the add records the begin call left on the device -> map entries, then the removals it decided (asynchronous)"""
        self.ctx.lcmap_add_resident(self.B)

    def lcmap_close_resident(self, wait=True):
        """lcmap_close on the device's own queries. wait: as lcmap_close above -> the number of closing filters; else nothing is
        waited for: the rows are always staged and every filter takes the second update and AbsorbError, the ones that do not
        close on neutral rows (H = 0, inn = 0) -> None"""
        n = self.ctx.lcmap_close_resident(self.B, wait=wait)
        if n is None or n > 0:
            self.ctx.update_joseph()
            self.ctx.absorb_error()
        return n

    def lcmap_stats(self):
        """[B] lcmap_stats_dtype; one synchronising read"""
        return self.ctx.lcmap_stats(0, self.B)

    def lcmap_cov_stats(self):
        """[B] lcmap_cov_stats_dtype (zeros while lc_point_cov and lc_revisit_gap are both off); one synchronising read"""
        if not getattr(self, "lc_cov_on", False):
            return np.zeros(self.B, dtype=L.lcmap_cov_stats_dtype)
        return self.ctx.lcmap_cov_stats(0, self.B)

    def enable_oos(self):
        """allocate the OOS list, gate distances and counters of the MSCKF update from dropped pool entries
        (xivo_hip_pool_oos_config), after enable_pool"""
        c = self.cfg
        if not self.pool_on:
            raise ValueError("use_oos needs the feature pool (feature_init='subfilter')")
        self.ctx.pool_oos_config(c.oos_max, max_obs=c.oos_max_obs, min_obs=c.oos_min_observations, Roos=float(c.oos_meas_std) ** 2)
        self.oos_on = True

    def pool_oos_collect(self, cands):
        self.ctx.pool_oos_collect(cands, B=self.B)

    def oos_stats(self):
        """[B] pool_oos_stats_dtype: oos_used / oos_gated / oos_surplus / oos_short per filter; one synchronising read"""
        return self.ctx.pool_oos_stats(0, self.B)

    def enable_device_lifecycle(self):
        """allocate the device-resident slot book and track staging (xivo_hip_life_config). The new feature's variances are
        computed here as the host life cycle computes them (std * std, src/estimator.cpp:349-353)."""
        c = self.cfg
        self.ctx.life_config(c.tracks_max, min_depth=c.min_depth, max_depth=c.max_depth, min_new_features=c.min_new_features,
                             var_xyz=self.life_var_xyz(c))

    @staticmethod
    def life_var_xyz(c):
        """the variances a new feature of the device life cycle starts with under configuration c"""
        fl = c.focal_length()
        std = np.array([c.initial_std_x / fl, c.initial_std_y / fl, c.initial_std_z])
        return std * std

    @staticmethod
    def tuning_entry(c):
        """one row of the tuning table (lib.tune_dtype) that stands for configuration c: the numbers the calls of this class
        pass as scalars - visual_meas_std ** 2 and MH_thresh (update), Qimu_matrix() / Qmodel_matrix() (propagate), the
        variances of enable_device_lifecycle - computed by the same expressions, so that a tuned filter and a plain run of c
        start from the same bits"""
        return L.tune_entry(c.visual_meas_std ** 2, c.MH_thresh, HipBackend.life_var_xyz(c), c.Qimu_matrix(), c.Qmodel_matrix())

    def enable_tuning(self, table):
        """per-filter noise parameters (xivo_hip_tune_config / _set): table [B] lib.tune_dtype, row b filter b's. update(),
        propagate(), propagate_resident() and life_end() then read the table on the device; the scalars they pass from cfg are
        still validated and otherwise not read. None: back to cfg's values. Refused with use_1pt_RANSAC (one threshold pair for
        every filter)."""
        if table is None:
            self.ctx.tune_config(None)
            self.tune = None
            return
        table = np.ascontiguousarray(table, dtype=L.tune_dtype)
        if table.shape != (self.B,):
            raise ValueError("enable_tuning takes one row per filter: a lib.tune_dtype array of shape [%d]" % self.B)
        if self.cfg.use_1pt_RANSAC:
            raise ValueError("enable_tuning with use_1pt_RANSAC is not supported: OnePointRANSAC takes one parameter set")
        self.ctx.tune_config(table[0])
        self.ctx.tune_set(table)
        self.tune = table

    def new_track_std(self):
        """the stds a new pool entry starts with: a new track is never triangulated yet, so with triangulation on they are the
        badtri stds (src/manager.cpp:585-586); pixels are divided by the focal length (src/estimator.cpp:351-352)"""
        c = self.cfg
        fl = c.focal_length()
        if c.triangulate_pre_subfilter:
            return [c.initial_std_x_badtri / fl, c.initial_std_y_badtri / fl, c.initial_std_z_badtri]
        return [c.initial_std_x / fl, c.initial_std_y / fl, c.initial_std_z]

    def enable_device_pool_lifecycle(self):
        """allocate the device-resident books and track staging of the "subfilter" life cycle (xivo_hip_pool_life_config), after
        enable_pool and on an empty pool"""
        c = self.cfg
        if not self.pool_on:
            raise ValueError("enable_device_pool_lifecycle needs the feature pool (feature_init='subfilter')")
        self.ctx.pool_life_config(c.tracks_max, max_group_lifetime=c.max_group_lifetime, initial_z=c.initial_z,
                                  std_xyz=self.new_track_std(), adaptive_z=c.adaptive_initial_depth)

    def pool_life_begin(self, off, ids, meas, strict):
        self.ctx.pool_life_begin(self.F, off, ids, meas, strict, B=self.B)

    def pool_life_begin_tracks(self, strict):
        self.ctx.pool_life_begin_tracks(self.F, strict, B=self.B)

    def pool_life_end(self):
        self.ctx.pool_life_end(self.B)

    def pool_life_book(self):
        """the in-state and the pool book read from the device (Context.pool_life_get_book)"""
        return self.ctx.pool_life_get_book(0, self.B)

    def pool_life_stats(self):
        return self.ctx.pool_life_stats(0, self.B)

    def enable_device_world(self, faults=None):
        """allocate the resident worlds of the device track source (xivo_hip_pcw_config): cfg.npts points per filter, the
        camera of cfg.cam (a distorted model goes down whole: xivo_hip_pcw_camera). faults: a dict of xivo_pcw_fault_opts'
        fields - the producer's track faults on (xivo_hip_pcw_fault_config); None: off"""
        cam = self.cfg.cam
        self.ctx.pcw_config(self.cfg.npts, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["cols"], cam["rows"])
        if cam["model"] != L_CAM_PINHOLE:
            self.ctx.pcw_camera(cam, self.cfg.pcw_max_radius)
        self.set_track_faults(faults)

    def set_track_faults(self, faults=None):
        """the producer's track faults on (a dict of xivo_pcw_fault_opts' fields; the counters start at 0) or off (None)"""
        from .pcw import fault_opts
        self.ctx.pcw_fault_config(None if faults is None else fault_opts(faults))
        self.faults_on = faults is not None

    def stream_share(self, W):
        """filters w, w + W, ... draw the same pixel-noise and fault words (xivo_hip_pcw_stream_share; 0: each its own)"""
        self.ctx.pcw_stream_share(W)

    def fault_score(self):
        """the open frame's gate decisions against the tracks' fault flags, between the update and the end call (asynchronous)"""
        self.ctx.pcw_fault_score(self.B)

    def fault_stats(self):
        """[B] pcw_fault_stats_dtype: the producer's and the score's counters; one synchronising read"""
        return self.ctx.pcw_fault_stats(0, self.B)

    def fault_flags(self):
        """the flag byte of every track the last make_tracks left -> [B, tracks_max] uint8"""
        return self.ctx.pcw_fault_flags(self.cfg.tracks_max, 0, self.B)

    def set_world(self, Xs, ids=None, next_id=None):
        """the world points [B, npts, 3] of every filter (ids None: nothing is tracked yet, next_id None: 10000)"""
        self.ctx.pcw_set_world(Xs, ids, next_id)

    def make_tracks(self, gsc, noise_px_std, seed, frame):
        """the frame's tracks from the resident worlds (asynchronous): gsc [B, 12] ground-truth camera poses"""
        self.ctx.pcw_tracks(gsc, noise_px_std, seed, frame, B=self.B)

    def life_begin_tracks(self):
        self.ctx.life_begin_tracks(self.F, B=self.B)

    def enable_device_imu(self, motion, rate, n_max, T_max, imu_dt, **sim):
        """allocate the device trajectory producer (xivo_hip_trajsim_config / _set): motion [B], rate [B] and the keyword
        arguments of BatchTrajectorySim (rot_amp, noise_accel, noise_gyro, grav_s, seed) plus rot_w; the camera is cfg.Wbc /
        cfg.Tbc; at most n_max samples per frame, a ground-truth log of T_max frames"""
        self.ctx.trajsim_config(n_max, T_max, imu_dt=imu_dt, Rbc=so3_exp(self.cfg.Wbc), Tbc=self.cfg.Tbc, **sim)
        self.ctx.trajsim_set(motion, rate)
        self._prop_opts = L.prop_options(self.Qimu, self.Qmodel, self.cfg.gravity,
                                         "RK4" if self.cfg.integration_method == "RK4" else "PD", self.cfg.stepsize)

    def make_imu(self, k0, n):
        """the records k0 + 1 .. k0 + n and the poses at sample k0 + n of every filter (asynchronous)"""
        self.ctx.trajsim_frame(k0, n, B=self.B)

    def propagate_resident(self):
        self.ctx.propagate_resident(opts=self._prop_opts, B=self.B)

    def make_tracks_resident(self, noise_px_std, seed, frame):
        self.ctx.pcw_tracks_resident(noise_px_std, seed, frame, B=self.B)

    def ground_truth(self):
        """the device's ground-truth log -> gt [n, B, 12] (Rsb column-major, Tsb); one synchronising read"""
        return self.ctx.trajsim_get_gt(0, self.B)

    def world_ids(self):
        """(ids [B, npts], next_id [B]) of the resident worlds; one synchronising read"""
        return self.ctx.pcw_get_world(0, self.B)

    def life_begin(self, off, ids, meas):
        self.ctx.life_begin(self.F, off, ids, meas, B=self.B)

    def life_end(self):
        self.ctx.life_end(self.B)

    def life_book(self):
        """(feat_id [B, F], feat_ref [B, F], group_refs [B, n_groups]) read from the device"""
        return self.ctx.life_get_book(0, self.B)

    def life_stats(self):
        return self.ctx.life_stats(0, self.B)

    def enable_pool(self):
        """allocate the device-resident feature pool of the "subfilter" life cycle"""
        c = self.cfg
        sf = c.subfilter
        self.ctx.pool_config(c.pool_max, c.anchor_max, Rtri=float(sf["visual_meas_std"]) ** 2, MH_thresh=float(sf["MH_thresh"]),
                             ready_steps=int(sf["ready_steps"]), min_depth=c.min_depth, max_depth=c.max_depth,
                             max_subfilter_outlier=c.max_subfilter_outlier, remove_outlier_counter=c.remove_outlier_counter)
        if c.triangulate_pre_subfilter:
            t = c.triangulation
            self.ctx.pool_triangulation(t["method"], zmin=t["zmin"], zmax=t["zmax"], max_theta_thresh=t["max_theta_thresh"],
                                        beta_thresh=t["beta_thresh"])
        if c.adaptive_initial_depth:
            a = c.adaptive_depth
            self.ctx.pool_adapt_depth_config(c.initial_z, median_weight=a["median_weight"],
                                             min_feature_lifetime=a["minimum_feature_lifetime"], min_z=c.min_depth,
                                             max_z=c.max_depth)
        self.pool_on = True

    def pool_step(self, xp, strict):
        return self.ctx.pool_step(xp, strict)

    def pool_anchor(self, slot):
        self.ctx.pool_anchor(slot)

    def pool_add(self, recs):
        """Feature::Initialize of new tracks; z0 from the resident init_z under adaptive_initial_depth"""
        self.ctx.pool_add_ex(recs, L.POOL_ADD_ADAPTIVE_Z if self.cfg.adaptive_initial_depth else 0)

    def adapt_depth(self):
        """AdaptInitialDepth on every filter -> init_z [B]"""
        return self.ctx.pool_adapt_depth(self.B)

    def tri_counts(self):
        return self.ctx.pool_tri_counts()

    def propagate(self, imu):
        self.ctx.propagate(imu, self.Qimu, self.Qmodel, self.cfg.gravity,
                           method="RK4" if self.cfg.integration_method == "RK4" else "PD", stepsize=self.cfg.stepsize)

    def edit(self, ops):
        self.ctx.edit_batch(self.F, ops)

    def set_pixels(self, xp):
        self.ctx.set_pixels(xp)

    def update(self, download=True):
        """the frame's measurement update and AbsorbError -> the inlier mask [B, F]; download=False (device life cycle): the
        mask and the status stay on the device, nothing synchronises, None is returned"""
        c = self.cfg
        R = c.visual_meas_std ** 2
        if self.oos_on:
            # jacobians -> MH gate -> [RANSAC] -> stack -> the OOS block of the frame's list -> its chi-square gate -> update
            self.ctx.jacobians_instate()
            self.ctx.mh_gate(R, c.MH_thresh, c.MH_adjust_factor, c.min_inliers if c.use_MH_gating else 1 << 30, want=False)
            if c.use_1pt_RANSAC:
                self.ctx.one_point_ransac(R, c.ransac_thresh, c.ransac_Chi2, want=False)
            self.ctx.stack(R)
            self.ctx.pool_oos_project(self.B)
            self.ctx.pool_oos_gate(self.B)
            self.ctx.update_joseph()
        elif c.use_1pt_RANSAC:
            # Estimator::OutlierRejection with use_1pt_RANSAC (src/manager.cpp:629-650): MH gating, then OnePointRANSAC on
            # its inliers; the update runs on what RANSAC keeps. (No gauge group / previous-frame group list in this
            # simplified life cycle: temporary reference group every time, every slot absorbed.)
            self.ctx.jacobians_instate()
            self.ctx.mh_gate(R, c.MH_thresh, c.MH_adjust_factor, c.min_inliers if c.use_MH_gating else 1 << 30, want=False)
            self.ctx.one_point_ransac(R, c.ransac_thresh, c.ransac_Chi2, want=False)
            self.ctx.stack(R)
            self.ctx.update_joseph()
        else:
            self.ctx.filter_update(R, c.MH_thresh, c.MH_adjust_factor, c.min_inliers, bool(c.use_MH_gating))
        mask = None
        if download:
            mask, _ = self.ctx.get_gate(self.F)
            # a filter whose S was not positive definite keeps its prior P and absorbs nothing (device side); surfaced here
            self.last_status = self.ctx.get_status(check=False)
            self.n_not_spd = getattr(self, "n_not_spd", 0) + int((self.last_status != 0).sum())
        if self.innov_on:   # between the update and AbsorbError, which consumes dx
            self.ctx.innov_record(self.frame_ts, self.B)
        self.ctx.absorb_error()
        return mask

    def sync(self):
        self.ctx.sync()

    def poses(self):
        p, _, _ = self.ctx.get_scene()
        return p["Rsb"].reshape(-1, 3, 3).transpose(0, 2, 1).copy(), p["Tsb"].copy()

    def enable_trajectory_log(self, T_max, cols=None):
        """device log of T_max frames (xivo_hip_traj_config); cols: the error-state columns whose covariance block is kept
        (default: the motion state Wsb Tsb Vsb bg ba)"""
        self.ctx.traj_config(T_max, TRAJ_LOG_COLS if cols is None else cols)

    def record(self, ts):
        """append the current estimate of every filter to the log (one launch, no synchronisation); ts in ns"""
        return self.ctx.traj_record(ts, self.B)

    def trajectory(self):
        """the whole log in one read -> dict(ts [n] ns, Rsb [n, B, 3, 3], Tsb / Vsb / bg / ba [n, B, 3], status [n, B],
        cov [n, B, k, k], cols [k])"""
        return _trajectory(self.ctx)

    def enable_innovation_log(self, T_max):
        """device log of T_max frames of every update's NIS (xivo_hip_innov_config); update() then records between the update
        and absorb_error, stamped with frame_ts (ns, set by the driver before the frame); 0 releases it. Refused with use_oos:
        the log counts every staged row, so its dof would include the empty rows of the OOS block"""
        if self.oos_on and T_max > 0:
            raise ValueError("innovation_log with use_oos is not supported: the log's dof would count the empty rows of the OOS block")
        if getattr(self, "lc_on", False) and T_max > 0:
            raise ValueError("innovation_log with loop_closure is not supported: the log holds one update per frame")
        self.ctx.innov_config(T_max)
        self.innov_on = T_max > 0

    def enable_map_log(self, T_max, n_out=None, world_cov=True):
        """device log of T_max frames of the in-state features (xivo_hip_map_config): the best n_out per filter (default: all
        feature slots), with the covariance of the world position when world_cov"""
        self.ctx.map_config(T_max, self.F if n_out is None else n_out, world_cov=world_cov)

    def record_map(self, ts):
        """append every filter's in-state features to the landmark log (one launch, no synchronisation); ts in ns"""
        return self.ctx.map_record(ts, self.B)

    def landmarks(self):
        """the whole landmark log in one read -> (pts [n, B, n_out] map_pt_dtype, n_pts [n, B], ts [n] ns)"""
        return self.ctx.map_read()

    def covariance(self):
        return self.ctx.download_P()

    def scene(self):
        return self.ctx.get_scene()

    def close(self):
        self.ctx.close()


class _Book:
    """slot book-keeping of one filter: gsel_ / fsel_ and who sits where (src/estimator.h:496-503)"""

    def __init__(self, n_groups, n_features):
        self.group_refs = [-1] * n_groups        # -1: free slot, else number of in-state features anchored there
        self.group_gen = [0] * n_groups          # how many groups have lived in the slot (tells a re-used slot apart)
        self.feat_id = [-1] * n_features         # track id held by feature slot j (-1: free)
        self.feat_ref = [-1] * n_features
        self.feat_key = [-1] * n_features        # loop_closure: the key of the slot's track, from the frame it was first seen
        self.id2slot = {}

    def drop_feature(self, j):
        del self.id2slot[self.feat_id[j]]
        self.group_refs[self.feat_ref[j]] -= 1
        self.feat_id[j] = -1; self.feat_ref[j] = -1

    def n_instate(self):
        return len(self.id2slot)


class _PoolBook:
    """host side of one filter's feature pool: which track sits in which entry, anchors and the group slot each links to"""

    def __init__(self, pool_max, anchor_max):
        self.ent_id = [-1] * pool_max            # track id held by pool entry e (-1: free)
        self.ent_anchor = [-1] * pool_max
        self.ent_born = [0] * pool_max           # camera frame the entry was created in
        self.ent_key = [-1] * pool_max           # loop_closure: the track's key, handed on to the slot book at admission
        self.id2ent = {}
        self.anc_used = [False] * anchor_max
        self.anc_life = [0] * anchor_max         # Group::lifetime (frames since creation)
        self.anc_link = [-1] * anchor_max        # group slot the anchor's group occupies (-1: not in the state)
        # use_oos (pool_lifecycle_device.h, plife_hist_*): the anchors' creation frames and every entry's observation ring
        self.anc_born = [0] * anchor_max
        self.hist_cnt = [0] * pool_max           # observations appended since the entry was taken (slot = count % max_obs)
        self.hist = [[] for _ in range(pool_max)]   # ring slots: (anchor, its creation frame, pixel)

    def hist_append(self, e, max_obs, a, frame, xp):
        """plife_hist_append"""
        if len(self.hist[e]) < max_obs:
            self.hist[e] = self.hist[e] + [None] * (max_obs - len(self.hist[e]))
        self.hist[e][self.hist_cnt[e] % max_obs] = (a, frame, (float(xp[0]), float(xp[1])))
        self.hist_cnt[e] += 1

    def valid_obs(self, e, max_obs, n_groups):
        """plife_valid_obs: (group slot, pixel) of the observations that count, oldest first"""
        cnt, out = self.hist_cnt[e], []
        for q in range(min(cnt, max_obs)):
            a, born, xp = self.hist[e][q if cnt <= max_obs else (cnt + q) % max_obs]
            if 0 <= a < len(self.anc_used) and self.anc_used[a] and self.anc_born[a] == born and 0 <= self.anc_link[a] < n_groups:
                out.append((self.anc_link[a], xp))
        return out

    def free_entry(self, e):
        del self.id2ent[self.ent_id[e]]
        self.ent_id[e] = -1; self.ent_anchor[e] = -1

    def unlink_slot(self, g):
        for a, s in enumerate(self.anc_link):
            if s == g:
                self.anc_link[a] = -1


def check_lifecycle(cfg):
    if cfg.lifecycle not in ("host", "device"):
        raise ValueError("lifecycle must be 'host' or 'device'")
    if cfg.lifecycle == "device" and cfg.feature_init != "immediate":
        raise ValueError("lifecycle='device' runs the 'immediate' life cycle only (feature_init=%r)" % (cfg.feature_init,))
    plc = getattr(cfg, "pool_lifecycle", "host")
    if plc not in ("host", "device"):
        raise ValueError("pool_lifecycle must be 'host' or 'device'")
    if plc == "device":
        if cfg.feature_init != "subfilter":
            raise ValueError("pool_lifecycle='device' runs the 'subfilter' life cycle only (feature_init=%r)" % (cfg.feature_init,))
        if cfg.lifecycle == "device":
            raise ValueError("pool_lifecycle='device' and lifecycle='device' exclude each other")
        if not 0 < cfg.tracks_max <= L.LIFE_MAX_TRACKS:
            raise ValueError("pool_lifecycle='device' needs 0 < tracks_max <= %d" % L.LIFE_MAX_TRACKS)
    src = getattr(cfg, "track_source", "host")
    if src not in ("host", "device"):
        raise ValueError("track_source must be 'host' or 'device'")
    imu = getattr(cfg, "imu_source", "host")
    if imu not in ("host", "device"):
        raise ValueError("imu_source must be 'host' or 'device'")
    if imu == "device" and src != "device":
        raise ValueError("imu_source='device' needs track_source='device'")
    if getattr(cfg, "use_oos", False):
        if cfg.feature_init != "subfilter":
            raise ValueError("use_oos needs feature_init='subfilter' (feature_init=%r)" % (cfg.feature_init,))
        if not 2 <= cfg.oos_max_obs <= L.OOS_MAX_OBS or not 2 <= cfg.oos_min_observations <= cfg.oos_max_obs or not 0 < cfg.oos_max <= 64:
            raise ValueError("use_oos needs 2 <= oos_min_observations <= oos_max_obs <= %d and 0 < oos_max <= 64" % L.OOS_MAX_OBS)
    lcl = getattr(cfg, "lc_lifecycle", "host")
    if lcl not in ("host", "device"):
        raise ValueError("lc_lifecycle must be 'host' or 'device'")
    if lcl == "device":
        if not getattr(cfg, "loop_closure", False):
            raise ValueError("lc_lifecycle='device' needs loop_closure")
        if plc == "device":
            raise ValueError("lc_lifecycle='device' runs with lifecycle='device' only: the device pool life cycle's pool book carries no keys")
        if cfg.lifecycle != "device":
            raise ValueError("lc_lifecycle='device' needs a device life cycle (lifecycle='device')")
    if getattr(cfg, "loop_closure", False):
        if lcl == "host" and (cfg.lifecycle == "device" or plc == "device"):
            raise ValueError("loop_closure runs with the host life cycles only: the device life cycles' track block carries no keys")
        if getattr(cfg, "use_oos", False):
            raise ValueError("loop_closure with use_oos is not supported: both stage rows of their own behind the frame's update")
        if not 0 < cfg.lc_map_max <= L.LCMAP_MAX_ENTRIES or not 0 < cfg.lc_max <= L.LCMAP_MAX_MATCHES or cfg.lc_min_matches < 1:
            raise ValueError("loop_closure needs 0 < lc_map_max <= %d, 0 < lc_max <= %d and lc_min_matches >= 1"
                             % (L.LCMAP_MAX_ENTRIES, L.LCMAP_MAX_MATCHES))
        if not cfg.lc_meas_std > 0 or cfg.lc_chi2 < 0 or cfg.lc_max_depth_var < 0:
            raise ValueError("loop_closure needs lc_meas_std > 0, lc_chi2 >= 0 and lc_max_depth_var >= 0")
        if getattr(cfg, "lc_point_cov", False) not in (False, True) or int(getattr(cfg, "lc_revisit_gap", 0)) != getattr(cfg, "lc_revisit_gap", 0) \
                or getattr(cfg, "lc_revisit_gap", 0) < 0:
            raise ValueError("loop_closure needs lc_point_cov False or True and an integer lc_revisit_gap >= 0")
    elif getattr(cfg, "lc_point_cov", False) or getattr(cfg, "lc_revisit_gap", 0):
        raise ValueError("lc_point_cov and lc_revisit_gap need loop_closure")
    if src == "device":
        if cfg.lifecycle != "device" and plc != "device":
            raise ValueError("track_source='device' needs lifecycle='device' or pool_lifecycle='device'")
        if not 0 < cfg.npts <= cfg.tracks_max:
            raise ValueError("track_source='device' needs 0 < npts <= tracks_max (npts=%d, tracks_max=%d)" % (cfg.npts, cfg.tracks_max))


def _op(b, kind, i0=0, i1=0, i2=0, v=()):
    o = np.zeros((), dtype=L.edit_dtype)
    o["b"], o["kind"], o["i0"], o["i1"], o["i2"] = b, kind, i0, i1, i2
    if len(v):
        o["v"][:len(v)] = v
    return o


class SequenceRunner:
    """Drives B sequences frame by frame through a backend (`HipBackend`; tests also run the same decisions against
    an oracle backend). `frame()` consumes the pending IMU records and one camera frame per filter."""

    def __init__(self, backend, cfg, B):
        check_lifecycle(cfg)
        self.be, self.cfg, self.B = backend, cfg, B
        self.device_lifecycle = cfg.lifecycle == "device"
        self.device_pool_lifecycle = cfg.pool_lifecycle == "device"
        self.device_lc = getattr(cfg, "lc_lifecycle", "host") == "device"      # the map is fed and queried on the device
        self.lc_wait = True          # ... and frame / frame_world wait for the close call's count (frame_resident never does)
        self._books = [_Book(cfg.n_groups, cfg.n_features) for _ in range(B)]
        self._n_updates = 0
        self._n_rejected = 0
        self.want_mask = False       # device life cycle: download the inlier mask of every frame (frame() then returns it)
        self.pools = None            # [B] _PoolBook in the "subfilter" life cycle
        self.vision_counter = 0      # camera frames so far (Estimator::vision_counter_)
        self._n_pool_dropped = 0     # new tracks dropped because the pool or the anchor table was full
        self.admitted = []           # (frame, filter, track id, sub-filter steps taken) of every pool entry that entered the state
        self.init_z = None           # [B] AdaptInitialDepth's init_z after the last frame (adaptive_initial_depth)
        self.timers = None       # set to {} to accumulate wall seconds per phase (adds a device sync per phase)
        self.noise_px_std, self.noise_seed = 0.0, 0   # frame_world: the device producer's pixel noise and its generator's key

    # books / n_updates / n_rejected: the host life cycle keeps them here; the device life cycle reads them from the device
    # on demand (one synchronising read each - not something to ask for every frame of a timed run)
    @property
    def books(self):
        if not self.device_lifecycle and not self.device_pool_lifecycle:
            return self._books
        if self.device_pool_lifecycle:
            bk = self.be.pool_life_book()
            fid, fref, grefs = bk["feat_id"], bk["feat_ref"], bk["group_refs"]
        else:
            fid, fref, grefs = self.be.life_book()
        out = []
        for b in range(self.B):
            bk = _Book(self.cfg.n_groups, self.cfg.n_features)
            bk.feat_id[:fid.shape[1]] = fid[b].tolist()
            bk.feat_ref[:fid.shape[1]] = fref[b].tolist()
            bk.group_refs = grefs[b].tolist()
            bk.id2slot = {i: j for j, i in enumerate(bk.feat_id) if i >= 0}
            out.append(bk)
        return out

    def _device_count(self, name):
        """a counter of the device life cycle in use summed over the filters, None with the host life cycle"""
        if self.device_pool_lifecycle:
            return int(self.be.pool_life_stats()[name].sum())
        return int(self.be.life_stats()[name].sum()) if self.device_lifecycle else None

    @property
    def n_updates(self):
        n = self._device_count("updates")
        return self._n_updates if n is None else n

    @n_updates.setter
    def n_updates(self, v):
        self._n_updates = v

    @property
    def n_rejected(self):
        n = self._device_count("rejected")
        return self._n_rejected if n is None else n

    @n_rejected.setter
    def n_rejected(self, v):
        self._n_rejected = v

    @property
    def n_pool_dropped(self):
        return int(self.be.pool_life_stats()["pool_dropped"].sum()) if self.device_pool_lifecycle else self._n_pool_dropped

    @n_pool_dropped.setter
    def n_pool_dropped(self, v):
        self._n_pool_dropped = v

    def _pack_tracks(self, tracks):
        """the tracks of all filters in the off / ids / meas layout of xivo_batch_visual"""
        off = np.zeros(self.B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(t[0]) for t in tracks])
        if off[-1] > 0:
            ids = np.concatenate([np.asarray(t[0], dtype=np.int64).reshape(-1) for t in tracks])
            meas = np.concatenate([np.asarray(t[1], dtype=np.float64).reshape(-1, 3) for t in tracks])
        else:
            ids, meas = np.zeros(0, dtype=np.int64), np.zeros((0, 3))
        return off, ids, meas

    def _device_frame(self, produce, begin, end, lc_wait=None):
        """one camera frame with the life cycle on the device: produce -> begin -> update -> end. produce: the (timer name, call)
        steps that bring the IMU records and the tracks to where the begin call reads them; begin / end: the pair of the life
        cycle. No per-feature work here and nothing is downloaded (unless want_mask). lc_lifecycle="device": the map's add
        call behind begin, its close call (and the second update) behind the update; lc_wait: the close call waits for the
        number of closing filters, as the host life cycle's does (None: the runner's lc_wait)."""
        import time
        lc_wait = self.lc_wait if lc_wait is None else lc_wait
        t0 = time.perf_counter()
        for name, step in produce:
            step()
            t0 = self._tick(name, t0) or t0
        begin()
        if self.device_lc:
            self.be.lcmap_add_resident()
        t0 = self._tick("edit", t0) or t0
        mask = self.be.update(download=self.want_mask)
        if self.device_lc:
            self.n_lc_closed = getattr(self, "n_lc_closed", 0) + (self.be.lcmap_close_resident(wait=lc_wait) or 0)
        t0 = self._tick("update", t0) or t0
        end()
        self._tick("edit", t0)
        return mask

    def _pack_keys(self, tracks, keys):
        """the keys of all filters' tracks in the order _pack_tracks packs the ids"""
        if keys is None:
            raise ValueError("loop_closure needs keys: one per track of every filter, parallel to tracks[b][0]")
        for b in range(self.B):
            if len(keys[b]) != len(tracks[b][0]):
                raise ValueError("keys[%d] is not parallel to tracks[%d][0]" % (b, b))
        return np.concatenate([np.asarray(k, dtype=np.int64).reshape(-1) for k in keys]) if self.B else np.zeros(0, dtype=np.int64)

    def _frame_host_tracks(self, imu, tracks, begin, end, keys=None):
        """_device_frame on host data: the IMU records go to propagate, the tracks of all filters go down in the off / ids /
        meas layout of xivo_batch_visual as begin(off, ids, meas) - with lc_lifecycle="device" as begin(off, ids, meas, keys)"""
        be, packed = self.be, []
        if self.device_lc:      # (the keys are checked before anything is enqueued)
            kp = self._pack_keys(tracks, keys)
            pack = lambda: packed.extend(self._pack_tracks(tracks) + (kp,))
        else:
            pack = lambda: packed.extend(self._pack_tracks(tracks))
        return self._device_frame([("propagate", lambda: imu is not None and be.propagate(imu)), ("host_pre", pack)],
                                  lambda: begin(*packed), end)

    def _frame_subfilter_device(self, imu, tracks):
        """one camera frame of the "subfilter" life cycle with the decisions on the device: propagate -> pool_life_begin (begin
        kernel, pool step, admit kernel) -> update -> pool_life_end (end kernel, AdaptInitialDepth). `admitted` stays empty -
        the counters admitted / admit_steps of pool_life_stats stand for it."""
        be = self.be
        self.vision_counter += 1
        strict = self.vision_counter >= self.cfg.strict_criteria_timesteps
        return self._frame_host_tracks(imu, tracks, lambda *t: be.pool_life_begin(*t, strict), be.pool_life_end)

    def _frame_device(self, imu, tracks, keys=None):
        """one camera frame of the "immediate" life cycle on the device: propagate -> life_begin -> update -> life_end; with
        lc_lifecycle="device" life_begin_keys -> lcmap_add_resident -> update -> lcmap_close_resident -> life_end (keys: per
        filter one key per track)"""
        if self.device_lc:
            return self._frame_host_tracks(imu, tracks, self.be.life_begin_keys, self.be.life_end, keys)
        return self._frame_host_tracks(imu, tracks, self.be.life_begin, self.be.life_end)

    def _produced_tracks_pair(self):
        """the begin / end pair of a frame on the tracks the device produced, by life cycle: the pool life cycle counts the
        frame and passes CandidateStrict, as _frame_subfilter_device does"""
        be = self.be
        end = be.pool_life_end if self.device_pool_lifecycle else be.life_end
        if getattr(be, "faults_on", False):   # track faults: the score between the update and the end call (enqueued, no wait)
            end_call = end

            def end():
                be.fault_score()
                return end_call()
        if not self.device_pool_lifecycle:
            return be.life_begin_tracks, end
        self.vision_counter += 1
        strict = self.vision_counter >= self.cfg.strict_criteria_timesteps
        return lambda: be.pool_life_begin_tracks(strict), end

    def frame_world(self, imu, gsc, frame, keys=None):
        """one camera frame whose tracks the device produces (track_source="device"): gsc [B, 12] the ground-truth camera pose
        of every filter (Rsc row-major, Tsc), frame the frame's number (the noise generator's counter). propagate -> pcw_tracks
        -> life_begin_tracks -> update -> life_end (pool_life_begin_tracks / pool_life_end with pool_lifecycle="device");
        nothing but the poses goes down and nothing comes back (unless want_mask). keys: ignored - with lc_lifecycle="device" the
        producer writes every track's world-point index as its key, and the close call's count of closing filters comes back."""
        if self.cfg.track_source != "device":
            raise ValueError("frame_world needs track_source='device'")
        be = self.be
        return self._device_frame([("propagate", lambda: imu is not None and be.propagate(imu)),
                                   ("tracks", lambda: be.make_tracks(gsc, self.noise_px_std, self.noise_seed, frame))],
                                  *self._produced_tracks_pair())

    def frame_resident(self, k0, n, frame, keys=None):
        """one camera frame at IMU sample k0 + n that takes no host data (imu_source="device"): the device produces the records
        k0 + 1 .. k0 + n and the ground-truth poses (make_imu), propagates over them, produces the tracks from the poses and
        runs the life cycle and the update; n = 0: the frame at t = 0, nothing to propagate. frame: the pixel noise
        generator's counter. Nothing is downloaded (unless want_mask). keys: ignored, as in frame_world; with
        lc_lifecycle="device" the close call does not wait: every filter takes the second update, neutral where it does not close."""
        if getattr(self.cfg, "imu_source", "host") != "device":
            raise ValueError("frame_resident needs imu_source='device'")
        be = self.be
        return self._device_frame([("imu", lambda: be.make_imu(k0, n)),
                                   ("propagate", lambda: n > 0 and be.propagate_resident()),
                                   ("tracks", lambda: be.make_tracks_resident(self.noise_px_std, self.noise_seed, frame))],
                                  *self._produced_tracks_pair(), lc_wait=False)

    def _tick(self, name, t0):
        if self.timers is None:
            return 0.0
        import time
        if name not in ("host_pre", "host_post") and hasattr(self.be, "sync"):
            self.be.sync()
        t1 = time.perf_counter()
        self.timers[name] = self.timers.get(name, 0.0) + (t1 - t0)
        return t1

    def _discard_empty_groups(self, b, ops):
        bk = self.books[b]
        for g, r in enumerate(bk.group_refs):
            if r == 0:
                ops.append(_op(b, L.EDIT_REMOVE_GROUP, g))
                bk.group_refs[g] = -1
                if self.pools is not None:
                    self.pools[b].unlink_slot(g)      # the device freezes the anchor at the group's last pose

    def _lc_keys(self, tracks, keys):
        """loop_closure: per filter {track id: key} of the frame (None when it is off)"""
        if not getattr(self.cfg, "loop_closure", False):
            return None
        if keys is None:
            raise ValueError("loop_closure needs keys: one per track of every filter, parallel to tracks[b][0]")
        out = []
        for b in range(self.B):
            if len(keys[b]) != len(tracks[b][0]):
                raise ValueError("keys[%d] is not parallel to tracks[%d][0]" % (b, b))
            out.append({int(i): int(k) for i, k in zip(tracks[b][0], keys[b])})
        return out

    def _lc_add(self, leaving):
        """loop_closure: the in-state features (b, slot, key) the tracker dropped, in filter order, go to the map before their edit"""
        if leaving:
            recs = np.zeros(len(leaving), dtype=L.lcmap_add_dtype)
            for i, (b, j, key) in enumerate(leaving):
                recs[i]["b"], recs[i]["feat"], recs[i]["key"] = b, j, key
            self.be.lcmap_add(recs)

    def _lc_close(self, xp, mask):
        """loop_closure: one query per in-state feature that was tracked this frame and kept by the gate, observed by the body
        pose at this frame's pixel; then the second update of the filters that close"""
        q = []
        for b in range(self.B):
            bk = self.books[b]
            for j in range(self.cfg.n_features):
                if bk.feat_id[j] >= 0 and mask[b, j] and not np.isnan(xp[b, j, 0]):
                    q.append((b, -1, bk.feat_key[j], (xp[b, j, 0], xp[b, j, 1])))
        self.n_lc_closed = getattr(self, "n_lc_closed", 0) + self.be.lcmap_close(np.array(q, dtype=L.lcmap_query_dtype))

    def frame(self, imu, tracks, keys=None):
        """imu: [B x K] xivo_imu_in records or None; tracks: per filter (ids [n], xp_and_depths [n x 3]); keys (loop_closure):
        per filter the key of every track, parallel to tracks[b][0] (lc_lifecycle="device": they go down with the tracks)."""
        lck = None if self.device_lc else self._lc_keys(tracks, keys)
        if self.cfg.feature_init == "subfilter":
            if self.device_pool_lifecycle:
                return self._frame_subfilter_device(imu, tracks)
            return self._frame_subfilter(imu, tracks, lck)
        if self.cfg.feature_init != "immediate":
            raise ValueError("feature_init must be 'immediate' or 'subfilter'")
        if self.device_lifecycle:
            return self._frame_device(imu, tracks, keys)
        import time
        cfg, be = self.cfg, self.be
        t0 = time.perf_counter()
        if imu is not None:
            be.propagate(imu)
        t0 = self._tick("propagate", t0) or t0
        # --- before the update: tracker-dropped features leave, tracked ones get their new pixel
        ops, leaving = [], []
        xp = np.full((self.B, cfg.n_features, 2), np.nan)     # the frame's pixels of the tracked in-state features
        for b in range(self.B):
            bk = self.books[b]
            ids, meas = tracks[b]
            pos = {int(i): k for k, i in enumerate(ids)}
            for j in range(cfg.n_features):
                fid = bk.feat_id[j]
                if fid < 0:
                    continue
                if fid in pos:
                    xp[b, j] = meas[pos[fid], :2]
                else:
                    ops.append(_op(b, L.EDIT_REMOVE_FEATURE, j))
                    leaving.append((b, j, bk.feat_key[j]))
                    bk.drop_feature(j)
            self._discard_empty_groups(b, ops)
        ops = np.array(ops, dtype=L.edit_dtype)
        t0 = self._tick("host_pre", t0) or t0
        if lck is not None:
            self._lc_add(leaving)
        be.edit(ops)
        be.set_pixels(xp)
        t0 = self._tick("edit", t0) or t0
        # --- measurement update on the tracked in-state features (every filter, ragged)
        mask = be.update()
        if lck is not None:
            self._lc_close(xp, mask)
        t0 = self._tick("update", t0) or t0
        self.n_updates += sum(1 for bk in self.books if bk.n_instate() > 0)
        # --- after the update: MH-rejected features leave, then new features enter with a new group
        ops = []
        fx, fy, cx, cy = cfg.cam["fx"], cfg.cam["fy"], cfg.cam["cx"], cfg.cam["cy"]
        fl = cfg.focal_length()
        std = np.array([cfg.initial_std_x / fl, cfg.initial_std_y / fl, cfg.initial_std_z])
        P3 = np.diag(std * std).T.reshape(-1)
        for b in range(self.B):
            bk = self.books[b]
            for j in range(cfg.n_features):
                if bk.feat_id[j] >= 0 and not mask[b, j]:
                    ops.append(_op(b, L.EDIT_REMOVE_FEATURE, j))
                    bk.drop_feature(j)
                    self.n_rejected += 1
            self._discard_empty_groups(b, ops)
            free = [j for j in range(cfg.n_features) if bk.feat_id[j] < 0]
            gfree = [g for g, r in enumerate(bk.group_refs) if r < 0]
            if not gfree or (len(free) < cfg.min_new_features and bk.n_instate() > 0):
                continue
            ids, meas = tracks[b]
            cand = [k for k in np.argsort(ids, kind="stable")
                    if int(ids[k]) not in bk.id2slot and cfg.min_depth < meas[k, 2] < cfg.max_depth]
            if not cand:
                continue
            g = gfree[0]
            ops.append(_op(b, L.EDIT_ADD_GROUP, g))
            bk.group_refs[g] = 0; bk.group_gen[g] += 1
            for j, k in zip(free, cand):
                x = [(meas[k, 0] - cx) / fx, (meas[k, 1] - cy) / fy, (1.0 / meas[k, 2] if getattr(cfg, "use_invdepth", False) else np.log(meas[k, 2]))]   # Feature::Initialize, feature.cpp:144-150
                ops.append(_op(b, L.EDIT_ADD_FEATURE, j, j, g, v=np.concatenate([x, meas[k, :2], P3])))
                bk.feat_id[j] = int(ids[k]); bk.feat_ref[j] = g; bk.id2slot[int(ids[k])] = j
                bk.feat_key[j] = lck[b][int(ids[k])] if lck is not None else -1
                bk.group_refs[g] += 1
        ops = np.array(ops, dtype=L.edit_dtype)
        t0 = self._tick("host_post", t0) or t0
        be.edit(ops)
        self._tick("edit", t0)
        return mask


    def _frame_subfilter(self, imu, tracks, lck=None):
        """one camera frame in the order of Estimator::UpdateStep (src/manager.cpp:18-130) with the feature pool"""
        cfg, be, B = self.cfg, self.be, self.B
        use_oos = bool(getattr(cfg, "use_oos", False))
        if self.pools is None:
            self.pools = [_PoolBook(cfg.pool_max, cfg.anchor_max) for _ in range(B)]
        self.vision_counter += 1
        if imu is not None:
            be.propagate(imu)
        for pb in self.pools:                                   # Group::IncrementLifetime (:36-41)
            pb.anc_life = [life + 1 if u else 0 for life, u in zip(pb.anc_life, pb.anc_used)]
        pos = [{int(i): k for k, i in enumerate(tracks[b][0])} for b in range(B)]
        # --- ProcessTracks (:171-250): in-state features the tracker dropped leave the state, pool entries it dropped
        # leave the pool, every other pool entry takes its sub-filter step
        ops, leaving = [], []
        xpp = np.full((B, cfg.pool_max, 2), np.nan)
        for b in range(B):
            bk, pb, meas = self.books[b], self.pools[b], tracks[b][1]
            for j in range(cfg.n_features):
                if bk.feat_id[j] >= 0 and bk.feat_id[j] not in pos[b]:
                    ops.append(_op(b, L.EDIT_REMOVE_FEATURE, j))
                    leaving.append((b, j, bk.feat_key[j]))
                    bk.drop_feature(j)
            self._discard_empty_groups(b, ops)
        if lck is not None:   # (the ops above go down with the admissions below: the map sees the features before either)
            self._lc_add(leaving)
        # --- OOS selection (use_oos): every live entry without a track, ascending, with its valid observations - after the groups
        # above left, before anything is freed. The device decides with the entry's status and depth (plife_oos_decide)
        if use_oos:
            cands = []
            for b in range(B):
                pb = self.pools[b]
                for e, fid in enumerate(pb.ent_id):
                    if fid >= 0 and fid not in pos[b]:
                        obs = pb.valid_obs(e, cfg.oos_max_obs, cfg.n_groups)
                        r = np.zeros((), dtype=L.pool_oos_cand_dtype)
                        r["b"], r["entry"], r["n_obs"] = b, e, len(obs)
                        for q, (g, px) in enumerate(obs):
                            r["group_sind"][q] = g; r["xp"][q] = px
                        cands.append(r)
            be.pool_oos_collect(np.array(cands, dtype=L.pool_oos_cand_dtype))
        for b in range(B):
            pb, meas = self.pools[b], tracks[b][1]
            for e, fid in enumerate(pb.ent_id):
                if fid < 0:
                    continue
                if fid in pos[b]:
                    xpp[b, e] = meas[pos[b][fid], :2]
                else:
                    pb.free_entry(e)
        order, n_cand, live = be.pool_step(xpp, self.vision_counter >= cfg.strict_criteria_timesteps)
        # --- SelectAndAddNewFeatures / ZeroGaugeXYAddFeatures (:332-450): candidates in device order into free slots
        for b in range(B):
            bk, pb = self.books[b], self.pools[b]
            for e, fid in enumerate(pb.ent_id):
                if fid >= 0 and not live[b, e]:
                    pb.free_entry(e)                            # sub-filter outlier (:236-240)
            free = [j for j in range(cfg.n_features) if bk.feat_id[j] < 0]
            gfree = [g for g, r in enumerate(bk.group_refs) if r < 0]
            for e in order[b, :n_cand[b]]:
                if not free:
                    break
                a = pb.ent_anchor[e]
                if pb.anc_link[a] < 0:
                    if not gfree:
                        continue                                # its group would need a free slot (:437-441)
                    g = gfree.pop(0)
                    ops.append(_op(b, L.EDIT_ADD_GROUP_ANCHOR, g, a))
                    pb.anc_link[a] = g
                    bk.group_refs[g] = 0; bk.group_gen[g] += 1
                g, j, fid = pb.anc_link[a], free.pop(0), pb.ent_id[e]
                ops.append(_op(b, L.EDIT_ADMIT_POOL, j, j, int(e)))
                self.admitted.append((self.vision_counter, b, fid, self.vision_counter - pb.ent_born[e]))
                bk.feat_id[j] = fid; bk.feat_ref[j] = g; bk.id2slot[fid] = j
                bk.feat_key[j] = pb.ent_key[e]
                bk.group_refs[g] += 1
                pb.free_entry(int(e))
        be.edit(np.array(ops, dtype=L.edit_dtype))
        xp = np.full((B, cfg.n_features, 2), np.nan)
        for b in range(B):
            bk, meas = self.books[b], tracks[b][1]
            for j in range(cfg.n_features):
                if bk.feat_id[j] >= 0:
                    xp[b, j] = meas[pos[b][bk.feat_id[j]], :2]
        be.set_pixels(xp)
        # --- OutlierRejection + FilterUpdate, then DiscardAffectedGroups
        mask = be.update()
        if lck is not None:
            self._lc_close(xp, mask)
        self.n_updates += sum(1 for bk in self.books if bk.n_instate() > 0)
        ops = []
        for b in range(B):
            bk = self.books[b]
            for j in range(cfg.n_features):
                if bk.feat_id[j] >= 0 and not mask[b, j]:
                    ops.append(_op(b, L.EDIT_REMOVE_FEATURE, j))
                    bk.drop_feature(j)
                    self.n_rejected += 1
            self._discard_empty_groups(b, ops)
        be.edit(np.array(ops, dtype=L.edit_dtype))
        # --- Group::Create(X_.Rsb, X_.Tsb) from the updated pose + InitializeJustCreatedTracks (:121-126, :575-600)
        fl = cfg.focal_length()
        if cfg.triangulate_pre_subfilter:   # a new track is never triangulated yet: the badtri stds (manager.cpp:585-586)
            std = [cfg.initial_std_x_badtri / fl, cfg.initial_std_y_badtri / fl, cfg.initial_std_z_badtri]
        else:
            std = [cfg.initial_std_x / fl, cfg.initial_std_y / fl, cfg.initial_std_z]
        slots = np.full(B, -1, dtype=np.int32)
        recs = []
        for b in range(B):
            bk, pb = self.books[b], self.pools[b]
            ids, meas = tracks[b]
            new = [k for k in np.argsort(ids, kind="stable") if int(ids[k]) not in bk.id2slot and int(ids[k]) not in pb.id2ent]
            if not new:
                continue
            afree = [a for a, u in enumerate(pb.anc_used) if not u]
            efree = [e for e, fid in enumerate(pb.ent_id) if fid < 0]
            if not afree:
                self.n_pool_dropped += len(new)
                continue
            a = afree[0]
            slots[b] = a
            pb.anc_used[a] = True; pb.anc_life[a] = 0; pb.anc_link[a] = -1
            pb.anc_born[a] = self.vision_counter
            self.n_pool_dropped += max(0, len(new) - len(efree))
            for e, k in zip(efree, new):
                r = np.zeros((), dtype=L.pool_new_dtype)
                r["b"], r["entry"], r["anchor"], r["xp"], r["z0"], r["std_xyz"] = b, e, a, meas[k, :2], cfg.initial_z, std
                recs.append(r)
                pb.ent_id[e] = int(ids[k]); pb.ent_anchor[e] = a; pb.ent_born[e] = self.vision_counter
                pb.ent_key[e] = lck[b][int(ids[k])] if lck is not None else -1
                pb.id2ent[int(ids[k])] = e
                pb.hist_cnt[e] = 0; pb.hist[e] = []          # plife_hist_reset
            # --- OOS history (use_oos): the frame's anchor observes every live entry that had a track, the new ones included
            if use_oos:
                for e, fid in enumerate(pb.ent_id):
                    if fid >= 0:
                        pb.hist_append(e, cfg.oos_max_obs, a, self.vision_counter, meas[pos[b][fid], :2])
        if (slots >= 0).any():
            be.pool_anchor(slots)
        if recs:
            be.pool_add(np.array(recs, dtype=L.pool_new_dtype))
        # --- AdaptInitialDepth (:131, after the new tracks took the old init_z)
        if cfg.adaptive_initial_depth:
            self.init_z = be.adapt_depth()
        # --- EnforceMaxGroupLifetime (:282-304): an anchor out of the state with no live entry is freed when too old
        for pb in self.pools:
            held = set(pb.ent_anchor)
            for a in range(cfg.anchor_max):
                if pb.anc_used[a] and pb.anc_link[a] < 0 and pb.anc_life[a] > cfg.max_group_lifetime and a not in held:
                    pb.anc_used[a] = False
        return mask


def initial_poses(cfg, sims, t0=0.0):
    """xivo_pose_in records at t0 from the ground truth of each simulator (the reference starts from cfg "X";
    velocity comes from the trajectory, scripts/imu_trajectories.py get_imu_sim init_Vsb)"""
    B = len(sims)
    poses = np.zeros(B, dtype=L.pose_dtype)
    Rbc = so3_exp(cfg.Wbc)
    for b, s in enumerate(sims):
        Rsb, Tsb = s.gsb(t0)
        poses[b]["Rsb"] = Rsb.T.reshape(-1); poses[b]["Tsb"] = Tsb
        poses[b]["Rbc"] = Rbc.T.reshape(-1); poses[b]["Tbc"] = cfg.Tbc
        poses[b]["Vsb"] = s.vel(t0)
        poses[b]["Rsg"] = np.eye(3).reshape(-1)
    return poses


def run_pcw(backend_factory, cfg, worlds, sims, total_time=4.0, imu_dt=0.0025, vision_dt=0.04, noise_vision_std=1.0,
            timers=None, trajectory_log=False, map_log=False, rpe_dt=1.0, innovation_log=False, noise_seed=0):
    """The loop of scripts/pyxivo_pcw.py:117-163 for B = len(sims) sequences at once.
    -> dict(ts [n] ns, Tsb [n x B x 3], Wsb [n x B x 3], gt_Tsb [n x B x 3], runner, backend)
    trajectory_log (True, or the error-state columns to keep): the estimate of every frame is recorded on the device
    (HipBackend.record) and read once at the end instead of a scene download per frame - the same Tsb / Wsb, plus
    `trajectory` (HipBackend.trajectory) and, with the pose columns logged, err6 / nees / anees / nees_used; and per sequence
    ate_aligned / ate_raw / rpe_pos / rpe_rot from the device (xivo_hip_traj_score; RPE over rpe_dt seconds as
    rpe_lag_frames turns them into frames, -1: no pair).
    map_log: the in-state features of every frame are recorded on the device after the frame (xivo_hip_map_record) and read
    once at the end; the runner's slot book gives the track id of each, the worlds the true point (with lifecycle="device" the
    book is on the device: one xivo_hip_life_get_book read per recorded frame). Adds `map` (pts, n_pts, ids,
    gt), landmark_err3 / landmark_nees / landmark_anees / landmarks_used, anees_landmark and landmarks_scored_mean. Off:
    nothing changes.
    innovation_log: every frame's update records its NIS on the device (HipBackend.enable_innovation_log) and the log is read
    once at the end: adds `innovation`, nis_per_dof [n], nis_per_dof_seq [B], nis_used [n], nis_records_left_out
    (_innovation). A backend without enable_innovation_log (the oracle) leaves the keys out.
    cfg.track_source = "device": the points of `worlds` go to the device once and every frame is SequenceRunner.frame_world
    on the ground-truth camera poses; the worlds' own generate_measurements is not called, the pixel noise is the device's
    stream keyed by noise_seed, and with map_log the world ids are downloaded once per recorded frame.
    cfg.loop_closure: every frame hands the worlds' last_point_index to the runner as the tracks' keys; adds `lcmap_stats`
    ([B] lcmap_stats_dtype) and `lcmap_cov_stats` ([B] lcmap_cov_stats_dtype, the counters of lc_point_cov / lc_revisit_gap)."""
    if getattr(cfg, "imu_source", "host") == "device":
        raise ValueError("run_pcw feeds the simulators' IMU messages one by one: imu_source='device' runs with run_pcw_batch "
                         "or SequenceRunner.frame_resident")
    B = len(sims)
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    Rbc = so3_exp(cfg.Wbc)
    poses0 = initial_poses(cfg, sims)
    P0 = np.repeat(cfg.P_init()[None], B, axis=0)
    be = backend_factory(cfg, B, poses0, P0)
    runner = SequenceRunner(be, cfg, B)
    runner.timers = timers
    dev_tracks = cfg.track_source == "device"
    lc = bool(getattr(cfg, "loop_closure", False))      # the worlds' point indices are the tracks' keys
    if dev_tracks:
        be.set_world(np.array([w.Xs for w in worlds]))
        runner.noise_px_std, runner.noise_seed = noise_vision_std, noise_seed
    m0 = [s.meas(0.0) for s in sims]
    feeder = ImuFeeder(B, 0.0, [m[1] for m in m0], [m[0] for m in m0])
    n_imu = int(round(total_time / imu_dt)); every = int(round(vision_dt / imu_dt))
    ts, est_T, est_W, gt_T, gt_R = [], [], [], [], []
    if trajectory_log:
        be.enable_trajectory_log((n_imu + every - 1) // every, _traj_cols(trajectory_log))
    mlog = _MapLog(be.ctx, (n_imu + every - 1) // every, cfg.n_features, B) if map_log else None
    ilog = bool(innovation_log) and hasattr(be, "enable_innovation_log")
    if ilog:
        be.enable_innovation_log((n_imu + every - 1) // every)
    for k in range(n_imu):
        t = k * imu_dt
        if k > 0:
            m = [s.meas(t) for s in sims]
            feeder.imu(t, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
        if k % every == 0:
            feeder.visual(t)
            tracks = []
            for b in range(B):
                Rsb, Tsb = sims[b].gsb(t)
                if dev_tracks:
                    tracks.append(np.concatenate([(Rsb @ Rbc).reshape(-1), Rsb @ cfg.Tbc + Tsb]))
                    continue
                tracks.append(worlds[b].generate_measurements(Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb, K, cfg.cam["cols"],
                                                              cfg.cam["rows"], noise_vision_std))
            if ilog:
                be.frame_ts = int(round(t * 1e9))
            if dev_tracks:
                runner.frame_world(feeder.take(), np.array(tracks), len(ts))
            else:
                runner.frame(feeder.take(), tracks, [w.last_point_index for w in worlds] if lc else None)
            ts.append(int(round(t * 1e9)))
            if trajectory_log:
                be.record(ts[-1])
                gt_R.append(np.array([s.gsb(t)[0] for s in sims]))
            else:
                R, T = be.poses()
                est_T.append(T); est_W.append(np.array([so3_log(r) for r in R]))
            gt_T.append(np.array([s.gsb(t)[1] for s in sims]))
            if mlog is not None:
                mlog.record(ts[-1], [bk.feat_id for bk in runner.books],
                            be.world_ids()[0] if dev_tracks else np.array([w.ids for w in worlds]), np.array([w.Xs for w in worlds]))
    out = dict(ts=np.array(ts), gt_Tsb=np.array(gt_T), runner=runner, backend=be)
    if lc and hasattr(be, "lcmap_stats"):
        out["lcmap_stats"] = be.lcmap_stats()
        if hasattr(be, "lcmap_cov_stats"):
            out["lcmap_cov_stats"] = be.lcmap_cov_stats()
    if mlog is not None:
        mlog.finish(out)
    if ilog:
        _innovation(be.ctx, out)
    if trajectory_log:
        traj = be.trajectory()
        est_T, est_W = traj["Tsb"], [[so3_log(r) for r in R] for R in traj["Rsb"]]
        _score(be.ctx, traj, np.array(gt_R), out["gt_Tsb"], out, rpe_lag_frames(rpe_dt, vision_dt))
    out["Tsb"], out["Wsb"] = np.array(est_T), np.array(est_W)
    return out


def run_pcw_cpp(cfg, worlds, sims, total_time=4.0, imu_dt=0.0025, vision_dt=0.04, noise_vision_std=1.0, device=0,
                innovation_log=False):
    """run_pcw with the C++ host side: the same messages go to xivo::hip::BatchEstimator (xivo_amd/host/batch_estimator.h)
    through its InertialMeas / VisualMeasPointCloud entry points instead of ImuFeeder + SequenceRunner.
    -> dict(ts, Tsb, Wsb, gt_Tsb, estimator); innovation_log: as in run_pcw, recorded by the C++ frame
    (BatchEstimator::EnableInnovationLog)"""
    from .batch import BatchEstimator
    B = len(sims)
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    Rbc = so3_exp(cfg.Wbc)
    est = BatchEstimator(cfg, B, initial_poses(cfg, sims), cfg.P_init(), device=device)
    n_imu = int(round(total_time / imu_dt)); every = int(round(vision_dt / imu_dt))
    ts, est_T, est_W, gt_T = [], [], [], []
    if innovation_log:
        est.enable_innovation_log((n_imu + every - 1) // every)
    for k in range(n_imu):
        t = k * imu_dt
        m = [s.meas(t) for s in sims]
        est.InertialMeas(t, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
        if k % every == 0:
            tracks = []
            for b in range(B):
                Rsb, Tsb = sims[b].gsb(t)
                tracks.append(worlds[b].generate_measurements(Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb, K, cfg.cam["cols"],
                                                              cfg.cam["rows"], noise_vision_std))
            est.VisualMeasPointCloud(t, tracks)
            R, T = est.gsb()
            ts.append(int(round(t * 1e9))); est_T.append(T); est_W.append(np.array([so3_log(r) for r in R]))
            gt_T.append(np.array([s.gsb(t)[1] for s in sims]))
    out = dict(ts=np.array(ts), Tsb=np.array(est_T), Wsb=np.array(est_W), gt_Tsb=np.array(gt_T), estimator=est)
    if innovation_log:
        _innovation(L.Context.borrow(est.host.xivo_batch_ctx(est.h), cfg.N, 2 * cfg.n_features, B), out)
    return out


def camera_poses(Rsb, Tsb, Rbc, Tbc):
    """ground-truth camera poses of B bodies -> (Rsc [B, 3, 3], Tsc [B, 3], gsc [B, 12] as xivo_hip_pcw_tracks takes them)"""
    Rsc, Tsc = Rsb @ Rbc, np.einsum("bij,j->bi", Rsb, Tbc) + Tsb
    return Rsc, Tsc, np.concatenate([Rsc.reshape(-1, 9), Tsc], axis=1)


def run_pcw_batch(cfg, B, total_time=2.0, imu_dt=0.0025, vision_dt=0.04, noise_vision_std=1.0, npts=1000, seed=0, device=0,
                  timers=None, trajectory_log=False, map_log=False, rpe_dt=1.0, innovation_log=False, track_source=None,
                  noise="numpy", noise_seed=0, imu_source=None, imu_noise="numpy"):
    """Thousands of sequences end to end: the vectorised simulators of xivo_amd/pcw.py (BatchTrajectorySim, BatchPCW) feed
    xivo::hip::BatchEstimator message by message. -> dict(ts, Tsb [n x B x 3], gt_Tsb, estimator)
    trajectory_log: as in run_pcw - one record launch per frame on the estimator's context and one read at the end instead of
    a pose download per frame; adds `trajectory`, err6 / nees / anees / nees_used and ate_aligned / ate_raw / rpe_pos / rpe_rot.
    map_log: as in run_pcw, on the estimator's context; the slot book is the estimator's (BatchEstimator.book).
    innovation_log: as in run_pcw; the C++ frame records between its update and AbsorbError (BatchEstimator::EnableInnovationLog).
    track_source ("host" / "device", default cfg.track_source): "device" keeps the worlds on the device
    (BatchEstimator::EnableDeviceWorld) and every frame hands down the ground-truth camera poses only
    (VisualMeasDeviceWorld; with cfg.track_faults the producer's track faults are on, every update is scored and the report
    gains "fault_stats": the counters' sums and per filter - the host-track arm hands the same options to BatchPCW.generate,
    which needs noise="philox", and reports the producer's five counters only); the pixel noise is then the stream of pcw.philox_normal keyed by noise_seed. noise="philox" gives
    the host track source the same stream and projection order (BatchPCW(noise="philox")), for comparing the two. With map_log
    and device tracks, the world's ids are read from the device once per recorded frame (xivo_hip_pcw_get_world: B x npts ids, a
    synchronising download - not for a timed run).
    imu_source ("host" / "device", default cfg.imu_source): "device" (needs device tracks) keeps the trajectory simulator on
    the device too (BatchEstimator::EnableDeviceImu): one FrameResident call per camera frame takes the place of the `every`
    InertialMeas calls and the frame call, nothing goes down during the run, and the ground truth is read from the device's log
    once at the end; only the initial poses and velocity come from the host simulator. The IMU noise is then the stream of
    pcw.trajsim_normals keyed by seed + 1 (the host simulator's seed); imu_noise="philox" gives the host IMU arm the same
    stream, for comparing the two. The IMU and the pixel stream share a generator: equal keys (seed + 1 == noise_seed) are
    refused when both are in use.
    timers: "sim_imu" and "sim_tracks" are the two simulators' shares, "sim" their sum; with device tracks "sim_tracks" is the
    ground-truth pose alone."""
    import copy
    import time
    from .batch import BatchEstimator
    from .pcw import BatchPCW, BatchTrajectorySim
    dev_tracks = (track_source or cfg.track_source) == "device"
    if track_source is not None or dev_tracks:
        cfg = copy.copy(cfg)
        cfg.track_source = "device" if dev_tracks else "host"
        if dev_tracks:
            cfg.npts = npts
        check_lifecycle(cfg)
    dev_imu = (imu_source or getattr(cfg, "imu_source", "host")) == "device"
    if imu_source is not None or dev_imu:
        cfg = copy.copy(cfg)
        cfg.imu_source = "device" if dev_imu else "host"
        check_lifecycle(cfg)
    if imu_noise not in ("numpy", "philox"):
        raise ValueError("imu_noise must be 'numpy' or 'philox'")
    if (dev_imu or imu_noise == "philox") and (dev_tracks or noise == "philox") and (seed + 1) % 2 ** 64 == noise_seed % 2 ** 64:
        raise ValueError("the IMU noise (key seed + 1 = %d) and the pixel noise (key noise_seed) would share their words: "
                         "choose different seeds" % (seed + 1))
    motion = ["lissajous" if b % 2 == 0 else "trefoil" for b in range(B)]
    rate = 0.08 + 0.04 * (np.arange(B) % 7) / 7
    sim = BatchTrajectorySim(motion, rate, seed=seed + 1, noise=imu_noise, noise_seed=seed + 1)
    faults = getattr(cfg, "track_faults", None)
    if faults is not None and not dev_tracks and noise != "philox":
        raise ValueError("track_faults on host tracks need noise='philox': they are draws of the device producer's generator")
    world = BatchPCW(B, npts=npts, seed=seed, noise=noise, noise_seed=noise_seed, faults=None if dev_tracks else faults)
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    sim_cam = cfg.cam if cfg.cam["model"] != L_CAM_PINHOLE else None      # both track sources simulate the estimator's camera
    Rbc = so3_exp(cfg.Wbc)
    poses = np.zeros(B, dtype=L.pose_dtype)
    R0, T0 = sim.gsb(0.0)
    poses["Rsb"] = R0.transpose(0, 2, 1).reshape(B, 9); poses["Tsb"] = T0; poses["Vsb"] = sim.vel(0.0)
    poses["Rbc"] = Rbc.T.reshape(-1); poses["Tbc"] = cfg.Tbc; poses["Rsg"] = np.eye(3).reshape(-1)
    est = BatchEstimator(cfg, B, poses, cfg.P_init(), device=device)
    host = est.host
    if dev_tracks:
        est.enable_device_world(world.Xs)
    n_imu = int(round(total_time / imu_dt)); every = int(round(vision_dt / imu_dt))
    if dev_imu:
        est.enable_device_imu(motion, rate, every, (n_imu + every - 1) // every, imu_dt, rot_amp=sim.rot_amp, rot_w=sim.rot_w,
                              noise_accel=sim.noise_accel, noise_gyro=sim.noise_gyro, grav_s=sim.grav_s, seed=seed + 1)
    ts, est_T, gt_T, gt_R = [], [], [], []
    ctx = None
    if trajectory_log:      # the estimator's own context (it stays the owner)
        ctx = L.Context.borrow(host.xivo_batch_ctx(est.h), cfg.N, 2 * cfg.n_features, B)
        ctx.traj_config((n_imu + every - 1) // every, _traj_cols(trajectory_log))
    mlog = None
    if map_log:
        mctx = ctx if ctx is not None else L.Context.borrow(host.xivo_batch_ctx(est.h), cfg.N, 2 * cfg.n_features, B)
        mctx.pcw_npts = npts
        mlog = _MapLog(mctx, (n_imu + every - 1) // every, cfg.n_features, B)
    ictx = None
    if innovation_log:
        est.enable_innovation_log((n_imu + every - 1) // every)
        ictx = ctx if ctx is not None else L.Context.borrow(host.xivo_batch_ctx(est.h), cfg.N, 2 * cfg.n_features, B)
    tm = timers if timers is not None else {}
    for k in range(n_imu):
        t = k * imu_dt
        if dev_imu and k % every != 0:
            continue
        if not dev_imu:
            t0 = time.perf_counter()
            accel, gyro = sim.meas(t, k)
            tm["sim_imu"] = tm.get("sim_imu", 0.0) + time.perf_counter() - t0
            est.InertialMeas(t, gyro, accel)
        if k % every == 0:
            t0 = time.perf_counter()
            if not dev_imu:
                Rsb, Tsb = sim.gsb(t)
                Rsc, Tsc, gsc = camera_poses(Rsb, Tsb, Rbc, cfg.Tbc)
            if not dev_tracks:
                off, ids, meas = world.generate(Rsc, Tsc, K, cfg.cam["cols"], cfg.cam["rows"], noise_vision_std, cam=sim_cam,
                                                max_radius=cfg.pcw_max_radius)
            t1 = time.perf_counter()
            tm["sim_tracks"] = tm.get("sim_tracks", 0.0) + t1 - t0
            mask = np.zeros((B, cfg.n_features), dtype=np.uint8) if est.want_mask else None   # (device life cycle: no download)
            if dev_imu:
                # samples k - every + 1 .. k since the last frame (none before the frame at t = 0)
                est.FrameResident(k - every if k else 0, every if k else 0, noise_vision_std, noise_seed, mask)
            elif dev_tracks:
                est.VisualMeasDeviceWorld(t, gsc, noise_vision_std, noise_seed, mask)
            elif host.xivo_batch_visual(est.h, float(t), off.ctypes.data, ids.ctypes.data, meas.ctypes.data,
                                        mask.ctypes.data if mask is not None else None) != 0:
                raise RuntimeError("VisualMeasPointCloud failed")
            if (est.device_lifecycle or est.device_pool_lifecycle) and timers is not None:
                # a device life cycle only enqueues the frame: a timed run waits for it here, so that "frame" ends where the
                # host life cycle's does (its last call synchronises); "frame_enqueue" is the host's share of it
                tm["frame_enqueue"] = tm.get("frame_enqueue", 0.0) + time.perf_counter() - t1
                est.sync()
            tm["frame"] = tm.get("frame", 0.0) + time.perf_counter() - t1
            ts.append(int(round(t * 1e9)))
            if not dev_imu:
                gt_T.append(Tsb)
            if ctx is not None:
                ctx.traj_record(ts[-1], B)
                if not dev_imu:
                    gt_R.append(Rsb)
            else:
                est_T.append(est.poses()["Tsb"].copy())
            if mlog is not None:
                mlog.record(ts[-1], [est.book(b)[0] for b in range(B)], mctx.pcw_get_world(0, B)[0] if dev_tracks else world.ids,
                            world.Xs)
    tm["sim_imu"] = tm.get("sim_imu", 0.0)
    tm["sim"] = tm["sim_imu"] + tm.get("sim_tracks", 0.0)
    if dev_imu:     # the ground truth of the whole run in one read of the device's log
        gctx = ctx if ctx is not None else L.Context.borrow(host.xivo_batch_ctx(est.h), cfg.N, 2 * cfg.n_features, B)
        gt = gctx.trajsim_get_gt(0, B)
        gt_T, gt_R = gt[:, :, 9:], gt[:, :, :9].reshape(gt.shape[0], B, 3, 3).transpose(0, 1, 3, 2)
    out = dict(ts=np.array(ts), gt_Tsb=np.array(gt_T), estimator=est)
    if faults is not None:
        # the producer's counters and (device tracks: the score's) four cells: the sums and per filter. Host tracks are not
        # scored; their producer counters are the restatement's
        if dev_tracks:
            st = est.fault_stats()
            per = {k: st[k].astype(np.int64) for k in st.dtype.names}
        else:
            per = {k: v.copy() for k, v in world.fault_stats.items()}
        out["fault_stats"] = dict(sum={k: int(v.sum()) for k, v in per.items()}, per_filter=per)
    if mlog is not None:
        mlog.finish(out)
    if ictx is not None:
        _innovation(ictx, out)
    if ctx is not None:
        traj = _trajectory(ctx)
        est_T = traj["Tsb"]
        _score(ctx, traj, np.array(gt_R), out["gt_Tsb"], out, rpe_lag_frames(rpe_dt, vision_dt))
    out["Tsb"] = np.array(est_T)
    return out
