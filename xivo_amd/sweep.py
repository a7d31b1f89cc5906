"""A tuning grid in one resident run: T tunings x W shared worlds = B filters of one context.

Every filter of a context reads its own visual_meas_std ** 2, MH_thresh, new-feature variances and IMU / model noise from the
resident tuning table (xivo_hip_tune_*, include/xivo_hip.h); the scores are per filter already (trajectory score, NEES,
innovation log). Filter b = t * W + w runs tuning t on world w: the W worlds, trajectories and noise streams are simulated
once and their tracks and IMU records tiled T times, so the tunings differ in nothing but their parameters.

grid()       the Cartesian product of the axes -> the configurations and the table
run_sweep()  the run, and per tuning the median / p90 aligned ATE, the RPE medians, the pose ANEES, NIS per degree of freedom
             and the rejected / not-SPD sums, next to the per-filter arrays
run_plain()  the same worlds through the same driver without a table: one configuration, W filters (what a sweep is compared to)

The C++ BatchEstimator takes no tuning table: the sweep runs on SequenceRunner / HipBackend."""
import copy
import itertools

import numpy as np

from . import lib as L
from .pcw import BatchPCW, BatchTrajectorySim, so3_exp
from .sequence import (HipBackend, ImuFeeder, L_CAM_PINHOLE, SequenceRunner, _innovation, _score, _traj_cols, camera_poses, check_lifecycle,
                       rpe_lag_frames)

# the fields of SequenceConfig a table row is computed from: plain attributes and "dict.key" entries of Qimu / Qmodel
TUNABLE = ("visual_meas_std", "MH_thresh", "initial_std_x", "initial_std_y", "initial_std_z",
           "Qimu.gyro", "Qimu.accel", "Qimu.gyro_bias", "Qimu.accel_bias", "Qmodel.Wsb", "Qmodel.Wbc", "Qmodel.Wsg")


def _set_field(cfg, name, value):
    if "." in name:
        d, k = name.split(".", 1)
        q = dict(getattr(cfg, d))      # (a copy: copy.copy(cfg) shares the dicts of cfg)
        q[k] = float(value)
        setattr(cfg, d, q)
    else:
        setattr(cfg, name, float(value))


def grid(cfg, axes):
    """axes: an ordered mapping from a tunable field (TUNABLE) to its values -> (cfgs [T], table [T] lib.tune_dtype), the
    Cartesian product with the last axis fastest. cfgs[t] is cfg with the axes' fields replaced; table[t] is
    HipBackend.tuning_entry(cfgs[t]): the numbers a plain run of cfgs[t] passes as scalars."""
    names = list(axes)
    for n in names:
        if n not in TUNABLE:
            raise ValueError("%r is not a tunable field (one of %s)" % (n, ", ".join(TUNABLE)))
    values = [[float(v) for v in np.atleast_1d(axes[n])] for n in names]
    if any(len(v) == 0 for v in values):
        raise ValueError("every axis needs at least one value")
    cfgs = []
    for combo in itertools.product(*values):
        c = copy.copy(cfg)
        for n, v in zip(names, combo):
            _set_field(c, n, v)
        cfgs.append(c)
    table = np.array([HipBackend.tuning_entry(c) for c in cfgs], dtype=L.tune_dtype)
    return cfgs, table


def check_sweep(cfg, axes):
    """what run_sweep cannot run, as ValueError: an axis that is no tunable field, and the configurations whose calls take one
    parameter set for every filter or would give every filter a world of its own"""
    for n in axes:
        if n not in TUNABLE:
            raise ValueError("%r is not a tunable field (one of %s)" % (n, ", ".join(TUNABLE)))
    if getattr(cfg, "use_oos", False):
        raise ValueError("run_sweep with use_oos is not supported: the OOS rows carry one oos_meas_std")
    if getattr(cfg, "loop_closure", False):
        raise ValueError("run_sweep with loop_closure is not supported: the loop-closure rows carry one lc_meas_std")
    if cfg.use_1pt_RANSAC:
        raise ValueError("run_sweep with use_1pt_RANSAC is not supported: OnePointRANSAC takes one parameter set")
    if cfg.track_source == "device" or getattr(cfg, "imu_source", "host") == "device":
        raise ValueError("run_sweep needs track_source='host' (and imu_source='host'): the device producers draw every "
                         "filter's noise from its own stream, so the tunings would not see the same world")
    if cfg.feature_init == "subfilter":
        if cfg.pool_lifecycle != "device":
            raise ValueError("run_sweep needs a device life cycle: pool_lifecycle='device' with feature_init='subfilter'")
        bad = [n for n in axes if n.startswith("initial_std_")]
        if bad:
            raise ValueError("run_sweep with feature_init='subfilter' cannot sweep %s: the pool life cycle does not read var_xyz"
                             % ", ".join(bad))
    elif cfg.lifecycle != "device":
        raise ValueError("run_sweep needs a device life cycle: lifecycle='device'")


def _tile_tracks(off, ids, meas, T):
    """the packed tracks of W filters, T times over: filter t * W + w gets the tracks of w"""
    if T == 1:
        return off, ids, meas
    n = int(off[-1])
    offs = np.concatenate([off[:-1] + t * n for t in range(T)] + [np.array([T * n], dtype=off.dtype)]).astype(np.int32)
    return offs, np.tile(ids, T), np.tile(meas, (T, 1))


def _run(cfg, W, T, table, total_time, imu_dt, vision_dt, noise_vision_std, npts, seed, device, rpe_dt, timers,
         track_source="host", noise_seed=0):
    import copy
    import time
    B = T * W
    if track_source not in ("host", "device"):
        raise ValueError("track_source must be 'host' or 'device'")
    dev_tracks = track_source == "device"
    if dev_tracks:
        # the W worlds tiled T times on the device, the producer's streams shared with period W: filter t * W + w draws the
        # words of filter w, so every tuning sees the same tracks - and the same track faults (cfg.track_faults)
        cfg = copy.copy(cfg)
        cfg.track_source, cfg.npts = "device", npts
        check_lifecycle(cfg)
    elif getattr(cfg, "track_faults", None) is not None:
        raise ValueError("track_faults need track_source='device': host tracks are not scored")
    motion = ["lissajous" if w % 2 == 0 else "trefoil" for w in range(W)]
    rate = 0.08 + 0.04 * (np.arange(W) % 7) / 7
    sim = BatchTrajectorySim(motion, rate, seed=seed + 1)
    world = BatchPCW(W, npts=npts, seed=seed)
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    sim_cam = cfg.cam if cfg.cam["model"] != L_CAM_PINHOLE else None
    Rbc = so3_exp(cfg.Wbc)
    poses = np.zeros(W, dtype=L.pose_dtype)
    R0, T0 = sim.gsb(0.0)
    poses["Rsb"] = R0.transpose(0, 2, 1).reshape(W, 9); poses["Tsb"] = T0; poses["Vsb"] = sim.vel(0.0)
    poses["Rbc"] = Rbc.T.reshape(-1); poses["Tbc"] = cfg.Tbc; poses["Rsg"] = np.eye(3).reshape(-1)
    be = HipBackend(cfg, B, np.tile(poses, T), np.repeat(cfg.P_init()[None], B, axis=0), device=device)
    if table is not None:
        be.enable_tuning(np.repeat(table, W))
    runner = SequenceRunner(be, cfg, B)
    if dev_tracks:
        be.set_world(np.tile(world.Xs, (T, 1, 1)))
        be.stream_share(W)
        runner.noise_px_std, runner.noise_seed = noise_vision_std, noise_seed
    n_imu = int(round(total_time / imu_dt)); every = int(round(vision_dt / imu_dt))
    n_frames = (n_imu + every - 1) // every
    be.enable_trajectory_log(n_frames, _traj_cols(True))
    be.enable_innovation_log(n_frames)
    a0, g0 = sim.meas(0.0, 0)
    feeder = ImuFeeder(W, 0.0, g0, a0)
    pool = cfg.feature_init == "subfilter"
    ts, gt_R, gt_T = [], [], []
    tm = timers if timers is not None else {}
    for k in range(n_imu):
        t = k * imu_dt
        if k > 0:
            accel, gyro = sim.meas(t, k)
            feeder.imu(t, gyro, accel)
        if k % every:
            continue
        feeder.visual(t)
        Rsb, Tsb = sim.gsb(t)
        Rsc, Tsc, gsc = camera_poses(Rsb, Tsb, Rbc, cfg.Tbc)
        if not dev_tracks:
            off, ids, meas = _tile_tracks(*world.generate(Rsc, Tsc, K, cfg.cam["cols"], cfg.cam["rows"], noise_vision_std, cam=sim_cam,
                                                          max_radius=cfg.pcw_max_radius), T)
        imu = feeder.take()
        if imu is not None and T > 1:
            imu = np.tile(imu, (T, 1))
        be.frame_ts = int(round(t * 1e9))
        t1 = time.perf_counter()
        if dev_tracks:      # the ground-truth camera poses tiled; the frame's number is the generator's counter
            runner.frame_world(imu, np.tile(gsc, (T, 1)), len(ts))
        else:
            if pool:
                runner.vision_counter += 1
                strict = runner.vision_counter >= cfg.strict_criteria_timesteps
                begin, end = (lambda: be.pool_life_begin(off, ids, meas, strict)), be.pool_life_end
            else:
                begin, end = (lambda: be.life_begin(off, ids, meas)), be.life_end
            runner._device_frame([("propagate", lambda: imu is not None and be.propagate(imu))], begin, end)
        if timers is not None:
            be.sync()
            tm["frame"] = tm.get("frame", 0.0) + time.perf_counter() - t1
        ts.append(be.frame_ts)
        be.record(ts[-1])
        gt_R.append(np.tile(Rsb, (T, 1, 1))); gt_T.append(np.tile(Tsb, (T, 1)))
    out = dict(ts=np.array(ts), gt_Tsb=np.array(gt_T), gt_Rsb=np.array(gt_R), runner=runner, backend=be, frames=len(ts))
    _innovation(be.ctx, out)
    _score(be.ctx, be.trajectory(), out["gt_Rsb"], out["gt_Tsb"], out, rpe_lag_frames(rpe_dt, vision_dt))
    out["life_stats"] = be.pool_life_stats() if pool else be.life_stats()
    if be.faults_on:
        out["fault_stats"] = be.fault_stats()
    return out


def summarize(out, T, W):
    """the per-tuning table of a run of T x W filters (filter t * W + w) from its per-filter arrays -> a list of T dicts:
    median and p90 of the aligned ATE over the worlds, the medians of the raw ATE and the two RPE figures, anees_pose (mean
    over the frames of the tuning's ensemble NEES of the pose, 6 when consistent), nis_per_dof (the tuning's sum of NIS over its
    sum of counted rows, 1 when consistent) and the sums of the rejected and not-SPD counters"""
    rows = []
    st = out["innovation"]["stats"]
    for t in range(T):
        s = slice(t * W, (t + 1) * W)
        ate = out["ate_aligned"][s]
        dof = int(st["filt_dof"][s].sum())
        with np.errstate(invalid="ignore"):
            nees = out["nees"][:, s] if "nees" in out else np.full((1, W), np.nan)
            fin = np.isfinite(nees)
            per_frame = np.where(fin.any(axis=1), np.where(fin, nees, 0.0).sum(axis=1) / np.maximum(fin.sum(axis=1), 1), np.nan)
        rows.append(dict(
            ate_aligned_m=float(np.median(ate)), ate_aligned_p90=float(np.percentile(ate, 90)),
            ate_raw_m=float(np.median(out["ate_raw"][s])),
            rpe_pos_m=float(np.median(out["rpe_pos"][s])), rpe_rot_m=float(np.median(out["rpe_rot"][s])),
            anees_pose=float(np.nanmean(per_frame)) if np.isfinite(per_frame).any() else float("nan"),
            nis_per_dof=float(st["filt_nis"][s].sum() / dof) if dof > 0 else float("nan"),
            rejected=int(out["life_stats"]["rejected"][s].sum()), not_spd=int(out["life_stats"]["not_spd"][s].sum())))
        if "fault_stats" in out:      # track faults: the score's four sums and the dropped tracks of the tuning
            fs = out["fault_stats"]
            rows[-1].update({k: int(fs[k][s].sum()) for k in ("outlier_rejected", "outlier_kept", "nominal_rejected", "nominal_kept",
                                                             "dropped")})
    return rows


def run_sweep(cfg, axes, worlds, total_time=4.0, imu_dt=0.0025, vision_dt=0.04, noise_vision_std=1.0, npts=1000, seed=0,
              device=0, rpe_dt=1.0, timers=None, track_source="host", noise_seed=0):
    """Run the grid of `axes` (grid()) on `worlds` shared worlds: one context of B = T x W filters, filter t * W + w tuning t on
    world w, one BatchTrajectorySim / BatchPCW of W sequences whose tracks and IMU records every tuning sees. Needs a device
    life cycle on host tracks (check_sweep). The trajectory log, the score and the innovation log are on.
    -> dict(axes, cfgs [T], table [T], T, W, summary [T] (summarize), and the run's per-filter arrays: ate_aligned / ate_raw /
    rpe_pos / rpe_rot [B], nees [n, B], nis_per_dof_seq [B], life_stats [B], trajectory, innovation, ts, gt_Tsb, runner,
    backend). timers: a dict that takes "frame", the seconds of the frame calls with a wait behind each.
    track_source="device" (cfg itself stays on host tracks): the W worlds are tiled T times on the device with
    xivo_hip_pcw_set_world, the producer's streams are shared with period W (xivo_hip_pcw_stream_share) and keyed by noise_seed,
    the ground-truth camera poses are tiled, the IMU stays the host's. cfg.track_faults then turns the producer's track faults
    on, and the summary gains per tuning the four sums of the score and `dropped`."""
    check_sweep(cfg, axes)
    W = int(worlds)
    if W <= 0:
        raise ValueError("run_sweep needs at least one world")
    cfgs, table = grid(cfg, axes)
    T = len(cfgs)
    out = _run(cfg, W, T, table, total_time, imu_dt, vision_dt, noise_vision_std, npts, seed, device, rpe_dt, timers,
               track_source, noise_seed)
    out.update(axes={n: [float(v) for v in np.atleast_1d(axes[n])] for n in axes}, cfgs=cfgs, table=table, T=T, W=W)
    out["summary"] = summarize(out, T, W)
    return out


def run_plain(cfg, worlds, total_time=4.0, imu_dt=0.0025, vision_dt=0.04, noise_vision_std=1.0, npts=1000, seed=0, device=0,
              rpe_dt=1.0, timers=None, track_source="host", noise_seed=0):
    """the W worlds of run_sweep(seed, npts) through the same driver with cfg's own parameters and no tuning table: what row t
    of a sweep is held against when cfg = cfgs[t]"""
    check_sweep(cfg, {})
    W = int(worlds)
    out = _run(cfg, W, 1, None, total_time, imu_dt, vision_dt, noise_vision_std, npts, seed, device, rpe_dt, timers,
               track_source, noise_seed)
    out.update(T=1, W=W)
    out["summary"] = summarize(out, 1, W)
    return out
