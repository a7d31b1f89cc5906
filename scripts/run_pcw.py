"""Run B point-cloud-world sequences at once on one MI355X (BASELINE configs 1 / 5 surrogate: TUM-VI sizes, N = 203,
<= 30 features) and report tracking error + where the time goes. Mirrors scripts/pyxivo_pcw.py's options."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import formats, pcw, sequence  # noqa: E402


def _consistency(out):
    """-traj-log: mean over the frames of the ensemble-mean pose NEES (6 for a consistent filter), and how many (frame,
    sequence) entries had a covariance block that was not positive definite (this rank's sequences)"""
    rep = {}
    if "anees" in out:
        rep.update({"anees_pose": float(np.nanmean(out["anees"])),
                    "nees_not_spd": int(out["nees"].size - out["nees_used"].sum())})
    if "ate_aligned" in out:         # per sequence, from the device (xivo_hip_traj_score); RPE: sequences with a pair
        def q(v):
            v = np.asarray(v)[np.asarray(v) >= 0]
            return {"median": float(np.median(v)), "p90": float(np.quantile(v, 0.9)), "max": float(v.max())} if v.size else None
        rep.update({"ate_aligned_m": q(out["ate_aligned"]), "rpe": {"pos_m": q(out["rpe_pos"]), "rot_rad": q(out["rpe_rot"])}})
    if "anees_landmark" in out:      # -map-log: 3 for a consistent map; landmarks scored per sequence and frame
        rep.update({"anees_landmark": out["anees_landmark"], "landmarks_scored_mean": out["landmarks_scored_mean"]})
    if "nis_per_dof" in out:         # -innov-log: 1 for a consistent filter; needs no ground truth
        seq = np.asarray(out["nis_per_dof_seq"]); seq = seq[np.isfinite(seq)]
        frm = np.asarray(out["nis_per_dof"])
        rep.update({"nis_per_dof": float(np.nanmean(frm)) if np.isfinite(frm).any() else None,
                    "nis_per_dof_sequences": {"median": float(np.median(seq)), "p90": float(np.quantile(seq, 0.9)),
                                              "max": float(seq.max())} if seq.size else None,
                    "nis_records_left_out": out["nis_records_left_out"]})
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-sequences", type=int, default=256)
    ap.add_argument("-npts", type=int, default=1000)
    ap.add_argument("-total_time", type=float, default=2.0)
    ap.add_argument("-imu_dt", type=float, default=0.0025)
    ap.add_argument("-vision_dt", type=float, default=0.04)
    ap.add_argument("-noise_vision_std", type=float, default=1.0)
    ap.add_argument("-integration_method", default="PrinceDormand")
    ap.add_argument("-as_coded_group_block", action="store_true", help="reproduce src/feature.cpp:675-676")
    ap.add_argument("-host", default="python", choices=["python", "cpp"],
                    help="host side of the frame loop: xivo_amd/sequence.py or xivo::hip::BatchEstimator (C++)")
    ap.add_argument("-vectorized", action="store_true",
                    help="thousands of sequences: vectorised simulators + the C++ host side (xivo_amd.sequence.run_pcw_batch)")
    ap.add_argument("-dump", default="", help="directory for per-sequence `ts Tsb Wsb` trajectories")
    ap.add_argument("-gpus", type=int, default=1,
                    help="BASELINE config 5 without a launcher: spawn this many ranks (one per GPU), sequence s on rank s mod gpus")
    ap.add_argument("-traj-log", dest="traj_log", action="store_true",
                    help="record every frame's estimate and motion-state covariance on the device (one read at the end) and "
                         "report anees_pose: the 6-dof pose NEES against the simulator's ground truth, ensemble mean per frame, "
                         "averaged over the frames (-host python and -vectorized)")
    ap.add_argument("-rpe-dt", dest="rpe_dt", type=float, default=1.0,
                    help="-traj-log: interval in seconds of the relative pose error (rpe), converted to camera frames with "
                         "-vision_dt (the nearest whole number, at least one frame; 0: no rpe); next to it ate_aligned_m, the ATE "
                         "after the least-squares rigid alignment, both scored on the device per sequence")
    ap.add_argument("-map-log", dest="map_log", action="store_true",
                    help="record every frame's in-state features, their world positions and covariances on the device (one read "
                         "at the end) and report anees_landmark: the 3-dof NEES of the world points against the simulator's, "
                         "ensemble mean per frame averaged over the frames, and the mean number of landmarks scored per "
                         "sequence and frame (-host python and -vectorized)")
    ap.add_argument("-innov-log", dest="innov_log", action="store_true",
                    help="record every update's normalised innovation squared on the device between the update and AbsorbError "
                         "(one read at the end) and report nis_per_dof: the ensemble's sum of NIS over its sum of counted "
                         "rows per frame, averaged over the frames (1 for a consistent filter; needs no ground truth), its "
                         "median / p90 / max over the sequences and the records left out (-host python and -vectorized)")
    ap.add_argument("-lifecycle", default="host", choices=["host", "device"],
                    help="who runs the per-frame feature life cycle: the host side (op lists, the default) or the device "
                         "(xivo_hip_life_begin / _end: nothing is downloaded during a frame)")
    ap.add_argument("-feature_init", default="immediate", choices=["immediate", "subfilter"],
                    help="life cycle of a new feature: it enters the state at once with the simulator's depth (the default), or "
                         "the reference's: from initial_z through the depth sub-filter in the device-resident feature pool")
    ap.add_argument("-pool-lifecycle", dest="pool_lifecycle", default="host", choices=["host", "device"],
                    help="-feature_init subfilter: who decides its life cycle, the host side around xivo_hip_pool_step (op lists, "
                         "the default) or the device (xivo_hip_pool_life_begin / _end: nothing is downloaded during a frame)")
    ap.add_argument("-tracks", default="host", choices=["host", "device"],
                    help="where a frame's tracks come from: the numpy point-cloud world, uploaded by the frame call (the "
                         "default), or the worlds resident on the device (xivo_hip_pcw_tracks: only the ground-truth camera "
                         "poses go down; pixel noise from its counter-based generator). Needs -lifecycle device, or "
                         "-feature_init subfilter -pool-lifecycle device, and -npts <= %d; not with -host cpp" % sequence.L.LIFE_MAX_TRACKS)
    ap.add_argument("-imu", default="host", choices=["host", "device"],
                    help="where the simulated IMU and the ground-truth poses come from: the numpy simulator, one message per "
                         "sample (the default), or the device (xivo_hip_trajsim_frame / xivo_hip_propagate_resident: one call per "
                         "camera frame, no host data; IMU noise from its counter-based generator). Needs -tracks device and "
                         "-vectorized; sim_imu_s is then the host's remaining share")
    ap.add_argument("-cam-model", dest="cam_model", default="pinhole", choices=sorted(pcw.SIM_CAMERAS),
                    help="the camera of the simulator and of the estimator (xivo_amd.pcw.SIM_CAMERAS): a distorted model runs "
                         "the sub-filter life cycle (-feature_init subfilter), with -vectorized or -tracks device")
    ap.add_argument("-max-radius", dest="max_radius", type=float, default=float("inf"),
                    help="-cam-model other than pinhole: a point whose normalised radius exceeds this is not visible (the guard "
                         "against a polynomial distortion's fold-back far off axis)")
    ap.add_argument("-use-oos", dest="use_oos", action="store_true",
                    help="MSCKF update from pool entries whose track ends (SequenceConfig.use_oos): needs -feature_init subfilter with "
                         "-host python, or -pool-lifecycle device with any host side; the report gains oos_used / oos_gated / oos_surplus / "
                         "oos_short")
    ap.add_argument("-oos-min-obs", dest="oos_min_obs", type=int, default=5,
                    help="-use-oos: observations an entry needs (OOS_update_min_observations)")
    ap.add_argument("-seed", type=int, default=0, help="-vectorized: the seed of the worlds and trajectories")
    d = sequence.SequenceConfig()
    ap.add_argument("-loop-closure", dest="loop_closure", action="store_true",
                    help="loop closure on the device-resident landmark map (SequenceConfig.loop_closure): the world-point index of "
                         "every track is its key, features that leave the state go to the map, returning points close the loop. "
                         "-host python; with the host life cycles, or (-lc-lifecycle device) inside -lifecycle device; the C++ "
                         "host side and the device pool life cycle carry no keys; the report gains the summed map counters (lcmap)")
    ap.add_argument("-lc-lifecycle", dest="lc_lifecycle", default="host", choices=["host", "device"],
                    help="-loop-closure: who feeds and queries the map - host: the runner's slot book, filter by filter, with a "
                         "download of the inlier mask every frame; device (needs -lifecycle device): the keys ride in the track "
                         "block and the resident book, the add records and the queries are made on the device "
                         "(SequenceConfig.lc_lifecycle)")
    ap.add_argument("-lc-map-max", dest="lc_map_max", type=int, default=d.lc_map_max, help="-loop-closure: map entries per sequence")
    ap.add_argument("-lc-max", dest="lc_max", type=int, default=d.lc_max, help="-loop-closure: matches per sequence and frame")
    ap.add_argument("-lc-min-matches", dest="lc_min_matches", type=int, default=d.lc_min_matches,
                    help="-loop-closure: kept matches a sequence needs to close")
    ap.add_argument("-lc-meas-std", dest="lc_meas_std", type=float, default=d.lc_meas_std, help="-loop-closure: loop_closure_meas_std (px)")
    ap.add_argument("-lc-chi2", dest="lc_chi2", type=float, default=d.lc_chi2, help="-loop-closure: gate of one match (0: none)")
    ap.add_argument("-lc-max-depth-var", dest="lc_max_depth_var", type=float, default=d.lc_max_depth_var,
                    help="-loop-closure: a feature whose depth variance is above this when it leaves is not stored (0: no test)")
    ap.add_argument("-lc-point-cov", dest="lc_point_cov", action="store_true",
                    help="-loop-closure: a stored point carries the covariance it left the state with and its matches are weighed "
                         "with it (SequenceConfig.lc_point_cov); the report gains lcmap_resting / _rested_frames / _bad_cov")
    ap.add_argument("-lc-revisit-gap", dest="lc_revisit_gap", type=int, default=d.lc_revisit_gap,
                    help="-loop-closure: N > 0 - a stored point closes the loop once per visit, a visit ending after N frames "
                         "without a match of it (SequenceConfig.lc_revisit_gap); 0: in every frame it is seen")
    ap.add_argument("-drop-prob", dest="drop_prob", type=float, default=0.0,
                    help="track faults (xivo_hip_pcw_fault_config): the chance per visible point and frame that its track is lost")
    ap.add_argument("-outlier-prob", dest="outlier_prob", type=float, default=0.0, help="track faults: the chance of a gross outlier")
    ap.add_argument("-outlier-px", dest="outlier_px", type=float, nargs=2, default=[20.0, 60.0], metavar=("MIN", "MAX"),
                    help="track faults: each component of an outlier's offset is +-[MIN, MAX] px")
    ap.add_argument("-outlier-sticky", dest="outlier_sticky", action="store_true",
                    help="track faults: an outlier's offset stays on the track until the track ends (default: one frame)")
    ap.add_argument("-tail-prob", dest="tail_prob", type=float, default=0.0, help="track faults: the chance of a heavy-tailed pixel noise draw")
    ap.add_argument("-tail-scale", dest="tail_scale", type=float, default=4.0, help="track faults: a tail draw multiplies noise_vision_std by this")
    ap.add_argument("-pixel-noise", dest="pixel_noise", default="numpy", choices=["numpy", "philox"],
                    help="-vectorized -tracks host: the pixel noise's generator - numpy's, or the device producer's counter-based "
                         "stream restated on the host (what -tracks device always draws)")
    a = ap.parse_args()
    faults = None
    if a.drop_prob or a.outlier_prob or a.tail_prob or a.outlier_sticky:
        try:
            faults = pcw.fault_opts(sticky=int(a.outlier_sticky), p_drop=a.drop_prob, p_outlier=a.outlier_prob, p_tail=a.tail_prob,
                                    outlier_min_px=a.outlier_px[0], outlier_max_px=a.outlier_px[1], tail_scale=a.tail_scale)
        except ValueError as e:
            ap.error("track faults: %s" % e)
        if a.tracks == "host" and not (a.vectorized and a.pixel_noise == "philox"):
            ap.error("the track-fault options with -tracks host need -vectorized -pixel-noise philox: the faults are draws of the "
                     "device producer's generator, which only that host arm restates (or use -tracks device)")
    if a.pixel_noise != "numpy" and not a.vectorized:
        ap.error("-pixel-noise philox runs with -vectorized")
    # (a sequence never brings more tracks than its world has points)
    life = dict(lifecycle=a.lifecycle, tracks_max=min(a.npts, sequence.L.LIFE_MAX_TRACKS))
    if a.cam_model != "pinhole":
        if a.feature_init != "subfilter":
            ap.error("-cam-model %s needs -feature_init subfilter (the immediate life cycle un-projects with a pinhole)" % a.cam_model)
        if not a.vectorized and a.tracks != "device":
            ap.error("-cam-model %s needs -vectorized or -tracks device (the per-sequence host worlds are pinhole)" % a.cam_model)
        if not a.max_radius > 0:
            ap.error("-max-radius must be positive")
        life.update(cam=pcw.SIM_CAMERAS[a.cam_model], pcw_max_radius=a.max_radius)
    if a.feature_init != "immediate" or a.pool_lifecycle != "host":
        life.update(feature_init=a.feature_init, pool_lifecycle=a.pool_lifecycle)
        try:      # before any rank is spawned: what check_lifecycle rejects
            sequence.check_lifecycle(sequence.SequenceConfig(**life))
        except ValueError as e:
            ap.error(str(e))
    if a.use_oos:
        if (a.vectorized or a.host != "python") and a.pool_lifecycle != "device":
            ap.error("-use-oos with -vectorized or -host cpp needs -pool-lifecycle device (the C++ host life cycle keeps no "
                     "observation history)")
        if a.innov_log:
            ap.error("-use-oos and -innov-log exclude each other (the log's dof would count the empty rows of the OOS block)")
        life.update(feature_init=a.feature_init, pool_lifecycle=a.pool_lifecycle, use_oos=True, oos_min_observations=a.oos_min_obs)
        try:
            sequence.check_lifecycle(sequence.SequenceConfig(**life))
        except ValueError as e:
            ap.error(str(e))
    if a.loop_closure:
        if a.vectorized or a.host != "python":
            ap.error("-loop-closure runs with -host python (the C++ host side has no loop closure)")
        if a.innov_log:
            ap.error("-loop-closure and -innov-log exclude each other (the log holds one update per frame)")
        life.update(feature_init=a.feature_init, pool_lifecycle=a.pool_lifecycle, loop_closure=True, lc_map_max=a.lc_map_max,
                    lc_max=a.lc_max, lc_min_matches=a.lc_min_matches, lc_meas_std=a.lc_meas_std, lc_chi2=a.lc_chi2,
                    lc_max_depth_var=a.lc_max_depth_var, lc_point_cov=bool(a.lc_point_cov), lc_revisit_gap=a.lc_revisit_gap,
                    lc_lifecycle=a.lc_lifecycle)
        try:
            sequence.check_lifecycle(sequence.SequenceConfig(**life))
        except ValueError as e:
            ap.error(str(e))
    elif a.lc_lifecycle != "host":
        ap.error("-lc-lifecycle device needs -loop-closure")
    if faults is not None:
        life.update(track_faults=faults)
    if a.tracks == "device":
        life.update(track_source="device", npts=a.npts)
        if a.host == "cpp" and not a.vectorized:
            ap.error("-tracks device runs with -host python or -vectorized")
        try:      # before any rank is spawned: what check_lifecycle rejects
            sequence.check_lifecycle(sequence.SequenceConfig(**life))
        except ValueError as e:
            ap.error(str(e))
    if a.imu == "device":
        life.update(imu_source="device")
        if not a.vectorized:
            ap.error("-imu device runs with -vectorized")
        try:      # before any rank is spawned: what check_lifecycle rejects
            sequence.check_lifecycle(sequence.SequenceConfig(**life))
        except ValueError as e:
            ap.error(str(e))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from xivo_amd.shard import spawn_ranks
        sys.exit(spawn_ranks([os.path.abspath(__file__)] + sys.argv[1:], a.gpus))
    if a.vectorized:
        cfg = sequence.SequenceConfig(integration_method=a.integration_method, fix_group_block=not a.as_coded_group_block, **life)
        tm = {}
        t0 = time.perf_counter()
        out = sequence.run_pcw_batch(cfg, a.sequences, total_time=a.total_time, imu_dt=a.imu_dt, vision_dt=a.vision_dt,
                                     noise_vision_std=a.noise_vision_std, npts=a.npts, timers=tm, trajectory_log=a.traj_log,
                                     map_log=a.map_log, rpe_dt=a.rpe_dt, innovation_log=a.innov_log, track_source=a.tracks,
                                     imu_source=a.imu, seed=a.seed, noise=a.pixel_noise)
        wall = time.perf_counter() - t0
        oos = {}
        if a.use_oos:     # the counters, and in how many sequences an entry was used at all
            ost = out["estimator"].oos_stats()
            oos = {k: int(ost[k].sum()) for k in ost.dtype.names}
            oos["oos_sequences_with_used"] = int((ost["oos_used"] > 0).sum())
        if "fault_stats" in out:     # track faults: the producer's counters and (-tracks device) the score's four cells, summed
            oos.update({"fault_" + k: v for k, v in out["fault_stats"]["sum"].items()})
        st = out["estimator"].stats(); out["estimator"].close()
        frames = len(out["ts"])
        ate = np.sqrt(np.mean(np.sum((out["Tsb"] - out["gt_Tsb"]) ** 2, axis=2), axis=0))
        print(json.dumps({
            "sequences": a.sequences, "frames_per_sequence": frames, "N": cfg.N, "integration": a.integration_method,
            "host": "cpp, vectorised simulators", "lifecycle": a.lifecycle, "tracks": a.tracks, "imu": a.imu,
            "feature_init": a.feature_init, "pool_lifecycle": a.pool_lifecycle, "cam_model": a.cam_model,
            **({"admitted": st["admitted"], "pool_dropped": st["pool_dropped"]} if a.feature_init == "subfilter" else {}), **oos,
            "ate_m": {"median": float(np.median(ate)), "p90": float(np.quantile(ate, 0.9)), "max": float(ate.max())},
            **_consistency(out),
            "updates": st["updates"], "mh_rejected": st["mh_rejected"], "wall_s": wall, "simulator_s": tm.get("sim", 0.0),
            # the two simulators' shares of simulator_s: IMU samples; the camera's ground-truth pose + (-tracks host) the tracks
            "sim_imu_s": tm.get("sim_imu", 0.0), "sim_tracks_s": tm.get("sim_tracks", 0.0),
            "frame_calls_s": tm.get("frame", 0.0), "host_cpp_lifecycle_s": st["host_seconds"],
            # -lifecycle device: the part of frame_calls_s before the stream is waited for (the frame is only enqueued)
            **({"frame_enqueue_s": tm["frame_enqueue"]} if "frame_enqueue" in tm else {}),
            "frames_per_s_in_frame_calls": a.sequences * frames / tm["frame"],
            "ms_per_frame_of_all_sequences": 1e3 * tm["frame"] / frames}))
        return
    # BASELINE config 5: under torch.distributed.run, sequence s runs on rank s mod world (one rank per GPU, no data-path
    # collective; the ranks only meet to add up the report)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    from xivo_amd.shard import sequence_to_gpu
    mine = [s_ for s_ in range(a.sequences) if sequence_to_gpu(s_, world) == rank]
    B = len(mine)
    cfg = sequence.SequenceConfig(integration_method=a.integration_method, fix_group_block=not a.as_coded_group_block, **life)
    worlds = [pcw.RandomPCW(npts=a.npts, seed=b) for b in mine]
    sims = [pcw.TrajectorySim("lissajous" if b % 2 == 0 else "trefoil", rate=0.08 + 0.04 * (b % 7) / 7, seed=1000 + b)
            for b in mine]
    timers = {}
    device = int(os.environ.get("LOCAL_RANK", 0))
    t0 = time.perf_counter()
    if a.host == "cpp":
        out = sequence.run_pcw_cpp(cfg, worlds, sims, total_time=a.total_time, imu_dt=a.imu_dt, vision_dt=a.vision_dt,
                                   noise_vision_std=a.noise_vision_std, device=device)
        st = out["estimator"].stats()
        timers = {"host_cpp_lifecycle": st["host_seconds"]}

        class _R:      # the report below reads these two counters
            n_updates, n_rejected = st["updates"], st["mh_rejected"]
        out["runner"] = _R
        out["estimator"].close()
    else:
        out = sequence.run_pcw(lambda c_, B_, p_, P_: sequence.HipBackend(c_, B_, p_, P_, device=device), cfg, worlds, sims,
                               total_time=a.total_time, imu_dt=a.imu_dt, vision_dt=a.vision_dt,
                               noise_vision_std=a.noise_vision_std, timers=timers, trajectory_log=a.traj_log,
                               map_log=a.map_log, rpe_dt=a.rpe_dt, innovation_log=a.innov_log)
        r_ = out["runner"]

        oos_st = out["backend"].oos_stats() if a.use_oos else None
        lc_st = out.get("lcmap_stats")
        fault_st = out["backend"].fault_stats() if faults is not None else None

        class _R:      # (read before the context goes: the device life cycle keeps the counters there)
            n_updates, n_rejected = r_.n_updates, r_.n_rejected
            oos = {k: int(oos_st[k].sum()) for k in oos_st.dtype.names} if oos_st is not None else {}
            if fault_st is not None:
                oos = dict(oos, **{"fault_" + k: int(fault_st[k].sum()) for k in fault_st.dtype.names})
            if lc_st is not None:     # the map counters summed over the sequences, and in how many a loop was closed at all
                oos = dict(oos, **{"lcmap_" + k: int(lc_st[k].sum()) for k in lc_st.dtype.names},
                           lcmap_sequences_with_closed=int((lc_st["closed_frames"] > 0).sum()))
                if out.get("lcmap_cov_stats") is not None:
                    oos = dict(oos, **{"lcmap_" + k: int(out["lcmap_cov_stats"][k].sum()) for k in out["lcmap_cov_stats"].dtype.names})
        out["runner"] = _R
        out["backend"].close()
    wall = time.perf_counter() - t0
    frames = len(out["ts"])
    ate = np.array([formats.ate_rmse(out["Tsb"][:, b], out["gt_Tsb"][:, b], align=False) for b in range(B)])
    dev = sum(timers.get(k, 0.0) for k in ("propagate", "edit", "update"))
    r = out["runner"]
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for k, b in enumerate(mine):
            formats.write_trajectory(os.path.join(a.dump, "seq%04d.txt" % b), out["ts"], out["Tsb"][:, k], out["Wsb"][:, k])
    n_upd, n_rej, oos = r.n_updates, r.n_rejected, getattr(r, "oos", {})
    if dist is not None:
        parts = [None] * world
        dist.all_gather_object(parts, (ate.tolist(), wall, dev, n_upd, n_rej, oos))
        oos = {k: sum(p_[5][k] for p_ in parts) for k in oos}
        ate = np.array(sum((p_[0] for p_ in parts), []))
        wall, dev = max(p_[1] for p_ in parts), max(p_[2] for p_ in parts)      # whole job = slowest rank
        n_upd, n_rej = sum(p_[3] for p_ in parts), sum(p_[4] for p_ in parts)
        B = a.sequences
    if rank != 0:
        return
    print(json.dumps({
        "sequences": B, "n_gpus": world, "frames_per_sequence": frames, "imu_samples_per_frame": int(round(a.vision_dt / a.imu_dt)),
        "N": cfg.N, "max_features": cfg.n_features, "integration": a.integration_method, "host": a.host,
        "lifecycle": a.lifecycle, "tracks": a.tracks, "feature_init": a.feature_init, "pool_lifecycle": a.pool_lifecycle,
        "cam_model": a.cam_model,
        "loop_closure": bool(a.loop_closure), **({"lc_lifecycle": a.lc_lifecycle} if a.loop_closure else {}),
        **({"lc_point_cov": bool(a.lc_point_cov), "lc_revisit_gap": a.lc_revisit_gap} if a.loop_closure else {}),
        "ate_m": {"median": float(np.median(ate)), "p90": float(np.quantile(ate, 0.9)), "max": float(ate.max())},
        **_consistency(out),
        "updates": n_upd, "mh_rejected": n_rej, **oos,
        "wall_s": wall, "device_path_s": dev,
        "phase_s": {k: round(v, 4) for k, v in sorted(timers.items())},
        "device_frames_per_s": B * frames / dev if dev > 0 else None,
        "ms_per_frame_per_batch": {k: round(1e3 * timers.get(k, 0.0) / frames, 3) for k in ("propagate", "edit", "update")},
        "ms_per_frame_of_all_sequences": round(1e3 * dev / frames, 3) if frames else None,
    }))


if __name__ == "__main__":
    main()
