"""Loop closure per frame at B sequences of the TUM-VI layout (N = 203, 30 feature slots, 15 group slots): who feeds and queries
the resident landmark map, host against device. The same vectorised point-cloud sequences (BatchTrajectorySim, BatchPCW: the
world-point index of a track is its key) go through the Python runner once with lc_lifecycle="host" (lifecycle="host":
SequenceRunner.frame's per-filter loops, its op lists, a download of the inlier mask and the close call's wait every frame) and
once with lc_lifecycle="device" (lifecycle="device": life_begin_keys -> lcmap_add_resident -> update -> lcmap_close_resident ->
life_end; the tracks and keys of all filters go down in one block), alternating, `--runs` times each after one short warm-up run
of either arm. Both arms get the same tracks, keys and IMU records from the same seeds, on one device, in one process.

Printed per arm and size: wall time of the frame call per frame of all sequences, each frame timed until the device has finished
it (median, min, max over the runs); the summed map counters, which must agree between the arms; anees_pose (the mean over
the frames of the ensemble's pose NEES, 6 for a consistent filter) and the median aligned ATE. What the device arm saves is host
time and a synchronisation - its kernels are a few microseconds of the frame - so the ratio says nothing about kernel throughput.

    python scripts/bench_lc_lifecycle.py --filters 256 4096 --total_time 0.6 --runs 3 --out profiles/lc_lifecycle_pcw.json
prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import lib as L          # noqa: E402
from xivo_amd import sequence          # noqa: E402
from xivo_amd.pcw import BatchPCW, BatchTrajectorySim, so3_exp      # noqa: E402


def _stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def run(arm, B, total_time, npts, seed=0, imu_dt=0.0025, vision_dt=0.04, noise=1.0, lc=None):
    """one run of B sequences -> (ms per frame, frames, the summed map counters, anees_pose, median aligned ATE)"""
    life = dict(lifecycle="device", lc_lifecycle="device", tracks_max=min(npts, L.LIFE_MAX_TRACKS)) if arm == "device" else {}
    cfg = sequence.SequenceConfig(loop_closure=True, **(lc or {}), **life)
    motion = ["lissajous" if b % 2 == 0 else "trefoil" for b in range(B)]
    rate = 0.08 + 0.04 * (np.arange(B) % 7) / 7
    sim = BatchTrajectorySim(motion, rate, seed=seed + 1)
    world = BatchPCW(B, npts=npts, seed=seed)
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    Rbc = so3_exp(cfg.Wbc)
    poses = np.zeros(B, dtype=L.pose_dtype)
    R0, T0 = sim.gsb(0.0)
    poses["Rsb"] = R0.transpose(0, 2, 1).reshape(B, 9); poses["Tsb"] = T0; poses["Vsb"] = sim.vel(0.0)
    poses["Rbc"] = Rbc.T.reshape(-1); poses["Tbc"] = cfg.Tbc; poses["Rsg"] = np.eye(3).reshape(-1)
    be = sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        runner = sequence.SequenceRunner(be, cfg, B)
        n_imu = int(round(total_time / imu_dt)); every = int(round(vision_dt / imu_dt))
        be.enable_trajectory_log((n_imu + every - 1) // every)
        accel0, gyro0 = sim.meas(0.0, 0)
        feeder = sequence.ImuFeeder(B, 0.0, gyro0, accel0)
        frame_s, gt_R, gt_T = 0.0, [], []
        for k in range(n_imu):
            t = k * imu_dt
            if k > 0:
                accel, gyro = sim.meas(t, k)
                feeder.imu(t, gyro, accel)
            if k % every:
                continue
            feeder.visual(t)
            Rsb, Tsb = sim.gsb(t)
            Rsc, Tsc, _ = sequence.camera_poses(Rsb, Tsb, Rbc, cfg.Tbc)
            off, ids, meas = world.generate(Rsc, Tsc, K, cfg.cam["cols"], cfg.cam["rows"], noise)
            idx = world.last_point_index
            tracks = [(ids[off[b]:off[b + 1]], meas[off[b]:off[b + 1]]) for b in range(B)]
            keys = [idx[off[b]:off[b + 1]] for b in range(B)]
            rec = feeder.take()
            be.sync()
            t0 = time.perf_counter()
            runner.frame(rec, tracks, keys)
            be.sync()
            frame_s += time.perf_counter() - t0
            be.record(int(round(t * 1e9)))
            gt_R.append(Rsb); gt_T.append(Tsb)
        out = {}
        sequence._score(be.ctx, be.trajectory(), np.array(gt_R), np.array(gt_T), out)
        st = be.lcmap_stats()
        frames = len(gt_T)
        return (1e3 * frame_s / frames, frames, {k: int(st[k].sum()) for k in st.dtype.names}, float(np.mean(out["anees"])),
                float(np.median(out["ate_aligned"])))
    finally:
        be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--total_time", type=float, default=0.6)
    ap.add_argument("--npts", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lc-min-matches", dest="lc_min_matches", type=int, default=sequence.SequenceConfig().lc_min_matches)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lc = dict(lc_min_matches=a.lc_min_matches)
    res = dict(total_time=a.total_time, npts=a.npts, runs=a.runs, lc_min_matches=a.lc_min_matches, sizes={})
    for arm in ("host", "device"):      # warm-up: code objects loaded, allocator warm
        run(arm, min(a.filters), min(a.total_time, 0.2), a.npts, lc=lc)
    for B in a.filters:
        ms, last = {"host": [], "device": []}, {}
        for _ in range(a.runs):
            for arm in ("host", "device"):
                m, frames, totals, anees, ate = run(arm, B, a.total_time, a.npts, lc=lc)
                ms[arm].append(m)
                last[arm] = dict(lcmap_totals=totals, anees_pose=anees, ate_aligned_median_m=ate)
        size = dict(frames=frames)
        for arm in ("host", "device"):
            size[arm] = dict(ms_per_frame_of_all_sequences=_stats(ms[arm]), **last[arm])
        size["host_over_device"] = size["host"]["ms_per_frame_of_all_sequences"]["median"] / size["device"]["ms_per_frame_of_all_sequences"]["median"]
        size["totals_agree"] = last["host"]["lcmap_totals"] == last["device"]["lcmap_totals"]
        res["sizes"][str(B)] = size
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not all(s["totals_agree"] for s in res["sizes"].values()):
        sys.exit("the map counters of the two arms differ")


if __name__ == "__main__":
    main()
