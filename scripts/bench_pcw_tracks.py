"""The device track producer alone (xivo_hip_pcw_tracks, pcw_tracks_kernel): --filters worlds of --npts points, --frames
camera frames of the trajectories run_pcw.py -vectorized flies. Prints one JSON line with the mean time per frame between two
stream events; meant to be run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_pcw_tracks.py --filters 4096`
for the kernel's own time (profiles/README.md)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import pcw, sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--npts", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise", type=float, default=1.0, help="pixel noise std (0: the generator is skipped)")
    ap.add_argument("--faults", action="store_true",
                    help="the fault instance of the kernel at the tests' probabilities: p_drop = p_outlier = p_tail = 0.2, sticky "
                         "offsets of 20 - 60 px, tail_scale 4")
    a = ap.parse_args()
    B = a.filters
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", npts=a.npts,
                                  tracks_max=min(a.npts, sequence.L.LIFE_MAX_TRACKS))
    sequence.check_lifecycle(cfg)
    sim = pcw.BatchTrajectorySim(["lissajous" if b % 2 == 0 else "trefoil" for b in range(B)], 0.08 + 0.04 * (np.arange(B) % 7) / 7)
    world = pcw.BatchPCW(B, npts=a.npts, seed=0)
    Rbc = pcw.so3_exp(cfg.Wbc)
    poses = np.zeros(B, dtype=sequence.L.pose_dtype)
    R0, T0 = sim.gsb(0.0)
    poses["Rsb"] = R0.transpose(0, 2, 1).reshape(B, 9); poses["Tsb"] = T0
    poses["Rbc"] = Rbc.T.reshape(-1); poses["Tbc"] = cfg.Tbc; poses["Rsg"] = np.eye(3).reshape(-1)
    be = sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        be.set_world(world.Xs)
        if a.faults:
            be.set_track_faults(dict(sticky=1, p_drop=0.2, p_outlier=0.2, p_tail=0.2, outlier_min_px=20.0, outlier_max_px=60.0, tail_scale=4.0))
        gsc = [sequence.camera_poses(*sim.gsb(0.04 * k), Rbc, cfg.Tbc)[2] for k in range(a.warmup + a.frames)]
        for k in range(a.warmup):
            be.make_tracks(gsc[k], a.noise, 0, k)
        be.sync()
        be.ctx.timer_begin()
        for k in range(a.warmup, a.warmup + a.frames):
            be.make_tracks(gsc[k], a.noise, 0, k)
        ms = be.ctx.timer_end()
        cnt = be.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)[0]
        # per filter and frame: 24 B per point and 8 B per id in, 32 B per track out (the ids that change are not counted)
        traffic = B * (a.npts * 32.0 + float(cnt.mean()) * 32.0)
        print(json.dumps({"filters": B, "npts": a.npts, "frames": a.frames, "noise_px_std": a.noise, "faults": bool(a.faults),
                          "ms_per_frame_between_events": ms / a.frames, "tracks_per_filter_mean": float(cnt.mean()),
                          "bytes_per_frame": traffic, "GBps_between_events": traffic / (ms / a.frames * 1e-3) / 1e9}))
    finally:
        be.close()


if __name__ == "__main__":
    main()
