"""The device trajectory producer alone (xivo_hip_trajsim_frame, trajsim_frame_kernel): --filters trajectories, --frames camera
frames of --samples IMU samples each, on the curves run_pcw.py -vectorized flies. Prints one JSON line with the mean time per
frame between two stream events; meant to be run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_trajsim.py --filters 4096` for the kernel's own time
(profiles/README.md). The kernel is a few dozen transcendentals per sample: what it saves is host time and a
synchronisation, not device time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=16, help="IMU samples per camera frame")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise", type=float, default=1.0, help="scale of the IMU noise (0: the generator is skipped)")
    a = ap.parse_args()
    B, n = a.filters, a.samples
    with L.Context(47, 8, B) as ctx:
        ctx.trajsim_config(n, a.warmup + a.frames, noise_accel=1e-4 * a.noise, noise_gyro=1e-5 * a.noise)
        ctx.trajsim_set([b % 2 for b in range(B)], 0.08 + 0.04 * (np.arange(B) % 7) / 7)
        for k in range(a.warmup):
            ctx.trajsim_frame(k * n, n)
        ctx.sync()
        ctx.timer_begin()
        for k in range(a.warmup, a.warmup + a.frames):
            ctx.trajsim_frame(k * n, n)
        ms = ctx.timer_end()
        recs, _ = ctx.trajsim_get(0, 1)
        assert recs.shape == (1, n) and np.isfinite(recs["accel"]).all()
        # per filter and frame: n records of 104 bytes and two poses of 96 bytes out
        traffic = B * (n * 104.0 + 192.0)
        print(json.dumps({"filters": B, "samples_per_frame": n, "frames": a.frames, "noise": a.noise,
                          "ms_per_frame_between_events": ms / a.frames, "bytes_per_frame": traffic,
                          "samples_per_s_between_events": B * n / (ms / a.frames * 1e-3)}))


if __name__ == "__main__":
    main()
