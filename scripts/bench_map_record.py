"""Time the landmark log's record launch at B filters of the TUM-VI layout (N = 203: 15 groups, 30 feature slots, every slot
in use), n_out = 30, with and without the world covariance, against the route the same data took before: xivo_hip_get_scene
plus xivo_hip_download_P of every filter.

map_record is timed with the context's device timer (HIP events around `--reps` back-to-back launches into a log of that
many frames, divided by the count) and as a host clock around one launch plus a synchronise; the download route is a host
clock around calls that end in a synchronise. Several runs each; medians, minima and maxima are printed.

    python scripts/bench_map_record.py --filters 4096 --runs 9
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import lib as L          # noqa: E402
from xivo_amd import synth             # noqa: E402
from xivo_amd.pcw import so3_exp       # noqa: E402


def _stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="record launches per device-timed run")
    a = ap.parse_args()
    B, ng, nf = a.filters, 15, 30
    N = 23 + 6 * ng + 3 * nf
    rng = np.random.default_rng(0)
    poses = np.zeros(B, dtype=L.pose_dtype)
    poses["Rsb"] = np.eye(3).reshape(-1); poses["Rsg"] = np.eye(3).reshape(-1)
    poses["Rbc"] = so3_exp(np.array([-1.57079633, 0.0, 0.0])).T.reshape(-1); poses["Tbc"] = [0.05, 0.0, 0.02]
    groups = np.zeros((B, ng), dtype=L.group_dtype)
    groups["Rsb"] = np.eye(3).reshape(-1); groups["Tsb"] = rng.normal(size=(B, ng, 3))
    feats = np.zeros((B, nf), dtype=L.feat_dtype)
    feats["sind"] = np.arange(nf)[None]; feats["ref_sind"] = rng.integers(0, ng, (B, nf))
    feats["x"][..., :2] = rng.uniform(-0.5, 0.5, (B, nf, 2)); feats["x"][..., 2] = np.log(rng.uniform(1.0, 4.0, (B, nf)))
    A = rng.uniform(-1, 1, (N, N))
    P1 = A @ A.T / N * 1e-2 + 1e-4 * np.eye(N)
    res = dict(filters=B, N=N, n_features=nf, n_out=nf, runs=a.runs, reps=a.reps)
    with L.Context(N, 2 * nf, B) as ctx:
        ctx.set_layout(N, 23, ng, 23 + 6 * ng, nf, synth.PINHOLE)
        ctx.set_scene(poses, groups, feats)
        chunk = 256
        for b0 in range(0, B, chunk):                                   # (one P for all, scaled per filter: distinct scores)
            nb = min(chunk, B - b0)
            ctx.upload_P(P1[None] * (1.0 + 1e-3 * np.arange(b0, b0 + nb))[:, None, None], b0=b0)
        for world in (True, False):
            ctx.map_config(a.reps, nf, world_cov=world)
            dev, wall = [], []
            for it in range(a.warmup + a.runs):
                ctx.map_reset(); ctx.sync()
                ctx.timer_begin()
                for _ in range(a.reps):
                    ctx.map_record()
                dev.append(ctx.timer_end() / a.reps)
                ctx.map_reset(); ctx.sync()
                t0 = time.perf_counter()
                ctx.map_record(); ctx.sync()
                wall.append(1e3 * (time.perf_counter() - t0))
            key = "world_cov" if world else "local_only"
            res[f"map_record_{key}_device_ms"] = _stats(dev[a.warmup:])
            res[f"map_record_{key}_wall_ms"] = _stats(wall[a.warmup:])
        t = []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            ctx.map_reset(); ctx.map_record()
            pts, n_pts, _ = ctx.map_read(nt=1)
            t.append(1e3 * (time.perf_counter() - t0))
        res["map_record_and_read_wall_ms"] = _stats(t[a.warmup:])
        res["record_bytes"] = int(pts.nbytes + n_pts.nbytes)
        t = []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            ctx.get_scene()
            Pd = ctx.download_P()
            t.append(1e3 * (time.perf_counter() - t0))
        res["get_scene_download_P_wall_ms"] = _stats(t[a.warmup:])
        res["download_bytes"] = int(Pd.nbytes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
