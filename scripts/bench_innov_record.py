"""Time the innovation log's record launch at B filters of the TUM-VI size (N = 203, 30 features: 60 row-pair compressed rows
of 21 non-zeros) against the route the same figure took before: xivo_hip_get_H and xivo_hip_download_P of every filter (the
host would still have to factor S).

innov_record is timed with the context's device timer (HIP events around `--reps` back-to-back launches into a log of that
many frames, divided by the count) and as a host clock around one launch plus a synchronise; the download route is a host
clock around calls that end in a synchronise (get_H on `--host-filters` filters, scaled to B). Several runs each; medians,
minima and maxima are printed.

    python scripts/bench_innov_record.py --filters 4096 --runs 9
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


def _stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="record launches per device-timed run")
    ap.add_argument("--host-filters", type=int, default=64, help="filters the get_H route is timed on (scaled to --filters)")
    a = ap.parse_args()
    B, N, F = a.filters, 203, 30
    nd = 16
    P, H, inn, dR = synth.s_level(N, F, nd, seed=1)
    res = dict(filters=B, N=N, rows=2 * F, runs=a.runs, reps=a.reps)
    with L.Context(N, 2 * F, B) as ctx:
        chunk = 256
        for b0 in range(0, B, chunk):
            idx = np.arange(b0, min(b0 + chunk, B)) % nd
            ctx.upload_P(P[idx], b0=b0)
            ctx.set_measurements(H[idx], inn[idx], dR[idx], b0=b0)
        ctx.update_joseph()
        res["route"] = ctx.last_route()
        ctx.innov_config(a.reps)
        dev, wall = [], []
        for it in range(a.warmup + a.runs):
            ctx.innov_reset(); ctx.sync()
            ctx.timer_begin()
            for _ in range(a.reps):
                ctx.innov_record()
            dev.append(ctx.timer_end() / a.reps)
            ctx.innov_reset(); ctx.sync()
            t0 = time.perf_counter()
            ctx.innov_record(); ctx.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
        res["innov_record_device_ms"] = _stats(dev[a.warmup:])
        res["innov_record_wall_ms"] = _stats(wall[a.warmup:])
        t = []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            ctx.innov_reset(); ctx.innov_record()
            recs, _ = ctx.innov_read(nt=1)
            st = ctx.innov_stats(nt=1)
            t.append(1e3 * (time.perf_counter() - t0))
        res["innov_record_read_stats_wall_ms"] = _stats(t[a.warmup:])
        res["record_bytes"] = int(recs.nbytes)
        res["nis_per_dof"] = float(st["frame_nis"][0] / st["frame_dof"][0])
        nh = min(a.host_filters, B)
        t = []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            for b in range(nh):
                ctx.get_H(b)
            t1 = time.perf_counter()
            Pd = ctx.download_P()
            t.append(1e3 * ((t1 - t0) * B / nh + time.perf_counter() - t1))
        res["get_H_download_P_wall_ms"] = _stats(t[a.warmup:])
        res["download_bytes"] = int(Pd.nbytes + B * (2 * F * N + 4 * F) * 8)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
