"""The per-frame feature life cycle of the "subfilter" mode at B filters of the TUM-VI layout (N = 203, 30 feature slots, 15 group
slots, 200 pool entries, 64 anchors), host against device: the same vectorised point-cloud sequences
(xivo_amd.sequence.run_pcw_batch, about 170 tracks per filter and frame at the default 1000 world points) run once with the C++
host life cycle (xivo_hip_pool_step with its downloads, op lists through xivo_hip_edit_batch, xivo_hip_set_pixels,
xivo_hip_pool_anchor, xivo_hip_pool_add, mask and status downloads) and once with xivo_hip_pool_life_begin / _end, alternating,
`--runs` times each.

Printed per side: wall time of the frame calls per frame of all sequences, each frame timed until the device has finished it
(the host side's last call synchronises; the device side only enqueues, so the timed run waits for the stream - its enqueue
share is printed next to it), median, min, max over the runs; the host book-keeping share; and whether both sides ended with
the same counters (updates, rejections, admissions, pool drops). Under
    rocprofv3 --kernel-trace --stats -- python scripts/bench_pool_lifecycle.py --filters 4096 --runs 1
the kernel times to read are pool_life_begin_kernel, pool_life_admit_kernel and pool_life_end_kernel against the
edit_batch_kernel, set_pixels_kernel, pool_anchor_kernel and pool_add_kernel launches they replace.

--tracks device compares two other arms, both with the device life cycle: "device" takes the host simulator's tracks through
xivo_hip_pool_life_begin (copy to page-locked staging and upload), "device_tracks" the tracks xivo_hip_pcw_tracks left in the
track block through xivo_hip_pool_life_begin_tracks; both draw the pixel noise from the counter-based stream
(BatchPCW(noise="philox")), so the counters must agree. Under rocprofv3 the three pool_life kernels then run on packed tracks
in one arm and on strided tracks in the other.

    python scripts/bench_pool_lifecycle.py --filters 4096 --total_time 1.0 --runs 3
prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xivo_amd import sequence          # noqa: E402


def _stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--total_time", type=float, default=1.0)
    ap.add_argument("--npts", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tracks", default="host", choices=["host", "device"],
                    help="device: the device life cycle on uploaded tracks against the device life cycle on produced tracks")
    a = ap.parse_args()
    res = dict(filters=a.filters, total_time=a.total_time, npts=a.npts, runs=a.runs, tracks=a.tracks)
    arms = ("host", "device") if a.tracks == "host" else ("device", "device_tracks")
    ms, host_s, updates, frames, enq = {k: [] for k in arms}, {k: [] for k in arms}, {}, 0, {k: [] for k in arms}
    for _ in range(a.runs):
        for life in arms:
            cfg = sequence.SequenceConfig(feature_init="subfilter", pool_lifecycle="host" if life == "host" else "device",
                                          tracks_max=a.npts)
            tm = {}
            kw = {} if a.tracks == "host" else dict(track_source="device" if life == "device_tracks" else "host", noise="philox")
            out = sequence.run_pcw_batch(cfg, a.filters, total_time=a.total_time, npts=a.npts, timers=tm, **kw)
            st = out["estimator"].stats()
            out["estimator"].close()
            frames = len(out["ts"])
            ms[life].append(1e3 * tm["frame"] / frames)
            host_s[life].append(1e3 * st["host_seconds"] / frames)
            if "frame_enqueue" in tm:
                enq[life].append(1e3 * tm["frame_enqueue"] / frames)
            updates[life] = (st["updates"], st["mh_rejected"], st["admitted"], st["pool_dropped"])
    res["frames"] = frames
    for life in arms:
        res[life] = dict(ms_per_frame_of_all_filters=_stats(ms[life]), host_bookkeeping_ms_per_frame=_stats(host_s[life]),
                         updates=updates[life])
        if enq[life]:
            res[life]["enqueue_ms_per_frame"] = _stats(enq[life])
    res["same_counters"] = updates[arms[0]] == updates[arms[1]]   # (updates, rejected, admitted, pool-dropped)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
