"""Time one frame of the out-of-state feature pool (xivo_hip_pool_step) next to the host-array path it replaces
(xivo_hip_subfilter_update on a host array + xivo_hip_candidate_order), at B filters x E entries.

Both paths run the same sub-filter step on the same entries; the host-array path also moves every entry
(sizeof(xivo_subfilter_feat) = 144 B) to the device and back. Wall times are host clocks around calls that end in a
device synchronise (both entry points synchronise before they return). Kernel times: run under
`rocprofv3 --kernel-trace --stats` (pool_step_kernel, subfilter_kernel).

    python scripts/bench_feature_pool.py --filters 4096 --entries 200 --iters 20
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4096)
    ap.add_argument("--entries", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, E, A, ng, nf = a.filters, a.entries, 16, 8, 4
    N = 23 + 6 * ng + 3 * nf
    cam = synth.PINHOLE
    rng = np.random.default_rng(0)
    poses = np.zeros(B, dtype=L.pose_dtype)
    Rbc = so3_exp(np.array([-1.57079633, 0.0, 0.0]))
    poses["Rsb"] = np.eye(3).reshape(-1); poses["Rbc"] = Rbc.T.reshape(-1); poses["Rsg"] = np.eye(3).reshape(-1)
    groups = np.zeros((B, ng), dtype=L.group_dtype)
    groups["Rsb"] = np.eye(3).reshape(-1)
    feats = np.zeros((B, 1), dtype=L.feat_dtype)
    feats["sind"] = -1
    opts = dict(Rtri=3.5 ** 2, MH_thresh=5.991, ready_steps=5, min_depth=0.05, max_depth=10.0, max_subfilter_outlier=0.01)
    with L.Context(N, 2 * nf, B) as ctx:
        ctx.set_layout(N, 23, ng, 23 + 6 * ng, nf, cam)
        ctx.set_scene(poses, groups, feats)
        ctx.pool_config(E, A, remove_outlier_counter=1e30, **opts)      # nothing leaves the pool: same work every frame
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        recs = np.zeros(B * E, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), E); recs["entry"] = np.tile(np.arange(E), B)
        recs["xp"][:, 0] = rng.uniform(20, 620, B * E); recs["xp"][:, 1] = rng.uniform(20, 460, B * E)
        recs["z0"] = 2.5; recs["std_xyz"] = [1.0 / 580, 1.0 / 580, 1.0]
        ctx.pool_add(recs)
        xp = (recs["xp"] + rng.normal(size=(B * E, 2))).reshape(B, E, 2)
        host, _, _ = ctx.pool_get()
        host["ref_sind"] = 0                    # group slot 0 = the anchor's pose (identity) for the host-array path
        t_pool, t_host = [], []
        for it in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            ctx.pool_step(xp, strict=False)
            t1 = time.perf_counter()
            sub = host.copy()
            sub["xp"] = xp
            upd = ctx.subfilter_update(sub, **opts)
            L.candidate_order(upd)
            t2 = time.perf_counter()
            if it >= a.warmup:
                t_pool.append(t1 - t0); t_host.append(t2 - t1)
    mb = B * E * np.dtype(L.subfilter_dtype).itemsize / 1e6
    print(json.dumps(dict(filters=B, entries=E, iters=a.iters,
                          pool_step_ms=dict(median=1e3 * float(np.median(t_pool)), min=1e3 * float(np.min(t_pool))),
                          host_array_ms=dict(median=1e3 * float(np.median(t_host)), min=1e3 * float(np.min(t_host))),
                          host_array_MB_each_way=round(mb, 1), pool_step_pixels_MB=round(B * E * 16 / 1e6, 1))))


if __name__ == "__main__":
    main()
