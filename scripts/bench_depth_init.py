"""Time the depth initialisation of new tracks on the device-resident feature pool at B filters x E entries:
one frame of xivo_hip_pool_step with pre-sub-filter triangulation off and on (the triangulation runs in pool_tri_kernel
ahead of pool_step_kernel, on the entries at their first step), and xivo_hip_pool_adapt_depth (AdaptInitialDepth).

Every iteration first re-adds a share --fresh of each filter's entries (xivo_hip_pool_add, not timed), so that share
is at its first step - the entries a frame's new tracks occupy - and every other entry takes a plain sub-filter step.
Wall times are host clocks around calls that end in a device synchronise. Kernel times: run under
`rocprofv3 --kernel-trace --stats` (pool_tri_kernel, pool_step_kernel, adapt_depth_kernel).

    python scripts/bench_depth_init.py --filters 4096 --entries 200 --fresh 0.1 --iters 20
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
    ap.add_argument("--fresh", type=float, default=0.1, help="share of entries at their first step in each frame")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--method", default="l1_angular")
    a = ap.parse_args()
    B, E, A, ng, nf = a.filters, a.entries, 4, 8, 4
    N = 23 + 6 * ng + 3 * nf
    cam = synth.PINHOLE
    rng = np.random.default_rng(0)
    Rbc = so3_exp(np.array([-1.57079633, 0.0, 0.0]))
    poses = np.zeros(B, dtype=L.pose_dtype)
    poses["Rsb"] = np.eye(3).reshape(-1); poses["Rbc"] = Rbc.T.reshape(-1); poses["Rsg"] = np.eye(3).reshape(-1)
    groups = np.zeros((B, ng), dtype=L.group_dtype)
    groups["Rsb"] = np.eye(3).reshape(-1)
    feats = np.zeros((B, nf), dtype=L.feat_dtype)              # in-state features for AdaptInitialDepth's depth set
    feats["sind"] = np.arange(nf)[None]; feats["x"][..., 2] = np.log(rng.uniform(1.0, 4.0, (B, nf)))
    opts = dict(Rtri=3.5 ** 2, MH_thresh=5.991, ready_steps=1, min_depth=0.05, max_depth=10.0, max_subfilter_outlier=0.01)
    n_fresh = max(1, int(round(a.fresh * E)))
    res = dict(filters=B, entries=E, fresh_per_filter=n_fresh, method=a.method)
    with L.Context(N, 2 * nf, B) as ctx:
        ctx.set_layout(N, 23, ng, 23 + 6 * ng, nf, cam)
        ctx.set_scene(poses, groups, feats)
        ctx.pool_config(E, A, remove_outlier_counter=1e30, **opts)      # nothing leaves the pool: same work every frame
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))                    # anchor at the identity pose
        cur = poses.copy()
        cur["Tsb"] = [0.15, 0.0, 0.02]                                  # the current pose: a baseline to triangulate over
        ctx.set_scene(cur, groups, feats)
        recs = np.zeros(B * E, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), E); recs["entry"] = np.tile(np.arange(E), B)
        # landmarks 1-6 m in front of the anchor camera; this frame's pixel is their projection from the current pose + 0.5 px
        fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        Xa = np.stack([rng.uniform(-1, 1, B * E), rng.uniform(-0.7, 0.7, B * E), rng.uniform(1.0, 6.0, B * E)], axis=1)
        Xc = Xa - Rbc.T @ np.array([0.15, 0.0, 0.02])
        recs["xp"][:, 0] = fx * Xa[:, 0] / Xa[:, 2] + cx; recs["xp"][:, 1] = fy * Xa[:, 1] / Xa[:, 2] + cy
        recs["z0"] = 2.5; recs["std_xyz"] = [1.0 / 580, 1.0 / 580, 1.0]
        ctx.pool_add(recs)
        xp = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1) + rng.normal(size=(B * E, 2)) * 0.5
        xp = xp.reshape(B, E, 2)
        fresh = recs.reshape(B, E)[:, :n_fresh].reshape(-1)
        for mode in ("off", "on"):
            ctx.pool_triangulation(a.method if mode == "on" else None)
            t = []
            for it in range(a.warmup + a.iters):
                ctx.pool_add(fresh)                                     # these entries are at their first step again
                t0 = time.perf_counter()
                ctx.pool_step(xp, strict=False)
                t.append(time.perf_counter() - t0)
            res[f"pool_step_tri_{mode}_ms"] = 1e3 * float(np.median(t[a.warmup:]))
        good, bad = ctx.pool_tri_counts()
        res["triangulations_good"], res["triangulations_bad"] = int(good.sum()), int(bad.sum())
        ctx.pool_adapt_depth_config(2.5, median_weight=0.99, min_feature_lifetime=1, min_z=0.05, max_z=10.0)
        t = []
        for it in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            z = ctx.pool_adapt_depth()
            t.append(time.perf_counter() - t0)
        res["adapt_depth_ms"] = 1e3 * float(np.median(t[a.warmup:]))
        res["init_z_median"] = float(np.median(z))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
