"""Trajectory log on the device (xivo_hip_traj_*): the record is an exact copy of the resident state and of the chosen
covariance entries, slices and the full-log status behave, and the NEES of the logged poses meets fp64 bounds against the
longdouble restatement of tests/traj_restate.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import traj_restate as tr
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, GROUP_BEGIN, N_GROUPS, N_FEATURES = 53, 23, 2, 6      # Np = 64 != N: the gather has to walk the padded leading dimension
CAM = dict(model=L.CAM_PINHOLE, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[])
COLS6 = [52, 0, 14, 3, 23, 7]                             # unsorted, with column 0 and the last state column


def _rot(w):
    return tr.so3_exp(w).astype(np.float64)


def _poses(rng, B):
    p = np.zeros(B, dtype=L.pose_dtype)
    for b in range(B):
        p[b]["Rsb"] = _rot(rng.normal(size=3)).T.reshape(-1)
        p[b]["Rbc"] = _rot(rng.normal(size=3)).T.reshape(-1)
        p[b]["Rsg"] = np.eye(3).reshape(-1)
        for k in ("Tsb", "Tbc", "Vsb", "bg", "ba"):
            p[b][k] = rng.normal(size=3)
    return p


def _spd(rng, B, n=N):
    out = []
    for _ in range(B):
        A = rng.uniform(-1, 1, size=(n, n))
        P = A @ A.T / n + 1e-3 * np.eye(n)
        out.append(np.tril(P) + np.tril(P, -1).T)
    return np.array(out)


def _context(rng, B, poses=None):
    ctx = L.Context(N, 2 * N_FEATURES, B)
    ctx.set_layout(N, GROUP_BEGIN, N_GROUPS, GROUP_BEGIN + 6 * N_GROUPS, N_FEATURES, CAM)
    _set_poses(ctx, _poses(rng, B) if poses is None else poses)
    return ctx


def _set_poses(ctx, poses):
    B = poses.shape[0]
    groups = np.zeros((B, N_GROUPS), dtype=L.group_dtype)
    groups["Rsb"][:] = np.eye(3).reshape(-1)
    feats = np.zeros((B, N_FEATURES), dtype=L.feat_dtype)
    feats["sind"] = -1
    ctx.set_scene(poses, groups, feats)


def _same(a, b):
    """two arrays (records included) hold the same bytes"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_state(recs, ctx):
    """one frame's records [B] against the resident scene and status, bit for bit"""
    poses, _, _ = ctx.get_scene()
    for k in ("Rsb", "Tsb", "Vsb", "bg", "ba"):
        assert np.array_equal(recs[k], poses[k]), k
    assert np.array_equal(recs["status"], ctx.get_status(check=False)) and not recs["reserved"].any()


@pytest.mark.parametrize("cols", [COLS6, [52], "32"], ids=["6", "1", "32"])
def test_gather_is_exact(built, cols):
    rng = np.random.default_rng(11)
    if cols == "32":
        cols = [0, 52] + [int(c) for c in rng.permutation(np.arange(1, 52))[:30]]
        cols = [cols[i] for i in rng.permutation(32)]
    B = 5
    with _context(rng, B) as ctx:
        P = _spd(rng, B)
        ctx.upload_P(P)
        ctx.traj_config(3, cols)
        assert ctx.traj_count() == 0
        assert ctx.traj_record(123) == 0 and ctx.traj_count() == 1
        recs, cov, ts = ctx.traj_read()
        Pd = ctx.download_P()
        assert recs.shape == (1, B) and cov.shape == (1, B, len(cols), len(cols)) and ts.tolist() == [123]
        assert np.array_equal(Pd, P)
        for b in range(B):
            assert np.array_equal(cov[0, b], Pd[b][cols][:, cols]), b
        _same_state(recs[0], ctx)
        # the raw packed order: entry (i, j), i >= j, at i (i + 1) / 2 + j
        packed = np.zeros((1, B, len(cols) * (len(cols) + 1) // 2))
        ctx._check(ctx.lib.xivo_hip_traj_read(ctx.h, 0, B, 0, 1, None, packed.ctypes.data, None))
        for b in range(B):
            assert np.array_equal(packed[0, b], tr.pack_lower(Pd[b], cols))


def test_lower_triangle_is_what_is_read(built):
    """xivo_hip_upload_P mirrors the lower triangle, so a P whose triangles differ comes from xivo_hip_p_set_block3, which
    stores the 3 x 3 block it is given as it is."""
    rng = np.random.default_rng(12)
    B = 2
    with _context(rng, B) as ctx:
        ctx.upload_P(_spd(rng, B))
        P3 = np.arange(1.0, 10.0).reshape(3, 3)           # P3[r, c] = 3 r + c + 1: not symmetric
        ctx.p_set_block3(1, 3, P3)
        cols = [5, 3, 0, 4]                               # positions of 3, 4, 5 in the list: 1, 3, 0
        ctx.traj_config(1, cols)
        ctx.traj_record()
        _, cov, _ = ctx.traj_read()
        pos = {3: 1, 4: 3, 5: 0}
        for r in range(3):
            for c in range(r + 1):
                assert cov[0, 1, pos[3 + r], pos[3 + c]] == P3[r, c] == cov[0, 1, pos[3 + c], pos[3 + r]], (r, c)
        Pd = ctx.download_P()
        low = np.tril(Pd[1]) + np.tril(Pd[1], -1).T
        assert np.array_equal(cov[0, 1], low[cols][:, cols]) and np.array_equal(cov[0, 0], Pd[0][cols][:, cols])


def test_slices_order_and_full_log(built):
    rng = np.random.default_rng(13)
    B = 5
    with _context(rng, B) as ctx:
        ctx.upload_P(_spd(rng, B))
        ctx.traj_config(3, COLS6)
        stamps = [5_000_000_000, 5_040_000_000, (1 << 40) + 7]
        frames = []
        for k, t in enumerate(stamps):
            if k == 1:
                ctx.p_zero_rc(2, 14, 1)                   # a recorded column of filter 2 goes to zero
            if k == 2:
                _set_poses(ctx, _poses(rng, B))
            assert ctx.traj_record(t) == k
            frames.append((ctx.get_scene()[0], ctx.download_P()))
        recs, cov, ts = ctx.traj_read()
        assert ts.tolist() == stamps and recs.shape == (3, B)
        for k, (poses, Pd) in enumerate(frames):
            assert np.array_equal(recs[k]["Rsb"], poses["Rsb"]) and np.array_equal(recs[k]["Tsb"], poses["Tsb"])
            for b in range(B):
                assert np.array_equal(cov[k, b], Pd[b][COLS6][:, COLS6]), (k, b)
        assert cov[0, 2, 2, 2] != 0 and not cov[1, 2, 2].any() and not cov[1, 2, :, 2].any()
        assert not np.array_equal(recs[1]["Tsb"], recs[2]["Tsb"])
        r2, c2, t2 = ctx.traj_read(b0=1, nb=3, t0=1, nt=2)
        assert _same(r2, recs[1:3, 1:4]) and _same(c2, cov[1:3, 1:4]) and t2.tolist() == stamps[1:]
        # a full log takes nothing more
        k = np.zeros(1, dtype=np.int32) - 1
        assert ctx.lib.xivo_hip_traj_record(ctx.h, B, 99, k.ctypes.data) == L.ERR_FULL and k[0] == -1
        assert ctx.traj_count() == 3
        r3, c3, t3 = ctx.traj_read()
        assert _same(r3, recs) and _same(c3, cov) and t3.tolist() == stamps
        # slices outside what is recorded, bad configurations: status codes, the log stays as it is
        buf = np.zeros(4 * B * L.traj_dtype.itemsize, dtype=np.uint8)
        for b0, nb, t0, nt in ((0, B + 1, 0, 1), (-1, 1, 0, 1), (0, 1, 0, 4), (0, 1, 3, 1), (0, 1, -1, 1), (4, 2, 0, 1)):
            assert ctx.lib.xivo_hip_traj_read(ctx.h, b0, nb, t0, nt, buf.ctypes.data, None, None) == -1, (b0, nb, t0, nt)
        for n_cols, cols in ((0, []), (33, list(range(32))), (2, [0, N]), (2, [-1, 0]), (3, [4, 9, 4])):
            o = np.zeros(1, dtype=L.traj_opts_dtype)
            o["T_max"], o["n_cols"] = 2, n_cols
            o["cols"][0, :len(cols)] = cols
            assert ctx.lib.xivo_hip_traj_config(ctx.h, o.ctypes.data) == -1, (n_cols, cols)
        assert ctx.lib.xivo_hip_traj_config(ctx.h, None) == -1 and ctx.lib.xivo_hip_traj_record(ctx.h, B + 1, 0, None) == -1
        assert ctx.traj_count() == 3 and np.array_equal(ctx.traj_read()[1], cov)
        # reset: count 0, the memory is kept, frame 0 is used again
        live = ctx.ctx_allocs()
        ctx.traj_reset()
        assert ctx.traj_count() == 0 and ctx.ctx_allocs() == live
        assert ctx.traj_record(77) == 0
        r4, c4, t4 = ctx.traj_read()
        assert t4.tolist() == [77] and _same(r4[0], recs[2]) and _same(c4[0], cov[2])


def test_unconfigured_context_returns_a_status(built):
    rng = np.random.default_rng(14)
    with _context(rng, 2) as ctx:
        buf = np.zeros(1024)
        assert ctx.lib.xivo_hip_traj_record(ctx.h, 2, 0, None) == -1
        assert ctx.lib.xivo_hip_traj_count(ctx.h) == -1 and ctx.lib.xivo_hip_traj_reset(ctx.h) == -1
        assert ctx.lib.xivo_hip_traj_read(ctx.h, 0, 1, 0, 0, buf.ctypes.data, None, None) == -1
        assert ctx.lib.xivo_hip_traj_nees(ctx.h, 0, 1, 0, 0, buf.ctypes.data, None, None, None, None) == -1
        ctx.traj_config(0)                                # releasing nothing is fine
    with L.Context(64, 16, 2) as ctx:                     # no layout, so no resident poses to record
        ctx.traj_config(2, [0, 1])
        assert ctx.lib.xivo_hip_traj_record(ctx.h, 2, 0, None) == -1 and ctx.traj_count() == 0


def test_allocation_accounting(built):
    rng = np.random.default_rng(15)
    B = 3
    with _context(rng, B) as ctx:
        ctx.upload_P(_spd(rng, B))
        live0, bytes0 = ctx.ctx_allocs()
        ctx.traj_config(4, list(range(6)))
        live1, bytes1 = ctx.ctx_allocs()
        assert live1 == live0 + 2 and bytes1 == bytes0 + 4 * B * (L.traj_dtype.itemsize + 21 * 8)
        ctx.traj_config(2, list(range(6)))                # reconfiguring replaces the blocks
        assert ctx.ctx_allocs() == (live0 + 2, bytes0 + 2 * B * (L.traj_dtype.itemsize + 21 * 8)) and ctx.traj_count() == 0
        ctx.traj_record()
        ctx.traj_nees(np.tile(np.eye(3), (1, B, 1, 1)), np.zeros((1, B, 3)))      # (its staging is the context's too)
        assert ctx.ctx_allocs()[0] == live0 + 3
        ctx.traj_config(0)
        assert ctx.ctx_allocs() == (live0, bytes0)
        assert ctx.lib.xivo_hip_traj_count(ctx.h) == -1


def test_after_a_real_frame(built):
    """propagate -> filter_update -> absorb on a small scene, then record: the record is the resident state, exactly"""
    from test_sequence_gpu import _start
    cfg = sequence.SequenceConfig(n_groups=5, n_features=14)
    B = 4
    poses, P0, rng = _start(cfg, B, 3)
    hb = sequence.HipBackend(cfg, B, poses, P0)
    try:
        ops = []
        fx, cx, cy = cfg.cam["fx"], cfg.cam["cx"], cfg.cam["cy"]
        for b in range(B):
            for g in range(2):
                ops.append(sequence._op(b, L.EDIT_ADD_GROUP, g))
            for q, j in enumerate(rng.permutation(cfg.n_features)[:6 + 2 * b]):
                xp = rng.uniform([80, 60], [560, 420])
                x = [(xp[0] - cx) / fx, (xp[1] - cy) / fx, np.log(rng.uniform(1.0, 6.0))]
                A = rng.normal(size=(3, 3)) * 0.01
                ops.append(sequence._op(b, L.EDIT_ADD_FEATURE, int(j), int(j), q % 2,
                                        v=np.concatenate([x, xp + rng.normal(size=2), (A @ A.T + 1e-5 * np.eye(3)).reshape(-1)])))
        hb.edit(np.array(ops, dtype=L.edit_dtype))
        imu = np.zeros((B, 1), dtype=L.imu_dtype)
        imu["gyro"], imu["accel"], imu["dt"] = [0.01, -0.02, 0.03], [0.1, 0.0, 9.8], 0.01
        before = hb.scene()[0]
        hb.propagate(imu)
        mask = hb.update()
        assert mask.any()
        cols = list(range(15)) + [cfg.N - 1, 23, 29]
        hb.enable_trajectory_log(2, cols)
        assert hb.record(40_000_000) == 0
        recs, cov, ts = hb.ctx.traj_read()
        _same_state(recs[0], hb.ctx)
        assert np.array_equal(recs[0]["status"], hb.last_status)
        assert not np.array_equal(recs[0]["Tsb"], before["Tsb"])      # (the frame moved the state)
        Pd = hb.covariance()
        for b in range(B):
            low = np.tril(Pd[b]) + np.tril(Pd[b], -1).T
            assert np.array_equal(cov[0, b], low[cols][:, cols]), b
        tj = hb.trajectory()
        R, T = hb.poses()
        assert np.array_equal(tj["Rsb"][0], R) and np.array_equal(tj["Tsb"][0], T) and tj["ts"].tolist() == [40_000_000]
    finally:
        hb.close()


def test_nees_against_the_longdouble_reference(built):
    """7 filters, 2 frames: Sigma blocks with cond from 1e1 to 1e6 on random orthogonal bases placed in P[0:6, 0:6], est poses
    and gt = retract(est, e) for known e with rotation errors from 0.05 to 0.5 rad.

    Bounds (eps = 2^-52): err6 against e to 64 eps max(1, |e|) - the exp / log round trip; nees against the longdouble
    reference to 50 eps cond(Sigma) relative - the first-order bound of a 6 x 6 Cholesky solve, cond from the reference's own
    eigenvalues of each block; anees against the mean of the finite entries to 8 eps B relative. The reference takes the
    same fp64 est / gt the device is given. The errors are not smaller than 0.05 because R_est^T R_gt is formed in fp64 with
    an absolute error of about eps per entry whatever the angle: the relative error of the rotation part of e is
    ~3 eps / |e|, and it enters nees about doubled; below |e| ~ 0.1 / sqrt(cond) that would exceed the solve's bound although
    the solve is not at fault."""
    rng = np.random.default_rng(16)
    B, T = 7, 2
    cols = [9, 4, 0, 52, 2, 5, 1, 3]                      # the pose columns scattered over the list
    conds = np.geomspace(1e1, 1e6, B * T).reshape(T, B)
    sizes = np.geomspace(0.05, 0.5, B * T)[rng.permutation(B * T)].reshape(T, B)
    bad = (1, 3)                                          # this (frame, filter) gets an indefinite block
    Sig = np.zeros((T, B, 6, 6)); e_known = np.zeros((T, B, 6))
    est = [_poses(rng, B) for _ in range(T)]
    gt_R = np.zeros((T, B, 3, 3)); gt_T = np.zeros((T, B, 3))
    for t in range(T):
        for b in range(B):
            eig = np.geomspace(1.0, conds[t, b], 6) * 1e-4
            if (t, b) == bad:
                eig[2] = -eig[2]
            Sig[t, b] = tr.spd_with_spectrum(rng, eig[rng.permutation(6)])
            w = rng.normal(size=3)
            e_known[t, b] = np.concatenate([w * sizes[t, b] / np.linalg.norm(w), rng.normal(size=3) * sizes[t, b]])
            Rg, Tg = tr.retract(est[t][b]["Rsb"].reshape(3, 3).T, est[t][b]["Tsb"], e_known[t, b])
            gt_R[t, b], gt_T[t, b] = Rg.astype(np.float64), Tg.astype(np.float64)
    with _context(rng, B, est[0]) as ctx:
        ctx.traj_config(T, cols)
        for t in range(T):
            P = _spd(rng, B)
            P[:, :6, :6] = Sig[t]
            ctx.upload_P(P)
            _set_poses(ctx, est[t])
            ctx.traj_record(t)
        _, cov, _ = ctx.traj_read()
        pos = [cols.index(k) for k in range(6)]
        assert np.array_equal(cov[:, :, pos][:, :, :, pos], Sig)
        err6, nees, anees, used = ctx.traj_nees(gt_R, gt_T)
        again = ctx.traj_nees(gt_R, gt_T)
        for a, b_ in zip((err6, nees, anees, used), again):
            assert a.tobytes() == b_.tobytes()            # same bits, NaN included
        worst = {"err6": 0.0, "nees": 0.0}
        for t in range(T):
            for b in range(B):
                e = e_known[t, b]
                d = float(np.max(np.abs(err6[t, b] - e))) / max(1.0, float(np.linalg.norm(e)))
                worst["err6"] = max(worst["err6"], d / tr.EPS)
                assert d <= 64 * tr.EPS, (t, b, d / tr.EPS)
                if (t, b) == bad:
                    assert np.isnan(nees[t, b])
                    continue
                e_ref = tr.pose_error(est[t][b]["Rsb"].reshape(3, 3).T, est[t][b]["Tsb"], gt_R[t, b], gt_T[t, b])
                ref = tr.nees_solve(Sig[t, b], e_ref)
                lam = np.linalg.eigvalsh(Sig[t, b])
                c = float(lam[-1] / lam[0])
                rel = abs(float(nees[t, b] - ref)) / float(ref)
                worst["nees"] = max(worst["nees"], rel / (tr.EPS * c))
                print("nees t %d b %d cond %.2e |e_rot| %.3f ref %.6e rel %.2e = %.2f eps cond" % (t, b, c, sizes[t, b], float(ref), rel, rel / (tr.EPS * c)))
                assert rel <= 50 * tr.EPS * c, (t, b, c, rel)
        print("worst: err6 %.2f eps, nees %.2f eps cond" % (worst["err6"], worst["nees"]))
        assert used.tolist() == [B, B - 1]
        for t in range(T):
            fin = nees[t][np.isfinite(nees[t])]
            assert abs(anees[t] - fin.astype(np.longdouble).mean()) <= 8 * tr.EPS * B * fin.mean()
        # a slice scores the same entries
        e2, n2, a2, u2 = ctx.traj_nees(gt_R[1:, 2:5], gt_T[1:, 2:5], b0=2, t0=1)
        assert e2.tobytes() == err6[1:, 2:5].tobytes() and n2.tobytes() == nees[1:, 2:5].tobytes() and u2.tolist() == [2]
        # without the pose columns in the log there is nothing to score
        ctx.traj_config(T, [0, 1, 2, 3, 4, 7])
        ctx.traj_record()
        gt = np.zeros((1, B, 12))
        assert ctx.lib.xivo_hip_traj_nees(ctx.h, 0, B, 0, 1, gt.ctypes.data, None, None, None, None) == -1


@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_frame_mean_is_the_stated_tree_bit_for_bit(built, B):
    """anees / n_used of xivo_hip_traj_nees against tests/traj_restate.py frame_mean_tree on the very nees values the call
    returns: below, at and above one pass of the 256 threads and above two. Filters 0, 256 (where there is one), the last one
    and a few between have a pose block that is not positive definite in one of the frames, so their nees is NaN and the
    filter must be skipped, not added. Additions and one division in a fixed order: the bound is equality. With B = 1 the only
    filter is such a one: nothing is finite, n_used = 0 and anees is NaN."""
    rng = np.random.default_rng(160 + B)
    T = 1 if B == 1 else 2
    bad = [sorted({0, B - 1} | ({256} if B > 256 else set()) | set(rng.integers(0, B, size=3).tolist())),
           sorted({B // 2, B - 1})][:T]
    est = [_poses(rng, B) for _ in range(T)]
    gt_R = np.zeros((T, B, 3, 3)); gt_T = np.zeros((T, B, 3))
    with _context(rng, B, est[0]) as ctx:
        ctx.traj_config(T, list(range(6)))
        for t in range(T):
            P = _spd(rng, B)
            P[bad[t], 2, 2] *= -1.0                          # a negative third pivot
            ctx.upload_P(P)
            _set_poses(ctx, est[t])
            ctx.traj_record(t)
            for b in range(B):
                e = rng.normal(size=6) * 0.1
                Rg, Tg = tr.retract(est[t][b]["Rsb"].reshape(3, 3).T, est[t][b]["Tsb"], e)
                gt_R[t, b], gt_T[t, b] = Rg.astype(np.float64), Tg.astype(np.float64)
        _, nees, anees, used = ctx.traj_nees(gt_R, gt_T)
    for t in range(T):
        assert np.flatnonzero(~np.isfinite(nees[t])).tolist() == bad[t]
        mean, n = tr.frame_mean_tree(nees[t])
        print("B %d frame %d: n_used %d (restated %d) anees %r (restated %r)" % (B, t, used[t], n, anees[t], mean))
        assert used[t] == n == B - len(bad[t])
        if n == 0:
            assert np.isnan(anees[t])
        else:
            assert anees[t].tobytes() == mean.tobytes()


def test_drivers_return_the_same_trajectory_with_the_log(built):
    """run_pcw / run_pcw_batch with trajectory_log: the estimates come from one read of the log at the end and equal the
    per-frame downloads of the run without it; scripts/run_pcw.py -traj-log reports a finite anees_pose."""
    B, total = 2, 0.4                                     # 10 camera frames
    cfg = sequence.SequenceConfig()
    runs = {}
    for on in (False, True):
        worlds = [pcw.RandomPCW(seed=10 + b) for b in range(B)]
        sims = [pcw.TrajectorySim("trefoil" if b == 1 else "lissajous", seed=200 + b) for b in range(B)]
        runs[on] = sequence.run_pcw(sequence.HipBackend, cfg, worlds, sims, total_time=total, trajectory_log=on)
        runs[on]["backend"].close()
    off, on = runs[False], runs[True]
    assert off["Tsb"].shape == (10, B, 3) and "trajectory" not in off
    assert np.array_equal(on["Tsb"], off["Tsb"]) and np.array_equal(on["Wsb"], off["Wsb"]) and np.array_equal(on["ts"], off["ts"])
    assert np.array_equal(on["trajectory"]["ts"], on["ts"]) and on["trajectory"]["cov"].shape == (10, B, 15, 15)
    assert on["anees"].shape == (10,) and np.isfinite(on["anees"]).all() and on["nees_used"].tolist() == [B] * 10
    assert np.abs(on["err6"][:, :, 3:] - (on["gt_Tsb"] - on["Tsb"])).max() == 0
    batch = {}
    for flag in (False, True):
        batch[flag] = sequence.run_pcw_batch(cfg, B, total_time=total, trajectory_log=flag)
        batch[flag]["estimator"].close()
    assert np.array_equal(batch[True]["Tsb"], batch[False]["Tsb"]) and batch[True]["anees"].shape == (10,)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-sequences", str(B), "-total_time", str(total),
                        "-traj-log"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print("anees_pose", rep["anees_pose"], "run_pcw anees per frame", np.round(on["anees"], 3))
    assert np.isfinite(rep["anees_pose"]) and rep["nees_not_spd"] == 0 and rep["frames_per_sequence"] == 10
