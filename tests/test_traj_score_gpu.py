"""Trajectory score on the device (xivo_hip_traj_score): aligned / unaligned ATE, the alignment and the RPE of logged poses
against the longdouble restatement of tests/score_restate.py at derived fp64 bounds, bit-identical slices, reflections,
degenerate shapes, left-out frames, lag edges, status codes, the drivers, and the reference's stored results.

Bounds (score_restate.bounds; eps = 2^-52, rho = rms |x - xbar| + rms |y - ybar|, kappa = sv0 / (sv1 + sv2)):
  |d ate|, |d ate_raw| <= 64 eps (rho + |xbar| + |ybar|);  |d R| <= 64 eps kappa;  |d T| <= 64 eps kappa |xbar| + 16 eps (|xbar| + |ybar|)
  |d sv| <= 32 eps sv0;  |d rpe_pos| <= 64 eps max |Tsb|;  |d rpe_rot| <= 64 eps + 64 eps max(1, max |log rot E|)
Every test prints the worst observed ratio to each bound."""
import os

import numpy as np
import pytest

import score_restate as sr
from test_traj_log_gpu import _context, _poses, _set_poses
from xivo_amd import formats, sequence
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 5
LD = np.longdouble


def _fill(ctx, rng, est_R, est_T, T_max=None):
    """log est_R [nt, nb, 3, 3] / est_T [nt, nb, 3] as frames 0 .. nt - 1 of filters 0 .. nb - 1 (no filter update needed)"""
    nt, nb = est_T.shape[:2]
    ctx.traj_config(nt if T_max is None else T_max, [0])
    poses = _poses(rng, ctx.batch)
    for t in range(nt):
        poses["Rsb"][:nb] = np.transpose(est_R[t], (0, 2, 1)).reshape(nb, 9)
        poses["Tsb"][:nb] = est_T[t]
        _set_poses(ctx, poses)
        ctx.traj_record(t)


def _trajectories(rng, nt, nb, noise=1e-2, offset=1e3):
    gt_R = np.zeros((nt, nb, 3, 3)); gt_T = np.zeros((nt, nb, 3)); est_R = np.zeros_like(gt_R); est_T = np.zeros_like(gt_T)
    for b in range(nb):
        gt_R[:, b], gt_T[:, b] = sr.smooth_trajectory(rng, nt, offset=offset)
        est_R[:, b], est_T[:, b] = sr.moved(rng, gt_R[:, b], gt_T[:, b], sr.rot(rng.normal(size=3)), rng.normal(size=3) * 2, noise)
    return est_R, est_T, gt_R, gt_T


def _compare(rec, ref, worst, tag, check_R=True):
    """one device record against one restatement dict under the derived bounds; worst[k] <- largest ratio seen"""
    bd = sr.bounds(ref)
    assert rec["n_used"] == ref["n_used"] and rec["n_pairs"] == ref["n_pairs"] and rec["flags"] == ref["flags"], tag

    def one(key, err, bound):
        ratio = float(err) / bound if bound > 0 else (0.0 if err == 0 else np.inf)
        worst[key] = max(worst.get(key, 0.0), ratio)
        assert ratio <= 1.0, (tag, key, float(err), bound, ratio)
    for k in ("ate", "ate_raw"):
        one(k, abs(LD(rec[k]) - ref[k]), bd["ate"])
    one("sv", np.abs(rec["sv"] - ref["sv"]).max(), bd["sv"])
    if check_R:
        one("R", np.abs(rec["R"].reshape(3, 3).T - ref["R"]).max(), bd["R"])
        one("T", np.abs(rec["T"] - ref["T"]).max(), bd["T"])
    if ref["n_pairs"] > 0:
        one("rpe_pos", abs(LD(rec["rpe_pos"]) - ref["rpe_pos"]), bd["rpe_pos"])
        one("rpe_rot", abs(LD(rec["rpe_rot"]) - ref["rpe_rot"]), bd["rpe_rot"])
    else:
        assert rec["rpe_pos"] == -1 and rec["rpe_rot"] == -1, tag


def _is_rotation(rec):
    R = rec["R"].reshape(3, 3).T.astype(LD)
    det = R[0] @ np.cross(R[1], R[2])
    return float(abs(det - 1)), float(np.abs(R.T @ R - np.eye(3)).max())


def _report(name, worst):
    print(name + " worst ratio to bound: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("nt", [3, 4, 63, 64, 65, 257])
def test_parity_with_the_restatement(built, nt):
    """gt: a smooth random trajectory about a point 1e3 from the origin (what breaks a one-pass sum); est: a rigid motion
    of it plus noise of 1e-2; align 0 / 1, lags 1 / 7"""
    rng = np.random.default_rng(100 + nt)
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    worst = {}
    with _context(rng, B) as ctx:
        _fill(ctx, rng, est_R, est_T)
        gt = sr.pack_gt(gt_R, gt_T)
        for align in (0, 1):
            for lag in (1, 7):
                out = ctx.traj_score(gt, align=align, rpe_lag=lag)
                assert out.shape == (B,) and not out["reserved"].any()
                for b in range(B):
                    ref = sr.score(est_R[:, b], est_T[:, b], gt_R[:, b], gt_T[:, b], align=bool(align), rpe_lag=lag)
                    assert ref["kappa"] <= 1e6 and 500 < ref["xbar_norm"] < 2000
                    assert ref["n_pairs"] == max(0, nt - lag)
                    _compare(out[b], ref, worst, (nt, align, lag, b))
                    if align:
                        assert out[b]["ate"] <= out[b]["ate_raw"]
                    else:
                        assert out[b]["ate"] == out[b]["ate_raw"] and np.array_equal(out[b]["R"].reshape(3, 3), np.eye(3)) and not out[b]["T"].any()
    _report("parity nt %d" % nt, worst)


def test_slices_are_bit_identical(built):
    rng = np.random.default_rng(21)
    nt = 12
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    with _context(rng, B) as ctx:
        _fill(ctx, rng, est_R, est_T, T_max=nt + 3)
        gt = sr.pack_gt(gt_R, gt_T)

        def call(b0, nb, t0, n):
            return ctx.traj_score(np.ascontiguousarray(gt[t0:t0 + n, b0:b0 + nb]), b0=b0, nb=nb, t0=t0, nt=n, align=True, rpe_lag=2)
        full = call(0, 5, 0, 12)
        assert call(0, 5, 0, 12).tobytes() == full.tobytes()                  # two calls, the same bytes
        assert call(2, 3, 0, 12).tobytes() == full[2:5].tobytes()
        tail = call(0, 5, 5, 7)
        assert call(4, 1, 5, 7).tobytes() == tail[4:5].tobytes() and tail.tobytes() != full.tobytes()
        last = call(0, 5, 11, 1)
        assert call(0, 1, 11, 1).tobytes() == last[0:1].tobytes()
        assert (full["n_used"] == 12).all() and (tail["n_used"] == 7).all() and (last["n_used"] == 1).all()
        assert (full["n_pairs"] == 10).all() and (tail["n_pairs"] == 5).all() and (last["n_pairs"] == 0).all()
        worst = {}
        for b in range(B):
            _compare(tail[b], sr.score(est_R[5:, b], est_T[5:, b], gt_R[5:, b], gt_T[5:, b], rpe_lag=2), worst, ("tail", b))
    _report("slices", worst)


def test_reflection_gets_a_rotation(built):
    """est = the mirror image of gt plus small noise: no rotation undoes it, the determinant correction has to act"""
    rng = np.random.default_rng(22)
    nt, noise = 8, 1e-3
    gt_T = rng.normal(size=(nt, B, 3)) + 5.0
    gt_R = np.tile(np.eye(3), (nt, B, 1, 1))
    est_T = gt_T * np.array([1.0, 1.0, -1.0]) + noise * rng.normal(size=gt_T.shape)
    worst = {}
    with _context(rng, B) as ctx:
        _fill(ctx, rng, gt_R, est_T)
        out = ctx.traj_score((gt_R, gt_T), align=True)
        for b in range(B):
            ref = sr.score(gt_R[:, b], est_T[:, b], gt_R[:, b], gt_T[:, b])
            assert ref["sv"][2] > 1e-3 * ref["sv"][0]                          # not coplanar: nowhere near the rounding of sv0
            d, o = _is_rotation(out[b])
            worst["det"] = max(worst.get("det", 0.0), d / (4 * sr.EPS)); worst["orth"] = max(worst.get("orth", 0.0), o / (8 * sr.EPS))
            assert d <= 4 * sr.EPS and o <= 8 * sr.EPS, (b, d / sr.EPS, o / sr.EPS)
            _compare(out[b], ref, worst, ("mirror", b))
            assert out[b]["ate"] > 10 * noise and out[b]["flags"] == 0
    _report("reflection", worst)


def test_degenerate_shapes(built):
    rng = np.random.default_rng(23)
    worst = {}
    # filters: 0, 1 collinear (est an exact rigid motion, so sv1 is rounding), 2, 3 coplanar with noise, 4 generic
    nt = 6
    gt_T = np.zeros((nt, B, 3)); gt_R = np.tile(np.eye(3), (nt, B, 1, 1)); est_T = np.zeros_like(gt_T)
    for b in range(B):
        c = rng.normal(size=3) * 10
        if b < 2:
            d = rng.normal(size=3)
            gt_T[:, b] = c + np.outer(rng.normal(size=nt), d)
        elif b < 4:
            u, v = rng.normal(size=3), rng.normal(size=3)
            gt_T[:, b] = c + np.outer(rng.normal(size=nt), u) + np.outer(rng.normal(size=nt), v)
        else:
            gt_T[:, b] = c + rng.normal(size=(nt, 3))
        est_T[:, b] = gt_T[:, b] @ sr.rot(rng.normal(size=3)).T + rng.normal(size=3)
        if b >= 2:
            est_T[:, b] += 1e-2 * rng.normal(size=(nt, 3))
    with _context(rng, B) as ctx:
        _fill(ctx, rng, gt_R, est_T)
        gt = sr.pack_gt(gt_R, gt_T)
        out6 = ctx.traj_score(gt, align=True, rpe_lag=1)
        for b in range(B):
            ref = sr.score(gt_R[:, b], est_T[:, b], gt_R[:, b], gt_T[:, b], rpe_lag=1)
            assert ref["flags"] == (1 if b < 2 else 0), b
            if b in (2, 3):
                assert ref["sv"][2] <= 1e-12 * ref["sv"][0] and ref["kappa"] <= 1e6
            _compare(out6[b], ref, worst, ("nt6", b), check_R=b >= 2)      # collinear: the minimum is unique, R is not
            d, o = _is_rotation(out6[b])
            assert d <= 4 * sr.EPS and o <= 8 * sr.EPS, (b, d / sr.EPS, o / sr.EPS)
        out2 = ctx.traj_score(np.ascontiguousarray(gt[:2]), nt=2, align=True, rpe_lag=1)
        out1 = ctx.traj_score(np.ascontiguousarray(gt[3:4]), t0=3, nt=1, align=True, rpe_lag=1)
        for b in range(B):
            ref = sr.score(gt_R[:2, b], est_T[:2, b], gt_R[:2, b], gt_T[:2, b], rpe_lag=1)
            assert out2[b]["flags"] & 1 and ref["flags"] == 1 and out2[b]["n_pairs"] == 1
            _compare(out2[b], ref, worst, ("nt2", b), check_R=False)
            d, o = _is_rotation(out2[b])
            assert d <= 4 * sr.EPS and o <= 8 * sr.EPS, (b, d / sr.EPS, o / sr.EPS)
            assert out1[b]["flags"] & 1 and out1[b]["ate"] == 0 and out1[b]["n_used"] == 1 and out1[b]["n_pairs"] == 0
            assert out1[b]["rpe_pos"] == -1 and out1[b]["rpe_rot"] == -1
            assert abs(out1[b]["ate_raw"] - np.linalg.norm(est_T[3, b] - gt_T[3, b])) <= 8 * sr.EPS * 40
            d, o = _is_rotation(out1[b])
            assert d <= 4 * sr.EPS and o <= 8 * sr.EPS
    _report("degenerate", worst)


def test_left_out_entries(built):
    rng = np.random.default_rng(24)
    nt = 12
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    est_T[3, 1, 2] = np.nan; est_T[7, 1, 0] = np.nan                          # filter 1: two frames of the log
    gt_clean = sr.pack_gt(gt_R, gt_T)
    gt_R[5, 3, 1, 1] = np.nan                                                 # filter 3: one ground-truth entry
    gt_T[:, 4] = np.inf                                                       # filter 4: nothing usable
    worst = {}
    with _context(rng, B) as ctx:
        _fill(ctx, rng, est_R, est_T)
        out = ctx.traj_score((gt_R, gt_T), align=True, rpe_lag=2)
        clean = ctx.traj_score(gt_clean, align=True, rpe_lag=2)
        for b in (0, 2):
            assert out[b:b + 1].tobytes() == clean[b:b + 1].tobytes()         # the other filters are unaffected
        for b in range(4):
            _compare(out[b], sr.score(est_R[:, b], est_T[:, b], gt_R[:, b], gt_T[:, b], rpe_lag=2), worst, ("nan", b))
        assert out["n_used"].tolist() == [12, 10, 12, 11, 0]
        assert out["n_pairs"].tolist() == [10, 6, 10, 8, 0]
        e = out[4]
        assert e["ate"] == -1 and e["ate_raw"] == -1 and e["n_used"] == 0 and e["rpe_pos"] == -1 and e["flags"] & 1
        assert np.array_equal(e["R"].reshape(3, 3), np.eye(3)) and not e["T"].any() and not e["sv"].any()
    _report("left out", worst)


def test_lag_edges(built):
    rng = np.random.default_rng(25)
    nt = 6
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    worst = {}
    with _context(rng, B) as ctx:
        _fill(ctx, rng, est_R, est_T)
        gt = sr.pack_gt(gt_R, gt_T)
        one = ctx.traj_score(gt, rpe_lag=nt - 1)
        assert (one["n_pairs"] == 1).all()
        for b in range(B):
            _compare(one[b], sr.score(est_R[:, b], est_T[:, b], gt_R[:, b], gt_T[:, b], rpe_lag=nt - 1), worst, ("lag", b))
        for lag in (0, nt, nt + 3):
            o = ctx.traj_score(gt, rpe_lag=lag)
            assert (o["n_pairs"] == 0).all() and (o["rpe_pos"] == -1).all() and (o["rpe_rot"] == -1).all()
            assert np.array_equal(o["ate"], one["ate"])
        opts = np.zeros(1, dtype=L.traj_score_opts_dtype); opts["align"], opts["rpe_lag"] = 1, -1
        out = np.zeros(B, dtype=L.traj_score_dtype)
        assert ctx.lib.xivo_hip_traj_score(ctx.h, 0, B, 0, nt, gt.ctypes.data, opts.ctypes.data, out.ctypes.data) == -1
        assert not out.view(np.uint8).any()
    _report("lag edges", worst)


def test_status_codes_and_allocations(built):
    rng = np.random.default_rng(26)
    nt = 4
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    gt = sr.pack_gt(gt_R, gt_T)
    opts = np.zeros(1, dtype=L.traj_score_opts_dtype); opts["align"] = 1
    out = np.zeros(B, dtype=L.traj_score_dtype); out["ate"] = 7.0
    with _context(rng, B) as ctx:
        def raw(b0, nb, t0, n, g=gt, o=opts, r=out):
            return ctx.lib.xivo_hip_traj_score(ctx.h, b0, nb, t0, n, g.ctypes.data if g is not None else None,
                                               o.ctypes.data if o is not None else None, r.ctypes.data if r is not None else None)
        live00, bytes00 = ctx.ctx_allocs()
        assert raw(0, B, 0, 0) == -1                                           # no log configured
        _fill(ctx, rng, est_R, est_T, T_max=nt + 2)
        live0, bytes0 = ctx.ctx_allocs()
        for b0, nb, t0, n in ((0, B, 0, nt + 1), (0, B, nt, 1), (0, B, -1, 1), (0, B + 1, 0, 1), (-1, 1, 0, 1), (4, 2, 0, 1), (0, 1, 0, -1)):
            assert raw(b0, nb, t0, n) == -1, (b0, nb, t0, n)
        assert raw(0, B, 0, nt, g=None) == -1 and raw(0, B, 0, nt, o=None) == -1 and raw(0, B, 0, nt, r=None) == -1
        assert raw(0, 0, 0, nt) == 0 and (out["ate"] == 7.0).all()             # nb = 0: fine, nothing written
        assert ctx.ctx_allocs() == (live0, bytes0)                             # none of these touched the device
        assert raw(0, B, 0, nt) == 0 and (out["n_used"] == nt).all()
        assert ctx.ctx_allocs() == (live0 + 1, bytes0 + nt * B * 96 + B * L.traj_score_dtype.itemsize)
        assert raw(1, 2, 1, 2, g=np.ascontiguousarray(gt[1:3, 1:3])) == 0      # a smaller call re-uses the staging
        assert ctx.ctx_allocs()[0] == live0 + 1
        assert raw(0, B, nt, 0) == 0 and (out["n_used"] == 0).all() and (out["ate"] == -1).all()      # an empty slice of frames
        ctx.traj_config(0)                                                     # the log goes, and its staging with it
        assert ctx.ctx_allocs() == (live00, bytes00)
        assert raw(0, B, 0, 0) == -1


def test_scratch_goes_with_the_context(built):
    """xivo_hip_destroy with the score's staging still held: the context's owner frees it with everything else. The hook
    reads a live context only (a destroyed one is no argument: -1 for NULL), so what is checked after the destroy is what the
    next context of the same shape owns: what a fresh one owned before, and after the same calls the same blocks again."""
    rng = np.random.default_rng(28)
    nt = 4
    est_R, est_T, gt_R, gt_T = _trajectories(rng, nt, B)
    gt = sr.pack_gt(gt_R, gt_T)
    with _context(rng, B) as ctx:
        fresh = ctx.ctx_allocs()
    ctx = _context(rng, B)
    assert ctx.ctx_allocs() == fresh
    _fill(ctx, rng, est_R, est_T)
    logged = ctx.ctx_allocs()
    first = ctx.traj_score(gt, rpe_lag=1)
    held = ctx.ctx_allocs()
    assert held == (logged[0] + 1, logged[1] + nt * B * 96 + B * L.traj_score_dtype.itemsize)       # the staging, accounted for
    lib = ctx.lib
    ctx.close()                                                                # xivo_hip_destroy, the staging still held
    assert ctx.h is None and lib.xivo_hip_selftest_ctx_allocs(None, None, None) == -1
    with _context(rng, B) as ctx:
        assert ctx.ctx_allocs() == fresh                                       # nothing of the destroyed context is left to this one
        _fill(ctx, rng, est_R, est_T)
        assert ctx.traj_score(gt, rpe_lag=1).tobytes() == first.tobytes()
        assert ctx.ctx_allocs() == held


def test_against_the_reference(built):
    """tests/golden/metrics_v1.npz: the device never above the reference's iterate (the closed form is the global minimum),
    two-sided within 4 x the gap measured between the reference and the restatement - the ATE and the alignment itself, R at
    4 x R_gap and T = ybar - R xbar at 3 |xbar| times that plus its own rounding, which ties the direction (gt onto est) and
    the column-major R of the record to the reference's gYX - RPE to 1e-10 relative"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics_v1.npz"))
    rng = np.random.default_rng(27)
    gap, R_gap = float(g["ate_gap"]), float(g["R_gap"])
    worst = {"ate_two_sided": 0.0, "rpe": 0.0, "R_ref": 0.0, "T_ref": 0.0}
    for nt in sorted(set(g["nt"].tolist())):
        idx = [i for i in range(len(g["nt"])) if g["nt"][i] == nt]
        for chunk in (idx[k:k + B] for k in range(0, len(idx), B)):
            nb = len(chunk)
            est_R = g["est_R"][chunk, :nt].transpose(1, 0, 2, 3); est_T = g["est_T"][chunk, :nt].transpose(1, 0, 2)
            gt = sr.pack_gt(g["gt_R"][chunk, :nt].transpose(1, 0, 2, 3), g["gt_T"][chunk, :nt].transpose(1, 0, 2))
            with _context(rng, B) as ctx:
                _fill(ctx, rng, est_R, est_T)
                ate = ctx.traj_score(np.ascontiguousarray(gt[:nt - 1]), nb=nb, nt=nt - 1, align=True)      # ComputeATE leaves the last pose out
                rpe = {lag: ctx.traj_score(gt, nb=nb, align=False, rpe_lag=lag) for lag in set(int(g["lag"][i]) for i in chunk)}
            for k, i in enumerate(chunk):
                assert ate[k]["n_used"] == g["n_ate"][i]
                assert ate[k]["ate"] <= g["ref_ate"][i] * (1 + 1e-9)
                two = abs(ate[k]["ate"] / g["ref_ate"][i] - 1)
                r = rpe[int(g["lag"][i])][k]
                rel = max(abs(r["rpe_pos"] / g["ref_rpe_pos"][i] - 1), abs(r["rpe_rot"] / g["ref_rpe_rot"][i] - 1))
                worst["ate_two_sided"] = max(worst["ate_two_sided"], two / (4 * gap)); worst["rpe"] = max(worst["rpe"], rel / 1e-10)
                n = int(g["n_ate"][i])
                xb, yb = np.linalg.norm(g["gt_T"][i, :n].mean(0)), np.linalg.norm(g["est_T"][i, :n].mean(0))
                dR = np.abs(ate[k]["R"].reshape(3, 3).T - g["ref_R"][i]).max() / (4 * R_gap)
                dT = np.abs(ate[k]["T"] - g["ref_T"][i]).max() / (4 * R_gap * 3 * xb + 16 * sr.EPS * (xb + yb))
                worst["R_ref"] = max(worst["R_ref"], dR); worst["T_ref"] = max(worst["T_ref"], dT)
                print("case %d nt %d: ate device %.15e reference %.15e rel %.2e (4 x gap = %.2e), rpe rel %.2e" %
                      (i, nt, ate[k]["ate"], g["ref_ate"][i], two, 4 * gap, rel))
                assert r["n_pairs"] == nt - g["lag"][i]
                assert two <= 4 * gap and rel <= 1e-10, (i, two, rel)
                assert dR <= 1.0 and dT <= 1.0, (i, dR, dT)
    _report("reference", worst)


def test_drivers_report_the_score(built):
    """run_pcw_batch with the log on returns the device's score per sequence; with the log off, exactly today's keys"""
    cfg = sequence.SequenceConfig()
    nseq, total = 4, 0.4                                                       # 10 camera frames
    on = sequence.run_pcw_batch(cfg, nseq, total_time=total, trajectory_log=True, rpe_dt=0.12)
    on["estimator"].close()
    off = sequence.run_pcw_batch(cfg, nseq, total_time=total)
    off["estimator"].close()
    assert set(off) == {"ts", "gt_Tsb", "estimator", "Tsb"} and np.array_equal(on["Tsb"], off["Tsb"])
    assert on["Tsb"].shape == (10, nseq, 3)
    for k in ("ate_aligned", "ate_raw", "rpe_pos", "rpe_rot"):
        assert on[k].shape == (nseq,) and np.isfinite(on[k]).all() and (on[k] >= 0).all(), k
    for b in range(nseq):
        assert on["ate_aligned"][b] <= on["ate_raw"][b] * (1 + 1e-12)
        host = formats.ate_rmse(on["Tsb"][:, b], on["gt_Tsb"][:, b], align=False)
        assert abs(on["ate_raw"][b] - host) <= 1e-12 * host, (b, on["ate_raw"][b], host)
        print("seq %d: ate_aligned %.4e ate_raw %.4e rpe_pos %.4e rpe_rot %.4e" % (b, on["ate_aligned"][b], on["ate_raw"][b],
                                                                                 on["rpe_pos"][b], on["rpe_rot"][b]))
