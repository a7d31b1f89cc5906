"""Landmark log on the device (xivo_hip_map_*): the copied fields are exact copies of the resident scene and of P's lower
triangle, the order is (score, pos), the world position and its covariance meet entrywise fp64 bounds against the longdouble
restatement of tests/map_restate.py, slices / the full-log status / the allocation accounting behave, and the landmark NEES
agrees with the restatement."""
import os

import numpy as np
import pytest

import map_restate as mr
import traj_restate as tr
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAM = dict(model=L.CAM_PINHOLE, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[])
# base shape: 3 groups, 6 feature slots, N = 59 - the padded leading dimension of P is 64 != N
BASE = dict(group_begin=23, n_groups=3, feature_begin=41, n_features=6)
# 70 feature slots: the sort and pass 2 cross a wave boundary (2 groups, N = 245)
WIDE = dict(group_begin=23, n_groups=2, feature_begin=35, n_features=70)


def _N(lay):
    return lay["feature_begin"] + 3 * lay["n_features"]


def _rot(rng):
    return mr.so3_exp(rng.normal(size=3)).astype(np.float64)


def _scene(rng, lay, B, present, invdepth):
    """random poses and anchors; present[b] = list positions that hold a feature. Slots are a random permutation of the list
    positions (pos != sind), features at random depths 0.5 .. 6 in front of their anchor cameras."""
    G, F = lay["n_groups"], lay["n_features"]
    poses = np.zeros(B, dtype=L.pose_dtype)
    groups = np.zeros((B, G), dtype=L.group_dtype)
    feats = np.zeros((B, F), dtype=L.feat_dtype)
    feats["sind"] = -1
    for b in range(B):
        poses[b]["Rsb"] = _rot(rng).T.reshape(-1); poses[b]["Rbc"] = _rot(rng).T.reshape(-1)
        poses[b]["Rsg"] = np.eye(3).reshape(-1)
        poses[b]["Tsb"], poses[b]["Tbc"] = rng.normal(size=3), rng.normal(size=3) * 0.3
        for g in range(G):
            groups[b, g]["Rsb"] = _rot(rng).T.reshape(-1); groups[b, g]["Tsb"] = rng.normal(size=3) * 2
        slots = rng.permutation(F)
        for j in present[b]:
            z = rng.uniform(0.5, 6.0)
            feats[b, j]["x"] = [rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), 1 / z if invdepth else np.log(z)]
            feats[b, j]["xp"] = rng.uniform([0, 0], [640, 480])
            feats[b, j]["sind"], feats[b, j]["ref_sind"] = slots[j], rng.integers(0, G)
    return poses, groups, feats


def _spd(rng, B, n):
    out = []
    for _ in range(B):
        A = rng.uniform(-1, 1, size=(n, n))
        P = A @ A.T / n + 1e-3 * np.eye(n)
        out.append(np.tril(P) + np.tril(P, -1).T)
    return np.array(out)


def _context(lay, B, invdepth=False):
    ctx = L.Context(_N(lay), 2 * lay["n_features"], B, flags=L.FLAG_INVDEPTH if invdepth else 0)
    ctx.set_layout(_N(lay), lay["group_begin"], lay["n_groups"], lay["feature_begin"], lay["n_features"], CAM)
    return ctx


def _check_filter(pts, n, rec, n_out, world, worst):
    """one filter's device entries [n_out] and count against the restated record (best first, at most n_out entries)"""
    assert n == len(rec)
    for e, r in enumerate(rec):
        p = pts[e]
        assert (p["pos"], p["sind"], p["ref_sind"], p["reserved"]) == (r["pos"], r["sind"], r["ref_sind"], 0), e
        assert p["cov_local"].tobytes() == r["cov_local"].tobytes() and p["xp"].tobytes() == r["xp"].tobytes(), e
        u = abs(float(mr.LD(p["score"]) - r["score"])) / float(np.spacing(p["score"]))
        dX = np.abs(mr.LD(1) * p["Xs"] - r["Xs"]) / (mr.EPS * r["Xs_mag"])
        worst["score_ulp"] = max(worst["score_ulp"], u); worst["Xs"] = max(worst["Xs"], float(dX.max()))
        assert u <= 4, (e, u)
        assert float(dX.max()) <= 32, (e, dX)
        if world:
            dC = np.abs(mr.LD(1) * p["cov_world"] - r["cov_world"]) / (mr.EPS * r["cov_world_mag"])
            worst["cov_world"] = max(worst["cov_world"], float(dC.max()))
            assert float(dC.max()) <= 64, (e, dC)
        else:
            assert not p["cov_world"].any()
    tail = pts[n:]
    assert (tail["pos"] == -1).all() and (tail["sind"] == -1).all() and not tail["ref_sind"].any() and not tail["reserved"].any()
    for k in ("Xs", "cov_local", "cov_world", "xp", "score"):
        assert not tail[k].any(), k


RAGGED = [list(range(6)), [], [4], [0, 1, 3, 4, 5], list(range(6))]      # all, none, one, an absent entry in the middle, ties


def _ragged_case(rng, invdepth, blocks=True):
    """B = 5 on the base shape. With `blocks` every feature block of P is overwritten with a NON-symmetric 3 x 3
    (xivo_hip_p_set_block3 stores it as given), so the lower triangle, the upper triangle and the score's nine entries can be
    told apart; filter 4 gets the same block in three slots: equal scores. Without: P stays symmetric positive definite."""
    B = 5
    ctx = _context(BASE, B, invdepth)
    poses, groups, feats = _scene(rng, BASE, B, RAGGED, invdepth)
    ctx.set_scene(poses, groups, feats)
    ctx.upload_P(_spd(rng, B, _N(BASE)))
    same = rng.uniform(0.01, 0.02, size=(3, 3)) + np.diag([0.05, 0.06, 0.07])
    for b in range(B if blocks else 0):
        scale = rng.permutation(6)
        for s in range(6):
            blk = rng.uniform(0.01, 0.02, size=(3, 3)) + np.diag([0.05, 0.06, 0.07]) * (1 + 0.3 * scale[s])
            if b == 4 and s in (feats[4, 1]["sind"], feats[4, 2]["sind"], feats[4, 5]["sind"]):
                blk = same
            ctx.p_set_block3(b, BASE["feature_begin"] + 3 * s, blk)
    return ctx, poses, groups, feats


@pytest.mark.parametrize("invdepth", [False, True], ids=["logz", "invdepth"])
def test_record_against_the_restatement(built, invdepth):
    """Bounds (eps = 2^-52, magnitudes from the restatement): |dXs| <= 32 eps (|Rsb_g| (|Rbc| |Xc| + |Tbc|) + |Tsb_g|),
    |d cov_world| <= 64 eps (|J| |Pcc| |J|^T) entrywise - the ~50 roundings of a 15-term double congruence on a computed J;
    score within 4 ulp (a pairwise tree of nine squares and a square root); everything copied is bit-identical."""
    rng = np.random.default_rng(21 + int(invdepth))
    ctx, poses, groups, feats = _ragged_case(rng, invdepth)
    worst = dict(score_ulp=0.0, Xs=0.0, cov_world=0.0)
    with ctx:
        Pd = ctx.download_P()
        assert not np.array_equal(Pd[0], Pd[0].T)                  # (the stored triangles differ)
        sc, gr, ft = ctx.get_scene()
        assert sc.tobytes() == poses.tobytes() and ft.tobytes() == feats.tobytes()
        kept = {}
        for n_out in (8, 4):                                        # above every count (zero-filled tail) / below it
            ctx.map_config(2, n_out)
            assert ctx.map_record(5) == 0
            pts, n_pts, ts = ctx.map_read()
            assert pts.shape == (1, 5, n_out) and ts.tolist() == [5]
            assert n_pts[0].tolist() == [min(len(p), n_out) for p in RAGGED]
            for b in range(5):
                rec = mr.record(poses[b], groups[b], feats[b], Pd[b], BASE, n_out, invdepth)
                _check_filter(pts[0, b], int(n_pts[0, b]), rec, n_out, True, worst)
            kept[n_out] = pts
        assert kept[4].tobytes() == kept[8][:, :, :4].tobytes()      # the best four are the first four of the best eight
        # order: distinct scores are separated by far more than rounding, the three equal blocks of filter 4 go by position
        for b in range(5):
            full = mr.record(poses[b], groups[b], feats[b], Pd[b], BASE, 8, invdepth)
            s = [float(e["score"]) for e in full]
            assert s == sorted(s)
            for a, c in zip(full, full[1:]):
                assert a["score"] == c["score"] or float(c["score"] - a["score"]) > 1e-9 * float(c["score"])
        tie = [e["pos"] for e in mr.record(poses[4], groups[4], feats[4], Pd[4], BASE, 8, invdepth)
               if e["sind"] in (feats[4, 1]["sind"], feats[4, 2]["sind"], feats[4, 5]["sind"])]
        assert tie == [1, 2, 5]
        p4 = kept[8][0, 4]
        i1, i2, i5 = (int(np.nonzero(p4["pos"] == j)[0][0]) for j in (1, 2, 5))
        assert i2 == i1 + 1 and i5 == i2 + 1 and p4["score"][i1] == p4["score"][i2] == p4["score"][i5]
        # without the flag: no world covariance, nothing to score
        ctx.map_config(1, 8, world_cov=False)
        ctx.map_record()
        pts, n_pts, _ = ctx.map_read()
        for b in range(5):
            rec = mr.record(poses[b], groups[b], feats[b], Pd[b], BASE, 8, invdepth, world=False)
            _check_filter(pts[0, b], int(n_pts[0, b]), rec, 8, False, worst)
        for k in ("Xs", "cov_local", "xp", "score", "pos", "sind", "ref_sind"):      # every other field: the same bits
            assert pts[k].tobytes() == kept[8][k].tobytes(), k
        gt = np.zeros((1, 5, 8, 3))
        assert ctx.lib.xivo_hip_map_nees(ctx.h, 0, 5, 0, 1, gt.ctypes.data, None, None, None, None) == -1
    print("worst: score %.2f ulp, Xs %.2f eps mag, cov_world %.2f eps mag" % (worst["score_ulp"], worst["Xs"], worst["cov_world"]))


def test_seventy_feature_slots(built):
    """2 groups, 70 slots, N = 245, B = 2, n_out = 70: keys and kept entries beyond one wave's 64"""
    rng = np.random.default_rng(23)
    B, lay = 2, WIDE
    present = [list(range(70)), sorted(rng.permutation(70)[:37].tolist())]
    worst = dict(score_ulp=0.0, Xs=0.0, cov_world=0.0)
    with _context(lay, B) as ctx:
        poses, groups, feats = _scene(rng, lay, B, present, False)
        ctx.set_scene(poses, groups, feats)
        ctx.upload_P(_spd(rng, B, _N(lay)))
        Pd = ctx.download_P()
        ctx.map_config(1, 70)
        ctx.map_record()
        pts, n_pts, _ = ctx.map_read()
        assert n_pts[0].tolist() == [70, 37]
        for b in range(B):
            rec = mr.record(poses[b], groups[b], feats[b], Pd[b], lay, 70)
            assert sorted(e["pos"] for e in rec) == present[b]
            _check_filter(pts[0, b], int(n_pts[0, b]), rec, 70, True, worst)
    print("worst: score %.2f ulp, Xs %.2f eps mag, cov_world %.2f eps mag" % (worst["score_ulp"], worst["Xs"], worst["cov_world"]))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_slices_full_log_reset_and_bad_calls(built):
    rng = np.random.default_rng(24)
    B = 5
    ctx, poses, groups, feats = _ragged_case(rng, False)
    with ctx:
        ctx.map_config(3, 6)
        stamps = [5_000_000_000, 5_040_000_000, (1 << 40) + 7]
        for k, t in enumerate(stamps):
            if k == 1:                                            # the scene moves between the frames
                poses["Tbc"] += 0.25
                ctx.set_scene(poses, groups, feats)
            if k == 2:
                feats[0, 3]["sind"] = -1
                ctx.set_scene(poses, groups, feats)
            assert ctx.map_record(t) == k and ctx.map_count() == k + 1
        pts, n_pts, ts = ctx.map_read()
        assert ts.tolist() == stamps and pts.shape == (3, B, 6) and n_pts.shape == (3, B)
        assert n_pts[:, 0].tolist() == [6, 6, 5] and not _same(pts[0], pts[1]) and 3 not in pts[2, 0]["pos"].tolist()
        p2, n2, t2 = ctx.map_read(b0=1, nb=3, t0=1, nt=2)
        assert _same(p2, pts[1:3, 1:4]) and _same(n2, n_pts[1:3, 1:4]) and t2.tolist() == stamps[1:]
        # a full log takes nothing more
        k = np.zeros(1, dtype=np.int32) - 1
        assert ctx.lib.xivo_hip_map_record(ctx.h, B, 99, k.ctypes.data) == L.ERR_FULL and k[0] == -1
        assert ctx.map_count() == 3
        p3, n3, t3 = ctx.map_read()
        assert _same(p3, pts) and _same(n3, n_pts) and t3.tolist() == stamps
        # slices outside what is recorded, bad options: status codes, the log stays as it is
        buf = np.zeros(4 * B * 6 * L.map_pt_dtype.itemsize, dtype=np.uint8)
        for b0, nb, t0, nt in ((0, B + 1, 0, 1), (-1, 1, 0, 1), (0, 1, 0, 4), (0, 1, 3, 1), (0, 1, -1, 1), (4, 2, 0, 1)):
            assert ctx.lib.xivo_hip_map_read(ctx.h, b0, nb, t0, nt, buf.ctypes.data, None, None) == -1, (b0, nb, t0, nt)
        for T, n_out, flags in ((2, 0, 1), (2, L.MAP_MAX_OUT + 1, 1), (2, -3, 0), (-1, 4, 1), (2, 4, 2)):
            o = np.zeros(1, dtype=L.map_opts_dtype)
            o["T_max"], o["n_out"], o["flags"] = T, n_out, flags
            assert ctx.lib.xivo_hip_map_config(ctx.h, o.ctypes.data) == -1, (T, n_out, flags)
        assert ctx.lib.xivo_hip_map_config(ctx.h, None) == -1 and ctx.lib.xivo_hip_map_record(ctx.h, B + 1, 0, None) == -1
        assert ctx.map_count() == 3 and _same(ctx.map_read()[0], pts)
        # reset: count 0, the memory is kept, frame 0 is used again
        live = ctx.ctx_allocs()
        ctx.map_reset()
        assert ctx.map_count() == 0 and ctx.ctx_allocs() == live
        assert ctx.map_record(77) == 0
        p4, n4, t4 = ctx.map_read()
        assert t4.tolist() == [77] and _same(p4[0], pts[2]) and _same(n4[0], n_pts[2])


def test_unconfigured_context_returns_a_status(built):
    rng = np.random.default_rng(25)
    with _context(BASE, 2) as ctx:
        buf = np.zeros(4096)
        assert ctx.lib.xivo_hip_map_record(ctx.h, 2, 0, None) == -1
        assert ctx.lib.xivo_hip_map_count(ctx.h) == -1 and ctx.lib.xivo_hip_map_reset(ctx.h) == -1
        assert ctx.lib.xivo_hip_map_read(ctx.h, 0, 1, 0, 0, buf.ctypes.data, None, None) == -1
        assert ctx.lib.xivo_hip_map_nees(ctx.h, 0, 1, 0, 0, buf.ctypes.data, None, None, None, None) == -1
        ctx.map_config(0)                                         # releasing nothing is fine
        ctx.map_config(2, 4)                                      # configured, but no scene yet: nothing to record
        assert ctx.lib.xivo_hip_map_record(ctx.h, 2, 0, None) == -1 and ctx.map_count() == 0
    with L.Context(64, 16, 2) as ctx:                             # no layout: the log cannot be configured
        o = np.zeros(1, dtype=L.map_opts_dtype)
        o["T_max"], o["n_out"], o["flags"] = 2, 4, 1
        assert ctx.lib.xivo_hip_map_config(ctx.h, o.ctypes.data) == -1
    big = dict(group_begin=23, n_groups=1, feature_begin=29, n_features=129)      # more slots than the sorting network holds
    with L.Context(_N(big), 16, 1) as ctx:
        ctx.set_layout(_N(big), 23, 1, 29, 129, CAM)
        o = np.zeros(1, dtype=L.map_opts_dtype)
        o["T_max"], o["n_out"], o["flags"] = 2, 4, 1
        assert ctx.lib.xivo_hip_map_config(ctx.h, o.ctypes.data) == -5


def test_allocation_accounting(built):
    """two blocks through the context's owner: [T][B][n_out] entries of 160 bytes and [T][B] counts of 4; the NEES staging
    is a third; T_max = 0 gives everything back"""
    rng = np.random.default_rng(26)
    B = 5
    ctx, poses, groups, feats = _ragged_case(rng, False)
    with ctx:
        live0, bytes0 = ctx.ctx_allocs()
        ctx.map_config(4, 6)
        assert ctx.ctx_allocs() == (live0 + 2, bytes0 + 4 * B * (6 * L.map_pt_dtype.itemsize + 4))
        ctx.map_config(2, 3)                                      # reconfiguring replaces the blocks and empties the log
        assert ctx.ctx_allocs() == (live0 + 2, bytes0 + 2 * B * (3 * L.map_pt_dtype.itemsize + 4)) and ctx.map_count() == 0
        ctx.map_record()
        ctx.map_nees(np.zeros((1, B, 3, 3)))                      # (its staging is the context's too)
        assert ctx.ctx_allocs()[0] == live0 + 3
        ctx.map_config(0)
        assert ctx.ctx_allocs() == (live0, bytes0)
        assert ctx.lib.xivo_hip_map_count(ctx.h) == -1


def test_nees_against_the_restatement(built):
    """B = 5 ragged filters, 2 frames. Truth = the recorded Xs + a known error of about one standard deviation; one truth is
    NaN (skipped), filter 3 of frame 1 has a negative definite P (its Sigma is not positive definite: NaN, not counted); in
    every other entry P is positive definite and J has full row rank (its Tsb_g block is I), so Sigma is too. The
    restatement solves with the recorded fp64 Xs / cov_world in longdouble: 1e-9 relative leaves seven digits for
    cond(Sigma) of a 3 x 3 block of a well-conditioned P."""
    rng = np.random.default_rng(27)
    B = 5
    ctx, poses, groups, feats = _ragged_case(rng, False, blocks=False)
    with ctx:
        ctx.map_config(2, 6)
        ctx.map_record(1)
        Pn = ctx.download_P()
        Pn[3] = -Pn[3]
        ctx.upload_P(Pn)
        ctx.map_record(2)
        pts, n_pts, _ = ctx.map_read()
        gt = np.full((2, B, 6, 3), np.nan)
        for t in range(2):
            for b in range(B):
                for e in range(int(n_pts[t, b])):
                    S = mr.unpack6(pts[t, b, e]["cov_world"])
                    gt[t, b, e] = pts[t, b, e]["Xs"] + rng.normal(size=3) * np.sqrt(np.abs(np.diag(S)))
        gt[0, 0, 2] = np.nan                                      # no truth for this entry
        gt[0, 4, 1, 1] = np.nan                                   # (one component is enough)
        err3, nees, anees, used = ctx.map_nees(gt)
        again = ctx.map_nees(gt)
        for a, b_ in zip((err3, nees, anees, used), again):
            assert a.tobytes() == b_.tobytes()                    # same bits, NaN included
        ref = np.full((2, B, 6), np.nan, dtype=mr.LD)
        worst = 0.0
        for t in range(2):
            for b in range(B):
                for e in range(6):
                    if e >= n_pts[t, b] or not np.isfinite(gt[t, b, e]).all():
                        assert np.isnan(nees[t, b, e]) and np.isnan(err3[t, b, e]).all(), (t, b, e)
                        continue
                    assert np.array_equal(err3[t, b, e], gt[t, b, e] - pts[t, b, e]["Xs"])
                    ref[t, b, e] = mr.nees3(pts[t, b, e]["Xs"], pts[t, b, e]["cov_world"], gt[t, b, e])
                    if t == 1 and b == 3:
                        assert np.isnan(float(ref[t, b, e])) and np.isnan(nees[t, b, e])
                        continue
                    rel = abs(float(mr.LD(nees[t, b, e]) - ref[t, b, e])) / float(ref[t, b, e])
                    worst = max(worst, rel)
                    assert rel <= 1e-9, (t, b, e, rel)
        print("worst relative nees error %.2e" % worst)
        total = sum(len(p) for p in RAGGED)
        assert used.tolist() == [total - 2, total - len(RAGGED[3])]
        for t in range(2):
            m, n = mr.anees(ref[t])
            assert n == used[t] and abs(float(mr.LD(anees[t]) - m)) <= 1e-9 * float(m)
        assert np.isfinite(anees).all() and (anees > 0).all()
        # a slice scores the same entries
        e2, n2, a2, u2 = ctx.map_nees(gt[1:, 1:4], b0=1, t0=1)
        assert e2.tobytes() == err3[1:, 1:4].tobytes() and n2.tobytes() == nees[1:, 1:4].tobytes()
        assert u2.tolist() == [int(np.isfinite(nees[1, 1:4]).sum())]


def test_frame_mean_is_the_stated_tree_bit_for_bit(built):
    """anees / n_used of xivo_hip_map_nees against tests/traj_restate.py frame_mean_tree on the very nees values the call returns.
    9 filters of n_out = 30 slots: a frame is 270 values, one pass of the 256 threads and 14 of a second. Frame 0: filters with
    30, 17 and 0 features (the slots behind n_pts are NaN), one truth missing; frame 1: every P negated, so no Sigma is
    positive definite and nothing is finite - n_used = 0, anees NaN. Additions and one division in a fixed order: the bound
    is equality."""
    rng = np.random.default_rng(270)
    B, lay, n_out = 9, WIDE, 30
    present = [sorted(rng.permutation(70)[:k].tolist()) for k in (30, 70, 17, 0, 45, 30, 1, 29, 64)]
    with _context(lay, B) as ctx:
        poses, groups, feats = _scene(rng, lay, B, present, False)
        ctx.set_scene(poses, groups, feats)
        ctx.upload_P(_spd(rng, B, _N(lay)))
        ctx.map_config(2, n_out)
        ctx.map_record(1)
        ctx.upload_P(-ctx.download_P())
        ctx.map_record(2)
        pts, n_pts, _ = ctx.map_read()
        assert n_pts[0].tolist() == [min(len(p), n_out) for p in present]
        gt = pts["Xs"] + rng.normal(size=(2, B, n_out, 3)) * 0.05
        gt[0, 1, 3] = np.nan
        _, nees, anees, used = ctx.map_nees(gt)
    expect = sum(min(len(p), n_out) for p in present) - 1
    assert int(np.isfinite(nees[0]).sum()) == expect and not np.isfinite(nees[1]).any()
    mean, n = tr.frame_mean_tree(nees[0])
    print("frame 0: n_used %d (restated %d) anees %r (restated %r)" % (used[0], n, anees[0], mean))
    assert used[0] == n == expect and anees[0].tobytes() == mean.tobytes()
    mean, n = tr.frame_mean_tree(nees[1])
    assert used[1] == n == 0 and np.isnan(anees[1]) and np.isnan(mean)


def test_after_a_real_frame(built):
    """propagate -> filter_update -> absorb on a small scene, then record: the record is the restatement applied to the
    downloaded scene and covariance"""
    from test_sequence_gpu import _start
    cfg = sequence.SequenceConfig(n_groups=5, n_features=14)
    B = 4
    poses, P0, rng = _start(cfg, B, 3)
    hb = sequence.HipBackend(cfg, B, poses, P0)
    lay = dict(group_begin=23, n_groups=5, feature_begin=53, n_features=14)
    worst = dict(score_ulp=0.0, Xs=0.0, cov_world=0.0)
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
        hb.propagate(imu)
        assert hb.update().any()
        hb.enable_map_log(1)
        assert hb.record_map(40_000_000) == 0
        pts, n_pts, ts = hb.landmarks()
        assert ts.tolist() == [40_000_000] and pts.shape == (1, B, 14)
        sp, sg, sf = hb.scene()
        Pd = hb.covariance()
        assert n_pts[0].tolist() == [6 + 2 * b for b in range(B)]
        for b in range(B):
            rec = mr.record(sp[b], sg[b], sf[b], Pd[b], lay, 14)
            _check_filter(pts[0, b], int(n_pts[0, b]), rec, 14, True, worst)
    finally:
        hb.close()
    print("worst: score %.2f ulp, Xs %.2f eps mag, cov_world %.2f eps mag" % (worst["score_ulp"], worst["Xs"], worst["cov_world"]))


def test_drivers_report_the_map(built):
    """run_pcw_batch with map_log: the same final pose as without it, ids through the estimator's slot book, a finite
    positive anees_landmark (no band: nobody has measured it); run_pcw (python runner) likewise."""
    B, total = 4, 0.4                                             # 10 camera frames
    cfg = sequence.SequenceConfig()
    batch = {}
    for flag in (False, True):
        batch[flag] = sequence.run_pcw_batch(cfg, B, total_time=total, map_log=flag)
    try:
        off, on = batch[False], batch[True]
        assert "map" not in off and np.array_equal(on["Tsb"], off["Tsb"]) and on["Tsb"].shape == (10, B, 3)
        m = on["map"]
        assert m["pts"].shape == (10, B, cfg.n_features) and np.array_equal(m["ts"], on["ts"])
        est = on["estimator"]
        for b in range(B):                                        # the last frame against the slot book as it stands now
            fid = est.book(b)[0]
            n = int(m["n_pts"][-1, b])
            assert n == int((fid >= 0).sum()) and n > 0
            assert m["ids"][-1, b, :n].tolist() == [int(fid[p]) for p in m["pts"][-1, b, :n]["pos"]]
            assert (m["ids"][-1, b, :n] >= 10000).all() and (m["ids"][-1, b, n:] == -1).all()
            assert np.isfinite(m["gt"][-1, b, :n]).all()          # every in-state feature is a visible point of the world
        assert np.isfinite(on["anees_landmark"]) and on["anees_landmark"] > 0 and on["landmarks_scored_mean"] > 0
        assert on["landmarks_used"].shape == (10,) and on["landmark_nees"].shape == (10, B, cfg.n_features)
        print("run_pcw_batch anees_landmark %.3f, landmarks scored per sequence and frame %.2f, per frame %s" % (
            on["anees_landmark"], on["landmarks_scored_mean"], np.round(on["landmark_anees"], 3)))
    finally:
        for r in batch.values():
            r["estimator"].close()
    runs = {}
    for flag in (False, True):
        worlds = [pcw.RandomPCW(seed=10 + b) for b in range(2)]
        sims = [pcw.TrajectorySim("trefoil" if b == 1 else "lissajous", seed=200 + b) for b in range(2)]
        runs[flag] = sequence.run_pcw(sequence.HipBackend, cfg, worlds, sims, total_time=total, map_log=flag)
    try:
        assert np.array_equal(runs[True]["Tsb"], runs[False]["Tsb"]) and np.array_equal(runs[True]["Wsb"], runs[False]["Wsb"])
        m = runs[True]["map"]
        for b, bk in enumerate(runs[True]["runner"].books):
            n = int(m["n_pts"][-1, b])
            assert m["ids"][-1, b, :n].tolist() == [bk.feat_id[p] for p in m["pts"][-1, b, :n]["pos"]] and n == bk.n_instate()
        assert np.isfinite(runs[True]["anees_landmark"]) and runs[True]["anees_landmark"] > 0
        # the world error of a landmark is what the simulator says: gt - Xs
        ok = np.isfinite(runs[True]["landmark_err3"]).all(axis=-1)
        assert ok.any() and np.array_equal(runs[True]["landmark_err3"][ok], (m["gt"] - m["pts"]["Xs"])[ok])
    finally:
        for r in runs.values():
            r["backend"].close()


def test_pyxivo_positions_and_covs(built):
    """pyxivo.Estimator.InstateFeaturePositionsAndCovs (device route) against the host accessors of the same estimator:
    the same features, positions to fp64 rounding of two evaluations of Xs (2 x 32 eps of the magnitudes), the covariance
    blocks and pixels exactly, ascending block norm."""
    from xivo_amd import pyxivo
    cfg = pyxivo.config_from_cfg(pyxivo.load_json_with_comments(os.path.join(HERE, "golden", "pcw_like_cfg.json")))
    imu = pcw.TrajectorySim("lissajous", seed=41)
    cfg.X0["Vsb"] = imu.vel(0.0)
    vision = pcw.RandomPCW(seed=5)
    K = np.array([[275.0, 0, 320.0], [0, 275.0, 240.0], [0, 0, 1.0]])
    Rbc = pcw.so3_exp(cfg.Wbc)
    est = pyxivo.Estimator(cfg, "", "lissajous", False)
    est.InitWithSimDepths()
    try:
        assert est.InstateFeaturePositionsAndCovs(10)[0] == 0          # before the first camera frame
        total, imu_dt, every = 0.2, 0.0025, 16
        for k in range(int(round(total / imu_dt))):
            t = k * imu_dt; ts = int(round(t * 1e9))
            accel, gyro = imu.meas(t)
            est.InertialMeas(ts, gyro[0], gyro[1], gyro[2], accel[0], accel[1], accel[2])
            if k % every == 0:
                Rsb, Tsb = imu.gsb(t)
                ids, meas = vision.generate_measurements(Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb, K, 640, 480, 1.0)
                est.VisualMeasPointCloud(ts, ids, meas)
        count = est.num_instate_features()
        assert count > 4
        host_ids = est.InstateFeatureIDs().tolist()
        host_X, host_cov, host_px = est.InstateFeaturePositions(), est.InstateFeatureCovs(), est.InstateFeatureMeas()
        for max_output in (count + 5, 4):
            n, X, cov, px, ids = est.InstateFeaturePositionsAndCovs(max_output)
            assert n == min(count, max_output) and X.shape == (n, 3) and cov.shape == (n, 6) and px.shape == (n, 2) and ids.shape == (n,)
            assert len(set(ids.tolist())) == n and set(ids.tolist()) <= set(host_ids)
            norms = []
            sp, sg, sf = est._scene()
            for i in range(n):
                k = host_ids.index(int(ids[i]))
                C9 = host_cov[k].reshape(3, 3)
                j = est._runner.books[0].id2slot[int(ids[i])]
                grp = sg[sf[j]["ref_sind"]]
                mag = mr.world_point_magnitude(mr.R(sp["Rbc"]), sp["Tbc"], mr.R(grp["Rsb"]), grp["Tsb"], sf[j]["x"], False)
                assert np.all(np.abs(X[i] - host_X[k]) <= 64 * mr.EPS * mag.astype(np.float64)), i
                assert cov[i].tolist() == [C9[c, r] for r, c in mr.SYM6] and px[i].tolist() == host_px[k].tolist()
                norms.append(np.linalg.norm(C9))
            assert all(a <= b * (1 + 1e-12) for a, b in zip(norms, norms[1:]))
    finally:
        est.close()
