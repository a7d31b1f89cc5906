"""GPU: depth initialisation of new tracks - two-view triangulation (xivo_hip_triangulate, xivo_hip_pool_triangulation) and
AdaptInitialDepth (xivo_hip_pool_adapt_depth, xivo_hip_pool_add_ex).

The device triangulators are checked against the numpy restatement of src/helpers.cpp:103-371 (tests/tri_restate.py, which
test_depth_init_cpu.py pins to the compiled reference); the pool's triangulation against the stand-alone entry point followed
by the host-array sub-filter path, bit for bit; AdaptInitialDepth against np.sort(d)[n // 2]."""
import numpy as np
import pytest

import tri_restate as T
from test_feature_pool_gpu import CAMS, NG, N, RBC, TBC, cm, context, empty_feats, perturb, pose_records, project_np
from xivo_amd import lib as L, pcw, synth
from xivo_amd.lib import Context, XivoHipError

pytestmark = pytest.mark.gpu

TH, BE = 0.1 * T.DEG, 0.25 * T.DEG
KINDS = ("good", "lowpar", "behind", "noisy", "degenerate", "threshold")


# ---------------------------------------------------------------- stand-alone triangulation vs the restatement
@pytest.mark.parametrize("method", T.METHODS)
def test_triangulate_matches_the_restatement(built, method):
    rng = np.random.default_rng(7)
    excluded = 0
    n_ill = [0]
    with Context(64, 16, 1) as ctx:
        for kind in KINDS:
            R12, t12, xc1, xc2, Xt, clean = T.random_problems(rng, 4000, kind)
            X, ret, good = ctx.triangulate(R12, t12, xc1, xc2, method, zmin=0.05, zmax=5.0, max_theta_thresh=TH, beta_thresh=BE)
            Xh, reth, info = T.triangulate(method, R12, t12, xc1, xc2, TH, BE, details=True)
            near = T.near_threshold(method, info, len(Xh), TH, BE)
            excluded += int(near.sum())
            assert np.array_equal(ret[~near], reth[~near]), (kind, int((ret != reth)[~near].sum()))
            fin = np.isfinite(Xh).all(axis=1)
            cond_ok = fin.copy()
            if method == "direct_linear_transform_svd":
                s = info["sigma"]
                cond_ok &= s[:, 2] / s[:, 0] >= 1e-3                      # the null vector is well defined
                n_ill[0] += int((~cond_ok).sum())
            if method == "direct_linear_transform_avg":
                cond_ok &= np.abs(np.linalg.norm(Xh, axis=1)) < 1e6
            # the depth test on X: where X is defined (the angular methods: always - same IEEE sequence on both sides)
            cmp = ~near & (cond_ok if method.startswith("direct") else np.ones_like(near))
            zgap = np.abs(Xh[:, 2] - 0.05) <= 1e-9 * 0.05
            zgap |= np.abs(Xh[:, 2] - 5.0) <= 1e-9 * 5.0
            cmp &= ~zgap
            assert np.array_equal(good[cmp], T.good(reth, Xh, 0.05, 5.0)[cmp]), (kind, int((good != T.good(reth, Xh, 0.05, 5.0))[cmp].sum()))
            scale = np.maximum(np.linalg.norm(Xh, axis=1), 1e-300)
            rel = np.linalg.norm(X - Xh, axis=1) / scale
            if kind in ("good", "behind", "noisy", "threshold"):
                assert rel[cond_ok].max(initial=0.0) <= 1e-10, (kind, rel[cond_ok].max())
            if clean and kind == "good":
                assert np.abs(X - Xt).max() <= 1e-8, kind                  # noise-free: the true point
    print(f"{method}: {excluded} return values excluded (within 1e-6 of a float threshold or at acos's domain edge); "
          f"{n_ill[0]} DLT problems with sigma3 / sigma1 < 1e-3")


def test_reference_unit_cases_on_the_device(built):
    """src/test/unittest_triangulation.cpp: Normal_Inputs passes with |z - 5| <= 0.5 for the three angular methods, the
    other cases fail - Angular_Reprojection_Error as tests/test_depth_init_cpu.py explains it"""
    with Context(64, 16, 1) as ctx:
        for case in T.UNIT_CASES:
            R12, t12, xc1, xc2 = T.unit_case(case)
            for m in T.ANGULAR:
                X, ret, _ = ctx.triangulate(R12[None], t12[None], xc1[None], xc2[None], m, max_theta_thresh=TH, beta_thresh=BE)
                Xh, reth = T.triangulate(m, R12[None], t12[None], xc1[None], xc2[None], TH, BE)
                assert ret[0] == reth[0], (case[0], m)
                if case[0] == "Normal_Inputs":
                    assert ret[0] and abs(X[0, 2] - 5.0) <= 0.5, m
                elif case[0] != "Angular_Reprojection_Error":
                    assert not ret[0], (case[0], m)


def test_triangulate_arguments(built):
    with Context(64, 16, 1) as ctx:
        one = np.eye(3)[None], np.array([[0.3, 0.0, 0.0]]), np.zeros((1, 2)), np.array([[0.1, 0.0]])
        for bad in (L.TRI_OFF, 6, -1):
            with pytest.raises(XivoHipError):
                ctx.triangulate(*one, bad)
        o = L.tri_options("l1_angular")
        o["struct_size"] = 32
        out = np.zeros(1, dtype=L.tri_out_dtype)
        pin = np.zeros(1, dtype=L.tri_in_dtype)
        assert ctx.lib.xivo_hip_triangulate(ctx.h, 1, L._ptr(pin), L._ptr(out), L._ptr(o)) == -1
        assert ctx.lib.xivo_hip_triangulate(ctx.h, 0, None, None, L._ptr(L.tri_options("l1_angular"))) == 0
        with pytest.raises(XivoHipError):
            ctx.pool_triangulation("l1_angular")           # no pool configured


# ---------------------------------------------------------------- the pool: triangulation at the first step
def pool_scene(rng, B, pm, cam, cams, invdepth, A=2, calib=False):
    """context with unlinked anchors 0..A-1 at perturbed poses and a pool of new tracks: points in front of their anchor
    camera, first pixel = their projection there, this frame's pixel = their projection from the current pose (+ noise)"""
    flags = L.FLAG_INVDEPTH if invdepth else 0
    poses = pose_records(rng, B)
    anchor_poses = [perturb(poses, rng, 0.05) for _ in range(A)]
    ctx = context(B, cam, flags)
    groups = np.zeros((B, NG), dtype=L.group_dtype)
    groups["Rsb"] = cm(np.eye(3))
    ctx.set_scene(poses, groups, empty_feats(B))
    if calib:
        set_intrinsics(ctx, cams)
    opts = dict(Rtri=3.5 ** 2, MH_thresh=5.991, ready_steps=1, min_depth=0.05, max_depth=8.0, max_subfilter_outlier=0.5)
    ctx.pool_config(pm, A, remove_outlier_counter=100.0, **opts)
    for a in range(A):
        ctx.set_scene(anchor_poses[a], groups, empty_feats(B))
        ctx.pool_anchor(np.full(B, a, dtype=np.int32))
    ctx.set_scene(poses, groups, empty_feats(B))
    recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
    recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B)
    recs["anchor"] = rng.integers(0, A, B * pm)
    keep = rng.random(B * pm) < 0.8
    Xa = np.stack([rng.uniform(-0.6, 0.6, B * pm), rng.uniform(-0.5, 0.5, B * pm), rng.uniform(0.8, 6.0, B * pm)], axis=1)
    xp_now = np.full((B, pm, 2), np.nan)
    for i in range(B * pm):
        b, e, a = recs["b"][i], recs["entry"][i], recs["anchor"][i]
        c = cams[b]
        recs["xp"][i] = project_np(c, Xa[i, 0] / Xa[i, 2], Xa[i, 1] / Xa[i, 2])
        Ra, Ta = anchor_poses[a][b]["Rsb"].reshape(3, 3).T, anchor_poses[a][b]["Tsb"]
        Rs, Ts = poses[b]["Rsb"].reshape(3, 3).T, poses[b]["Tsb"]
        Xs = Ra @ (RBC @ Xa[i] + TBC) + Ta                      # world point
        Xc = RBC.T @ (Rs.T @ (Xs - Ts) - TBC)                   # current camera
        if Xc[2] > 0.1 and keep[i]:
            xp_now[b, e] = np.array(project_np(c, Xc[0] / Xc[2], Xc[1] / Xc[2])) + rng.normal(size=2) * 0.3
    recs["z0"] = 2.5; recs["std_xyz"] = [0.002, 0.002, 0.5]
    keep &= np.isfinite(xp_now.reshape(-1, 2)[:, 0])
    ctx.pool_add(recs[keep])
    return ctx, poses, anchor_poses, groups, recs, keep, xp_now, opts


def set_intrinsics(ctx, cams):
    dim = {0: 4, 1: 5, 2: 9, 3: 8}[cams[0]["model"]]
    ctx.set_calib(cam_begin=23, cam_dim=dim)
    cal = np.zeros(len(cams), dtype=L.calib_dtype)
    for b, c in enumerate(cams):
        cal[b]["intr"] = L.cam_intr(c); cal[b]["Cg"] = cm(np.eye(3)); cal[b]["Ca"] = cm(np.eye(3))
    ctx.set_calib_state(cal)


def g12_restated(pose, anc):
    """pool_kernels.hip pool_g12 in plain fp64, same association, no contraction: bit for bit"""
    Rsb, Rbc, Ra0 = pose["Rsb"], pose["Rbc"], anc["Rsb"]           # column-major 9
    Tbc, Tsb, Tsa = pose["Tbc"], pose["Tsb"], anc["Tsb"]
    Rc, Ra, Tc, Ta = np.zeros(9), np.zeros(9), np.zeros(3), np.zeros(3)
    for i in range(3):
        for j in range(3):
            Rc[i + 3 * j] = (Rsb[i] * Rbc[3 * j] + Rsb[i + 3] * Rbc[1 + 3 * j]) + Rsb[i + 6] * Rbc[2 + 3 * j]
            Ra[i + 3 * j] = (Ra0[i] * Rbc[3 * j] + Ra0[i + 3] * Rbc[1 + 3 * j]) + Ra0[i + 6] * Rbc[2 + 3 * j]
        Tc[i] = ((Rsb[i] * Tbc[0] + Rsb[i + 3] * Tbc[1]) + Rsb[i + 6] * Tbc[2]) + Tsb[i]
        Ta[i] = ((Ra0[i] * Tbc[0] + Ra0[i + 3] * Tbc[1]) + Ra0[i + 6] * Tbc[2]) + Tsa[i]
    d = Tc - Ta
    R12, t12 = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            R12[i, j] = (Ra[3 * i] * Rc[3 * j] + Ra[1 + 3 * i] * Rc[1 + 3 * j]) + Ra[2 + 3 * i] * Rc[2 + 3 * j]
        t12[i] = (Ra[3 * i] * d[0] + Ra[1 + 3 * i] * d[1]) + Ra[2 + 3 * i] * d[2]
    return R12, t12


def run_pool_tri(B, pm, cam_name, per_filter, invdepth, method, seed):
    cam = CAMS[cam_name]
    rng = np.random.default_rng(seed)
    cams = []
    for b in range(B):
        c = dict(cam)
        if per_filter:
            c.update(fx=cam["fx"] * (1 + 0.01 * (b % 7)), fy=cam["fy"] * (1 - 0.01 * (b % 5)), cx=cam["cx"] + b % 3, cy=cam["cy"] - b % 4)
        cams.append(c)
    ctx, poses, anchor_poses, groups, recs, keep, xp, opts = pool_scene(rng, B, pm, cam, cams, invdepth, calib=per_filter)
    with ctx:
        ent0, apose, aslot = ctx.pool_get()
        live = ent0["ref_sind"] >= 0
        assert (aslot == -1).all()
        ctx.pool_triangulation(method, zmin=0.05, zmax=5.0, max_theta_thresh=TH, beta_thresh=BE)
        order, n, live_d = ctx.pool_step(xp, False)
        ent, _, _ = ctx.pool_get()
        good_d, bad_d = ctx.pool_tri_counts()
        # stand-alone: g12 restated, xc2 = the device's un-projection of this frame's pixel (pool_add on a scratch context)
        bb, ee = np.nonzero(live)
        R12 = np.zeros((len(bb), 3, 3)); t12 = np.zeros((len(bb), 3))
        for k, (b, e) in enumerate(zip(bb, ee)):
            R12[k], t12[k] = g12_restated(poses[b], apose[b, ent0["ref_sind"][b, e]])
        flags = L.FLAG_INVDEPTH if invdepth else 0
        with context(B, cam, flags) as sc:
            sc.set_scene(poses, groups, empty_feats(B))
            if per_filter:
                set_intrinsics(sc, cams)
            sc.pool_config(pm, 1)
            sc.pool_anchor(np.zeros(B, dtype=np.int32))
            r = np.zeros(len(bb), dtype=L.pool_new_dtype)
            r["b"], r["entry"], r["xp"], r["z0"] = bb, ee, xp[bb, ee], 1.0
            sc.pool_add(r)
            xc2 = sc.pool_get()[0]["x"][bb, ee, :2]
            X, ret, good = ctx.triangulate(R12, t12, ent0["x"][bb, ee, :2], xc2, method, zmin=0.05, zmax=5.0,
                                           max_theta_thresh=TH, beta_thresh=BE)
            # x of a good triangulation: (X/z, Y/z, log z) - log z through the device's pool_add (same libm call)
            z = np.where(good, X[:, 2], 1.0)
            r["xp"] = xp[bb, ee]; r["z0"] = z
            sc.pool_add(r)
            xz = sc.pool_get()[0]["x"][bb, ee, 2]
        assert np.array_equal(good_d, np.bincount(bb[good], minlength=B)) and np.array_equal(bad_d, np.bincount(bb[~good], minlength=B))
        host = ent0.copy()
        host["x"][bb[good], ee[good], 0] = X[good, 0] / z[good]
        host["x"][bb[good], ee[good], 1] = X[good, 1] / z[good]
        host["x"][bb[good], ee[good], 2] = xz[good]
        # host-array sub-filter step from those states, anchor poses in scene slots 0..A-1
        g2 = groups.copy()
        g2[:, :apose.shape[1]] = apose
        ctx.set_scene(poses, g2, empty_feats(B))
        sub = host.copy()
        sub["xp"] = np.where(np.isnan(xp), 0.0, xp)
        sub["ref_sind"] = np.where(live, host["ref_sind"], 0)
        upd = ctx.subfilter_update(sub, **opts)
        assert np.array_equal(live_d, live)
        for f in ("x", "P", "xp", "outlier_counter", "score", "status", "init_counter", "candidate"):
            assert np.array_equal(ent[f][live], upd[f][live]), f          # bit for bit
        return int(good.sum()), int((~good).sum())


@pytest.mark.parametrize("B,pm,cam,per_filter,invdepth,method", [
    (3, 40, "pinhole", False, False, "l1_angular"), (17, 64, "pinhole", True, True, "l1_angular"),
    (9, 48, "equi", True, False, "l2_angular"), (9, 48, "radtan", False, True, "linf_angular"),
    (9, 48, "atan", True, False, "direct_linear_transform_svd"), (5, 30, "radtan", True, False, "direct_linear_transform_avg"),
    (1024, 8, "pinhole", False, False, "l1_angular"), (2, 512, "equi", False, True, "l1_angular")])
def test_pool_triangulation_is_standalone_then_host_path(built, B, pm, cam, per_filter, invdepth, method):
    ng, nb = run_pool_tri(B, pm, cam, per_filter, invdepth, method, seed=B + pm)
    assert ng > 0 and nb > 0, (ng, nb)
    print(f"{method} B={B} pm={pm} {cam}: {ng} good / {nb} bad triangulations")


def test_pool_triangulation_off_is_bit_identical(built):
    """enabled, then disabled before the step = never enabled"""
    outs = []
    for toggle in (False, True):
        rng = np.random.default_rng(3)
        cams = [CAMS["pinhole"]] * 6
        ctx, poses, _, groups, _, _, xp, _ = pool_scene(rng, 6, 32, CAMS["pinhole"], cams, False)
        with ctx:
            if toggle:
                ctx.pool_triangulation("l1_angular")
                ctx.pool_triangulation(None)
            res = ctx.pool_step(xp, False)
            xp2 = xp + 0.5
            res2 = ctx.pool_step(xp2, True)
            outs.append((res, res2, ctx.pool_get()[0], ctx.pool_tri_counts()))
    (a1, a2, ea, ca), (b1, b2, eb, cb) = outs
    for u, v in zip(a1 + a2, b1 + b2):
        assert np.array_equal(u, v)
    assert ea.tobytes() == eb.tobytes()
    assert (ca[0] == 0).all() and (cb[0] == 0).all() and (cb[1] == 0).all()


# ---------------------------------------------------------------- AdaptInitialDepth
def adapt_setup(rng, B, pm, F, invdepth):
    flags = L.FLAG_INVDEPTH if invdepth else 0
    cam = CAMS["pinhole"]
    cams = [cam] * B
    ctx, poses, _, groups, _, keep, xp, opts = pool_scene(rng, B, pm, cam, cams, invdepth)
    # two steps: ready_steps = 1 makes entries READY at init_counter 2
    ctx.pool_step(xp, False)
    xp = np.where(rng.random((B, pm, 1)) < 0.1, np.nan, xp + rng.normal(size=xp.shape) * 0.3)
    ctx.pool_step(xp, False)
    # ragged in-state feature lists: filter b has b % (F + 1) features
    feats = np.zeros((B, F), dtype=L.feat_dtype)
    feats["sind"] = -1
    for b in range(B):
        k = b % (F + 1)
        z = rng.uniform(0.5, 8.0, k)
        feats[b, :k]["sind"] = np.arange(k); feats[b, :k]["ref_sind"] = 0
        feats[b, :k]["x"] = np.stack([rng.normal(size=k) * 0.1, rng.normal(size=k) * 0.1, 1.0 / z if invdepth else np.log(z)], 1)
    ctx.set_scene(poses, groups, feats)
    return ctx, feats


def expected_depths(feats, ent, min_life, invdepth):
    f = feats[feats["sind"] >= 0]["x"][:, 2]
    sel = (ent["ref_sind"] >= 0) & (ent["status"] == 1)                  # XIVO_FEAT_READY
    sel &= ent["init_counter"] > min_life
    p = ent[sel]["x"][:, 2]
    x = np.concatenate([f, p])
    return 1.0 / x if invdepth else np.exp(x)


@pytest.mark.parametrize("invdepth", [False, True])
def test_adapt_depth_is_the_median_update(built, invdepth):
    rng = np.random.default_rng(5 + invdepth)
    B, pm, F = 37, 64, 4
    ctx, feats = adapt_setup(rng, B, pm, F, invdepth)
    with ctx:
        ent, _, _ = ctx.pool_get()
        beta, min_z, max_z, z0 = 0.7, 0.3, 4.0, 2.5
        with pytest.raises(XivoHipError):
            ctx.pool_adapt_depth()                              # not configured
        # every live entry has init_counter 2 here: lifetime 2 excludes them all (the test is `>`), 1 keeps them
        ctx.pool_adapt_depth_config(z0, median_weight=beta, min_feature_lifetime=2, min_z=min_z, max_z=max_z)
        zl = ctx.pool_adapt_depth()
        ctx.pool_adapt_depth_config(z0, median_weight=beta, min_feature_lifetime=1, min_z=min_z, max_z=max_z)
        z1 = ctx.pool_adapt_depth()
        z2 = ctx.pool_adapt_depth()
        # every median out of [min_z, max_z]: init_z stays (config resets it to initial_z)
        ctx.pool_adapt_depth_config(z0, median_weight=beta, min_feature_lifetime=1, min_z=100.0, max_z=200.0)
        z3 = ctx.pool_adapt_depth()
    assert (z3 == z0).all()
    live = ent["ref_sind"] >= 0
    assert (ent["init_counter"][live] == 2).all() and (ent["status"][live] == 1).any()
    differ = 0
    for b in range(B):
        d = expected_depths(feats[b], ent[b], 2, invdepth)
        want = z0
        if len(d) and min_z <= np.sort(d)[len(d) // 2] <= max_z:
            want = (1 - beta) * z0 + beta * np.sort(d)[len(d) // 2]
        assert abs(zl[b] - want) <= 4e-16 * max(want, 1.0), (b, zl[b], want)
        differ += int(len(d) != len(expected_depths(feats[b], ent[b], 1, invdepth)))
    assert differ > 0
    branches = set()
    for b in range(B):
        d = expected_depths(feats[b], ent[b], 1, invdepth)
        want, want2 = z0, z0
        if len(d):
            m = np.sort(d)[len(d) // 2]
            if min_z <= m <= max_z:
                want = (1 - beta) * z0 + beta * m
                want2 = (1 - beta) * z1[b] + beta * m
                branches.add("update")
            else:
                branches.add("out of range")
        else:
            branches.add("empty")
        assert abs(z1[b] - want) <= 4e-16 * max(want, 1.0), (b, z1[b], want)
        assert abs(z2[b] - want2) <= 4e-16 * max(want2, 1.0), (b, z2[b], want2)
    assert "update" in branches, branches


def test_adapt_depth_empty_set_and_pool_add_ex(built):
    rng = np.random.default_rng(9)
    cam = CAMS["pinhole"]
    with context(3, cam) as ctx:
        ctx.set_scene(pose_records(rng, 3), np.zeros((3, NG), dtype=L.group_dtype), empty_feats(3))
        ctx.pool_config(8, 2)
        ctx.pool_anchor(np.zeros(3, dtype=np.int32))
        recs = np.zeros(3, dtype=L.pool_new_dtype)
        recs["b"] = [0, 1, 2]; recs["entry"] = 4; recs["xp"] = [[300.0, 200.0]] * 3; recs["z0"] = 1.7
        recs["std_xyz"] = [0.01, 0.01, 0.3]
        with pytest.raises(XivoHipError):
            ctx.pool_add_ex(recs, L.POOL_ADD_ADAPTIVE_Z)        # no init_z yet
        with pytest.raises(XivoHipError):
            ctx.pool_add_ex(recs, 2)                            # unknown option bit
        ctx.pool_adapt_depth_config(3.25, median_weight=0.99, min_feature_lifetime=5, min_z=0.05, max_z=5.0)
        assert np.array_equal(ctx.pool_adapt_depth(), [3.25] * 3)   # empty depth set: init_z stays
        ctx.pool_add_ex(recs, 0)
        e0 = ctx.pool_get()[0][:, 4].copy()
        r2 = recs.copy(); r2["entry"] = 5; r2["z0"] = 0.0              # ignored with the flag
        ctx.pool_add_ex(r2, L.POOL_ADD_ADAPTIVE_Z)
        e1 = ctx.pool_get()[0][:, 5].copy()
    with context(3, cam) as ref:
        ref.set_scene(pose_records(np.random.default_rng(9), 3), np.zeros((3, NG), dtype=L.group_dtype), empty_feats(3))
        ref.pool_config(8, 2)
        ref.pool_anchor(np.zeros(3, dtype=np.int32))
        ref.pool_add(recs)
        r3 = recs.copy(); r3["entry"] = 5; r3["z0"] = 3.25
        ref.pool_add(r3)
        e = ref.pool_get()[0]
    assert e0.tobytes() == e[:, 4].tobytes() and e1.tobytes() == e[:, 5].tobytes()


# ---------------------------------------------------------------- end to end: the "subfilter" life cycle with both options
import os                                                           # noqa: E402

from xivo_amd import formats, sequence                             # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ATE_BOUND = 0.8          # the bound test_feature_pool_gpu.py states for the "subfilter" life cycle


def depth_init_cfg(**kw):
    """initial_z deliberately wrong (the PCW scenes' landmarks lie 2-8 m away); both options on, TUM-VI's values"""
    c = dict(feature_init="subfilter", initial_z=0.6, initial_std_z=0.5, max_group_lifetime=60,
             subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2), pool_max=128, anchor_max=16,
             triangulate_pre_subfilter=True, adaptive_initial_depth=True,
             adaptive_depth=dict(median_weight=0.99, minimum_feature_lifetime=2),
             initial_std_x_badtri=2.0, initial_std_y_badtri=2.0, initial_std_z_badtri=1.0)
    c.update(kw)
    return sequence.SequenceConfig(**c)


def test_cpp_batch_estimator_depth_init_equals_python_runner(built):
    """BatchEstimator::EnableDepthInit takes the Python runner's decisions every frame with both options on"""
    B = 4
    cfg = depth_init_cfg()
    mk = lambda: ([pcw.RandomPCW(seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    w1, s1 = mk()
    py = sequence.run_pcw(sequence.HipBackend, cfg, w1, s1, total_time=1.2)
    w2, s2 = mk()
    cp = sequence.run_pcw_cpp(cfg, w2, s2, total_time=1.2)
    try:
        run = py["runner"]
        for b in range(B):
            fid, fref, gref = cp["estimator"].book(b)
            bk = run.books[b]
            assert list(fid) == bk.feat_id and list(fref) == bk.feat_ref and list(gref) == bk.group_refs
        st = cp["estimator"].stats()
        assert st["admitted"] == len(run.admitted) > 0 and st["pool_dropped"] == run.n_pool_dropped
        assert st["updates"] == run.n_updates and st["mh_rejected"] == run.n_rejected
        assert np.abs(run.init_z - cp["estimator"].init_z()).max() <= 1e-10 * np.abs(run.init_z).max()
        assert np.abs(py["Tsb"] - cp["Tsb"]).max() < 1e-10 and np.abs(py["Wsb"] - cp["Wsb"]).max() < 1e-10
        g, bad = py["backend"].tri_counts()
        assert g.sum() > 0 and bad.sum() > 0
    finally:
        py["backend"].close(); cp["estimator"].close()


def test_depth_init_batch_equals_single_runs(built):
    B = 12
    cfg = depth_init_cfg(pool_max=64)
    worlds = lambda: [pcw.RandomPCW(seed=b) for b in range(B)]
    sims = lambda: [pcw.TrajectorySim("lissajous" if b % 2 == 0 else "trefoil", rate=0.08 + 0.001 * b, seed=300 + b)
                    for b in range(B)]
    out = sequence.run_pcw(sequence.HipBackend, cfg, worlds(), sims(), total_time=0.8)
    try:
        T, W, Z = out["Tsb"], out["Wsb"], out["runner"].init_z.copy()
        P = out["backend"].covariance()
    finally:
        out["backend"].close()
    ws, ss = worlds(), sims()
    for b in range(B):
        o1 = sequence.run_pcw(sequence.HipBackend, cfg, [ws[b]], [ss[b]], total_time=0.8)
        try:
            assert np.array_equal(o1["Tsb"][:, 0], T[:, b]) and np.array_equal(o1["Wsb"][:, 0], W[:, b]), b
            assert np.array_equal(o1["backend"].covariance()[0], P[b]) and o1["runner"].init_z[0] == Z[b], b
        finally:
            o1["backend"].close()


def test_pyxivo_client_loop_with_triangulation_and_adaptive_depth(built):
    """the pyxivo client loop from a cfg dict with both options on (TUM-VI's keys, initial_z wrong): init_z moves toward
    the scene's median depth, the pose error stays within the life cycle's bound"""
    from xivo_amd import pyxivo
    raw = pyxivo.load_json_with_comments(os.path.join(HERE, "golden", "pcw_like_cfg.json"))
    raw.update({"initial_z": 0.6, "initial_std_z": 0.5, "max_group_lifetime": 60, "triangulate_pre_subfilter": True,
                "triangulation": {"method": "l1_angular", "zmin": 0.05, "zmax": 10.0, "max_theta_thresh": 0.1,
                                  "beta_thesh": 0.25},
                "initial_std_x_badtri": 2.0, "initial_std_y_badtri": 2.0, "initial_std_z_badtri": 1.0,
                "adaptive_initial_depth": {"median_weight": 0.99, "minimum_feature_lifetime": 2},
                "subfilter": {"visual_meas_std": 3.5, "MH_thresh": 8.991, "ready_steps": 2}})
    cfg = pyxivo.config_from_cfg(raw)
    assert cfg.triangulate_pre_subfilter and cfg.adaptive_initial_depth
    cfg.pool_max, cfg.anchor_max = L.POOL_MAX_ENTRIES, 64
    imu = pcw.TrajectorySim("lissajous", seed=41)
    cfg.X0["Vsb"] = imu.vel(0.0)
    vision = pcw.RandomPCW(seed=5)
    K = np.array([[275.0, 0, 320.0], [0, 275.0, 240.0], [0, 0, 1.0]])
    est = pyxivo.Estimator(cfg, "", "lissajous", False)
    total, imu_dt, vis_dt = 2.4, 0.0025, 0.04
    packets = [(k * imu_dt, 0) for k in range(int(round(total / imu_dt)))] + [(k * vis_dt, 1) for k in range(int(round(total / vis_dt)))]
    packets.sort(key=lambda p: (round(p[0] * 1e9), p[1]))
    est_T, gt_T, zs = [], [], []
    try:
        for t, kind in packets:
            ts = int(round(t * 1e9))
            if kind == 0:
                accel, gyro = imu.meas(t)
                est.InertialMeas(ts, gyro[0], gyro[1], gyro[2], accel[0], accel[1], accel[2])
            else:
                Rsb, Tsb = imu.gsb(t)
                ids, meas = vision.generate_measurements(Rsb @ RBC, Rsb @ cfg.Tbc + Tsb, K, 640, 480, 1.0)
                est.VisualMeasPointCloud(ts, ids, meas)
                est_T.append(est.gsb()[:, 3]); gt_T.append(Tsb)
                zs.append(float(est._runner.init_z[0]))
                last_depths = meas[:, 2]
        run = est._runner
        assert run.admitted and est.num_instate_features() > 5
        good, bad = est._be.tri_counts()
        _, _, feats = est._be.scene()
        f = feats[0][feats[0]["sind"] >= 0]
        m = np.median(np.exp(f["x"][:, 2]))
        print("depth init: init_z", zs[0], "->", zs[-1], "in-state median depth", m, "scene median", np.median(last_depths),
              "triangulations good / bad", int(good[0]), int(bad[0]))
        assert good[0] > 0
        # init_z follows the median of the in-state and mature pool depths (each in its anchor frame): it leaves the wrong
        # initial_z for the depths of the scene
        scene = np.median(last_depths)
        assert abs(zs[-1] - scene) < 0.7 * abs(cfg.initial_z - scene) and zs[-1] > 2 * cfg.initial_z
        assert cfg.min_depth <= min(zs) and max(zs) <= cfg.max_depth
        ate = formats.ate_rmse(np.array(est_T), np.array(gt_T), align=False)
        print("ATE", ate)
        assert ate < ATE_BOUND, ate
    finally:
        est.close()
