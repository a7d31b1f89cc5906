"""GPU: the per-element geometry at its branch points and rank changes (inputs, restatements and bounds:
tests/geometry_edge_cases.py; their preconditions: tests/test_geometry_edges_cpu.py) - the camera models through
xivo_hip_jacobians_instate (plain and camera-calibration contexts) and xivo_hip_pool_add, SO(3) exp through
xivo_hip_absorb_error, log through xivo_hip_traj_nees and xivo_hip_traj_score, the Givens coefficient through xivo_hip_givens /
xivo_hip_qr, the OOS null-space rows at rank 2 and with a repeated group slot.

The device is compared with the 80-bit restatement under a bound taken from the fp64 reference's own error (never from the
device); where the reference cameras themselves return NaN or a wrong bearing the device must return the same, as coded."""
import math

import numpy as np
import pytest

import geometry_edge_cases as ge
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import cm, oracle_jacobians, scene_arrays, spd
from xivo_amd import lib as L
from xivo_amd import synth
from xivo_amd.lib import Context

pytestmark = pytest.mark.gpu
LD = ge.LD
R_VIS, MH, MULT = 2.25, 5.991, 1.1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the g++ build of camera_device.h over the camera inputs, and the families' bounds measured on it"""
    tmp = tmp_path_factory.mktemp("camera_edges")
    ref = ge.camera_reference(ge.build_driver(tmp), tmp)
    bounds = ge.camera_bounds(ref)
    for fam, (worst, b) in bounds.items():
        print("camera family %-9s host build vs 80-bit: worst %.3e  bound %.3e  cap %.0e" % (fam, worst, b, ge.CAPS[fam]))
    return ref, {k: v[1] for k, v in bounds.items()}


@pytest.fixture(scope="module")
def rot_bounds():
    b = ge.rotation_bounds()
    for fam, (worst, bd) in b.items():
        print("rotation family %-3s oracle fp64 vs 80-bit: worst %.3e  bound %.3e  cap %.0e" % (fam, worst, bd, ge.CAPS["rotation"]))
    return {k: v[1] for k, v in b.items()}


def identity_scene(B, ng, F):
    """identity Rsb, Rbc and group rotations, zero translations: Xcn = (x0, x1, exp(x2)) exactly"""
    poses = np.zeros(B, dtype=L.pose_dtype); groups = np.zeros((B, ng), dtype=L.group_dtype)
    feats = np.zeros((B, F), dtype=L.feat_dtype)
    eye = np.eye(3).reshape(-1)
    poses["Rsb"] = eye; poses["Rbc"] = eye; poses["Rsg"] = eye; groups["Rsb"] = eye
    feats["sind"] = np.arange(F)[None, :]
    return poses, groups, feats


# ---------------------------------------------------------------- cameras
@pytest.mark.parametrize("calib", [False, True], ids=["plain", "calib"])
@pytest.mark.parametrize("name", list(ge.CAMS))
def test_camera_project_at_its_branch_points(built, host, name, calib):
    """camera_project / camera_project_jacc through xivo_hip_jacobians_instate. With identity rotations, zero translations and
    x[2] = 0 the normalised point is (x0, x1) exactly and the feature block of J is camera_project's own 2 x 2 block (its
    products with 0 and 1 are exact); inn = 0 - xp. Finite inputs against the 80-bit restatement under the families' bounds;
    the equidistant camera on its axis: xp = (cx, cy) and an all-NaN block; atan below R = 1e-4: the pinhole's Jacobians
    exactly, d / dw = 0."""
    ref, bounds = host
    cam, r = ge.CAMS[name], ref[name]
    pts = r["pts"]
    F, B = len(pts), 2
    dim = int(r["dim"][0])
    lay = orc.calib_layout(1, F, temporal=False, imu=False, camera_dim=dim) if calib else orc.Layout(1, F)
    poses, groups, feats = identity_scene(B, 1, F)
    feats["x"][:, :, :2] = np.array(pts)[None]
    with Context(lay.N, 2 * F, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, 1, lay.feature_begin, F, cam)
        if calib:
            ctx.set_calib(-1, -1, lay.cam_begin, lay.cam_dim)
            cal = np.zeros(B, dtype=L.calib_dtype)
            cal["intr"] = L.cam_intr(cam); cal["Cg"] = cm(np.eye(3)); cal["Ca"] = cm(np.eye(3))
            ctx.set_calib_state(cal)
        ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate()
        J, inn = ctx.get_jacobians()
        Jc = ctx.get_jacobians_calib(F=F) if calib else None
    fmax = max(cam["fx"], cam["fy"])
    worst = dict(pixels=0.0, jac=0.0)
    for b in range(B):
        for i, (x, y) in enumerate(pts):
            blk, xp_dev = J[b, i][:, 18:20], -inn[b, i]
            assert np.array_equal(J[b, i][:, 15:17], blk, equal_nan=True)        # d / dTsbr = dxp_dXcn: the same block
            if i not in ge.finite_points(name):
                assert ge.same_bits(xp_dev, [cam["cx"], cam["cy"]]) and np.isnan(blk).all(), (name, i, blk)
                continue
            xp, Jl, jacc, _, br = ge.project(cam, x, y, LD)
            worst["pixels"] = max(worst["pixels"], float(np.abs(xp_dev.astype(LD) - xp).max()))
            worst["jac"] = max(worst["jac"], float(np.abs(blk.astype(LD) - Jl).max()) / fmax)
            if br == "singular":
                assert np.array_equal(blk, [[cam["fx"], 0.0], [0.0, cam["fy"]]])
            if calib:
                got = Jc[b, i][:, 13:13 + dim]
                worst["jac"] = max(worst["jac"], float(np.abs(got.astype(LD) - jacc[:, :dim]).max()) / fmax)
                assert not Jc[b, i][:, 13 + dim:].any()
                if br == "singular":
                    want = np.zeros((2, 5)); want[0, 0] = x; want[0, 2] = 1; want[1, 1] = y; want[1, 3] = 1
                    assert np.array_equal(got, want)
    print("%s %s: device vs 80-bit pixels %.3e (bound %.3e), Jacobians / max(fx, fy) %.3e (bound %.3e)"
          % (name, "calib" if calib else "plain", worst["pixels"], bounds["pixels"], worst["jac"], bounds["jac"]))
    assert worst["pixels"] <= bounds["pixels"] and worst["jac"] <= bounds["jac"]
    if name == "atan":                      # the jump at R = 1e-4, as coded: about 1.078 times the pinhole's Jacobian
        assert J[0, 3][0, 18] / J[0, 2][0, 18] > 1.07


@pytest.mark.parametrize("name", list(ge.CAMS))
def test_camera_unproject_at_its_branch_points(built, host, name):
    """camera_unproject through xivo_hip_pool_add (Feature::Initialize). As coded: the equidistant camera returns the optical
    axis (0, +-0) for every pixel of the column u == cx, atan un-projects with f = 1 up to R = 0.01; the rest against the
    80-bit restatement under the family's bound."""
    ref, bounds = host
    cam, r = ge.CAMS[name], ref[name]
    pix = np.array(r["pix"])
    pm, B, ng = len(pix), 2, 2
    N = 23 + 6 * ng + 3
    poses, groups, feats = identity_scene(B, ng, 1)
    feats["sind"] = -1
    with Context(N, 2, B) as ctx:
        ctx.set_layout(N, 23, ng, 23 + 6 * ng, 1, cam)
        ctx.set_scene(poses, groups, feats)
        ctx.pool_config(pm, 2)
        ctx.pool_anchor(np.ones(B, dtype=np.int32))
        recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B); recs["anchor"] = 1
        recs["xp"] = np.tile(pix, (B, 1)); recs["z0"] = 2.0; recs["std_xyz"] = 0.1
        ctx.pool_add(recs)
        ent, _, _ = ctx.pool_get()
    worst = 0.0
    for b in range(B):
        for i, (u, v) in enumerate(pix):
            got = ent[b, i]["x"][:2]
            assert np.isfinite(got).all()
            if i in ge.UNPROJECT_EXACT[name]:
                assert ge.same_bits(got, ge.UNPROJECT_EXACT[name][i]), (name, i, got)
            worst = max(worst, float(np.abs(got.astype(LD) - ge.unproject(cam, u, v, LD)[0]).max()))
    print("%s: device UnProject vs 80-bit %.3e (bound %.3e)" % (name, worst, bounds["unproject"]))
    assert worst <= bounds["unproject"]
    if name == "atan":                      # f = 1 just below R = 0.01, tan(R w) / (2 tan(w / 2) R), about 0.9275, just above
        assert abs(math.hypot(*ent[0, 1]["x"][:2]) / ge.ATAN_UNPROJECT_R - 1) < 2 * ge.OFF
        assert math.hypot(*ent[0, 2]["x"][:2]) / ge.ATAN_UNPROJECT_R < 0.93


@pytest.mark.parametrize("name", ["atan", "radtan", "equi"])
def test_track_producer_pixels_at_the_camera_branch_points(built, host, name):
    """xivo_hip_pcw_camera + xivo_hip_pcw_tracks (pcw_tracks_kernel<model>, pixels only): world points (x, y, 1) before a camera
    at the identity pose. Every point inside the image is a track, in order; z = 1 exactly; the equidistant camera's axis gives
    (cx, cy)."""
    from xivo_amd import pcw, sequence
    ref, bounds = host
    cam, pts = ge.CAMS[name], np.array(ref[name]["pts"])
    n, B = len(pts), 2
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", npts=n, tracks_max=n, n_groups=2, n_features=4,
                                  min_new_features=2)
    sims = [pcw.TrajectorySim("lissajous", seed=b) for b in range(B)]
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        be.ctx.pcw_camera(cam, np.inf)
        be.set_world(np.tile(np.column_stack([pts, np.ones(n)])[None], (B, 1, 1)))
        gsc = np.zeros((B, 12)); gsc[:, [0, 4, 8]] = 1.0
        be.make_tracks(gsc, 0.0, 5, 0)
        cnt, _, meas = be.ctx.pcw_get_tracks(n, 0, B)
    finally:
        be.close()
    # the radtan point at radius 1 leaves the 640 x 480 image (v = 537.8): no track; every other point is one, in order
    inside = [i for i, xp in enumerate(ref[name]["xp"]) if 0 < xp[0] < cam["cols"] and 0 < xp[1] < cam["rows"]]
    assert len(inside) == n - (name == "radtan")
    assert cnt.tolist() == [len(inside)] * B and np.array_equal(meas[:, :len(inside), 2], np.ones((B, len(inside))))
    worst = 0.0
    for b in range(B):
        for t, i in enumerate(inside):
            if i not in ge.finite_points(name):
                assert ge.same_bits(meas[b, t, :2], [cam["cx"], cam["cy"]])
                continue
            worst = max(worst, float(np.abs(meas[b, t, :2].astype(LD) - ge.project(cam, *pts[i], LD)[0]).max()))
    print("%s: track producer pixels vs 80-bit %.3e (bound %.3e)" % (name, worst, bounds["pixels"]))
    assert worst <= bounds["pixels"]


def test_equidistant_feature_on_the_axis_fails_its_filter_only(built):
    """One in-state feature exactly on the optical axis of an equidistant camera (its NaN Jacobian, as the reference computes it)
    among ordinary ones: that filter reports a non-zero status and keeps its prior bit for bit, its neighbours in the batch
    update as the oracle does."""
    cam = synth.EQUI
    ng, nf, B = 4, 9, 3
    sc = synth.g_level(ng, nf, nf, B, seed=21, cam=cam)
    lay = orc.Layout(ng, nf, N=sc["N"])
    poses, groups, feats, xp = scene_arrays(sc, cam)
    # filter 1: the current pose and the anchor of feature 0 become the identity, so that Xcn = Xc = (0, 0, z) exactly
    eye = np.eye(3).reshape(-1)
    r0 = int(sc["ref"][1, 0])
    poses[1]["Rsb"] = eye; poses[1]["Tsb"] = 0; poses[1]["Rbc"] = eye; poses[1]["Tbc"] = 0
    groups[1, r0]["Rsb"] = eye; groups[1, r0]["Tsb"] = 0
    feats[1, 0]["x"] = [0.0, 0.0, math.log(3.0)]
    P = np.array([spd(lay.N, 80 + b) * 1e-4 for b in range(B)])
    with Context(lay.N, 2 * nf, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, ng, lay.feature_begin, nf, cam)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate()
        J, inn = ctx.get_jacobians()
        ctx.filter_update(R_VIS, MH, MULT, 5, use_gating=False)
        st = ctx.get_status(check=False)
        err = ctx.get_err(); Pn = ctx.download_P()
    assert np.isnan(J[1, 0][:, 18:20]).all() and ge.same_bits(feats[1, 0]["xp"] - inn[1, 0], [cam["cx"], cam["cy"]])
    assert np.isfinite(J[0]).all() and np.isfinite(J[2]).all() and np.isfinite(J[1, 1:]).all()
    assert st[1] != 0 and st[0] == 0 and st[2] == 0
    assert Pn[1].tobytes() == P[1].tobytes()
    for b in (0, 2):
        Js, inns, _ = oracle_jacobians(sc, cam, lay, xp, b)
        H, i_, dR = orc.stack_measurements(Js, inns, sc["ref"][b], sc["sind"][b], lay, R_VIS)
        e_ref, P_ref, _ = orc.update_joseph(H, P[b], i_, dR)
        assert rel_fro(Pn[b], P_ref) < TOL_P and rel_fro(err[b], e_ref) < TOL_DX


# ---------------------------------------------------------------- SO(3) exp: xivo_hip_absorb_error
def _rot_of(rec):
    return np.asarray(rec).reshape(3, 3).T


def _plant_dx(ctx, N, B, cols, vals):
    """dx[b, cols] = vals[b] through a measurement update: P = I, H selects the columns, R = 3, inn = 4 vals: S = 4 I, K = H^T / 4
    (powers of two: exact), every other component of dx is 0. -> the dx the device holds"""
    M = len(cols)
    H = np.zeros((B, M, N)); H[:, np.arange(M), cols] = 1.0
    ctx.upload_P(np.tile(np.eye(N), (B, 1, 1)))
    ctx.set_measurements(H, 4.0 * np.asarray(vals), np.full((B, M), 3.0))
    ctx.update_joseph()
    assert (ctx.get_status() == 0).all()
    return ctx.get_err()


def test_so3_exp_through_absorb_error(built, rot_bounds):
    """R <- R exp(w) on Wsb, Wbc, Wsg and six group slots of eight filters, |w| from 0 over both sides of the 1e-10 threshold to
    pi, about three unit axes and a skew one: the retracted rotations against R exp(w) in 80-bit for the w the device
    itself held (read back), absolute per entry. w = 0 leaves R bit for bit. (At |w| = 1e-8 the coded (1 - cos th) / th^2 is 0,
    not 0.5: the effect on R is th^2 / 2 = 5e-17, below 2^-53 - which is why the bound is absolute.)"""
    full, wsg = ge.exp_inputs()
    B, ng = ge.EXP_B, ge.EXP_NG
    lay = orc.Layout(ng, 1)
    N = lay.N
    slots = [orc.WSB, orc.WBC] + [lay.group_begin + 6 * g for g in range(ng)]
    cols = [c + k for c in slots for k in range(3)] + [orc.WSG, orc.WSG + 1]
    vals = np.array([[full[b][s][1][k] for s in range(len(slots)) for k in range(3)] + list(wsg[b][1][:2]) for b in range(B)])
    poses, groups, feats = identity_scene(B, ng, 1)
    feats["sind"] = -1
    for b in range(B):
        poses[b]["Rsb"] = cm(full[b][0][0]); poses[b]["Rbc"] = cm(full[b][1][0]); poses[b]["Rsg"] = cm(wsg[b][0])
        for g in range(ng):
            groups[b, g]["Rsb"] = cm(full[b][2 + g][0])
    with Context(N, len(cols), B) as ctx:
        ctx.set_layout(N, lay.group_begin, ng, lay.feature_begin, 1, synth.PINHOLE)
        ctx.set_scene(poses, groups, feats)
        dx = _plant_dx(ctx, N, B, cols, vals)
        ctx.absorb_error()
        pose_d, group_d, _ = ctx.get_scene()
        assert np.abs(ctx.get_err()).max() == 0.0
    assert np.array_equal(dx[:, cols], vals)              # (the update's arithmetic on powers of two is exact)
    worst, taylor, zeros = 0.0, 0, 0
    for b in range(B):
        got = [_rot_of(pose_d[b]["Rsb"]), _rot_of(pose_d[b]["Rbc"])] + [_rot_of(group_d[b, g]["Rsb"]) for g in range(ng)]
        items = [(got[s], full[b][s][0], dx[b, slots[s]:slots[s] + 3]) for s in range(len(slots))]
        items.append((_rot_of(pose_d[b]["Rsg"]), wsg[b][0], np.array([dx[b, orc.WSG], dx[b, orc.WSG + 1], 0.0])))
        for Rd, R0, w in items:
            th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
            taylor += th < ge.EXP_THRESHOLD
            if th == 0.0:
                zeros += 1
                assert Rd.tobytes() == R0.tobytes()
            worst = max(worst, float(np.abs(Rd.astype(LD) - R0.astype(LD) @ ge.so3_exp_ld(w)).max()))
    print("so3 exp: device vs 80-bit %.3e (bound %.3e); %d retractions below the threshold, %d with w = 0" % (worst, rot_bounds["exp"], taylor, zeros))
    assert taylor >= 12 and zeros >= 4
    assert worst <= rot_bounds["exp"]


def test_50th_absorb_renormalises_rsg(built, rot_bounds):
    """State::operator+= every 50th call: Rsg <- exp(log(Rsg) with z zeroed) for Rsg = identity, a small tilt without z and a
    rotation of 2.5 rad; 49 absorbs of dx = 0 before leave Rsg bit for bit. The bound is the sum of the log family's and the
    exp family's: the error of log enters exp with a derivative of norm <= 1."""
    B = len(ge.ZERO_Z_RSG)
    lay = orc.Layout(1, 1)
    poses, groups, feats = identity_scene(B, 1, 1)
    feats["sind"] = -1
    for b in range(B):
        poses[b]["Rsg"] = cm(ge.ZERO_Z_RSG[b])
    with Context(lay.N, 2, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, 1, lay.feature_begin, 1, synth.PINHOLE)
        ctx.set_scene(poses, groups, feats)
        _plant_dx(ctx, lay.N, B, [orc.TSB], np.zeros((B, 1)))
        for _ in range(49):
            ctx.absorb_error()
        p49, _, _ = ctx.get_scene()
        ctx.absorb_error()
        p50, _, _ = ctx.get_scene()
    worst = 0.0
    for b in range(B):
        assert p49[b]["Rsg"].tobytes() == poses[b]["Rsg"].tobytes()
        worst = max(worst, float(np.abs(_rot_of(p50[b]["Rsg"]).astype(LD) - ge.zero_log_z_ld(ge.ZERO_Z_RSG[b])).max()))
    bd = rot_bounds["exp"] + rot_bounds["log"]
    print("50th absorb: Rsg device vs 80-bit %.3e (bound %.3e)" % (worst, bd))
    assert p50[0]["Rsg"].tobytes() == poses[0]["Rsg"].tobytes()          # the identity stays the identity
    assert np.abs(_rot_of(p50[2]["Rsg"]) - ge.ZERO_Z_RSG[2]).max() > 0.1  # 2.5 rad about a skew axis loses its z part
    assert worst <= bd


# ---------------------------------------------------------------- SO(3) log: xivo_hip_traj_nees, xivo_hip_traj_score
def _traj_context(B, T):
    lay = orc.Layout(1, 1)
    ctx = Context(lay.N, 2, B)
    ctx.set_layout(lay.N, lay.group_begin, 1, lay.feature_begin, 1, synth.PINHOLE)
    ctx.upload_P(np.tile(np.eye(lay.N), (B, 1, 1)))
    ctx.traj_config(T, list(range(6)))
    return ctx


def _record(ctx, B, Rs):
    poses, groups, feats = identity_scene(B, 1, 1)
    feats["sind"] = -1
    for b in range(B):
        poses[b]["Rsb"] = cm(Rs[b])
    ctx.set_scene(poses, groups, feats)
    ctx.traj_record()


def test_so3_log_through_traj_nees(built, rot_bounds):
    """err6[:3] = log(R_est^T R_gt) of fp64 matrices with R_gt = fl(R_est exp(w)): angles 0 (bitwise equal matrices), both sides
    of the n2 < 1e-20 branch, both sides of the trace's sign change at 2 pi / 3, 2.5 rad about +-x, +-y, +-z (Shepperd's three
    t <= 0 branches), pi - 1e-8 and pi. Against the 80-bit log of the 80-bit product of the same matrices: components,
    absolute; at exactly pi, where the axis' sign is free, |w| and exp(w) against the product."""
    cases = ge.log_cases()
    B = 8
    T = -(-len(cases) // B)
    slot = [cases[i % len(cases)] for i in range(T * B)]
    gt_R = np.array([c["R_gt"] for c in slot]).reshape(T, B, 3, 3)
    with _traj_context(B, T) as ctx:
        for t in range(T):
            _record(ctx, B, [slot[t * B + b]["R_est"] for b in range(B)])
        err6, _, _, _ = ctx.traj_nees(gt_R, np.zeros((T, B, 3)))
    worst = 0.0
    for i, c in enumerate(slot):
        w = err6[i // B, i % B, :3]
        _, wld = ge.log_reference(c)
        e = ge.log_error(w, c, wld)
        worst = max(worst, e)
        assert e <= rot_bounds["log"], (c["angle"], c["tag"], e, w)
        if c["angle"] == 0.0:
            assert np.abs(w).max() <= rot_bounds["log"]
    print("so3 log (traj_nees): device vs 80-bit %.3e (bound %.3e) over %d cases" % (worst, rot_bounds["log"], len(cases)))


def test_so3_log_through_traj_score_rpe(built, rot_bounds):
    """rpe_rot of two frames with a planted relative rotation M per filter (est = (I, M), truth = (I, I)): |log M|, against the
    80-bit log's norm. The norm of a 3-vector is off by at most sqrt(3) times its components' error."""
    cases = ge.rpe_cases()
    B = len(cases)
    gt = np.zeros((2, B, 12)); gt[:, :, [0, 4, 8]] = 1.0
    with _traj_context(B, 2) as ctx:
        _record(ctx, B, [np.eye(3)] * B)
        _record(ctx, B, [c["R_gt"] for c in cases])
        out = ctx.traj_score(gt, align=False, rpe_lag=1)
    bd = math.sqrt(3.0) * rot_bounds["log"]
    for b, c in enumerate(cases):
        wld = ge.log_reference(c)[1]
        e = abs(float(LD(out[b]["rpe_rot"]) - np.sqrt(wld @ wld)))
        print("rpe_rot angle %.12g: device %.17g, error %.3e (bound %.3e)" % (c["angle"], out[b]["rpe_rot"], e, bd))
        assert out[b]["n_pairs"] == 1 and e <= bd, (c["angle"], e)


# ---------------------------------------------------------------- Givens coefficient
def test_givens_coefficient_at_its_branch_points(built):
    """xivo_hip_givens on 12-row problems and xivo_hip_qr on 72-row ones (it refuses rows <= nx, as the reference CHECKs), both
    at nx = 70: one column chunk boundary. Their first pivot pairs sit on both sides of eps = (double)1e-4f, at a = b = 0, at
    a = 0 and in both |b| > |a| and |b| <= |a| (the CPU test shows that every branch runs and that none turns on rounding).
    A wrong branch moves entries by about 1e-4."""
    x, Hx, Hf = ge.givens_problems()
    xq_in, Hxq_in, _ = ge.givens_problems(qr=True)
    with Context(8, 2, 1) as ctx:
        ro, xd, Hxd, Hfd = ctx.givens(x, Hx, Hf)
        rq, xq, Hxq = ctx.qr(xq_in, Hxq_in)
    for p in range(len(ge.GIVENS_PAIRS)):
        r, xo, Hxo, Hfo = orc.givens_eliminate(x[p], Hx[p], Hf[p])
        assert ro[p] == r
        assert np.abs(xd[p] - xo).max() < 1e-10 and np.abs(Hxd[p] - Hxo).max() < 1e-10 and np.abs(Hfd[p] - Hfo).max() < 1e-10
        r, xo, Hxo = orc.qr_compress(xq_in[p], Hxq_in[p])
        assert rq[p] == r
        assert np.abs(xq[p] - xo).max() < 1e-10 and np.abs(Hxq[p] - Hxo).max() < 1e-10, (p, np.abs(Hxq[p] - Hxo).max())


# ---------------------------------------------------------------- OOS rows when the geometry degenerates
def _oos_records(B, feats_list):
    oos = np.zeros((B, len(feats_list)), dtype=L.oos_dtype)
    for b in range(B):
        for o, (Xs, obs) in enumerate(feats_list):
            oos[b, o]["Xs"] = Xs; oos[b, o]["n_obs"] = len(obs)
            for q, (g, pix) in enumerate(obs):
                oos[b, o]["group_sind"][q] = g; oos[b, o]["xp"][q] = pix
    return oos


ROOS = 3.5 ** 2


def _run_oos(sc, cam, ng, fl, whole, anchor=16, B=2):
    """one in-state feature (anchored at group `anchor`) stacked, then the OOS features fl projected behind it and the update
    -> (rows_out, [get_H(b)], dx, P+, P, the oracle's in-state (H, inn, diagR))"""
    lay = orc.Layout(ng, 1)
    n_rows = sum(2 * ng - 3 if whole else 2 * len(obs) - 3 for _, obs in fl)
    poses, groups, feats = identity_scene(B, ng, 1)
    poses["Tbc"] = sc["Tbc"]
    for g in range(ng):
        groups[:, g]["Rsb"] = cm(sc["gR"][g]); groups[:, g]["Tsb"] = sc["gT"][g]
    x_in = np.array([0.1, -0.05, math.log(4.0)])
    args = (sc["gR"][anchor], sc["gT"][anchor], sc["Rsb"], sc["Tsb"], sc["Rbc"], sc["Tbc"], cam, lay, anchor, 0)
    pix_in = -orc.compute_jacobian(x_in, [0.0, 0.0], *args)[1] + np.array([0.4, -0.3])
    feats["x"] = x_in; feats["xp"] = pix_in; feats["ref_sind"] = anchor; feats["sind"] = 0
    P = np.array([spd(lay.N, 40 + b) * 1e-4 for b in range(B)])
    with Context(lay.N, 2 + n_rows + 16, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, ng, lay.feature_begin, 1, cam)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, 5); ctx.stack(R_VIS)
        rows = ctx.oos_project(_oos_records(B, fl), ROOS, whole_buffer=whole)
        got = [ctx.get_H(b) for b in range(B)]
        ctx.update_joseph()
        assert (ctx.get_status() == 0).all()
        err = ctx.get_err(); Pn = ctx.download_P()
    Jo, inn_o, _ = orc.compute_jacobian(x_in, pix_in, *args)
    return rows, got, err, Pn, P, orc.stack_measurements(np.array([Jo]), np.array([inn_o]), np.array([anchor]), np.array([0]), lay, R_VIS)


def _check_oos(got, err, Pn, P, H, inn, dR):
    """the staged rows against the oracle's, then the update on exactly those rows"""
    for b in range(len(P)):
        gH, ginn, gdR = got[b]
        assert gH.shape == H.shape
        assert rel_fro(gH, H) < 1e-10 and rel_fro(ginn, inn) < 1e-9 and np.array_equal(gdR, dR)
        e_ref, P_ref, _ = orc.update_joseph(H, P[b], inn, dR)
        assert rel_fro(Pn[b], P_ref) < TOL_P and rel_fro(err[b], e_ref) < TOL_DX


@pytest.mark.parametrize("whole", [False, True], ids=["top2k", "whole_buffer"])
@pytest.mark.parametrize("k", ge.OOS_K)
def test_oos_rows_at_rank_2_and_with_a_repeated_group(built, k, whole):
    """Four OOS features per filter: an ordinary one, one seen k times from ONE pose (Hf has rank 2: the kernel has 2k - 2
    vectors, the device reserves and writes 2k - 3: the first 2k - 3 columns of Eigen's basis, A[:, :2k-3]^T Hx,
    A[:, :2k-3]^T r, diagR = Roos), another ordinary one behind it (its row offset), and one that lists a group slot twice,
    (17, 17, 18) (the read-modify-write of the group block). Rows against the oracle's, then the update on exactly those
    rows. Whole-buffer mode: the rows behind the 2k - 3 are zero rows with inn = 0."""
    sc, cam, ng = ge.oos_scene(), ge.OOS_CAM, ge.OOS_NG
    fl = ge.oos_features(k)
    lay = orc.Layout(ng, 1)
    per = 2 * ng - 3 if whole else None
    rows, got, err, Pn, P, (H, inn, dR) = _run_oos(sc, cam, ng, fl, whole)
    assert rows.tolist() == [sum(per if whole else 2 * len(obs) - 3 for _, obs in fl)] * len(P)
    for i, (Xs, obs) in enumerate(fl):
        n = len(obs)
        Hxp, rp, A = orc.oos_jacobian(Xs, obs, sc["gR"], sc["gT"], sc["Rbc"], sc["Tbc"], cam, lay, whole_buffer_groups=ng if whole else 0)
        if i == 1:                              # rank 2: one more kernel vector than rows reserved - the (2k - 2)th is dropped
            assert Hxp.shape[0] == (2 * ng if whole else 2 * n) - 2
            keep = [j for j in range(Hxp.shape[0]) if j != 2 * n - 3]
            Hxp, rp, A = Hxp[keep], rp[keep], A[:, keep]
        assert Hxp.shape[0] == (per if whole else 2 * n - 3)
        assert np.abs(A.T @ np.vstack([ge.oos_hf(Xs, obs), np.zeros((A.shape[0] - 2 * n, 3))])).max() < 1e-9
        if whole:
            assert np.abs(Hxp[2 * n - 3:]).max() == 0 and np.abs(rp[2 * n - 3:]).max() == 0
        H = np.vstack([H, Hxp]); inn = np.concatenate([inn, rp]); dR = np.concatenate([dR, np.full(len(rp), ROOS)])
    _check_oos(got, err, Pn, P, H, inn, dR)


@pytest.mark.parametrize("name", list(ge.CAMS))
def test_oos_project_at_the_camera_branch_points(built, name):
    """camera_project inside oos_kernel: per finite camera input one OOS feature at Xs = (x, y, 1) seen from the identity pose
    (so that its normalised point there is (x, y) exactly) and from an ordinary one. The single projected row and its residual
    against the oracle's at the tolerances of tests/test_glevel_gpu.py: a wrong branch at the atan threshold moves the row by 8 %."""
    sc, cam = ge.oos_camera_scene(), ge.CAMS[name]
    fl = ge.oos_camera_features(name)
    lay = orc.Layout(2, 1)
    rows, got, err, Pn, P, (H, inn, dR) = _run_oos(sc, cam, 2, fl, False, anchor=1)
    assert rows.tolist() == [len(fl)] * len(P)
    for Xs, obs in fl:
        Hxp, rp, _ = orc.oos_jacobian(Xs, obs, sc["gR"], sc["gT"], sc["Rbc"], sc["Tbc"], cam, lay)
        assert Hxp.shape[0] == 1 and np.isfinite(Hxp).all()
        H = np.vstack([H, Hxp]); inn = np.concatenate([inn, rp]); dR = np.concatenate([dR, [ROOS]])
    _check_oos(got, err, Pn, P, H, inn, dR)
