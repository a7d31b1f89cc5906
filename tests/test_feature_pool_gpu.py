"""GPU: the resident out-of-state feature pool (xivo_hip_pool_*, XIVO_EDIT_ADD_GROUP_ANCHOR / _ADMIT_POOL) and the
"subfilter" life cycle of a new track built on it (xivo_amd/sequence.py, xivo_amd/pyxivo.py).

The pool must be the existing host-array path moved onto the device: xivo_hip_pool_step is checked bit for bit against
xivo_hip_subfilter_update + xivo_hip_candidate_order on the same entries, Feature::Initialize's un-projection against a
numpy restatement of the reference cameras, the new edit kinds against the edits they stand for."""
import os

import numpy as np
import pytest

import xivo_oracle as orc
from xivo_amd import formats, pcw, sequence, synth
from xivo_amd import lib as L
from xivo_amd.lib import Context, XivoHipError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAMS = {"pinhole": synth.PINHOLE, "equi": synth.EQUI, "radtan": synth.RADTAN, "atan": synth.ATAN}
NG, NF = 8, 4
N = 23 + 6 * NG + 3 * NF
RBC = pcw.so3_exp(np.array([-1.57079633, 0.0, 0.0]))
TBC = np.array([0.02, -0.01, 0.03])


def cm(R):
    """3x3 -> column-major 9 (the C ABI's layout)"""
    return np.asarray(R).T.reshape(-1)


def pose_records(rng, B):
    poses = np.zeros(B, dtype=L.pose_dtype)
    for b in range(B):
        poses[b]["Rsb"] = cm(pcw.so3_exp(rng.normal(size=3) * 0.2)); poses[b]["Tsb"] = rng.normal(size=3) * 0.3
        poses[b]["Rbc"] = cm(RBC); poses[b]["Tbc"] = TBC; poses[b]["Rsg"] = cm(np.eye(3))
    return poses


def context(B, cam, flags=0):
    ctx = Context(N, 2 * NF, B, flags=flags)
    ctx.set_layout(N, 23, NG, 23 + 6 * NG, NF, cam)
    return ctx


def empty_feats(B):
    f = np.zeros((B, 1), dtype=L.feat_dtype)
    f["sind"] = -1
    return f


def perturb(poses, rng, s):
    out = poses.copy()
    for b in range(len(out)):
        out[b]["Rsb"] = cm(pcw.so3_exp(rng.normal(size=3) * s) @ out[b]["Rsb"].reshape(3, 3).T)
        out[b]["Tsb"] = out[b]["Tsb"] + rng.normal(size=3) * s
    return out


def project_np(cam, x, y):
    """Project() of common/camera_{pinhole,atan,radtan,equidist}.h: normalised coordinates -> pixel (no Jacobian)"""
    fx, fy, cx, cy, d = cam["fx"], cam["fy"], cam["cx"], cam["cy"], list(cam["d"]) + [0.0] * 5
    if cam["model"] == 0:
        return fx * x + cx, fy * y + cy
    if cam["model"] == 1:
        w = d[0]
        R = np.sqrt(x * x + y * y)
        f = np.where((R < 1e-4) | (w == 0), 1.0, np.arctan(2.0 * np.tan(w / 2) * R) / np.maximum(R, 1e-300) / w)
        return fx * f * x + cx, fy * f * y + cy
    if cam["model"] == 2:
        p1, p2, k1, k2, k3 = d[:5]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
        return (cx + fx * (rad * x + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)),
                cy + fy * (rad * y + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)))
    k0, k1, k2, k3 = d[:4]
    th = np.arctan2(np.sqrt(x * x + y * y), 1.0)
    phi = np.arctan2(y, x)
    r = th + k0 * th ** 3 + k1 * th ** 5 + k2 * th ** 7 + k3 * th ** 9
    return fx * r * np.cos(phi) + cx, fy * r * np.sin(phi) + cy


def unproject_np(cam, u, v, max_iter=15):
    """UnProject() of the four reference cameras, restated (iterations and stopping rule of the reference: max_iter steps)"""
    fx, fy, cx, cy, d = cam["fx"], cam["fy"], cam["cx"], cam["cy"], list(cam["d"]) + [0.0] * 5
    if cam["model"] == 0:                                              # camera_pinhole.h:39-53
        return (u - cx) / fx, (v - cy) / fy
    if cam["model"] == 1:                                              # camera_atan.h:94-128
        w = d[0]
        w2 = 2.0 * np.tan(w * 0.5)
        t0, t1 = (u - cx) / fx, (v - cy) / fy
        R = np.sqrt(t0 * t0 + t1 * t1)
        RR = R if w == 0 else np.tan(R * w) / w2
        f = np.where(R > 0.01, RR / np.where(R > 0, R, 1.0), 1.0)
        return f * t0, f * t1
    if cam["model"] == 2:                                              # camera_radtan.h:100-168 (Newton on distort(xc) = xk)
        p1, p2, k1, k2, k3 = d[:5]
        xk0, xk1 = (u - cx) / fx, (v - cy) / fy
        x, y = xk0.copy(), xk1.copy()
        for _ in range(max_iter):
            t2, t3 = x * x, y * y
            t8 = t2 + t3
            t20 = k1 * t8 + k2 * t8 * t8 + k3 * t8 ** 3 + 1.0
            t18 = k1 * x * 2.0 + k2 * t8 * x * 4.0 + k3 * t8 * t8 * x * 6.0
            t19 = k1 * y * 2.0 + k2 * t8 * y * 4.0 + k3 * t8 * t8 * y * 6.0
            t6, t7 = p1 * x * 2.0, p2 * y * 2.0
            f0 = t20 * x + t6 * y + p2 * (t2 * 2.0 + t8) - xk0
            f1 = t7 * x + t20 * y + p1 * (t3 * 2.0 + t8) - xk1
            g00, g01 = t20 + p2 * x * 6.0 + p1 * y * 2.0 + t18 * x, t6 + t7 + t19 * x
            g10, g11 = t6 + t7 + t18 * y, t20 + p2 * x * 2.0 + p1 * y * 6.0 + t19 * y
            det = g00 * g11 - g10 * g01
            x, y = x - (g11 * f0 - g01 * f1) / det, y - (-g10 * f0 + g00 * f1) / det
        return x, y
    k0, k1, k2, k3 = d[:4]                                             # camera_equidist.h:97-160
    xn, yn = u - cx, v - cy
    phi = np.arctan2(fx * yn, fy * xn)
    rth = xn / (fx * np.cos(phi))
    th = rth.copy()
    for _ in range(max_iter):
        x0 = th + k0 * th ** 3 + k1 * th ** 5 + k2 * th ** 7 + k3 * th ** 9 - rth
        x1 = 1 + 3 * k0 * th ** 2 + 5 * k1 * th ** 4 + 7 * k2 * th ** 6 + 9 * k3 * th ** 8
        d2 = 4 * th * x0 * (3 * k0 + 10 * k1 * th ** 2 + 21 * k2 * th ** 4 + 36 * k3 * th ** 6) + 2 * x1 * x1
        th = th - 2 * x0 * x1 / d2
    return np.tan(th) * np.cos(phi), np.tan(th) * np.sin(phi)


def pixels(rng, cam, n):
    """pixels inside the image, away from the principal point: the ATAN model un-projects with f = 1 below a normalised
    radius of 0.01 while it projects with the full model from 1e-4 on (camera_atan.h:39-41 vs :105-107), so the
    round trip only holds outside that disc"""
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(0.05, 0.9, n) * 0.5 * min(cam["rows"], cam["cols"])
    return cam["cx"] + rad * np.cos(ang), cam["cy"] + rad * np.sin(ang)


# ---------------------------------------------------------------- pool_add: Feature::Initialize / Camera::UnProject
@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("per_filter", [False, True])
def test_pool_add_unprojects_every_camera_model(built, name, per_filter):
    cam = CAMS[name]
    B, pm = 5, 40
    rng = np.random.default_rng(3)
    cams = []
    for b in range(B):
        c = dict(cam)
        if per_filter:          # per-filter intrinsics (online camera calibration): scaled focal lengths, shifted centre
            c.update(fx=cam["fx"] * (1 + 0.01 * b), fy=cam["fy"] * (1 - 0.01 * b), cx=cam["cx"] + b, cy=cam["cy"] - b)
        cams.append(c)
    with context(B, cam) as ctx:
        poses = pose_records(rng, B)
        ctx.set_scene(poses, np.zeros((B, NG), dtype=L.group_dtype), empty_feats(B))
        if per_filter:
            dim = {0: 4, 1: 5, 2: 9, 3: 8}[cam["model"]]
            ctx.set_calib(cam_begin=23, cam_dim=dim)
            cal = np.zeros(B, dtype=L.calib_dtype)
            for b in range(B):
                cal[b]["intr"] = L.cam_intr(cams[b]); cal[b]["Cg"] = cm(np.eye(3)); cal[b]["Ca"] = cm(np.eye(3))
            ctx.set_calib_state(cal)
        ctx.pool_config(pm, 2)
        ctx.pool_anchor(np.ones(B, dtype=np.int32))
        recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B); recs["anchor"] = 1
        us, vs = pixels(rng, cam, B * pm)
        recs["xp"][:, 0], recs["xp"][:, 1] = us, vs
        recs["z0"] = rng.uniform(0.5, 8.0, B * pm)
        recs["std_xyz"] = rng.uniform(0.001, 0.2, (B * pm, 3))
        ctx.pool_add(recs[::-1])            # record order is free
        ent, _, _ = ctx.pool_get()
    for b in range(B):
        r = recs[b * pm:(b + 1) * pm]
        e = ent[b]
        x0, x1 = unproject_np(cams[b], r["xp"][:, 0], r["xp"][:, 1])
        assert np.abs(e["x"][:, 0] - x0).max() < 1e-12 and np.abs(e["x"][:, 1] - x1).max() < 1e-12
        assert np.abs(e["x"][:, 2] - np.log(r["z0"])).max() < 1e-15 * 4      # device libm log: within an ulp or two
        P = np.zeros((pm, 9)); P[:, [0, 4, 8]] = r["std_xyz"] ** 2
        assert np.array_equal(e["P"], P)
        assert (e["ref_sind"] == 1).all() and (e["status"] == 0).all() and (e["init_counter"] == 0).all()
        assert (e["outlier_counter"] == 0).all() and np.array_equal(e["xp"], r["xp"])
        u, v = project_np(cams[b], e["x"][:, 0], e["x"][:, 1])
        assert np.abs(u - r["xp"][:, 0]).max() < 1e-9 and np.abs(v - r["xp"][:, 1]).max() < 1e-9, name


def test_pool_add_inverse_depth_and_bad_records(built):
    cam = synth.PINHOLE
    with context(2, cam, flags=L.FLAG_INVDEPTH) as ctx:
        ctx.set_scene(pose_records(np.random.default_rng(1), 2), np.zeros((2, NG), dtype=L.group_dtype), empty_feats(2))
        with pytest.raises(XivoHipError) as e:
            ctx.pool_config(L.POOL_MAX_ENTRIES + 1, 4)
        assert e.value.status == -5
        ctx.pool_config(8, 4)
        recs = np.zeros(2, dtype=L.pool_new_dtype)
        recs["b"] = [0, 1]; recs["entry"] = [3, 3]; recs["anchor"] = 2; recs["xp"] = [[100.0, 90.0], [400.0, 300.0]]
        recs["z0"] = [2.0, 4.0]; recs["std_xyz"] = [0.01, 0.01, 0.1]
        with pytest.raises(XivoHipError):
            ctx.pool_add(recs)                  # anchor 2 was never created
        ctx.pool_anchor([2, 2])
        for bad in ({"entry": 8}, {"anchor": 4}, {"z0": 0.0}, {"b": 2}):
            r = recs.copy()
            for k, v in bad.items():
                r[k][0] = v
            with pytest.raises(XivoHipError):
                ctx.pool_add(r)
        with pytest.raises(XivoHipError):
            ctx.pool_add(np.concatenate([recs, recs[:1]]))    # one record per entry
        ctx.pool_add(recs)
        ent, _, _ = ctx.pool_get()
    assert ent[0, 3]["x"][2] == 0.5 and ent[1, 3]["x"][2] == 0.25
    assert (ent["ref_sind"] == np.array([[-1] * 3 + [2] + [-1] * 4] * 2)).all()


# ---------------------------------------------------------------- pool_step vs subfilter_update + candidate_order
def run_pool_vs_host(B, pm, invdepth, strict_frames, cam=synth.PINHOLE, frames=4, seed=0):
    """Fills every filter's pool (filter b % 5 == 3 stays empty; filter b % 7 == 5 drops every track in frame 1), links
    anchors 0 and 1 to in-state slots 0 and 1 (then moves those groups, so the linked pose differs from the frozen one)
    and runs `frames` frames of pool_step next to the host-array path on the same entries."""
    rng = np.random.default_rng(seed)
    A = 4
    flags = L.FLAG_INVDEPTH if invdepth else 0
    opts = dict(Rtri=3.5 ** 2, MH_thresh=5.991, ready_steps=1, min_depth=0.05, max_depth=8.0, max_subfilter_outlier=0.5)
    remove = 2.5
    poses = pose_records(rng, B)
    anchor_poses = [perturb(poses, rng, 0.05) for _ in range(A)]
    with context(B, cam, flags) as ctx:
        groups = np.zeros((B, NG), dtype=L.group_dtype)
        groups["Rsb"] = cm(np.eye(3))
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.upload_P(np.repeat(np.eye(N)[None], B, axis=0))
        ctx.pool_config(pm, A, remove_outlier_counter=remove, **opts)
        for a in range(A):
            ctx.set_scene(anchor_poses[a], groups, empty_feats(B))
            ctx.pool_anchor(np.full(B, a, dtype=np.int32))
        ctx.set_scene(poses, groups, empty_feats(B))
        # new tracks: points seen from their anchor, pixels of the current frame near their projection
        recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B)
        recs["anchor"] = rng.integers(0, A, B * pm)
        us, vs = pixels(rng, cam, B * pm)
        recs["xp"][:, 0], recs["xp"][:, 1] = us, vs
        recs["z0"] = rng.uniform(1.0, 6.0, B * pm); recs["std_xyz"] = [0.002, 0.002, 0.3]
        keep = (recs["b"] % 5 != 3) & (rng.random(B * pm) < 0.85)       # empty pools, and free entries in between
        ctx.pool_add(recs[keep])
        ops = []
        for b in range(B):
            for g, a in ((0, 0), (1, 1)):
                o = np.zeros((), dtype=L.edit_dtype); o["b"], o["kind"], o["i0"], o["i1"] = b, L.EDIT_ADD_GROUP_ANCHOR, g, a
                ops.append(o)
        ctx.edit_batch(1, np.array(ops))
        # move the linked groups; slots 4..7 hold the frozen poses of anchors 0..3 for the host path
        _, groups, _ = ctx.get_scene()
        for g in (0, 1):
            for b in range(B):
                groups[b, g]["Rsb"] = cm(pcw.so3_exp(rng.normal(size=3) * 0.02) @ groups[b, g]["Rsb"].reshape(3, 3).T)
                groups[b, g]["Tsb"] = groups[b, g]["Tsb"] + rng.normal(size=3) * 0.02
        for a in range(A):
            groups[:, 4 + a]["Rsb"] = anchor_poses[a]["Rsb"]; groups[:, 4 + a]["Tsb"] = anchor_poses[a]["Tsb"]
        ent0, _, slots = ctx.pool_get()
        assert (slots[:, 0] == 0).all() and (slots[:, 1] == 1).all() and (slots[:, 2:] == -1).all()
        host = ent0.copy()
        live = host["ref_sind"] >= 0
        anchor = host["ref_sind"].copy()
        host_slot = np.where(anchor < 2, anchor, 4 + anchor)
        for fr in range(frames):
            poses = perturb(poses, rng, 0.01)
            ctx.set_scene(poses, groups, empty_feats(B))
            xp = np.full((B, pm, 2), np.nan)
            xp[live] = host["xp"][live] + rng.normal(size=(live.sum(), 2)) * 2.0
            wild = live & (rng.random((B, pm)) < 0.05)
            xp[wild] += 60.0                                              # outliers: ratio > 1, counter grows
            if fr == 1:
                xp[np.arange(B) % 7 == 5] = np.nan                        # all tracks of these filters dropped
            xp[live & (rng.random((B, pm)) < 0.03)] = np.nan              # single drops
            strict = fr in strict_frames
            order, n, live_d = ctx.pool_step(xp, strict)
            # host-array path on the same entries
            sub = host.copy()
            sub["xp"] = np.where(np.isnan(xp), 0.0, xp)
            sub["ref_sind"] = np.where(live, host_slot, 0)
            upd = ctx.subfilter_update(sub, **opts)
            tracked = live & ~np.isnan(xp[..., 0])
            live_h = tracked & ~(upd["outlier_counter"] > remove)
            upd["candidate"] = np.where(live_h, upd["candidate"], 0)
            order_h, n_h, _ = L.candidate_order(upd, strict=strict)
            assert np.array_equal(live_d, live_h)
            assert np.array_equal(n, n_h) and np.array_equal(order, order_h)
            ent, _, _ = ctx.pool_get()
            for f in ("x", "P", "xp", "outlier_counter", "score", "status", "init_counter", "candidate"):
                assert np.array_equal(ent[f][live_h], upd[f][live_h]), f     # bit for bit
            assert (ent["ref_sind"][~live_h] == -1).all() and np.array_equal(ent["ref_sind"][live_h], anchor[live_h])
            host[tracked] = upd[tracked]
            live = live_h
        return ctx, host, live, order, n


@pytest.mark.parametrize("B,pm,invdepth,strict_frames", [
    (1, 1, False, (1, 3)), (1, 64, True, (2,)), (70, 64, False, (0, 2)), (70, 200, True, (1, 3)),
    (70, L.POOL_MAX_ENTRIES, False, (2, 3)), (1024, 200, False, (3,)), (1024, 1, True, (0,))])
def test_pool_step_is_the_host_array_path_bit_for_bit(built, B, pm, invdepth, strict_frames):
    run_pool_vs_host(B, pm, invdepth, strict_frames, seed=B + pm)


@pytest.mark.parametrize("name", ["equi", "radtan"])
def test_pool_step_other_cameras(built, name):
    run_pool_vs_host(9, 64, False, (2,), cam=CAMS[name], seed=5)


def test_pool_step_matches_the_oracle(built):
    """the device sub-filter step against oracle.subfilter_update (float64 restatement of feature.cpp:246-297)"""
    cam = synth.PINHOLE
    rng = np.random.default_rng(11)
    B, pm = 2, 16
    poses = pose_records(rng, B)
    opts = dict(Rtri=3.5 ** 2, MH_thresh=5.991, ready_steps=2, min_depth=0.05, max_depth=8.0, max_subfilter_outlier=0.5)
    with context(B, cam) as ctx:
        groups = np.zeros((B, NG), dtype=L.group_dtype)
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.pool_config(pm, 2, remove_outlier_counter=100.0, **opts)
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B)
        us, vs = pixels(rng, cam, B * pm)
        recs["xp"][:, 0], recs["xp"][:, 1] = us, vs
        recs["z0"] = 2.5; recs["std_xyz"] = [0.002, 0.002, 1.0]
        ctx.pool_add(recs)
        state = [dict(x=np.array([*unproject_np(cam, r["xp"][0], r["xp"][1]), np.log(2.5)]), P=np.diag([4e-6, 4e-6, 1.0]),
                      ic=0, oc=0.0) for r in recs]
        Rb = [poses[b]["Rsb"].reshape(3, 3).T for b in range(B)]
        for fr in range(3):
            p2 = perturb(poses, rng, 0.02)
            ctx.set_scene(p2, groups, empty_feats(B))
            xp = (recs["xp"] + rng.normal(size=(B * pm, 2))).reshape(B, pm, 2)
            ctx.pool_step(xp)
            ent, _, _ = ctx.pool_get()
            for i, s in enumerate(state):
                b = i // pm
                s["x"], s["P"], st, s["ic"], s["oc"] = orc.subfilter_update(
                    s["x"], s["P"], xp[b, i % pm], p2[b]["Rsb"].reshape(3, 3).T, p2[b]["Tsb"], RBC, TBC, Rb[b],
                    poses[b]["Tsb"], cam, opts["Rtri"], opts["MH_thresh"], opts["ready_steps"], s["ic"], s["oc"])
                e = ent[b, i % pm]
                assert np.abs(e["x"] - s["x"]).max() < 1e-12
                assert np.abs(e["P"].reshape(3, 3).T - s["P"]).max() < 1e-12
                assert e["status"] == st and e["init_counter"] == s["ic"] and abs(e["outlier_counter"] - s["oc"]) < 1e-12


# ---------------------------------------------------------------- the pool's edit kinds
def test_admit_pool_equals_add_feature_and_anchor_groups(built):
    cam = synth.PINHOLE
    rng = np.random.default_rng(21)
    B, pm = 2, 8
    poses = pose_records(rng, 1)
    poses = np.concatenate([poses, poses])
    X = rng.normal(size=(N, N))
    P0 = X @ X.T / N + np.eye(N)
    with context(B, cam) as ctx:
        groups = np.zeros((B, NG), dtype=L.group_dtype)
        groups["Rsb"] = cm(np.eye(3))
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.upload_P(np.stack([P0, P0]))
        ctx.pool_config(pm, 3)
        ctx.pool_anchor([0, 0])
        recs = np.zeros(2, dtype=L.pool_new_dtype)
        recs["b"] = [0, 1]; recs["entry"] = [5, 5]; recs["xp"] = [[210.0, 130.0]] * 2; recs["z0"] = 3.0
        recs["std_xyz"] = [0.003, 0.004, 0.2]
        ctx.pool_add(recs)
        ctx.pool_step(np.where(np.arange(pm)[None, :, None] == 5, [[[212.0, 128.0]]], np.nan).repeat(B, 0))
        ent, _, _ = ctx.pool_get()
        e = ent[0, 5]
        assert np.array_equal(ent[1, 5]["x"], e["x"])
        with pytest.raises(XivoHipError):           # anchor 0 is not linked to an in-state group yet
            op = np.zeros(1, dtype=L.edit_dtype); op["kind"], op["i0"], op["i1"], op["i2"] = L.EDIT_ADMIT_POOL, 0, 2, 5
            ctx.edit_batch(1, op)
        ops = np.zeros(4, dtype=L.edit_dtype)
        ops["b"] = [0, 0, 1, 1]
        ops["kind"] = [L.EDIT_ADD_GROUP_ANCHOR, L.EDIT_ADMIT_POOL, L.EDIT_ADD_GROUP, L.EDIT_ADD_FEATURE]
        ops["i0"] = [3, 0, 3, 0]; ops["i1"] = [0, 2, 0, 2]; ops["i2"] = [0, 5, 0, 3]
        ops["v"][3, :3] = e["x"]; ops["v"][3, 3:5] = e["xp"]; ops["v"][3, 5:14] = e["P"]
        ctx.edit_batch(1, ops)
        P = ctx.download_P()
        _, g, f = ctx.get_scene()
        ent2, ap, sl = ctx.pool_get()
        assert np.array_equal(P[0], P[1])
        assert g[0, 3].tobytes() == g[1, 3].tobytes() and f[0, 0].tobytes() == f[1, 0].tobytes()
        assert ent2[0, 5]["ref_sind"] == -1 and ent2[1, 5]["ref_sind"] == 0 and sl[0, 0] == 3 and sl[1, 0] == -1
        with pytest.raises(XivoHipError):           # the entry was admitted: it is free now
            op = np.zeros(1, dtype=L.edit_dtype); op["kind"], op["i0"], op["i1"], op["i2"] = L.EDIT_ADMIT_POOL, 0, 2, 5
            ctx.edit_batch(1, op)
        # AddGroupToState with a non-current anchor pose: anchor 1 made at one pose, added to slot 5 at another
        ctx.pool_anchor([1, 1])
        Pb = ctx.download_P()
        moved = perturb(poses, rng, 0.1)
        ctx.set_scene(moved, g, f)
        op = np.zeros(1, dtype=L.edit_dtype); op["b"], op["kind"], op["i0"], op["i1"] = 1, L.EDIT_ADD_GROUP_ANCHOR, 5, 1
        ctx.edit_batch(1, op)
        P2 = ctx.download_P()[1]
        _, g2, _ = ctx.get_scene()
        ref = Pb[1].copy()
        o = 23 + 6 * 5
        for src in (0, 3):                          # rows then columns, Wsb then Tsb (estimator.cpp:808-816)
            ref[o + src:o + src + 3, :] = ref[src:src + 3, :]
            ref[:, o + src:o + src + 3] = ref[:, src:src + 3]
        assert np.array_equal(P2, ref)
        assert np.array_equal(g2[1, 5]["Rsb"], poses[1]["Rsb"]) and np.array_equal(g2[1, 5]["Tsb"], poses[1]["Tsb"])
        # REMOVE_GROUP of a linked slot freezes the anchor at the group's LAST pose (after it has moved in the state)
        g2[1, 5]["Tsb"] = g2[1, 5]["Tsb"] + 0.25
        ctx.set_scene(moved, g2, f)
        op = np.zeros(1, dtype=L.edit_dtype); op["b"], op["kind"], op["i0"] = 1, L.EDIT_REMOVE_GROUP, 5
        ctx.edit_batch(1, op)
        _, ap, sl = ctx.pool_get()
        assert sl[1, 1] == -1 and ap[1, 1].tobytes() == g2[1, 5].tobytes()
        with pytest.raises(XivoHipError):           # pool_anchor may not overwrite a linked anchor
            ctx.pool_anchor([0, -1])


# ---------------------------------------------------------------- the "subfilter" life cycle end to end
ATE_BOUND = 0.8          # measured 0.56 (lissajous seed 41, 2.4 s); the immediate life cycle with simulator depths: ~0.02
LANDMARK_BOUND = 1.0     # median distance of an in-state landmark to its world point, measured 0.69 m


def test_pyxivo_client_loop_without_sim_depths(built):
    """scripts/pyxivo_pcw.py's loop (the client of test_sequence_gpu.py) WITHOUT InitWithSimDepths: features start from
    initial_z in the pool and enter through the sub-filter"""
    from xivo_amd import pyxivo
    cfg = pyxivo.config_from_cfg(pyxivo.load_json_with_comments(os.path.join(HERE, "golden", "pcw_like_cfg.json")))
    cfg.initial_z, cfg.initial_std_z, cfg.subfilter = 5.0, 0.5, dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2)
    cfg.max_group_lifetime = 60
    cfg.pool_max, cfg.anchor_max = L.POOL_MAX_ENTRIES, 64     # room for every visible track (the reference has no cap)
    imu = pcw.TrajectorySim("lissajous", seed=41)
    cfg.X0["Vsb"] = imu.vel(0.0)
    vision = pcw.RandomPCW(seed=5)
    K = np.array([[275.0, 0, 320.0], [0, 275.0, 240.0], [0, 0, 1.0]])
    est = pyxivo.Estimator(cfg, "", "lissajous", False)
    total, imu_dt, vis_dt = 2.4, 0.0025, 0.04
    packets = [(k * imu_dt, 0) for k in range(int(round(total / imu_dt)))] + [(k * vis_dt, 1) for k in range(int(round(total / vis_dt)))]
    packets.sort(key=lambda p: (round(p[0] * 1e9), p[1]))
    est_T, gt_T = [], []
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
        run = est._runner
        assert run.admitted, "no feature entered the state"
        frames = np.array([a[0] for a in run.admitted]); steps = np.array([a[3] for a in run.admitted])
        assert (steps >= 1).all()                                            # never in the frame that created it
        late = frames >= cfg.strict_criteria_timesteps
        assert late.any() and (steps[late] > cfg.subfilter["ready_steps"]).all()   # CandidateStrict: READY only
        assert est.num_instate_features() > 5
        P = est.P()
        assert np.isfinite(P).all() and np.linalg.eigvalsh(0.5 * (P + P.T)).min() > -1e-9
        ate = formats.ate_rmse(np.array(est_T), np.array(gt_T), align=False)
        Xs = est.InstateFeaturePositions()
        d = np.linalg.norm(Xs[:, None, :] - vision.Xs[None], axis=2).min(axis=1)
        print("subfilter life cycle: ATE", ate, "landmark median", np.median(d), "admitted", len(steps),
              "pool drops", run.n_pool_dropped)
        assert ate < ATE_BOUND, ate
        assert np.median(d) < LANDMARK_BOUND, d
    finally:
        est.close()


def test_run_pcw_subfilter_batch_equals_single_runs(built):
    """64 sequences on one context in the "subfilter" life cycle are 64 independent filters, bit for bit"""
    B = 64
    cfg = sequence.SequenceConfig(feature_init="subfilter", initial_z=5.0, initial_std_z=0.5, max_group_lifetime=60,
                                  subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2), pool_max=64,
                                  anchor_max=16)
    worlds = lambda: [pcw.RandomPCW(seed=b) for b in range(B)]
    sims = lambda: [pcw.TrajectorySim("lissajous" if b % 2 == 0 else "trefoil", rate=0.08 + 0.001 * b, seed=300 + b)
                    for b in range(B)]
    out = sequence.run_pcw(sequence.HipBackend, cfg, worlds(), sims(), total_time=0.8)
    try:
        T, W = out["Tsb"], out["Wsb"]
        assert out["runner"].admitted and np.isfinite(T).all()
        P = out["backend"].covariance()
    finally:
        out["backend"].close()
    ws, ss = worlds(), sims()
    for b in range(B):
        o1 = sequence.run_pcw(sequence.HipBackend, cfg, [ws[b]], [ss[b]], total_time=0.8)
        try:
            assert np.array_equal(o1["Tsb"][:, 0], T[:, b]) and np.array_equal(o1["Wsb"][:, 0], W[:, b]), b
            assert np.array_equal(o1["backend"].covariance()[0], P[b]), b
        finally:
            o1["backend"].close()


def test_cpp_batch_estimator_subfilter_equals_python_runner(built):
    """xivo::hip::BatchEstimator::EnableSubfilter takes the decisions of the Python runner's "subfilter" life cycle every
    frame - identical slot books, admissions and pool drops - and ends in the same state (the initial std is divided by
    the focal length on each host: hypot vs sqrt, last-ulp differences at most)"""
    B = 4
    cfg = sequence.SequenceConfig(feature_init="subfilter", initial_z=5.0, initial_std_z=0.5, max_group_lifetime=60,
                                  subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2), pool_max=128,
                                  anchor_max=16)
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
        assert np.abs(py["Tsb"] - cp["Tsb"]).max() < 1e-10 and np.abs(py["Wsb"] - cp["Wsb"]).max() < 1e-10
    finally:
        py["backend"].close(); cp["estimator"].close()
