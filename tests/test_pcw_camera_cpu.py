"""CPU-only: the track producer's projection through the estimator's camera models (pcw_project with an xivo_cam,
xivo_amd/csrc/pcw_device.h) under a host compiler - tests/pcw_camera_driver.cpp, a stand-alone program built plain and with
-fsanitize=address,undefined - against pcw.project_points_cam, the numpy restatement of the same evaluation order, and against
the same restatement in 80-bit floats (tests/pcw_camera_cases.py). Pinhole and radtan are polynomial: equal to the last bit
(x86-64 g++ without -mfma fuses nothing). atan and equidistant go through libm's atan / atan2 / sin / cos / tan, which numpy
need not share: within the bound of pcw_camera_cases (four times the host build's own error against the 80-bit restatement,
itself below 1e-9 px). Then the max_radius guard, a distortion that folds back, and BatchPCW.generate without a camera."""
import numpy as np
import pytest

import pcw_camera_cases as CC
import pcw_restate as R
from xivo_amd import pcw


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcw_camera")
    return d, {"plain": CC.build_driver(d), "sanitized": CC.build_driver(d, ["-fsanitize=address,undefined", "-g"], "pcw_camera_driver_san")}


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("model", ["pinhole", "radtan", "atan", "equi"])
def test_host_build_against_the_restatements(drivers, model, build):
    """3 worlds of 257 points, 3 frames, the guard on: the decisions equal those of the fp64 and of the 80-bit restatement;
    z is bit-equal; u, v are bit-equal to the fp64 restatement (pinhole, radtan) or within the bound (atan, equidistant), and
    within the bound of the 80-bit restatement (all four)"""
    tmp, exe = drivers[0], drivers[1][build]
    c = CC.case(model)
    CC.assert_margins(c)
    ref = CC.host_error(exe, tmp, c)
    bound = 4 * ref
    print("%s: host build against the 80-bit restatement: max |du|, |dv| = %.3e px; bound %.3e px" % (model, ref, bound))
    assert 0 < bound <= CC.CAP
    seen = removed = 0
    for t in range(CC.T):
        vis, u, v, z = CC.driver_frame(exe, tmp, c, t)
        w = CC.project(c, t)
        p = CC.project(c, t, CC.LD)
        assert np.array_equal(vis, w[0]) and np.array_equal(vis, p[0]), t
        assert z.tobytes() == w[3].tobytes(), t
        if model in ("pinhole", "radtan"):
            assert u.tobytes() == w[1].tobytes() and v.tobytes() == w[2].tobytes(), t
        else:
            assert max(np.abs(u - w[1])[vis].max(), np.abs(v - w[2])[vis].max()) <= bound, t
        assert max(np.abs(u - p[1])[vis].max(), np.abs(v - p[2])[vis].max()) <= bound, t
        seen += int(vis.sum())
        removed += int(CC.project(c, t, max_radius=np.inf)[0].sum() - vis.sum())
    assert seen > 50 and removed > 0      # (the guard took points an unguarded camera sees)


def test_the_pinhole_model_is_the_pinhole_of_today(drivers):
    """XIVO_CAM_PINHOLE without a guard: u, v, z and the decisions of pcw.project_points, byte for byte"""
    tmp, exe = drivers[0], drivers[1]["plain"]
    c = CC.case("pinhole")
    cam = c["cam"]
    K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
    for t in range(CC.T):
        vis, u, v, z = CC.driver_frame(exe, tmp, c, t, max_radius=np.inf)
        g = c["gsc"][t]
        w = pcw.project_points(c["Xs"], g[:, :9].reshape(-1, 3, 3), g[:, 9:], K, cam["cols"], cam["rows"])
        assert np.array_equal(vis, w[0])
        for a, b in zip((u, v, z), w[1:]):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_guard_and_fold_back(drivers, build):
    """a radial distortion r (1 - 0.3 r^2) maps a point at normalised radius 1.8 back to 12 px from the principal point: visible
    without the guard, not visible with max_radius = 1; a point at radius 0.5 is visible either way, one at 0.999 / 1.001 is
    on either side of the guard. The host build, the fp64 and the 80-bit restatement agree on every decision"""
    tmp, exe = drivers[0], drivers[1][build]
    cam = CC.FOLD_CAM
    X = np.array([[1.8 * 4.0, 0.1 * 4.0, 4.0], [0.5 * 4.0, 0.0, 4.0], [0.999 * 2.0, 0.0, 2.0], [1.001 * 2.0, 0.0, 2.0], [0.0, 0.0, -1.0]])
    g = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (len(X), 1))
    want = {np.inf: [True, True, True, True, False], 1.0: [False, True, True, False, False]}
    for max_radius, w in want.items():
        vis, uvz = CC.run_driver(exe, tmp, cam, max_radius, X, g)
        assert vis.tolist() == w, max_radius
        for dtype in (float, CC.LD):
            Xs, gg = X[None].astype(dtype), g[:1].astype(dtype)
            r = pcw.project_points_cam(Xs, gg[:, :9].reshape(-1, 3, 3), gg[:, 9:], cam, max_radius)
            assert r[0][0].tolist() == w, (max_radius, dtype)
            if dtype is float:
                assert uvz[:, 0].tobytes() == r[1][0].tobytes() and uvz[:, 1].tobytes() == r[2][0].tobytes()
    # the folded pixel lies well inside the image, near the principal point
    assert abs(uvz[0, 0] - 320.0) < 20 and abs(uvz[0, 1] - 240.0) < 5


def test_generate_without_a_camera_is_unchanged():
    """BatchPCW.generate(cam=None) - the default - gives the bytes of the pinhole paths as they were: the philox arm equals the
    restatement of tests/pcw_restate.py, the numpy arm the einsum formula with the world's own generator"""
    Bn, npts = 3, 257
    Xs, gsc = R.box_world(Bn, npts, 4), R.moving_poses(Bn, 3, 4)
    w = pcw.BatchPCW(Bn, Xs=Xs, noise="philox", noise_seed=77)
    w2 = pcw.BatchPCW(Bn, Xs=Xs, noise="philox", noise_seed=77)
    rs = R.Restate(Xs)
    for t in range(3):
        Rsc, Tsc = gsc[t][:, :9].reshape(-1, 3, 3), gsc[t][:, 9:]
        off, ids, meas = w.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], 1.0)
        off2, ids2, meas2 = w2.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], 1.0, cam=None, max_radius=np.inf)
        r = rs.step(gsc[t], 1.0, 77, t)
        for a, b, c in zip((off, ids, meas), (off2, ids2, meas2), (r["off"], r["track_ids"], r["meas"])):
            assert a.tobytes() == b.tobytes() == c.tobytes(), t
    wn, rng = pcw.BatchPCW(Bn, Xs=Xs, seed=5), np.random.default_rng(5)
    Rsc, Tsc = gsc[0][:, :9].reshape(-1, 3, 3), gsc[0][:, 9:]
    off, ids, meas = wn.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], 1.0)
    Xc = np.einsum("bpj,bji->bpi", Xs - Tsc[:, None, :], Rsc)
    z = np.where(Xc[..., 2] > 0, Xc[..., 2], 1.0)
    u, v = R.K[0, 0] * Xc[..., 0] / z + R.K[0, 2], R.K[1, 1] * Xc[..., 1] / z + R.K[1, 2]
    vis = (Xc[..., 2] > 0) & (u >= 0) & (v >= 0) & (u <= R.CAM["imw"]) & (v <= R.CAM["imh"])
    noise = 1.0 * rng.standard_normal(u.shape + (2,))
    sel = np.nonzero(vis)
    want = np.stack([u[sel] + noise[sel][:, 0], v[sel] + noise[sel][:, 1], Xc[..., 2][sel]], axis=1)
    assert meas.tobytes() == np.ascontiguousarray(want).tobytes() and off[-1] == vis.sum() > 0


def test_generate_with_a_camera_follows_project_points_cam():
    """with a camera both noise arms take their pixels from project_points_cam; the ids follow the same walk"""
    c = CC.case("equi")
    w = pcw.BatchPCW(CC.B, Xs=c["Xs"], noise="philox", noise_seed=3)
    walk = CC.Walk(c)
    for t in range(CC.T):
        g = c["gsc"][t]
        off, ids, meas = w.generate(g[:, :9].reshape(-1, 3, 3), g[:, 9:], None, None, None, 0.0, cam=c["cam"], max_radius=c["max_radius"])
        r = walk.step(t, CC.NPTS)
        assert np.array_equal(np.diff(off), r["cnt"])
        for b in range(CC.B):
            assert np.array_equal(ids[off[b]:off[b + 1]], r["track_ids"][b, :r["cnt"][b]])
            assert meas[off[b]:off[b + 1]].tobytes() == r["meas"][b, :r["cnt"][b]].tobytes()


def test_symbols_are_declared_and_bound():
    import os
    import re
    with open(os.path.join(CC.ROOT, "include", "xivo_hip.h")) as f:
        assert re.search(r"int\s+xivo_hip_pcw_camera\(xivo_hip_ctx\*\s*ctx,\s*const xivo_cam\*\s*cam,\s*double max_radius\);", f.read())
    with open(os.path.join(CC.ROOT, "xivo_amd", "lib.py")) as f:
        assert '"xivo_hip_pcw_camera": [C.c_void_p, C.c_void_p, C.c_double]' in f.read()
