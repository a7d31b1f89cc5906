"""CPU side of the geometry edge cases (tests/geometry_edge_cases.py): the g++ build of xivo_amd/csrc/camera_device.h at the
camera models' branch points, the as-coded results there, the oracle's IEEE results, the golden fixture of the reference's
own Project, and the preconditions of tests/test_geometry_edges_gpu.py - every family's bound below its cap, fp64 and 80-bit
on the same side of every threshold, every branch of the Givens coefficient and of Shepperd's method taken, the rank
decision of the OOS inputs a factor ten away from Eigen's threshold."""
import math
import os

import numpy as np
import pytest

import geometry_edge_cases as ge
import xivo_oracle as orc

LD = ge.LD
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("camera_edges")
    exe = ge.build_driver(tmp)
    return ge.camera_reference(exe, tmp)


# ---------------------------------------------------------------- cameras
def test_camera_bounds_stay_below_their_caps(host):
    for fam, (worst, b) in ge.camera_bounds(host).items():
        print("camera family %-9s host build vs 80-bit: worst %.3e  bound %.3e  cap %.0e" % (fam, worst, b, ge.CAPS[fam]))
        assert worst <= b < ge.CAPS[fam]


def test_fp64_and_80_bit_take_the_same_camera_branch(host):
    cam = ge.CAMS["atan"]
    for (x, y), want in zip(ge.PROJECT_POINTS["atan"], ge.ATAN_BRANCH):
        assert ge.project(cam, x, y)[4] == ge.project(cam, x, y, LD)[4] == want, (x, y)
    for (u, v), want in zip(ge.unproject_pixels("atan"), ge.ATAN_UNPROJECT_BRANCH):
        assert ge.unproject(cam, u, v)[1] == ge.unproject(cam, u, v, LD)[1] == want, (u, v)
    # the thresholds are approached to 1e-6 relative, from both sides, and never hit
    R = [math.hypot(x, y) for x, y in ge.PROJECT_POINTS["atan"][2:4]]
    assert R[0] < ge.ATAN_R < R[1] and max(abs(r / ge.ATAN_R - 1) for r in R) < 2 * ge.OFF
    assert min(abs(r / ge.ATAN_R - 1) for r in R) > 0.5 * ge.OFF
    for (u, v), want in zip(ge.unproject_pixels("equi"), ["column", "column", "column", "off", "off"]):
        assert ge.unproject(ge.CAMS["equi"], u, v)[1] == ge.unproject(ge.CAMS["equi"], u, v, LD)[1] == want


def test_host_build_matches_the_fp64_restatement(host):
    """the restatement in np.float64 repeats camera_device.h's order of evaluation: the two differ by libm's and numpy's
    elementary functions at the most - inside the families' bounds - and agree on every NaN"""
    b = {k: v[1] for k, v in ge.camera_bounds(host).items()}
    for name, cam in ge.CAMS.items():
        r = host[name]
        fmax = max(cam["fx"], cam["fy"])
        for i, (x, y) in enumerate(r["pts"]):
            xp, J, jacc, dim, _ = ge.project(cam, x, y)
            assert dim == r["dim"][i]
            assert np.array_equal(np.isnan(J), np.isnan(r["J"][i])) and np.array_equal(np.isnan(jacc), np.isnan(r["jacc"][i]))
            assert np.abs(xp - r["xp"][i]).max() <= b["pixels"]
            if i in ge.finite_points(name):
                assert np.abs(J - r["J"][i]).max() / fmax <= b["jac"] and np.abs(jacc - r["jacc"][i]).max() / fmax <= b["jac"]
        for i, (u, v) in enumerate(r["pix"]):
            assert np.abs(ge.unproject(cam, u, v)[0] - r["xc"][i]).max() <= b["unproject"]


def test_as_coded_results_of_the_host_build(host):
    # equidistant on the optical axis: the pixel is the principal point, the Jacobian -y / 0: all NaN
    cam, r = ge.CAMS["equi"], host["equi"]
    for i in ge.NAN_POINTS["equi"]:
        assert ge.same_bits(r["xp"][i], [cam["cx"], cam["cy"]]) and np.isnan(r["J"][i]).all(), r["pts"][i]
    for i in ge.finite_points("equi"):
        assert np.isfinite(r["J"][i]).all() and np.isfinite(r["jacc"][i]).all()
    # equidistant UnProject on the column u == cx: the optical axis whatever v is, with the sign of v - cy on the zero
    for name, exact in ge.UNPROJECT_EXACT.items():
        for i, want in exact.items():
            assert ge.same_bits(host[name]["xc"][i], want), (name, i, host[name]["xc"][i])
    # atan below R = 1e-4: the pinhole's Jacobians exactly, d / dw = 0; the jump to about 1.078 times that above
    cam, r = ge.CAMS["atan"], host["atan"]
    for i, (br, (x, y)) in enumerate(zip(ge.ATAN_BRANCH, r["pts"])):
        if br == "singular":
            assert ge.same_bits(r["J"][i], [[cam["fx"], 0.0], [0.0, cam["fy"]]])
            want = np.zeros((2, 9)); want[0, 0] = x; want[0, 2] = 1; want[1, 1] = y; want[1, 3] = 1
            assert ge.same_bits(r["jacc"][i], want)
    jump = r["J"][3][0, 0] / r["J"][2][0, 0]
    print("atan Project: du/dx below R = 1e-4 %.4f, above %.4f (x %.4f)" % (r["J"][2][0, 0], r["J"][3][0, 0], jump))
    assert abs(jump - 2 * math.tan(0.5 * cam["d"][0]) / cam["d"][0]) < 1e-6 and jump > 1.07
    # atan UnProject: f = 1 at and below R = 0.01, the full model above
    lo, hi = r["xc"][1], r["xc"][2]
    shrink = cam["d"][0] / (2 * math.tan(0.5 * cam["d"][0]))           # tan(R w) / (2 tan(w / 2) R) for small R: about 0.9275
    assert abs(math.hypot(*lo) / ge.ATAN_UNPROJECT_R - 1) < 2 * ge.OFF
    assert abs(math.hypot(*hi) / ge.ATAN_UNPROJECT_R - shrink) < 1e-4 and shrink < 0.93
    # radtan: Newton's iteration stays finite at the centre and at radius 1; pinhole at the principal point
    assert np.isfinite(host["radtan"]["xc"]).all() and np.isfinite(host["radtan"]["J"]).all()
    assert np.abs(host["radtan"]["xc"][1] - [0.6, 0.8]).max() < 1e-9
    assert ge.same_bits(host["pinhole"]["xp"][0], [ge.CAMS["pinhole"]["cx"], ge.CAMS["pinhole"]["cy"]])


def test_oracle_cameras_return_ieee_results_instead_of_raising(host):
    b = {k: v[1] for k, v in ge.camera_bounds(host).items()}
    for name, cam in ge.CAMS.items():
        r = host[name]
        fmax = max(cam["fx"], cam["fy"])
        for i, p in enumerate(r["pts"]):
            xp, J = orc.camera_project(cam, p)
            jacc = orc.camera_project_jacc(cam, p)
            assert isinstance(xp, np.ndarray) and J.shape == (2, 2) and jacc.shape == (2, r["dim"][i])
            assert np.array_equal(np.isnan(J), np.isnan(r["J"][i]))
            assert np.abs(xp - r["xp"][i]).max() <= b["pixels"]
            if i in ge.finite_points(name):
                assert np.abs(J - r["J"][i]).max() / fmax <= b["jac"]
                assert np.abs(jacc - r["jacc"][i][:, :r["dim"][i]]).max() / fmax <= b["jac"]
    xp, J = orc.camera_project(ge.CAMS["equi"], (0.0, 0.0))
    assert ge.same_bits(xp, [ge.CAMS["equi"]["cx"], ge.CAMS["equi"]["cy"]]) and np.isnan(J).all()
    xp, J = orc.camera_project(dict(ge.CAMS["atan"], d=[0.0]), (0.2, 0.1))      # w == 0: 1 / w = inf, the singular branch
    assert np.isfinite(xp).all() and ge.same_bits(J, [[ge.CAMS["atan"]["fx"], 0.0], [0.0, ge.CAMS["atan"]["fy"]]])


def test_golden_v8_pins_the_restatement_to_the_reference(host):
    """tests/golden/golden_v8.npz holds the reference cameras' own Project at these inputs: the same NaNs, the pixels and
    Jacobians inside the families' bounds of the 80-bit restatement (the reference's build is one more fp64 evaluation)"""
    G = np.load(os.path.join(HERE, "golden", "golden_v8.npz"))
    b = {k: v[1] for k, v in ge.camera_bounds(host).items()}
    for name, cam in ge.CAMS.items():
        assert np.array_equal(G[name + "_xc"], np.array(ge.PROJECT_POINTS[name]))
        fmax = max(cam["fx"], cam["fy"])
        for i, (x, y) in enumerate(ge.PROJECT_POINTS[name]):
            xp, J, _, _, _ = ge.project(cam, x, y, LD)
            gxp, gJ = G[name + "_xp"][i], G[name + "_jac"][i]
            assert np.array_equal(np.isnan(gJ), np.isnan(host[name]["J"][i])), (name, i)
            if i in ge.finite_points(name):
                assert float(np.abs(gxp.astype(LD) - xp).max()) <= b["pixels"], (name, i)
                assert float(np.abs(gJ.astype(LD) - J).max()) / fmax <= b["jac"], (name, i)
            else:
                assert ge.same_bits(gxp, host[name]["xp"][i]) and np.isnan(gJ).all()


# ---------------------------------------------------------------- SO(3)
def test_rotation_bounds_stay_below_their_cap():
    for fam, (worst, b) in ge.rotation_bounds().items():
        print("rotation family %-3s oracle fp64 vs 80-bit: worst %.3e  bound %.3e  cap %.0e" % (fam, worst, b, ge.CAPS["rotation"]))
        assert worst <= b < ge.CAPS["rotation"]


def test_fp64_and_80_bit_take_the_same_so3_branch():
    below = 0
    for w in ge.exp_cases():
        th64 = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        wl = w.astype(LD)
        thld = np.sqrt(wl @ wl)
        assert (th64 < ge.EXP_THRESHOLD) == bool(thld < ge.EXP_THRESHOLD)
        assert th64 == 0 or abs(th64 / ge.EXP_THRESHOLD - 1) > 0.5 * ge.OFF
        below += th64 < ge.EXP_THRESHOLD
    assert below == 3 * len(ge.AXES)                     # 0, 1e-12 and the angle just under the threshold
    seen = set()
    for c in ge.log_cases():
        M = c["R_est"].T @ c["R_gt"]
        b64 = ge.log_branch(M)
        assert b64 == ge.log_branch(c["R_est"].astype(LD).T @ c["R_gt"].astype(LD), LD), c["angle"]
        assert b64[0] == (c["angle"] < 2 * math.pi / 3) and b64[1] == (c["angle"] < ge.LOG_N2_ANGLE)
        assert b64[2] == (c["tag"] == "pi")
        if c["angle"] == 0.0:
            assert c["R_gt"].tobytes() == c["R_est"].tobytes()
        if c["tag"].startswith("shepperd"):
            assert ge.shepperd_branch(M) == int(c["tag"][-1])      # 2.5 rad about x, y, z: the three t <= 0 branches
        seen.add(ge.shepperd_branch(M))
    assert seen == {0, 1, 2, 3}
    for R in ge.ZERO_Z_RSG:
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15


def test_80_bit_exp_and_log_invert_each_other():
    """the restatements against each other: log(exp(w)) = w for |w| < pi, to 80-bit accuracy"""
    for w in ge.exp_cases():
        if np.linalg.norm(w) < math.pi - 1e-3:
            assert float(np.abs(ge.so3_log_ld(ge.so3_exp_ld(w)) - w.astype(LD)).max()) < 1e-17


# ---------------------------------------------------------------- Givens coefficient
@pytest.mark.parametrize("which", ["givens", "qr"])
def test_every_branch_of_the_givens_coefficient_runs(which):
    x, Hx, Hf = ge.givens_problems(qr=which == "qr")
    with ge.GivensRecorder() as rec:
        firsts = []
        for p in range(len(ge.GIVENS_PAIRS)):
            firsts.append(len(rec.calls))
            if which == "givens":
                orc.givens_eliminate(x[p], Hx[p], Hf[p])
            else:
                orc.qr_compress(x[p], Hx[p])
    for p, (a, b) in enumerate(ge.GIVENS_PAIRS):
        assert rec.calls[firsts[p]][:2] == (a, b)
    got = [rec.calls[f][2] for f in firsts]
    assert got == ["identity", "b<=a", "identity", "b>a", "b>a", "b<=a", "identity", "b<=a"]
    assert {c[2] for c in rec.calls} == {"identity", "b>a", "b<=a"}
    nonzero = [abs(c[1]) for c in rec.calls if c[1] != 0.0]
    assert min(abs(v / ge.EPS - 1) for v in nonzero) > 1e-9          # no rotation's branch turns on rounding
    assert min(abs(v / ge.EPS - 1) for v in nonzero) < 2 * ge.OFF    # and the threshold is approached


# ---------------------------------------------------------------- OOS rows
@pytest.mark.parametrize("k", ge.OOS_K)
def test_oos_rank_decisions_have_a_margin(k):
    sc = ge.oos_scene()
    lay = orc.Layout(ge.OOS_NG, 1)
    for i, (Xs, obs) in enumerate(ge.oos_features(k)):
        ratio, rank = ge.third_pivot_ratio(ge.oos_hf(Xs, obs))
        print("k %d feature %d: third pivot / threshold %.3e, rank %d" % (k, i, ratio, rank))
        assert ratio < 0.1 or ratio > 10.0
        assert rank == (2 if i == 1 else 3)
        Hxp, rp, A = orc.oos_jacobian(Xs, obs, sc["gR"], sc["gT"], sc["Rbc"], sc["Tbc"], ge.OOS_CAM, lay)
        n = len(obs)
        assert Hxp.shape[0] == 2 * n - rank and A.shape == (2 * n, 2 * n - rank)
        assert np.abs(A.T @ ge.oos_hf(Xs, obs)).max() < 1e-9            # null-space rows of Hf


@pytest.mark.parametrize("name", list(ge.CAMS))
def test_oos_camera_inputs_have_rank_3_with_a_margin(name):
    sc = ge.oos_camera_scene()
    for Xs, obs in ge.oos_camera_features(name):
        ratio, rank = ge.third_pivot_ratio(ge.oos_hf(Xs, obs, sc, ge.CAMS[name]))
        assert ratio > 10.0 and rank == 3, (name, Xs, ratio)
