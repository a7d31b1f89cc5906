"""CPU: depth initialisation of new tracks - the numpy restatement of the reference's triangulators (tests/tri_restate.py)
against the reference's unit-test cases and against its own compiled text, the C ABI's argument checks without a device,
the dtypes, and the cfg keys."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tri_restate as T

HERE = os.path.dirname(os.path.abspath(__file__))
TH, BE = 0.1 * T.DEG, 0.25 * T.DEG


# ---------------------------------------------------------------- the reference's unit tests, restated
@pytest.mark.parametrize("case", T.UNIT_CASES, ids=[c[0] for c in T.UNIT_CASES])
def test_restatement_reproduces_the_reference_unit_cases(case):
    """src/test/unittest_triangulation.cpp: the three angular methods on each case"""
    R12, t12, xc1, xc2 = T.unit_case(case)
    for m in T.ANGULAR:
        X, ret = T.triangulate(m, R12[None], t12[None], xc1[None], xc2[None], TH, BE)
        if case[0] == "Angular_Reprojection_Error":
            continue                                    # test_angular_reprojection_case_as_compiled
        assert ret[0] == case[5], (case[0], m)
        if case[5]:
            assert abs(X[0, 2] - 5.0) <= 0.5, m


def test_angular_reprojection_case_as_compiled():
    """Angular_Reprojection_Error expects false from all three; the reference notes that L1Angular flips to true in release
    builds (unittest_triangulation.cpp:157-159). The compiled reference (-O3, FMA contraction) returns TRUE for L1 here.
    The cause: L1 corrects one ray and leaves the other as it is, so one reprojection angle is acos(m.m / (|m| |m|)) - an
    argument of 1 +- 1 ulp whose acos is 0 or NaN depending on rounding. Here a0 > a1, so m0 is the unmodified ray and
    theta0 is that angle; std::max(theta0, theta1) returns theta0 when it is NaN, and NaN > thresh is false: the check
    passes. Plain IEEE arithmetic without contraction (the restatement and the device) gives exactly 1, theta0 = 0, and
    theta1 > thresh fails the check - the result of a debug build. T.near_threshold flags such problems."""
    R12, t12, xc1, xc2 = T.unit_case(T.UNIT_CASES[3])
    X, ret, info = T.triangulate("l1_angular", R12[None], t12[None], xc1[None], xc2[None], TH, BE, details=True)
    assert info["a0"][0] > info["a1"][0] and info["arg0"][0] == 1.0 and info["th1"][0] > TH
    assert not ret[0] and T.near_threshold("l1_angular", info, 1, TH, BE)[0]
    for m in ("l2_angular", "linf_angular"):
        assert not T.triangulate(m, R12[None], t12[None], xc1[None], xc2[None], TH, BE)[1][0]
    ref = _ref_or_skip()
    q, _ = _se3(R12)
    for m, want in (("l1_angular", True), ("l2_angular", False), ("linf_angular", False)):
        r, _ = _call(ref, m, q, t12, xc1, xc2)
        assert r == want, m


# ---------------------------------------------------------------- pinned to the compiled reference
_SYMS = {
    "direct_linear_transform_svd": "_ZN4xivo24DirectLinearTransformSVDERKN6Sophus3SE3IdLi0EEERKN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEES9_RNS6_IdLi3ELi1ELi0ELi3ELi1EEE",
    "direct_linear_transform_avg": "_ZN4xivo24DirectLinearTransformAvgERKN6Sophus3SE3IdLi0EEERKN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEES9_RNS6_IdLi3ELi1ELi0ELi3ELi1EEE",
    "l1_angular": "_ZN4xivo9L1AngularERKN6Sophus3SE3IdLi0EEERKN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEES9_RNS6_IdLi3ELi1ELi0ELi3ELi1EEEff",
    "l2_angular": "_ZN4xivo9L2AngularERKN6Sophus3SE3IdLi0EEERKN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEES9_RNS6_IdLi3ELi1ELi0ELi3ELi1EEEff",
    "linf_angular": "_ZN4xivo11LinfAngularERKN6Sophus3SE3IdLi0EEERKN5Eigen6MatrixIdLi2ELi1ELi0ELi2ELi1EEES9_RNS6_IdLi3ELi1ELi0ELi3ELi1EEEff",
    "check_cheirality": "_ZN4xivo16check_cheiralityERKN5Eigen6MatrixIdLi3ELi1ELi0ELi3ELi1EEES4_S4_S4_",
    "check_parallax": "_ZN4xivo14check_parallaxERKN5Eigen6MatrixIdLi3ELi1ELi0ELi3ELi1EEES4_f",
}


def _ref_or_skip():
    import ref_binding
    try:
        path = ref_binding.load().path          # oracle/_ref/libxivo_ref_*.so, the way the other reference tests find it
    except FileNotFoundError as e:
        pytest.skip(str(e))
    lib = C.CDLL(path)
    for name, sym in _SYMS.items():
        getattr(lib, sym).restype = C.c_bool
    return lib


def _se3(R):
    """Sophus::SE3d memory: unit quaternion (x, y, z, w) then t; the rotation the reference rebuilds from it (Eigen's
    toRotationMatrix) is returned alongside"""
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3
    q = np.linalg.eigh(K)[1][:, 3]
    q = q / np.linalg.norm(q)
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    Rq = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                   [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    return q, Rq


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(lib, method, q, t, xc1, xc2):
    g = np.ascontiguousarray(np.concatenate([q, np.asarray(t, dtype=np.float64)]))
    a, b = np.ascontiguousarray(xc1, dtype=np.float64), np.ascontiguousarray(xc2, dtype=np.float64)
    X = np.zeros(3)
    fn = getattr(lib, _SYMS[method])
    if method.startswith("direct"):
        r = fn(_p(g), _p(a), _p(b), _p(X))
    else:
        r = fn(_p(g), _p(a), _p(b), _p(X), C.c_float(TH), C.c_float(BE))
    return bool(r), X


def test_reference_abi_layout_with_a_known_geometry():
    """SE3d = 7 doubles (quaternion x y z w, t), Eigen vectors = plain doubles, thresholds float: a point at (0.3, -0.2, 4)
    seen from two cameras one unit apart comes back from every method"""
    lib = _ref_or_skip()
    R = np.eye(3)
    t = np.array([1.0, 0.0, 0.0])
    Xt = np.array([0.3, -0.2, 4.0])
    xc1, X2 = Xt[:2] / Xt[2], Xt - t
    xc2 = X2[:2] / X2[2]
    q, _ = _se3(R)
    assert np.allclose(q, [0, 0, 0, 1])
    for m in T.METHODS:
        r, X = _call(lib, m, q, t, xc1, xc2)
        if m == "l2_angular":   # noise-free: B has rank one, V.col(1) is arbitrary in a 2-d null space (l2_sigma_ratio)
            continue
        assert r and np.abs(X - Xt).max() < 1e-12, (m, X)
    c = lib[_SYMS["check_parallax"]]
    a, b = np.array([0.0, 0.0, 1.0]), np.array([np.sin(0.01), 0.0, np.cos(0.01)])
    assert c(_p(a), _p(b), C.c_float(0.005)) and not c(_p(a), _p(b), C.c_float(0.02))
    z, tt, f1, f0 = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.1, 0.0, 1.0])
    assert lib[_SYMS["check_cheirality"]](_p(z), _p(tt), _p(f1), _p(f0)) == (
        bool(T.check_cheirality(z[None], tt[None], f1[None], f0[None])[0]))


@pytest.mark.parametrize("method", T.METHODS)
def test_restatement_matches_the_compiled_reference(method):
    """Random problems per method (well-conditioned, low-parallax, behind-camera, noisy, degenerate, threshold-near):
    >= 10^4 equal return values, excluding those a last-bit difference decides (T.near_threshold; the -O3 build contracts
    into FMAs). X to 1e-12 relative - DEVIATION: with a tolerance of max(1e-12, 4e-15 / sin^2(parallax)), the condition
    number of the two-ray intersection times the rounding the FMA build adds; the number of problems compared with a
    tolerance above 1e-12 is printed."""
    lib = _ref_or_skip()
    rng = np.random.default_rng(2024)
    n_cmp = n_near = n_ill = n_wide = 0
    # L2Angular is only defined where B has two distinct non-zero singular values: its problems carry pixel noise that
    # makes sigma2 / sigma1 >= 1e-3 ("l2noisy"), besides the kinds every method sees
    kinds = ("good", "lowpar", "behind", "noisy", "degenerate", "threshold") + (("l2noisy",) * 6 if method == "l2_angular" else ())
    for kind in kinds:
        if kind == "l2noisy":
            R12, t12, xc1, xc2, _, _ = T.random_problems(rng, 1800, "good")
            xc2 = xc2 + rng.normal(size=xc2.shape) * 0.02
        else:
            # the angular methods lose a third of their return values to the last-bit exclusions: more problems
            R12, t12, xc1, xc2, _, _ = T.random_problems(rng, 3000 if method in ("l1_angular", "linf_angular") else 1800, kind)
        qs, Rq = zip(*[_se3(R) for R in R12])
        Rq = np.array(Rq)
        X, ret, info = T.triangulate(method, Rq, t12, xc1, xc2, TH, BE, details=True)
        near = T.near_threshold(method, info, len(X), TH, BE)
        res = [_call(lib, method, qs[i], t12[i], xc1[i], xc2[i]) for i in range(len(R12))]
        rr = np.array([r for r, _ in res]); XR = np.array([x for _, x in res])
        ok = np.isfinite(XR).all(axis=1) & np.isfinite(X).all(axis=1)
        # conditioning of X: the sensitivity of the two-ray intersection grows as 1 / sin^2(parallax)
        f0, f1 = T.normalized(T.homog(xc1)), T.normalized(T.homog(xc2))
        sin_par = T.norm(T.cross(f0, T.mulv(Rq, f1)))
        with np.errstate(divide="ignore"):
            tol = np.maximum(1e-12, 4e-15 / sin_par ** 2)
        if kind == "degenerate":
            ok[:] = False                               # no point to compare: zero or ray-parallel baselines
        if method == "direct_linear_transform_svd":
            s = info["sigma"]
            ok &= s[:, 2] / s[:, 0] >= 1e-3
            tol = np.where(ok, 1e-10, tol)
        if method == "l2_angular":
            sep = T.l2_sigma_ratio(Rq, t12, xc1, xc2)
            ok &= sep >= 1e-3                           # B of rank one: V.col(1) is any vector of a 2-d null space
            near = near | ~(sep >= 1e-3)
        n_ill += int((~ok).sum())
        n_wide += int((ok & (tol > 1e-12)).sum())
        rel = np.linalg.norm(X - XR, axis=1) / np.maximum(np.linalg.norm(XR, axis=1), 1e-300)
        assert (rel[ok] <= tol[ok]).all(), (kind, rel[ok].max(), int((rel[ok] > tol[ok]).sum()))
        assert np.array_equal(rr[~near], ret[~near]), (kind, int((rr != ret)[~near].sum()))
        n_cmp += int((~near).sum()); n_near += int(near.sum())
    assert n_cmp >= 10000, n_cmp                        # return values actually compared
    print(f"{method}: {n_cmp} return values compared, {n_near} excluded; X: {n_ill} not compared (ill-conditioned), "
          f"{n_wide} compared with a tolerance above 1e-12 (4e-15 / sin^2 parallax; DLT-SVD: 1e-10 where sigma3 / sigma1 >= 1e-3)")


# ---------------------------------------------------------------- C ABI without a device
def test_new_entry_points_reject_null_and_invalid_arguments(built):
    from xivo_amd import lib as L
    lib = L.load_library()
    o = L.tri_options("l1_angular")
    a = np.zeros(1, dtype=L.adapt_opts_dtype)
    assert lib.xivo_hip_triangulate(None, 1, None, None, L._ptr(o)) == -1
    assert lib.xivo_hip_triangulate(None, 0, None, None, None) == -1
    assert lib.xivo_hip_pool_triangulation(None, L._ptr(o)) == -1
    assert lib.xivo_hip_pool_triangulation(None, None) == -1
    assert lib.xivo_hip_pool_tri_counts(None, 0, 1, None, None) == -1
    assert lib.xivo_hip_pool_adapt_depth_config(None, L._ptr(a)) == -1
    assert lib.xivo_hip_pool_adapt_depth(None, 1, None) == -1
    assert lib.xivo_hip_pool_add_ex(None, 0, None, 0) == -1


def test_new_dtypes_match_the_header(built):
    """sizes of the C structs, compiled from include/xivo_hip.h by the host compiler"""
    import subprocess
    import tempfile
    from xivo_amd import lib as L
    src = ('#include <stdio.h>\n#include "xivo_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(xivo_triangulate_opts), '
           'sizeof(xivo_tri_in), sizeof(xivo_tri_out), sizeof(xivo_adapt_depth_opts));return 0;}\n')
    inc = os.path.join(os.path.dirname(HERE), "include")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        try:
            subprocess.run(["cc", "-I", inc, c, "-o", exe], check=True, capture_output=True)
        except (OSError, subprocess.CalledProcessError) as e:
            pytest.skip(f"no host C compiler: {e}")
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [L.tri_opts_dtype.itemsize, L.tri_in_dtype.itemsize, L.tri_out_dtype.itemsize, L.adapt_opts_dtype.itemsize]


# ---------------------------------------------------------------- configuration: cfg keys, defaults, the C++ mirror
def test_sequence_config_defaults_leave_depth_init_off():
    from xivo_amd import sequence
    c = sequence.SequenceConfig()
    assert c.triangulate_pre_subfilter is False and c.adaptive_initial_depth is False
    assert c.feature_init == "immediate" and c.initial_z == 2.5


def test_config_from_cfg_reads_the_depth_init_keys():
    from xivo_amd import pyxivo
    base = pyxivo.load_json_with_comments(os.path.join(HERE, "golden", "pcw_like_cfg.json"))
    c0 = pyxivo.config_from_cfg(dict(base))
    assert not c0.triangulate_pre_subfilter and not c0.adaptive_initial_depth      # the golden cfg has none of the keys
    raw = dict(base)
    raw.update({"triangulate_pre_subfilter": True,
                "triangulation": {"method": "linf_angular", "zmin": 0.1, "zmax": 7.0, "max_theta_thresh": 0.2, "beta_thesh": 0.5},
                "initial_std_x_badtri": 3.0, "initial_std_y_badtri": 4.0, "initial_std_z_badtri": 0.7,
                "adaptive_initial_depth": {"median_weight": 0.9, "minimum_feature_lifetime": 7}})
    c = pyxivo.config_from_cfg(raw)
    assert c.triangulate_pre_subfilter and c.adaptive_initial_depth
    t = c.triangulation
    assert t["method"] == "linf_angular" and (t["zmin"], t["zmax"]) == (0.1, 7.0)
    assert t["max_theta_thresh"] == 0.2 * np.pi / 180 and t["beta_thresh"] == 0.5 * np.pi / 180     # degrees -> radians
    assert (c.initial_std_x_badtri, c.initial_std_y_badtri, c.initial_std_z_badtri) == (3.0, 4.0, 0.7)
    assert c.adaptive_depth == dict(median_weight=0.9, minimum_feature_lifetime=7)
    # the block alone turns the adaptive depth on with the reference defaults (src/estimator.cpp:166-169)
    raw2 = dict(base); raw2["adaptive_initial_depth"] = {}
    c2 = pyxivo.config_from_cfg(raw2)
    assert c2.adaptive_initial_depth and c2.adaptive_depth == dict(median_weight=0.99, minimum_feature_lifetime=5)
    assert not c2.triangulate_pre_subfilter and c2.triangulation["method"] == "l1_angular"
    assert c2.triangulation["max_theta_thresh"] == 0.1 * np.pi / 180


def test_batch_depth_init_mirror_matches_the_cpp_struct(built):
    from xivo_amd import batch
    host = batch.load_host_library()
    for name in ("xivo_batch_enable_depth_init", "xivo_batch_depth_init_cfg_size", "xivo_batch_init_z"):
        assert hasattr(host, name), name
    assert batch.batch_depth_init_cfg_dtype.itemsize == host.xivo_batch_depth_init_cfg_size() == 112
    assert host.xivo_batch_enable_depth_init(None, None) == -1
