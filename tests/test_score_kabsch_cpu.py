"""CPU-only: the closed-form alignment of the trajectory score (score_kabsch, xivo_amd/csrc/score_device.h) under a host
compiler. tests/score_kabsch_driver.cpp is compiled with g++ against the header alone and called once per matrix H; what it
prints is bit-exact. The same function runs in traj_score_kernel; here its degenerate branches - H = 0, rank 1, rank 1 along a
coordinate axis (the axis fallback of score_orth_unit), a non-finite H - and its scaling are reached without a GPU.

Checked for every H, with numpy's SVD of H as the reference (eps = 2^-52, kappa = sv0 / (sv1 + sv2)):
  R is a rotation: |det R - 1| <= 4 eps, |R^T R - I| <= 8 eps (what tests/test_traj_score_gpu.py asks of the device)
  |d sv| <= 32 eps sv0 (the bound of the GPU tests), sv descending
  trace(R^T H) >= sv0 + sv1 + d sv2 - 64 eps sv0, d = sign det H: R attains the maximum the closed form is defined by, whether
    or not R itself is determined (a sum of nine products of entries <= sv0, each to an eps or two, and R to its own bound)
  where the rotation is determined (kappa <= 1e6): |R - U diag(1, 1, det(U V^T)) V^T| <= 64 eps kappa, with
    kappa = sv0 / (sv1 + d sv2) here: for a mirrored H (d = -1) the maximiser is unique only while sv1 > sv2 - which column
    takes the sign is then the question - and sv1 = sv2 (H = a reflection of a rotation) leaves a circle of maximisers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_restate as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
EPS = sr.EPS


@pytest.fixture(scope="module")
def kabsch(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/score_kabsch_driver.cpp"
    exe = str(tmp_path_factory.mktemp("score_kabsch") / "driver")
    # -ffp-contract=off: the products and sums as written, the fused multiply-adds only where the header calls fma
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "score_kabsch_driver.cpp"), "-o", exe], check=True)

    def call(H):
        H = np.asarray(H, dtype=np.float64)
        out = subprocess.run([exe] + [float(v).hex() for v in H.ravel()], check=True, capture_output=True, text=True).stdout.split()
        v = [float.fromhex(t) for t in out[:12]]
        return np.array(v[:9]).reshape(3, 3), np.array(v[9:]), int(out[12])
    return call


def test_header_is_plain_cxx_for_a_host_compiler():
    """HIP's header only under hipcc, no header of the project: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "score_device.h")).read().split("#pragma once")[1]
    assert '#include "' not in text
    assert text.count("hip/") == 1 and text.index("#if defined(__HIPCC__)") < text.index("hip/") < text.index("#else")


def _is_rotation(R, tag):
    R = R.astype(np.longdouble)
    det = R[0] @ np.cross(R[1], R[2])
    assert abs(det - 1) <= 4 * EPS and np.abs(R.T @ R - np.eye(3)).max() <= 8 * EPS, (tag, float(abs(det - 1)) / EPS)


def _check(kabsch, H, tag, flag, worst):
    """-> (R, sv) of the driver after the checks that hold for every finite H"""
    H = np.asarray(H, dtype=np.float64)
    R, sv, got_flag = kabsch(H)
    U, s, Vt = np.linalg.svd(H)
    assert got_flag == flag, (tag, got_flag, sv)
    _is_rotation(R, tag)
    assert sv[0] >= sv[1] >= sv[2] >= 0, (tag, sv)
    r_sv = np.abs(sv - s).max() / (32 * EPS * s[0]) if s[0] > 0 else float(sv.any())
    d = float(np.sign(np.linalg.det(U) * np.linalg.det(Vt)))
    best = np.longdouble(s[0]) + s[1] + d * s[2]
    got = (R.astype(np.longdouble) * H.astype(np.longdouble)).sum()                  # trace(R^T H)
    r_tr = float(best - got) / (64 * EPS * s[0]) if s[0] > 0 else 0.0
    worst["sv"] = max(worst.get("sv", 0.0), r_sv); worst["trace"] = max(worst.get("trace", 0.0), r_tr)
    assert r_sv <= 1.0 and r_tr <= 1.0, (tag, r_sv, r_tr)
    kappa = s[0] / (s[1] + d * s[2]) if s[1] + d * s[2] > 0 else np.inf
    if flag == 0 and kappa <= 1e6:
        r_R = np.abs(R - U @ np.diag([1.0, 1.0, d]) @ Vt).max() / (64 * EPS * kappa)
        worst["R"] = max(worst.get("R", 0.0), r_R)
        assert r_R <= 1.0, (tag, r_R, kappa)
    return R, sv


def _planted(rng, s, mirror=False):
    U, V = sr.rot(rng.normal(size=3)), sr.rot(rng.normal(size=3))
    if mirror:
        U = U @ np.diag([1.0, 1.0, -1.0])
    return U @ np.diag(s) @ V.T


def test_determined_rotations(kabsch):
    """generic, mirrored (det H < 0: the determinant correction acts on the smallest column), coplanar (sv2 = 0), close
    singular values, kappa = 1e6, and the same at scales where a squared column norm would overflow or vanish unscaled"""
    rng = np.random.default_rng(40)
    worst = {}
    for k in range(6):
        _check(kabsch, rng.normal(size=(3, 3)), ("generic", k), 0, worst)
    for k, s in enumerate(([3.0, 2.0, 1.0], [3.0, 2.0, 1e-3], [1.0, 1.0 - 1e-9, 0.5], [1.0, 1.0, 1.0], [1e6, 0.7, 0.3], [2.0, 1.0, 0.0])):
        for mirror in (False, True):
            H = _planted(rng, s, mirror)
            R, sv = _check(kabsch, H, ("planted", k, mirror), 0, worst)
            for scale in (1e200, 1e-200):
                R2, sv2 = _check(kabsch, H * scale, ("scaled", k, mirror, scale), 0, worst)
                assert mirror and s[1] == s[2] or np.abs(R2 - R).max() <= 64 * EPS * max(1.0, s[0] / (s[1] + s[2]))
    print("score_kabsch worst ratio to bound: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_rank_one_and_zero(kabsch):
    """rank 1: the flag, a rotation that still takes v0 onto u0 (the minimum is unique even though R is not); along a
    coordinate axis nothing is left of the second column and score_orth_unit falls back to an axis; H = 0: R = I"""
    rng = np.random.default_rng(41)
    worst = {}
    for k in range(4):
        u, v = rng.normal(size=3), rng.normal(size=3)
        R, sv = _check(kabsch, np.outer(u, v), ("rank1", k), 1, worst)
        assert np.abs(R @ (v / np.linalg.norm(v)) - u / np.linalg.norm(u)).max() <= 16 * EPS
    for i in range(3):
        for j in range(3):
            for sign in (1.0, -1.0):
                H = np.zeros((3, 3)); H[i, j] = sign * 2.5
                R, sv = _check(kabsch, H, ("axis", i, j, sign), 1, worst)
                assert sv.tolist() == [2.5, 0.0, 0.0] and R[i, j] == sign and np.abs(R).sum() == 3.0      # a signed permutation
    R, sv, flag = kabsch(np.zeros((3, 3)))
    assert flag == 1 and np.array_equal(R, np.eye(3)) and not sv.any()
    R, sv = _check(kabsch, np.outer([1.0, 2.0, 0.0], [3.0, 0.0, 1.0]) * 1e-170, "tiny rank1", 1, worst)      # squares underflow unscaled


def test_non_finite_input_gives_the_identity(kabsch):
    for bad in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0), (1, 2), (2, 1)):
            H = np.arange(9.0).reshape(3, 3); H[pos] = bad
            R, sv, flag = kabsch(H)
            assert flag == 1 and np.array_equal(R, np.eye(3)) and not sv.any(), (bad, pos)
