"""Trajectory score, what can be checked without a GPU: the symbol and the record layouts, bad calls come back as status codes
before any device work, the test-side restatement the GPU tests compare against (tests/score_restate.py) is right, and it
agrees with what the reference's ComputeATE / ComputeRPE returned for the stored trajectories (tests/golden/metrics_v1.npz)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import score_restate as sr
from xivo_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics_v1.npz")


def test_library_exports_the_trajectory_score(built):
    from xivo_amd import lib as L
    lib = L.load_library()
    assert "xivo_hip_traj_score" in L.ALL_SYMBOLS and hasattr(lib, "xivo_hip_traj_score")


def test_dtypes_match_the_header(built):
    """sizeof / offsetof of the two structs as a C compiler sees include/xivo_hip.h, against the numpy dtypes"""
    from xivo_amd import lib as L
    fields = ["ate", "ate_raw", "rpe_pos", "rpe_rot", "R", "T", "sv", "n_used", "n_pairs", "flags", "reserved"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "xivo_hip.h"\nint main(void) {\n'
    src += '  printf("%zu %zu %zu %zu", sizeof(xivo_traj_score), sizeof(xivo_traj_score_opts), offsetof(xivo_traj_score_opts, align), offsetof(xivo_traj_score_opts, rpe_lag));\n'
    for f in fields:
        src += '  printf(" %%zu", offsetof(xivo_traj_score, %s));\n' % f
    src += "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "t.c"), "w") as f:
            f.write(src)
        subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(tmp, "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [L.traj_score_dtype.itemsize, L.traj_score_opts_dtype.itemsize, L.traj_score_opts_dtype.fields["align"][1],
                       L.traj_score_opts_dtype.fields["rpe_lag"][1]] == [168, 8, 0, 4]
    assert got[4:] == [L.traj_score_dtype.fields[f][1] for f in fields]
    assert list(L.traj_score_dtype.names) == fields


def test_calls_without_a_context_return_status_codes(built):
    """No context, so no device: the entry point has to refuse on its arguments alone (this runs on a machine without a GPU)."""
    from xivo_amd import lib as L
    lib = L.load_library()
    gt = np.zeros((2, 1, 12)); o = np.zeros(1, dtype=L.traj_score_opts_dtype); out = np.zeros(1, dtype=L.traj_score_dtype)
    out["ate"] = 7.0
    assert lib.xivo_hip_traj_score(None, 0, 1, 0, 2, gt.ctypes.data, o.ctypes.data, out.ctypes.data) == -1
    assert lib.xivo_hip_traj_score(None, 0, 0, 0, 0, None, None, None) == -1
    assert out["ate"][0] == 7.0


def _case(rng, nt, noise, offset=0.0):
    gt_R, gt_T = sr.smooth_trajectory(rng, nt, offset=offset)
    g_R, g_T = sr.rot(rng.normal(size=3)), rng.normal(size=3) * 2
    est_R, est_T = sr.moved(rng, gt_R, gt_T, g_R, g_T, noise)
    return est_R, est_T, gt_R, gt_T, g_R, g_T


def test_restatement_agrees_with_the_host_ate():
    """formats.ate_rmse aligns est onto gt, the score gt onto est: a rigid motion keeps lengths, so the RMSE is the same"""
    rng = np.random.default_rng(0)
    for nt, noise in ((5, 1e-2), (40, 1e-1), (200, 1e-3)):
        est_R, est_T, gt_R, gt_T, _, _ = _case(rng, nt, noise)
        s = sr.score(est_R, est_T, gt_R, gt_T, align=True)
        host = formats.ate_rmse(est_T, gt_T, align=True)
        assert abs(float(s["ate"]) - host) <= 1e-12 * max(1.0, host), (nt, float(s["ate"]), host)
        assert abs(float(s["ate_raw"]) - formats.ate_rmse(est_T, gt_T, align=False)) <= 1e-12 * float(s["ate_raw"])
        assert s["ate"] <= s["ate_raw"] and s["n_used"] == nt and s["flags"] == 0
        raw = sr.score(est_R, est_T, gt_R, gt_T, align=False)
        assert raw["ate"] == raw["ate_raw"] == s["ate_raw"] and np.array_equal(raw["R"], np.eye(3)) and not raw["T"].any()
        assert np.array_equal(raw["sv"], s["sv"])


def test_restatement_recovers_a_planted_motion():
    rng = np.random.default_rng(1)
    for nt in (3, 4, 50):
        est_R, est_T, gt_R, gt_T, g_R, g_T = _case(rng, nt, 0.0)
        s = sr.score(est_R, est_T, gt_R, gt_T, align=True, rpe_lag=1)
        assert np.abs(s["R"] - g_R).max() <= 1e-12 and np.abs(s["T"] - g_T).max() <= 1e-12, nt
        assert float(s["ate"]) <= 1e-13 and abs(np.linalg.det(s["R"]) - 1) <= 4 * sr.EPS
        assert s["n_pairs"] == nt - 1


def test_restatement_is_invariant_under_a_common_motion():
    rng = np.random.default_rng(2)
    est_R, est_T, gt_R, gt_T, _, _ = _case(rng, 30, 1e-2)
    a = sr.score(est_R, est_T, gt_R, gt_T, align=True, rpe_lag=4)
    q_R, q_T = sr.rot(rng.normal(size=3)), rng.normal(size=3) * 5
    b = sr.score(np.array([q_R @ r for r in est_R]), est_T @ q_R.T + q_T, np.array([q_R @ r for r in gt_R]), gt_T @ q_R.T + q_T,
                 align=True, rpe_lag=4)
    for k in ("ate", "ate_raw", "rpe_pos", "rpe_rot"):
        assert abs(float(a[k]) - float(b[k])) <= 1e-12 * max(1.0, float(a[k])), k
    assert np.abs(a["sv"] - b["sv"]).max() <= 1e-12 * a["sv"][0]
    assert np.abs(b["R"] - q_R @ a["R"] @ q_R.T).max() <= 1e-12                # the alignment is conjugated with the motion


def test_restatement_rpe_is_zero_for_a_constant_left_factor():
    """est = g gt: dgY = (g gX1)^-1 (g gX2) = dgX, so E = I whatever the lag; and a case with a known E"""
    rng = np.random.default_rng(3)
    gt_R, gt_T = sr.smooth_trajectory(rng, 25)
    g_R, g_T = sr.rot(rng.normal(size=3)), rng.normal(size=3)
    est_R, est_T = np.array([g_R @ r for r in gt_R]), gt_T @ g_R.T + g_T
    for lag in (1, 7, 24):
        s = sr.score(est_R, est_T, gt_R, gt_T, align=False, rpe_lag=lag)
        assert s["n_pairs"] == 25 - lag and float(s["rpe_pos"]) <= 1e-14 and float(s["rpe_rot"]) <= 1e-14, lag
    assert sr.score(est_R, est_T, gt_R, gt_T, rpe_lag=25)["n_pairs"] == 0
    assert sr.score(est_R, est_T, gt_R, gt_T, rpe_lag=25)["rpe_pos"] == -1
    # est(t) = gt(t) d^t for a constant right factor d = (exp(w), p): dgX = I-to-gt steps differ by exactly d at lag 1 from
    # identity poses: gt = identity everywhere, est(t) = d^t, so E = d
    w, p = np.array([0.1, -0.2, 0.05]), np.array([0.3, 0.1, -0.2])
    d = np.eye(4); d[:3, :3] = sr.rot(w); d[:3, 3] = p
    g = np.eye(4); eR, eT = [], []
    for _ in range(6):
        eR.append(g[:3, :3].copy()); eT.append(g[:3, 3].copy()); g = g @ d
    s = sr.score(np.array(eR), np.array(eT), np.tile(np.eye(3), (6, 1, 1)), np.zeros((6, 3)), align=False, rpe_lag=1)
    assert abs(float(s["rpe_pos"]) - np.linalg.norm(p)) <= 1e-14 and abs(float(s["rpe_rot"]) - np.linalg.norm(w)) <= 1e-14


def test_left_out_frames_and_degenerate_shapes():
    rng = np.random.default_rng(4)
    est_R, est_T, gt_R, gt_T, _, _ = _case(rng, 12, 1e-2)
    est_T[3, 1] = np.nan; gt_R[8, 0, 0] = np.inf
    s = sr.score(est_R, est_T, gt_R, gt_T, rpe_lag=2)
    keep = np.ones(12, dtype=bool); keep[[3, 8]] = False
    t = sr.score(est_R[keep], est_T[keep], gt_R[keep], gt_T[keep])
    assert s["n_used"] == 10 and s["ate"] == t["ate"] and np.array_equal(s["R"], t["R"])
    assert s["n_pairs"] == 10 - 4                         # pairs (1,3) (3,5) (6,8) (8,10) are out
    none = sr.score(est_R * np.nan, est_T, gt_R, gt_T, rpe_lag=1)
    assert none["n_used"] == 0 and none["ate"] == -1 and none["ate_raw"] == -1 and none["rpe_pos"] == -1 and none["flags"] == 1
    one = sr.score(est_R[:1], est_T[:1], gt_R[:1], gt_T[:1], rpe_lag=1)
    assert one["flags"] == 1 and float(one["ate"]) == 0 and one["n_pairs"] == 0 and one["rpe_rot"] == -1


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_against_the_reference(golden):
    """The stored results of the reference's ComputeATE / ComputeRPE (tests/golden/make_golden_metrics.py). The closed form is
    the global minimum, so it is never above the reference's iterate (one-sided, 1e-9 relative); two-sided the restatement is
    within 4 x the gap measured when the fixture was made (ate_gap, R_gap are the maxima of these very differences on the
    machine that made it: the margin is for another LAPACK or longdouble, as on the device); RPE has no iteration: 1e-10."""
    g = golden
    assert len(g["nt"]) >= 6 and float(g["rpe_gap"]) <= 1e-10
    for i in range(len(g["nt"])):
        nt, n, lag = int(g["nt"][i]), int(g["n_ate"][i]), int(g["lag"][i])
        eR, eT, xR, xT = g["est_R"][i, :nt], g["est_T"][i, :nt], g["gt_R"][i, :nt], g["gt_T"][i, :nt]
        assert lag == 1 + int(round(float(g["dt"][i]) * 1e9 / int(g["period_ns"])))
        a = sr.score(eR[:n], eT[:n], xR[:n], xT[:n], align=True)
        assert float(a["ate"]) <= g["ref_ate"][i] * (1 + 1e-9)
        assert abs(g["ref_ate"][i] / float(a["ate"]) - 1) <= 4 * float(g["ate_gap"])
        assert np.abs(a["R"] - g["ref_R"][i]).max() <= 4 * float(g["R_gap"])
        # T = ybar - R xbar on both sides: |d T| <= 3 |d R|max |xbar| and the rounding of forming it
        assert np.abs(a["T"] - g["ref_T"][i]).max() <= 4 * float(g["R_gap"]) * 3 * a["xbar_norm"] + 16 * sr.EPS * (a["xbar_norm"] + a["ybar_norm"])
        r = sr.score(eR, eT, xR, xT, align=False, rpe_lag=lag)
        assert r["n_pairs"] == nt - lag
        assert abs(float(r["rpe_pos"]) / g["ref_rpe_pos"][i] - 1) <= 1e-10 and abs(float(r["rpe_rot"]) / g["ref_rpe_rot"][i] - 1) <= 1e-10


def test_seconds_to_frames():
    """the drivers' conversion of -rpe-dt: the nearest whole number of camera frames, at least one; 0 (or less) is lag 0,
    which the C ABI reads as no RPE"""
    from xivo_amd.sequence import rpe_lag_frames
    assert [rpe_lag_frames(dt, 0.04) for dt in (1.0, 0.12, 0.05, 0.04, 0.01, 1e-9)] == [25, 3, 1, 1, 1, 1]
    assert rpe_lag_frames(0.0, 0.04) == 0 and rpe_lag_frames(-1.0, 0.04) == 0
