"""Landmark log, what can be checked without a GPU: the symbols exist, bad calls come back as status codes before any device
work, the numpy mirror of xivo_map_pt has the C struct's size and offsets, and the test-side restatement the GPU tests compare
against (tests/map_restate.py) is right: its Jacobian agrees with finite differences through the retraction, its Xs with the
host accessor of xivo_amd/pyxivo.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import map_restate as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SYMBOLS = ("xivo_hip_map_config", "xivo_hip_map_record", "xivo_hip_map_count", "xivo_hip_map_reset",
               "xivo_hip_map_read", "xivo_hip_map_nees")


def test_library_exports_the_landmark_log(built):
    from xivo_amd import lib as L
    lib = L.load_library()
    for name in MAP_SYMBOLS:
        assert name in L.ALL_SYMBOLS and hasattr(lib, name), name
    assert L.MAP_MAX_OUT == 128 and L.MAP_WORLD_COV == 1
    assert L.map_opts_dtype.itemsize == 12
    assert b"full" in lib.xivo_hip_strerror(L.ERR_FULL)


def test_record_dtype_is_the_c_struct(tmp_path):
    """sizeof / offsetof of xivo_map_pt as a C compiler lays it out against xivo_amd.lib.map_pt_dtype"""
    from xivo_amd import lib as L
    fields = ("Xs", "cov_local", "cov_world", "xp", "score", "pos", "sind", "ref_sind", "reserved")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xivo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %u", sizeof(xivo_map_pt), sizeof(xivo_map_opts), XIVO_MAP_MAX_OUT, (unsigned)XIVO_MAP_WORLD_COV);\n'
                   + "".join('  printf(" %%zu", offsetof(xivo_map_pt, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:4] == [L.map_pt_dtype.itemsize, L.map_opts_dtype.itemsize, L.MAP_MAX_OUT, L.MAP_WORLD_COV]
    assert got[4:] == [L.map_pt_dtype.fields[f][1] for f in fields]
    assert L.map_pt_dtype.itemsize == 160


def test_calls_without_a_context_return_status_codes(built):
    """No context, so no device: every entry point has to refuse on its arguments alone (this runs on a machine without a GPU)."""
    from xivo_amd import lib as L
    lib = L.load_library()
    o = np.zeros(1, dtype=L.map_opts_dtype)
    o["T_max"], o["n_out"], o["flags"] = 4, 6, L.MAP_WORLD_COV
    k = C.c_int(7)
    buf = np.zeros(64)
    assert lib.xivo_hip_map_config(None, o.ctypes.data) == -1
    assert lib.xivo_hip_map_record(None, 1, 0, C.byref(k)) == -1 and k.value == 7
    assert lib.xivo_hip_map_count(None) == -1
    assert lib.xivo_hip_map_reset(None) == -1
    assert lib.xivo_hip_map_read(None, 0, 1, 0, 1, buf.ctypes.data, None, None) == -1
    assert lib.xivo_hip_map_nees(None, 0, 1, 0, 1, buf.ctypes.data, None, None, None, None) == -1


def _geometry(rng, invdepth):
    Rbc, Rg = mr.so3_exp(rng.normal(size=3)), mr.so3_exp(rng.normal(size=3))
    Tbc, Tg = rng.normal(size=3), rng.normal(size=3) * 3
    z = rng.uniform(0.5, 6.0)
    x = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), 1 / z if invdepth else np.log(z)])
    return Rbc, Tbc, Rg, Tg, x


@pytest.mark.parametrize("invdepth", [False, True], ids=["logz", "invdepth"])
def test_jacobian_agrees_with_finite_differences_through_the_retraction(invdepth):
    """Central differences with step h = 1e-6 of the restated Xs through the restated absorb retraction: the truncation error
    is h^2 / 6 times a third derivative (of the order of |J| for rotations of unit vectors and depths in 0.5 .. 6), the
    rounding error eps_longdouble |Xs| / h ~ 1e-12: 1e-7 |J| bounds both with orders of magnitude to spare and still tells a
    wrong sign or a wrong block (an error of the order of |J|) apart."""
    rng = np.random.default_rng(3 + int(invdepth))
    for _ in range(8):
        geo = _geometry(rng, invdepth)
        J = mr.jacobian(*geo, invdepth)
        Jfd = mr.jacobian_fd(*geo, invdepth, h=1e-6)
        assert J.shape == (3, 15)
        nrm = float(np.sqrt((J * J).sum()))
        assert float(np.max(np.abs(J - Jfd))) <= 1e-7 * nrm
        for k0 in range(0, 15, 3):                                    # no block is trivially zero
            assert float(np.abs(J[:, k0:k0 + 3]).max()) > 1e-3
    # the retraction is R exp(w) (right multiplication), T + dT, x + dx
    Rbc, Tbc, Rg, Tg, x = geo
    d = np.zeros(15); d[0:3] = [0.1, -0.2, 0.05]; d[9:12] = [1, 2, 3]; d[12:15] = [0.01, 0.02, 0.03]
    R2, T2, G2, Tg2, x2 = mr.absorb(Rbc, Tbc, Rg, Tg, x, d)
    assert float(np.abs(R2 - Rbc @ mr.so3_exp(d[0:3])).max()) == 0 and float(np.abs(G2 - Rg).max()) == 0
    ld = lambda v: np.asarray(v, dtype=mr.LD)
    assert float(np.abs(Tg2 - (ld(Tg) + ld(d[9:12]))).max()) == 0 and float(np.abs(x2 - (ld(x) + ld(d[12:15]))).max()) == 0
    assert float(np.abs(T2 - Tbc).max()) == 0


@pytest.mark.parametrize("invdepth", [False, True], ids=["logz", "invdepth"])
def test_world_point_agrees_with_the_host_accessor(invdepth):
    """xivo_amd.pyxivo.Estimator.InstateFeaturePositions computes Feature::Xs on the host from a downloaded scene: the same
    scene through the restatement, to fp64 rounding of the host's evaluation (32 eps of the magnitudes)."""
    from xivo_amd import lib as L
    from xivo_amd import pyxivo
    rng = np.random.default_rng(5)
    G, F = 3, 6
    pose = np.zeros((), dtype=L.pose_dtype)
    groups = np.zeros(G, dtype=L.group_dtype)
    feats = np.zeros(F, dtype=L.feat_dtype)
    pose["Rbc"] = mr.so3_exp(rng.normal(size=3)).astype(np.float64).T.reshape(-1); pose["Tbc"] = rng.normal(size=3)
    for g in range(G):
        groups[g]["Rsb"] = mr.so3_exp(rng.normal(size=3)).astype(np.float64).T.reshape(-1); groups[g]["Tsb"] = rng.normal(size=3) * 2
    feats["sind"] = -1
    slots = [0, 2, 3, 5]
    for j in slots:
        z = rng.uniform(0.5, 6.0)
        feats[j]["x"] = [rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), 1 / z if invdepth else np.log(z)]
        feats[j]["sind"], feats[j]["ref_sind"] = j, rng.integers(0, G)
    est = object.__new__(pyxivo.Estimator)
    est.cfg = types.SimpleNamespace(use_invdepth=invdepth)
    est._scene = lambda: (pose, groups, feats)
    est._slots = lambda: slots
    host = est.InstateFeaturePositions()
    assert host.shape == (len(slots), 3)
    for row, j in zip(host, slots):
        g = groups[feats[j]["ref_sind"]]
        geo = (mr.R(pose["Rbc"]), pose["Tbc"], mr.R(g["Rsb"]), g["Tsb"], feats[j]["x"], invdepth)
        ref, mag = mr.world_point(*geo), mr.world_point_magnitude(*geo)
        assert np.all(np.abs(row - ref) <= 32 * mr.EPS * mag), j


def test_restated_record_orders_packs_and_scores():
    """the pieces of map_restate.record on a case small enough to check by hand"""
    lay = dict(group_begin=23, n_groups=1, feature_begin=29, n_features=3)
    N = 38
    P = np.zeros((N, N))
    P[29:32, 29:32] = [[4, 9, 9], [1, 5, 9], [2, 3, 6]]               # slot 0: stored block with a different upper triangle
    P[32:35, 32:35] = np.eye(3)                                       # slot 1: norm sqrt(3)
    P[35:38, 35:38] = np.eye(3)                                       # slot 2: the same norm
    assert abs(float(mr.score(P, lay, 0)) - np.sqrt(16 + 81 + 81 + 1 + 25 + 81 + 4 + 9 + 36)) < 1e-15
    assert mr.order([2.0, 1.0, 1.0, 0.5], [0, 1, 2, 3]) == [3, 1, 2, 0]
    from xivo_amd import lib as L
    pose = np.zeros((), dtype=L.pose_dtype); pose["Rbc"] = np.eye(3).reshape(-1)
    groups = np.zeros(1, dtype=L.group_dtype); groups[0]["Rsb"] = np.eye(3).reshape(-1); groups[0]["Tsb"] = [1, 2, 3]
    feats = np.zeros(4, dtype=L.feat_dtype)
    feats["sind"] = [2, -1, 0, 1]; feats["x"][:, 2] = np.log(2.0)
    rec = mr.record(pose, groups, feats, P, lay, n_out=2)
    assert [e["pos"] for e in rec] == [0, 3] and [e["sind"] for e in rec] == [2, 1]      # equal scores: by position; n_out cuts
    assert np.allclose(np.asarray(rec[0]["Xs"], dtype=float), [1, 2, 5])
    full = mr.record(pose, groups, feats, P, lay, n_out=8, world=False)
    assert [e["pos"] for e in full] == [0, 3, 2] and full[2]["cov_local"].tolist() == [4, 1, 2, 5, 3, 6]   # lower triangle
    assert mr.columns(lay, 0, 2) == [15, 16, 17, 18, 19, 20, 23, 24, 25, 26, 27, 28, 35, 36, 37]
    S = np.diag([4.0, 1.0, 0.25])
    assert abs(float(mr.nees3([0, 0, 0], mr.pack6(S), [2, 1, 0.5])) - 3.0) < 1e-15
    S[1, 1] = -1
    assert np.isnan(float(mr.nees3([0, 0, 0], mr.pack6(S), [2, 1, 0.5])))
    m, n = mr.anees([1.0, np.nan, 3.0])
    assert float(m) == 2.0 and n == 2


def test_truth_lookup_by_track_id():
    from xivo_amd import sequence
    ids = np.array([[-1, 10002, 10000, -1], [10001, -1, -1, 10000]])
    Xs = np.arange(24.0).reshape(2, 4, 3)
    fid = np.array([[10000, -1, 10001], [10000, 10001, 10007]])
    gt = sequence.truth_by_track(ids, Xs, fid)
    assert np.array_equal(gt[0, 0], Xs[0, 2]) and np.isnan(gt[0, 1]).all() and np.isnan(gt[0, 2]).all()
    assert np.array_equal(gt[1, 0], Xs[1, 3]) and np.array_equal(gt[1, 1], Xs[1, 0]) and np.isnan(gt[1, 2]).all()
