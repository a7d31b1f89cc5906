"""Trajectory log, what can be checked without a GPU: the symbols exist, bad calls come back as status codes before any device
work, and the test-side restatement the GPU tests compare against (tests/traj_restate.py) is right."""
import ctypes as C

import numpy as np

import traj_restate as tr

TRAJ_SYMBOLS = ("xivo_hip_traj_config", "xivo_hip_traj_record", "xivo_hip_traj_count", "xivo_hip_traj_reset",
                "xivo_hip_traj_read", "xivo_hip_traj_nees")


def test_library_exports_the_trajectory_log(built):
    from xivo_amd import lib as L
    lib = L.load_library()
    for name in TRAJ_SYMBOLS:
        assert name in L.ALL_SYMBOLS and hasattr(lib, name), name
    assert L.traj_dtype.itemsize == 176 and L.traj_dtype.fields["status"][1] == 168
    assert L.traj_opts_dtype.itemsize == 8 + 4 * L.TRAJ_MAX_COLS
    assert b"full" in lib.xivo_hip_strerror(L.ERR_FULL)


def test_calls_without_a_context_return_status_codes(built):
    """No context, so no device: every entry point has to refuse on its arguments alone (this runs on a machine without a GPU)."""
    from xivo_amd import lib as L
    lib = L.load_library()
    o = np.zeros(1, dtype=L.traj_opts_dtype)
    o["T_max"], o["n_cols"] = 4, 6
    o["cols"][0, :6] = range(6)
    k = C.c_int(7)
    buf = np.zeros(64)
    assert lib.xivo_hip_traj_config(None, o.ctypes.data) == -1
    assert lib.xivo_hip_traj_record(None, 1, 0, C.byref(k)) == -1 and k.value == 7
    assert lib.xivo_hip_traj_count(None) == -1
    assert lib.xivo_hip_traj_reset(None) == -1
    assert lib.xivo_hip_traj_read(None, 0, 1, 0, 1, buf.ctypes.data, None, None) == -1
    assert lib.xivo_hip_traj_nees(None, 0, 1, 0, 1, buf.ctypes.data, None, None, None, None) == -1


def test_packed_index_is_the_row_by_row_lower_triangle():
    n = 32
    seen = [tr.pack_index(i, j) for i in range(n) for j in range(i + 1)]
    assert seen == list(range(n * (n + 1) // 2)) and seen[-1] == 527
    P = np.arange(49.0).reshape(7, 7)                     # not symmetric: P[r, c] = 7 r + c tells the triangles apart
    cols = [5, 0, 3]
    got = tr.pack_lower(P, cols)
    assert got.tolist() == [P[5, 5], P[5, 0], P[0, 0], P[5, 3], P[3, 0], P[3, 3]]
    assert np.array_equal(tr.unpack_block(got, [1, 2]), [[P[0, 0], P[3, 0]], [P[3, 0], P[3, 3]]])
    i, j = np.tril_indices(n)                             # the order xivo_amd.lib.Context.traj_read unpacks with
    assert [tr.pack_index(a, b) for a, b in zip(i, j)] == list(range(n * (n + 1) // 2))


def test_solve_restatement_matches_numpy():
    rng = np.random.default_rng(0)
    for n in (3, 6):
        A = rng.normal(size=(n, n)) + n * np.eye(n); b = rng.normal(size=n)
        x = tr.solve_ld(A, b)
        assert x.dtype == np.longdouble
        assert np.max(np.abs(x.astype(float) - np.linalg.solve(A, b))) < 1e-13 * np.max(np.abs(x))
        assert float(np.max(np.abs(np.asarray(A, dtype=np.longdouble) @ x - b))) < 64 * float(np.finfo(np.longdouble).eps)


def test_nees_restatement_cholesky_against_the_solve():
    """|L^-1 e|^2 = e^T S^-1 e: the Cholesky expression the kernel uses against the general solve, both in longdouble (to
    longdouble rounding times cond), and its fp64 evaluation against that reference to the bound the GPU test asks for."""
    rng = np.random.default_rng(1)
    eps_ld = float(np.finfo(np.longdouble).eps)
    for cond in (1e1, 1e3, 1e6):
        eig = np.geomspace(1e-4, 1e-4 * cond, 6)
        S = tr.spd_with_spectrum(rng, eig)
        assert np.array_equal(S, S.T)
        e = rng.normal(size=6) * 1e-2
        ref = tr.nees_solve(S, e)
        c = float(np.linalg.eigvalsh(S)[-1] / np.linalg.eigvalsh(S)[0])
        assert abs(float(tr.nees_cholesky(S, e) - ref)) <= 50 * eps_ld * c * float(ref)
        assert abs(float(tr.nees_cholesky(S, e, np.float64)) - float(ref)) <= 50 * tr.EPS * c * float(ref)
        assert abs(float(ref) - e @ np.linalg.solve(S, e)) <= 50 * tr.EPS * c * float(ref)
    S[2, 2] = -S[2, 2]
    assert np.isnan(tr.nees_cholesky(S, e))


def test_pose_error_inverts_the_retraction():
    rng = np.random.default_rng(2)
    for scale in (1e-3, 0.1, 0.5):
        R = tr.so3_exp(rng.normal(size=3)); T = rng.normal(size=3)
        e = np.concatenate([rng.normal(size=3), rng.normal(size=3)])
        e[:3] *= scale / np.linalg.norm(e[:3])
        Rg, Tg = tr.retract(R, T, e)
        assert float(np.max(np.abs(Rg.T @ Rg - np.eye(3)))) < 1e-17
        back = tr.pose_error(R, T, Rg, Tg)
        assert float(np.max(np.abs(back - e))) < 64 * float(np.finfo(np.longdouble).eps) * max(1.0, float(np.linalg.norm(e)))
