"""The feature-level kernels (csrc/glevel_kernels.hip and AbsorbError in csrc/state_kernels.hip, through capi_glevel.hip) and
the propagation tail (csrc/propagate_kernels.hip through capi_propagate.hip) on both sides of every launch-shape limit,
against plain float64 restatements (the oracle, or a numpy expression of the same operation).

GLEVEL_EDGE_CASES names, per case, the kernel and the limit it targets, which side of the limit the shape is on, the entry
point and the shape. Where the launch picks by size (the gate's block size, the OOS-compression instantiation, the tail
kernel and its passes of 256 columns) the case also names the answer of xivo_hip_selftest_glevel_launch - the same function
the launch calls - and the GPU test asserts the stage label the library recorded under FLAG_PROFILE. Where a loop inside one
kernel crosses a pass (relaxation and RANSAC over 64 features a wave, stacking over 256 rows, absorbing over 256 state
columns, QR / Givens over 64 pivot columns) the case names the passes. tests/test_glevel_edges_cpu.py checks both against the
hook and the loop bounds where no GPU is, and that the cases reach every instantiation."""
import ctypes as C

import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import scene_arrays, oracle_jacobians, spd
from xivo_amd import synth
from xivo_amd.lib import (Context, XivoHipError, FLAG_PROFILE, FLAG_FIX_GROUP_BLOCK, FLAG_NO_LDLT_FALLBACK, oos_dtype,
                          imu_dtype, calib_dtype, cam_intr)

pytestmark = pytest.mark.gpu

GATE, OOSC, TAIL = 0, 1, 2            # XIVO_HIP_LAUNCH_GATE / _OOS_COMPRESS / _PROP_TAIL
FIX23, GEN = "propagate_cov_fixed_kernel<23>", "propagate_cov_kernel"
OC = ["oos_compress_kernel<36,1>", "oos_compress_kernel<64,1>", "oos_compress_kernel<36,2>"]
R_VIS, MH, MULT, MIN_INL = 2.25, 5.991, 1.1, 5
R_RS, THRESH_RS, CHI2_RS = 1.0, 2.0, 5.89
ROOS = 3.5 ** 2


def _gate(B, F, cal):
    nt = 1024 if B < 256 else 256
    if cal:
        nt = 512 if B < 256 else 256
    return (GATE, B, F, int(cal), nt, "gate_sparse_kernel@%d" % nt)


def _tail(nm, N):
    if nm > 40:
        return (TAIL, nm, N, 0, -1, "")
    return (TAIL, nm, N, 0, -(-(N - nm) // 256), FIX23 if nm == 23 else GEN)


def _oosc(ng, rows):
    cols = 6 + 6 * ng + 1
    pick = 0 if cols <= 64 and rows <= 144 else 1 if cols <= 64 and rows <= 256 else 2 if cols <= 128 and rows <= 144 else -1
    return (OOSC, ng, rows, 0, pick, OC[pick] if pick >= 0 else "")


# name, kernel, limit, side ("in": the last size inside the branch, "out": the first outside, "refused"), entry point, shape,
# hook (kind, a, b, c, answer, label) or None, passes (the loop passes the limit counts) or None
GLEVEL_EDGE_CASES = [
    # ---- propagation tail: propagate_cov_fixed_kernel<23> / propagate_cov_kernel, 256 tail columns a pass
    ("cov23_n279", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "in", "propagate_cov", dict(nm=23, N=279, B=5), _tail(23, 279), None),
    ("cov23_n280", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "out", "propagate_cov", dict(nm=23, N=280, B=5), _tail(23, 280), None),
    ("cov23_n535", "propagate_cov_fixed_kernel<23>", "N - 23 <= 512", "in", "propagate_cov", dict(nm=23, N=535, B=3), _tail(23, 535), None),
    ("cov23_n536", "propagate_cov_fixed_kernel<23>", "N - 23 <= 512", "out", "propagate_cov", dict(nm=23, N=536, B=3), _tail(23, 536), None),
    ("cov23_n23", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "in", "propagate_cov", dict(nm=23, N=23, B=5), _tail(23, 23), None),
    ("cov24_n280", "propagate_cov_kernel", "N - nm <= 256", "in", "propagate_cov", dict(nm=24, N=280, B=5), _tail(24, 280), None),
    ("cov24_n281", "propagate_cov_kernel", "N - nm <= 256", "out", "propagate_cov", dict(nm=24, N=281, B=5), _tail(24, 281), None),
    ("cov24_n24", "propagate_cov_kernel", "N - nm <= 256", "in", "propagate_cov", dict(nm=24, N=24, B=5), _tail(24, 24), None),
    ("cov40_n296", "propagate_cov_kernel", "N - nm <= 256", "in", "propagate_cov", dict(nm=40, N=296, B=5), _tail(40, 296), None),
    ("cov40_n297", "propagate_cov_kernel", "N - nm <= 256", "out", "propagate_cov", dict(nm=40, N=297, B=5), _tail(40, 297), None),
    ("cov40_n40", "propagate_cov_kernel", "N - nm <= 256", "in", "propagate_cov", dict(nm=40, N=40, B=5), _tail(40, 40), None),
    ("cov40_n300", "propagate_cov_kernel", "nm <= 40 (MAXM)", "in", "propagate_cov", dict(nm=40, N=300, B=6), _tail(40, 300), None),
    ("cov41_refused", "propagate_cov_kernel", "nm <= 40 (MAXM)", "refused", "propagate_cov", dict(nm=41, N=300, B=5), _tail(41, 300), None),
    ("cov23_b0", "propagate_cov_fixed_kernel<23>", "filter b0 + blockIdx.x", "in", "propagate_cov", dict(nm=23, N=300, B=7, b0=2, nb=3), _tail(23, 300), None),
    ("cov24_b0", "propagate_cov_kernel", "filter b0 + blockIdx.x", "in", "propagate_cov", dict(nm=24, N=300, B=7, b0=3, nb=4), _tail(24, 300), None),
    ("prop_n279", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "in", "propagate", dict(N=279, B=5), _tail(23, 279), None),
    ("prop_n280", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "out", "propagate", dict(N=280, B=5), _tail(23, 280), None),
    ("prop_n281", "propagate_cov_fixed_kernel<23>", "N - 23 <= 256", "out", "propagate", dict(N=281, B=5), _tail(23, 281), None),
    ("prop_n400", "propagate_cov_fixed_kernel<23>", "N - 23 <= 512", "in", "propagate", dict(N=400, B=3), _tail(23, 400), None),
    ("prop_n535", "propagate_cov_fixed_kernel<23>", "N - 23 <= 512", "in", "propagate", dict(N=535, B=3), _tail(23, 535), None),
    ("prop_n536", "propagate_cov_fixed_kernel<23>", "N - 23 <= 512", "out", "propagate", dict(N=536, B=3), _tail(23, 536), None),
    ("calib39_n312", "propagate_cov_kernel", "N - nm <= 256", "out", "propagate_calib", dict(nf=80, N=312, B=3), _tail(39, 312), None),
    # ---- gate: block size by batch (and LDS), relaxation over 64 features a pass, no gating at present <= min_inliers
    ("gate_b255", "gate_sparse_kernel", "batch < 256", "in", "mh_gate", dict(B=255, ng=5, F=20), _gate(255, 20, 0), None),
    ("gate_b256", "gate_sparse_kernel", "batch < 256", "out", "mh_gate", dict(B=256, ng=5, F=20), _gate(256, 20, 0), None),
    ("gate_calib_b255", "gate_sparse_kernel", "batch < 256 (wide LDS)", "in", "mh_gate_calib", dict(B=255, ng=6, F=14), _gate(255, 14, 1), None),
    ("gate_calib_b256", "gate_sparse_kernel", "batch < 256 (wide LDS)", "out", "mh_gate_calib", dict(B=256, ng=6, F=14), _gate(256, 14, 1), None),
    ("gate_f64", "relax_threshold", "F <= 64", "in", "mh_gate", dict(B=5, ng=4, F=64), _gate(5, 64, 0), 1),
    ("gate_f65", "relax_threshold", "F <= 64", "out", "mh_gate", dict(B=5, ng=4, F=65), _gate(5, 65, 0), 2),
    ("gate_f128", "relax_threshold", "F <= 128", "in", "mh_gate", dict(B=5, ng=4, F=128), _gate(5, 128, 0), 2),
    ("gate_f129", "relax_threshold", "F <= 128", "out", "mh_gate", dict(B=5, ng=4, F=129), _gate(5, 129, 0), 3),
    # ---- RANSAC: one wave per filter over 64 features a pass, more filters than CUs
    ("ransac_f64", "ransac_select_kernel", "F <= 64", "in", "one_point_ransac", dict(B=257, ng=5, F=64), None, 1),
    ("ransac_f65", "ransac_select_kernel", "F <= 64", "out", "one_point_ransac", dict(B=257, ng=5, F=65), None, 2),
    ("ransac_f80", "ransac_select_kernel", "F <= 64", "out", "one_point_ransac", dict(B=257, ng=5, F=80), None, 2),
    # ---- stacking (256 threads a filter over M = 2F rows) and the whole feature-level update
    ("fu_m256", "stack_kernel", "M <= 256", "in", "filter_update", dict(B=5, ng=8, F=128), None, 1),
    ("fu_m258", "stack_kernel", "M <= 256", "out", "filter_update", dict(B=5, ng=8, F=129), None, 2),
    ("fu_fmax", "xivo_hip_create", "round16(2F) / 16 <= 24", "in", "filter_update", dict(B=3, ng=4, F=192), None, 192),
    ("fu_fmax_refused", "xivo_hip_create", "round16(2F) / 16 <= 24", "refused", "filter_update", dict(B=3, ng=4, F=193), None, 193),
    # ---- OOS rows: one lane per observation, 2 XIVO_OOS_MAX_OBS rows in LDS
    ("oos_obs16", "oos_kernel", "n_obs <= 16", "in", "oos_project", dict(B=3, ng=16, F=6, k=(2, 16, 9)), None, 16),
    ("oos_obs17", "oos_kernel", "n_obs <= 16", "refused", "oos_project", dict(B=3, ng=16, F=6, k=(2, 17, 9)), None, 17),
    # ---- OOS compression: the instantiation by columns 6 + 6 n_groups + 1 and rows
    ("oosc_c61_r120", "oos_compress_kernel", "<36,1>: columns <= 64", "in", "compress_oos", dict(B=3, ng=9, rows=120), _oosc(9, 120), None),
    ("oosc_c67_r120", "oos_compress_kernel", "<36,1>: columns <= 64", "out", "compress_oos", dict(B=3, ng=10, rows=120), _oosc(10, 120), None),
    ("oosc_c61_r144", "oos_compress_kernel", "<36,1>: rows <= 144", "in", "compress_oos", dict(B=3, ng=9, rows=144), _oosc(9, 144), None),
    ("oosc_c61_r145", "oos_compress_kernel", "<36,1>: rows <= 144", "out", "compress_oos", dict(B=3, ng=9, rows=145), _oosc(9, 145), None),
    ("oosc_c61_r256", "oos_compress_kernel", "<64,1>: rows <= 256", "in", "compress_oos", dict(B=3, ng=9, rows=256), _oosc(9, 256), None),
    ("oosc_c61_r257", "oos_compress_kernel", "<64,1>: rows <= 256", "out", "compress_oos", dict(B=3, ng=9, rows=257), _oosc(9, 257), None),
    ("oosc_c67_r144", "oos_compress_kernel", "<36,2>: rows <= 144", "in", "compress_oos", dict(B=3, ng=10, rows=144), _oosc(10, 144), None),
    ("oosc_c67_r145", "oos_compress_kernel", "<36,2>: rows <= 144", "out", "compress_oos", dict(B=3, ng=10, rows=145), _oosc(10, 145), None),
    ("oosc_c127_r144", "oos_compress_kernel", "<36,2>: columns <= 128", "in", "compress_oos", dict(B=3, ng=20, rows=144), _oosc(20, 144), None),
    ("oosc_c133_r144", "oos_compress_kernel", "<36,2>: columns <= 128", "out", "compress_oos", dict(B=3, ng=21, rows=144), _oosc(21, 144), None),
    # ---- Givens / QR: pivot columns in chunks of 64, MAXC = 8
    ("qr_nx64", "givens_kernel", "nx <= 64", "in", "qr", dict(nb=3, nx=64, rows=70), None, 1),
    ("qr_nx65", "givens_kernel", "nx <= 64", "out", "qr", dict(nb=3, nx=65, rows=80), None, 2),
    ("qr_nx448", "givens_kernel", "nx <= 448", "in", "qr", dict(nb=3, nx=448, rows=460), None, 7),
    ("qr_nx449", "givens_kernel", "nx <= 448", "out", "qr", dict(nb=3, nx=449, rows=460), None, 8),
    ("qr_nx512", "givens_kernel", "nx <= 512 (MAXC 8)", "in", "qr", dict(nb=3, nx=512, rows=520), None, 8),
    ("qr_nx513", "givens_kernel", "nx <= 512 (MAXC 8)", "refused", "qr", dict(nb=3, nx=513, rows=520), None, 9),
    ("givens_nf64", "givens_kernel", "nf <= 64", "in", "givens", dict(nb=3, nf=64, nx=80, rows=70), None, 1),
    ("givens_nf65", "givens_kernel", "nf <= 64", "refused", "givens", dict(nb=3, nf=65, nx=80, rows=70), None, 2),
    # ---- AbsorbError: 256 threads a filter over the state width
    ("absorb_n256", "absorb_error_kernel", "N <= 256", "in", "absorb_error", dict(B=5, ng=4, F=10, N=256), None, 1),
    ("absorb_n257", "absorb_error_kernel", "N <= 256", "out", "absorb_error", dict(B=5, ng=4, F=10, N=257), None, 2),
    ("absorb_n400", "absorb_error_kernel", "N <= 256", "out", "absorb_error", dict(B=5, ng=4, F=10, N=400), None, 2),
]
CASES = {c[0]: c for c in GLEVEL_EDGE_CASES}


def hook(lib, kind, a, b, c):
    buf = C.create_string_buffer(64)
    return lib.xivo_hip_selftest_glevel_launch(kind, a, b, c, buf, len(buf)), buf.value.decode()


def make(ng, nf, F, B, seed, cam=synth.PINHOLE, N=None, flags=0, M_max=None):
    sc = synth.g_level(ng, nf, F, B, seed=seed, cam=cam, N=N)
    lay = orc.Layout(ng, nf, N=sc["N"])
    ctx = Context(lay.N, M_max or 2 * F, B, flags=flags | FLAG_PROFILE)
    ctx.set_layout(lay.N, lay.group_begin, ng, lay.feature_begin, nf, cam)
    poses, groups, feats, xp = scene_arrays(sc, cam)
    return sc, lay, ctx, poses, groups, feats, xp


def stage(ctx, name):
    p = ctx.profile_get()[name]
    return p["kernel"], p["launches"]


def _check_label(case, ctx, stage_name):
    h = case[6]
    got, n = stage(ctx, stage_name)
    assert n >= 1 and got == h[5], (case[0], got, h[5])


# ---------------------------------------------------------------- propagation
def _cases(entry):
    return [c[0] for c in GLEVEL_EDGE_CASES if c[4] == entry]


@pytest.mark.parametrize("name", _cases("propagate_cov"))
def test_propagate_cov_edges(built, name):
    """xivo_hip_propagate_cov: P[:nm,:nm] = Pmm, P[:nm,nm:] = Phi P[:nm,nm:], P[nm:,:nm] = P[nm:,:nm] Phi^T on the filters
    [b0, b0 + nb); every other filter, and every entry of a filter outside the motion rows and columns, bit for bit."""
    case = CASES[name]
    sh = case[5]
    nm, N, B = sh["nm"], sh["N"], sh["B"]
    b0, nb = sh.get("b0", 0), sh.get("nb", B)
    rng = np.random.default_rng(N * 131 + nm)
    P = np.array([spd(N, 7 * N + b) for b in range(B)])
    Phi = np.eye(nm)[None] + 0.05 * rng.normal(size=(nb, nm, nm))
    Pmm = np.array([spd(nm, 900 + b) for b in range(nb)])
    with Context(N, 2, B, flags=FLAG_PROFILE) as ctx:
        ctx.upload_P(P)
        if case[3] == "refused":
            with pytest.raises(XivoHipError) as e:
                ctx.propagate_cov(Phi, Pmm, b0=b0)
            assert e.value.status == -1
            assert np.array_equal(ctx.download_P(), P)
            return
        ctx.propagate_cov(Phi, Pmm, b0=b0)
        got = ctx.download_P()
        _check_label(case, ctx, "other")
    for b in range(B):
        if not b0 <= b < b0 + nb:
            assert np.array_equal(got[b], P[b]), b
            continue
        k = b - b0
        exp = P[b].copy()
        exp[:nm, :nm] = Pmm[k]
        exp[:nm, nm:] = Phi[k] @ P[b][:nm, nm:]
        exp[nm:, :nm] = P[b][nm:, :nm] @ Phi[k].T
        assert rel_fro(got[b], exp) < 1e-11, (b, rel_fro(got[b], exp))
        assert np.array_equal(got[b][nm:, nm:], P[b][nm:, nm:]), b


@pytest.mark.parametrize("method", ["RK4", "PrinceDormand"])
@pytest.mark.parametrize("name", _cases("propagate"))
def test_propagate_edges(built, name, method):
    """xivo_hip_propagate (state kernel + propagate_cov_fixed_kernel<23>) at state widths on both sides of the tail's passes,
    against the oracle's Estimator::Propagate; trailing zero slots widen the state."""
    case = CASES[name]
    N, B = case[5]["N"], case[5]["B"]
    sc, lay, ctx, poses, groups, feats, xp = make(3, 6, 6, B, N, N=N)
    rng = np.random.default_rng(N)
    st = []
    for b in range(B):
        X = orc.MotionState(sc["Rsb"][b], sc["Tsb"][b], rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.01,
                            rng.normal(size=3) * 0.05, orc.so3_exp(np.array([0.02, -0.03, 0.0])))
        st.append(X)
        poses[b]["Vsb"] = X.Vsb; poses[b]["bg"] = X.bg; poses[b]["ba"] = X.ba; poses[b]["Rsg"] = X.Rsg.T.reshape(-1)
    P = np.array([spd(N, 50 + b) * 1e-3 for b in range(B)])
    imu = np.zeros(B, dtype=imu_dtype)
    imu["gyro"] = rng.normal(size=(B, 3)) * 0.3; imu["accel"] = rng.normal(size=(B, 3)) + np.array([0, 0, 9.8])
    imu["slope_gyro"] = rng.normal(size=(B, 3)) * 5.0; imu["slope_accel"] = rng.normal(size=(B, 3)) * 20.0
    imu["dt"] = 0.0045 * (1.0 + 0.1 * np.arange(B))
    Qi = np.diag(rng.uniform(1e-6, 1e-4, 12)); A = rng.normal(size=(23, 23)) * 1e-4; Qm = A @ A.T
    g = np.array([0.0, 0.0, -9.796])
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.propagate(imu, Qi, Qm, g, method=method, stepsize=0.002)
        Pn = ctx.download_P()
        pose_d, _, _ = ctx.get_scene()
        _check_label(case, ctx, "propagate_tail")
    for b in range(B):
        Xr, Pr = orc.propagate(st[b], P[b], imu["gyro"][b], imu["accel"][b], imu["slope_gyro"][b], imu["slope_accel"][b],
                               float(imu["dt"][b]), Qi, Qm, g, method=method, stepsize=0.002)
        assert rel_fro(Pn[b], Pr) < 1e-11, (b, rel_fro(Pn[b], Pr))
        assert np.abs(pose_d[b]["Rsb"].reshape(3, 3).T - Xr.Rsb).max() < 1e-12
        assert np.abs(pose_d[b]["Tsb"] - Xr.Tsb).max() < 1e-12 and np.abs(pose_d[b]["Vsb"] - Xr.Vsb).max() < 1e-12


def test_propagate_calib_edge(built):
    """xivo_hip_propagate_calib at the largest motion size it is built for (kMotionSize 39: td + Cg / Ca + intrinsics), at a
    width whose tail takes a second pass of propagate_cov_kernel."""
    case = CASES["calib39_n312"]
    nf, B = case[5]["nf"], case[5]["B"]
    cam = synth.RADTAN
    lay = orc.calib_layout(4, nf, True, True, 9)
    assert lay.motion_size == 39 and lay.N == case[5]["N"]
    sc = synth.g_level(4, nf, nf, B, seed=5, cam=cam)
    poses, groups, feats, xp = scene_arrays(sc, cam)
    rng = np.random.default_rng(105)
    calib = np.zeros(B, dtype=calib_dtype)
    st, Cgs, Cas = [], [], []
    for b in range(B):
        X = orc.MotionState(sc["Rsb"][b], sc["Tsb"][b], rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.01,
                            rng.normal(size=3) * 0.05, orc.so3_exp(np.array([0.02, -0.03, 0.0])))
        st.append(X)
        poses[b]["Vsb"] = X.Vsb; poses[b]["bg"] = X.bg; poses[b]["ba"] = X.ba; poses[b]["Rsg"] = X.Rsg.T.reshape(-1)
        Cg = np.eye(3) + 0.02 * rng.normal(size=(3, 3)); Ca = np.triu(np.eye(3) + 0.02 * rng.normal(size=(3, 3)))
        Cgs.append(Cg); Cas.append(Ca)
        calib[b]["gyro"] = rng.normal(size=3) * 0.3; calib[b]["Cg"] = Cg.T.reshape(-1); calib[b]["Ca"] = Ca.T.reshape(-1)
        calib[b]["td"] = 0.004 * (b + 1); calib[b]["intr"] = cam_intr(cam)
    P = np.array([spd(lay.N, 70 + b) * 1e-3 for b in range(B)])
    imu = np.zeros((B, 2), dtype=imu_dtype)
    imu["gyro"] = rng.normal(size=(B, 2, 3)) * 0.3; imu["accel"] = rng.normal(size=(B, 2, 3)) + np.array([0, 0, 9.8])
    imu["slope_gyro"] = rng.normal(size=(B, 2, 3)) * 5.0; imu["slope_accel"] = rng.normal(size=(B, 2, 3)) * 20.0
    imu["dt"] = (0.0047 * (1.0 + 0.1 * np.arange(B)))[:, None]
    Qi = np.diag(rng.uniform(1e-6, 1e-4, 12)); A = rng.normal(size=(39, 39)) * 1e-4; Qm = A @ A.T
    g = np.array([0.0, 0.0, -9.796])
    with Context(lay.N, 2 * nf, B, flags=FLAG_PROFILE) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, 4, lay.feature_begin, nf, cam)
        ctx.set_calib(lay.td, lay.Cg, lay.cam_begin, lay.cam_dim)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats); ctx.set_calib_state(calib)
        ctx.propagate_calib(imu, Qi, Qm, g, method="RK4", stepsize=0.002)
        Pn = ctx.download_P()
        pose_d, _, _ = ctx.get_scene()
        _check_label(case, ctx, "propagate_tail")
    for b in range(B):
        Xr, Pr = st[b], P[b]
        for k in range(2):
            Xr, Pr = orc.propagate(Xr, Pr, imu["gyro"][b, k], imu["accel"][b, k], imu["slope_gyro"][b, k], imu["slope_accel"][b, k],
                                   float(imu["dt"][b, k]), Qi, Qm, g, method="RK4", stepsize=0.002, Cg=Cgs[b], Ca=Cas[b], layout=lay)
        assert rel_fro(Pn[b], Pr) < 1e-11, (b, rel_fro(Pn[b], Pr))
        assert np.abs(pose_d[b]["Tsb"] - Xr.Tsb).max() < 1e-12 and np.abs(pose_d[b]["Vsb"] - Xr.Vsb).max() < 1e-12


# ---------------------------------------------------------------- gate
@pytest.mark.parametrize("name", _cases("mh_gate"))
def test_gate_edges(built, name):
    """xivo_hip_mh_gate: distances (1e-9) and mask against the oracle's MHGating. Filter 1 has three wild pixels, filter 2
    nearly all (the relaxation loop runs more than once), filter 3 only min_inliers present entries (no gating: every present
    entry is an inlier) and filter 4 one more than that (gated)."""
    case = CASES[name]
    sh = case[5]
    B, ng, F = sh["B"], sh["ng"], sh["F"]
    cam = synth.PINHOLE
    sc, lay, ctx, poses, groups, feats, xp = make(ng, F, F, B, F * 1000 + B)
    feats["xp"][1, [2, 7, 11]] += 40.0; xp[1, [2, 7, 11]] += 40.0
    feats["xp"][2, 3:] += np.linspace(40, 90, F - 3)[:, None]; xp[2, 3:] += np.linspace(40, 90, F - 3)[:, None]
    feats["xp"][3:5, 1] += 80.0; xp[3:5, 1] += 80.0
    present = np.ones((B, F), dtype=bool)
    for b, keep in ((3, MIN_INL), (4, MIN_INL + 1)):
        present[b, keep:] = False
        feats["sind"][b, keep:] = -1
    P = np.array([spd(lay.N, 10 + b % 7) * 1e-4 for b in range(B)])
    with ctx:
        ctx.upload_P(P)
        ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate()
        mask, dist = ctx.mh_gate(R_VIS, MH, MULT, MIN_INL)
        _check_label(case, ctx, "mh_gate")
    relaxed = 0
    for b in range(B):
        idx = np.nonzero(present[b])[0]
        Js, inns, _ = oracle_jacobians(sc, cam, lay, xp, b)
        d = orc.mh_distances(Js[idx], P[b], inns[idx], R_VIS)
        exp = np.zeros(F, dtype=bool)
        if len(idx) <= MIN_INL:
            exp[idx] = True
        else:
            m, _, th = orc.mh_gate(d, MH, MULT, MIN_INL)
            exp[idx] = m
            relaxed = max(relaxed, round(np.log(th / MH) / np.log(MULT)))
            assert np.allclose(dist[b][idx], d, rtol=1e-9, atol=0), b
        assert np.array_equal(mask[b], exp), (b, np.nonzero(mask[b] != exp))
    assert mask[3, 1] and not mask[4, 1] and (~mask[1]).sum() >= 3
    assert relaxed >= 2, relaxed


@pytest.mark.parametrize("name", _cases("mh_gate_calib"))
def test_gate_calib_edges(built, name):
    """The gate of an online-calibration build (whole rows, gate_sparse_kernel's wide LDS scratch) at 255 | 256 filters."""
    case = CASES[name]
    B, ng, nf = case[5]["B"], case[5]["ng"], case[5]["F"]
    import test_calib_gpu as tc
    cam, lay, sc, poses, groups, feats, xp, calib, cals, ctx0 = tc.setup("equi", True, True, True, B=B, ng=ng, nf=nf, seed=4)
    ctx0.close()
    feats["xp"][2, [1, 5]] += 50.0; xp[2, [1, 5]] += 50.0
    P = np.array([spd(lay.N, 5 + b % 7) * 1e-4 for b in range(B)])
    with Context(lay.N, 2 * nf, B, flags=FLAG_PROFILE) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, ng, lay.feature_begin, nf, cam)
        ctx.set_calib(lay.td, lay.Cg, lay.cam_begin, lay.cam_dim)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats); ctx.set_calib_state(calib)
        ctx.jacobians_instate()
        mask, dist = ctx.mh_gate(R_VIS, MH, MULT, MIN_INL)
        _check_label(case, ctx, "mh_gate")
    for b in range(B):
        Js, inns, _ = tc.oracle_rows(sc, cam, lay, xp, cals, b)
        d = orc.mh_distances(Js, P[b], inns, R_VIS)
        m, _, _ = orc.mh_gate(d, MH, MULT, MIN_INL)
        assert np.array_equal(mask[b], m) and rel_fro(dist[b], d) < 1e-9, b
    assert (~mask[2]).sum() >= 2


# ---------------------------------------------------------------- RANSAC
@pytest.mark.parametrize("name", _cases("one_point_ransac"))
def test_ransac_edges(built, name):
    """xivo_hip_one_point_ransac with F on both sides of 64 (one wave walks the features 64 at a time) and more filters than
    the chip has CUs, against the oracle's OnePointRANSAC; P and the state come back as they were."""
    import test_ransac_gpu as tr
    case = CASES[name]
    B, ng, F = case[5]["B"], case[5]["ng"], case[5]["F"]
    cam = synth.RADTAN
    sc = synth.g_level(ng, F, F, B, seed=F, cam=cam)
    lay = orc.Layout(ng, F, N=sc["N"])
    rng = np.random.default_rng(F)
    poses, groups, feats, xp = scene_arrays(sc, cam)
    xp = xp - sc["pix_noise"] + rng.normal(size=xp.shape) * 0.3
    gauge = np.zeros(B, dtype=np.int32)
    for b in range(B):
        kind = b % 4
        n_present = F - (b % 3)
        feats["sind"][b, n_present:] = -1
        if kind in (0, 2):
            far = rng.choice(n_present, size=5, replace=False)
            xp[b, far[:-1]] += rng.choice([-1, 1], size=(4, 2)) * rng.uniform(2.0, 4.0, size=(4, 2))
            xp[b, far[-1]] += 35.0
        elif kind == 3:
            xp[b, :n_present] += rng.choice([-1, 1], size=(n_present, 2)) * rng.uniform(2.5, 3.5, size=(n_present, 2))
        gauge[b] = -1 if b % 7 == 3 else int(rng.integers(0, ng))
    feats["xp"] = xp
    P = np.array([spd(lay.N, 300 + b % 11) * 1e-4 for b in range(B)])
    with Context(lay.N, 2 * F, B, flags=FLAG_PROFILE) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, ng, lay.feature_begin, F, cam)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate()
        mh_mask, _ = ctx.mh_gate(R_RS, MH, MULT, MIN_INL)
        keep, chi, nrej = ctx.one_point_ransac(R_RS, THRESH_RS, CHI2_RS, gauge=gauge)
        assert np.array_equal(ctx.download_P(), P)
        assert stage(ctx, "other")[0] == "ransac_rescue_kernel"
    kinds = set()
    for b in range(B):
        idx = np.nonzero(mh_mask[b])[0]
        st = tr._state(sc, b, xp[b])
        out = orc.one_point_ransac(tr._sub(st, idx), P[b], xp[b][idx], cam, lay, R_RS, THRESH_RS, CHI2_RS, int(gauge[b]), range(ng))
        exp = np.zeros(F, dtype=bool); exp[idx[out["inliers"]]] = True
        assert np.array_equal(keep[b], exp), b
        assert nrej[b] == len(out["rejected"]), b
        for i, d in out["chi2"].items():
            assert abs(chi[b, idx[i]] - d) < 1e-7 * max(1.0, d), (b, i)
        low = out["low"]
        kinds.add("early" if low.all() else "prior" if not low.any() else "partial")
        if len(out["rejected"]):
            kinds.add("rejected")
    assert kinds >= {"early", "prior", "partial", "rejected"}, kinds


# ---------------------------------------------------------------- stacking + update
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", _cases("filter_update"))
def test_filter_update_edges(built, name, fix):
    """xivo_hip_filter_update (jac -> gate -> stack -> update) with M = 2F rows on both sides of the stack kernel's 256-row
    pass, with and without FIX_GROUP_BLOCK, and at the largest F xivo_hip_create allows: P+ and dx against the reference
    flow over the inliers only."""
    case = CASES[name]
    B, ng, F = case[5]["B"], case[5]["ng"], case[5]["F"]
    cam = synth.EQUI
    if case[3] == "refused":                          # 25 block rows: refused before anything is allocated
        with pytest.raises(XivoHipError) as e:
            Context(23 + 6 * ng + 3 * F, 2 * F, B, flags=FLAG_FIX_GROUP_BLOCK if fix else 0)
        assert e.value.status == -5
        return
    sc, lay, ctx, poses, groups, feats, xp = make(ng, F, F, B, 40 + F, cam=cam, flags=FLAG_FIX_GROUP_BLOCK if fix else 0)
    feats["xp"][1, [0, 5, F - 1]] += 55.0; xp[1, [0, 5, F - 1]] += 55.0
    P = np.array([spd(lay.N, 30 + b) * 1e-4 for b in range(B)])
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.filter_update(R_VIS, MH, MULT, MIN_INL, use_gating=True)
        assert stage(ctx, "stack_H")[0] == "stack_kernel"
        err = ctx.get_err(); Pn = ctx.download_P()
        assert (ctx.get_status() == 0).all()
        mask, _ = ctx.get_gate(F)
    assert not mask[1, F - 1]
    for b in range(B):
        Js, inns, _ = oracle_jacobians(sc, cam, lay, xp, b)
        m, _, _ = orc.mh_gate(orc.mh_distances(Js, P[b], inns, R_VIS), MH, MULT, MIN_INL)
        assert np.array_equal(mask[b], m), b
        idx = np.nonzero(m)[0]
        H, inn, dR = orc.stack_measurements(Js[idx], inns[idx], sc["ref"][b][idx], sc["sind"][b][idx], lay, R_VIS, fix_group_block=fix)
        e_ref, P_ref, _ = orc.update_joseph(H, P[b], inn, dR)
        assert rel_fro(Pn[b], P_ref) < TOL_P and rel_fro(err[b], e_ref) < TOL_DX, (b, rel_fro(Pn[b], P_ref), rel_fro(err[b], e_ref))


# ---------------------------------------------------------------- OOS rows
def _oos_list(sc, lay, cam, ks_per_filter, seed):
    """[B, n] OOS features, filter b's feature o seen from ks_per_filter[b][o] distinct groups; returns (array, obs)"""
    B = len(ks_per_filter)
    n = max(len(k) for k in ks_per_filter)
    rng = np.random.default_rng(seed)
    oos = np.zeros((B, n), dtype=oos_dtype)
    obs_all = {}
    for b in range(B):
        for o, k in enumerate(ks_per_filter[b]):
            Xs = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3, 6)])
            gs = rng.permutation(lay.n_groups)[:min(k, 16)]
            oos[b, o]["Xs"] = Xs; oos[b, o]["n_obs"] = k
            obs = []
            for q, g in enumerate(gs):
                _, _, inn = orc.oos_jacobian_internal(Xs, sc["gR"][b, g], sc["gT"][b, g], sc["Rbc"][b], sc["Tbc"][b], [0, 0], cam, lay, int(g))
                pix = -inn + rng.normal(0, 1.0, 2)
                oos[b, o]["group_sind"][q] = g; oos[b, o]["xp"][q] = pix
                obs.append((int(g), pix))
            obs_all[b, o] = (Xs, obs)
    return oos, obs_all


def _oracle_stack(sc, lay, cam, xp, b, obs_all, n, whole=0):
    Js, inns, _ = oracle_jacobians(sc, cam, lay, xp, b)
    H, inn, dR = orc.stack_measurements(Js, inns, sc["ref"][b], sc["sind"][b], lay, R_VIS)
    n0 = H.shape[0]
    for o in range(n):
        if (b, o) not in obs_all:
            continue
        Xs, obs = obs_all[b, o]
        Hxp, rp, _ = orc.oos_jacobian(Xs, obs, sc["gR"][b], sc["gT"][b], sc["Rbc"][b], sc["Tbc"][b], cam, lay, whole_buffer_groups=whole)
        H = np.vstack([H, Hxp]); inn = np.concatenate([inn, rp]); dR = np.concatenate([dR, np.full(len(rp), ROOS)])
    return H, inn, dR, n0


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("name", _cases("oos_project"))
def test_oos_project_edges(built, name, whole):
    """xivo_hip_oos_project[_ex] with n_obs = 2 and 16 (XIVO_OOS_MAX_OBS), in the top-2k and the whole-buffer mode: the rows
    (1e-10), inn (1e-9) and diagR against the oracle's SlowGivens rows, then the update. n_obs = 17 is refused and leaves
    the staged measurement as it was."""
    case = CASES[name]
    B, ng, F, ks = case[5]["B"], case[5]["ng"], case[5]["F"], case[5]["k"]
    cam = synth.PINHOLE
    per = [list(ks), list(ks[::-1]), [ks[1], ks[2], ks[0]]]   # the same features in another order per filter
    wr = 2 * ng - 3
    sc, lay, ctx, poses, groups, feats, xp = make(ng, F, F, B, 60 + ng, M_max=2 * F + len(ks) * wr + 32)
    oos, obs_all = _oos_list(sc, lay, cam, per, 61)
    P = np.array([spd(lay.N, 40 + b) * 1e-4 for b in range(B)])
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, MIN_INL); ctx.stack(R_VIS)
        if case[3] == "refused":
            before = [ctx.get_H(b) for b in range(B)]
            with pytest.raises(XivoHipError) as e:
                ctx.oos_project(oos, ROOS, whole_buffer=whole)
            assert e.value.status == -1
            after = [ctx.get_H(b) for b in range(B)]
            for x, y in zip(before, after):
                assert all(np.array_equal(u, v) for u, v in zip(x, y))
            return
        rows = ctx.oos_project(oos, ROOS, whole_buffer=whole)
        assert stage(ctx, "other")[0] == "oos_kernel"
        got = [ctx.get_H(b) for b in range(B)]
        ctx.update_joseph()
        err = ctx.get_err(); Pn = ctx.download_P()
        assert (ctx.get_status() == 0).all()
    for b in range(B):
        assert rows[b] == sum(wr if whole else 2 * k - 3 for k in per[b])
        H, inn, dR, _ = _oracle_stack(sc, lay, cam, xp, b, obs_all, len(ks), whole=ng if whole else 0)
        gH, ginn, gdR = got[b]
        assert gH.shape == H.shape
        assert rel_fro(gH, H) < 1e-10 and rel_fro(ginn, inn) < 1e-9 and np.allclose(gdR, dR)
        e_ref, P_ref, _ = orc.update_joseph(H, P[b], inn, dR)
        assert rel_fro(Pn[b], P_ref) < TOL_P and rel_fro(err[b], e_ref) < TOL_DX, b


def _ks_for(rows, kmax, n=None):
    """n observation counts k (2 <= k <= kmax; n: as few as can be) whose OOS rows 2k - 3 add up to rows"""
    rmax = 2 * kmax - 3
    if n is None:
        n = -(-rows // rmax)
        if (rows - n) % 2:
            n += 1
    r = [1] * n
    left = rows - n
    for i in range(n):
        add = min(left, rmax - 1)
        r[i] += add
        left -= add
    assert left == 0 and sum(r) == rows
    return [(x + 3) // 2 for x in r]


@pytest.mark.parametrize("name", _cases("compress_oos"))
def test_compress_oos_edges(built, name):
    """xivo_hip_compress_oos on both sides of each oos_compress_kernel instantiation (columns 6 + 6 n_groups + 1, the largest
    OOS block's rows): the stage label of the instantiation the hook names, the rows each filter reports (the non-zero
    columns when compressed, the rows themselves when declined - then the rows come back bit for bit), and P+ / dx equal to
    the oracle's update on the uncompressed rows."""
    case = CASES[name]
    B, ng, T = case[5]["B"], case[5]["ng"], case[5]["rows"]
    pick = case[6][4]
    cam = synth.EQUI
    F = 6
    kmax = min(ng, 16)
    k0 = _ks_for(T, kmax)
    per = [k0, _ks_for(T - 20, kmax, len(k0)), [3] * len(k0)]   # the largest block, a smaller one, one under the trigger
    sc, lay, ctx, poses, groups, feats, xp = make(ng, F, F, B, 70 + ng, cam=cam, M_max=2 * F + T + 32)
    oos, obs_all = _oos_list(sc, lay, cam, per, 71 + T)
    P = np.array([spd(lay.N, 90 + b) * 1e-4 for b in range(B)])
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, MIN_INL); ctx.stack(R_VIS)
        rows = ctx.oos_project(oos, ROOS)
        assert rows.max() == T
        Hfull = [ctx.get_H(b) for b in range(B)]
        n_before = stage(ctx, "other")[1]
        crow = ctx.compress_oos(1.0)
        label, n_after = stage(ctx, "other")
        if pick >= 0:
            assert label == case[6][5] and n_after == n_before + 1, (label, n_after, n_before)
        else:
            assert label == "oos_kernel" and n_after == n_before, (label, n_after, n_before)
        got = [ctx.get_H(b) for b in range(B)]
        ctx.update_joseph()
        err = ctx.get_err(); Pn = ctx.download_P()
        assert (ctx.get_status() == 0).all()
    for b in range(B):
        H, inn, dR, n0 = _oracle_stack(sc, lay, cam, xp, b, obs_all, oos.shape[1])
        assert H.shape[0] - n0 == rows[b]
        ncols = int(np.count_nonzero(np.abs(H[n0:]).sum(0)))
        exp_rows = ncols if (pick >= 0 and rows[b] > ncols) else rows[b]
        assert crow[b] == exp_rows, (b, crow[b], exp_rows, ncols)
        if pick < 0:
            assert all(np.array_equal(u, v) for u, v in zip(got[b], Hfull[b]))
        else:
            Hc, ic, _ = got[b]
            A, Cc = Hfull[b][0][n0:n0 + rows[b]], Hc[n0:n0 + crow[b]]
            assert rel_fro(Cc.T @ Cc, A.T @ A) < 1e-12
        e_ref, P_ref, _ = orc.update_joseph(H, P[b], inn, dR)
        assert rel_fro(Pn[b], P_ref) < TOL_P and rel_fro(err[b], e_ref) < TOL_DX, (b, rel_fro(Pn[b], P_ref), rel_fro(err[b], e_ref))


# ---------------------------------------------------------------- Givens / QR
@pytest.mark.parametrize("name", _cases("qr") + _cases("givens"))
def test_givens_qr_edges(built, name):
    """xivo_hip_qr / xivo_hip_givens at the pivot-column chunks of 64 and the MAXC = 8 limit, against the oracle's
    xivo::QR / xivo::Givens (1e-10); nx = 513 and nf = 65 are refused."""
    case = CASES[name]
    sh = case[5]
    nb, nx, rows = sh["nb"], sh["nx"], sh["rows"]
    rng = np.random.default_rng(nx * 7 + rows)
    x = rng.normal(size=(nb, rows)); Hx = rng.normal(size=(nb, rows, nx))
    Hx[1] *= 3.0                                                  # one problem differs in scale from its neighbours
    with Context(8, 2, 1, flags=FLAG_PROFILE) as ctx:
        if case[4] == "qr":
            if case[3] == "refused":
                with pytest.raises(XivoHipError) as e:
                    ctx.qr(x, Hx)
                assert e.value.status == -1
                return
            ro, xd, Hxd = ctx.qr(x, Hx)
        else:
            Hf = rng.normal(size=(nb, rows, sh["nf"]))
            if case[3] == "refused":
                with pytest.raises(XivoHipError) as e:
                    ctx.givens(x, Hx, Hf)
                assert e.value.status == -1
                return
            ro, xd, Hxd, Hfd = ctx.givens(x, Hx, Hf)
        assert stage(ctx, "other")[0] == "givens_kernel"
    for b in range(nb):
        if case[4] == "qr":
            r, xo, Hxo = orc.qr_compress(x[b], Hx[b])
            assert np.abs(np.tril(Hxd[b][:r], -1)).max() < 1e-4          # (givens() leaves |b| < eps = 1e-4f alone)
        else:
            r, xo, Hxo, Hfo = orc.givens_eliminate(x[b], Hx[b], Hf[b])
            assert np.abs(Hfd[b] - Hfo).max() < 1e-10
        assert ro[b] == r
        assert np.abs(xd[b] - xo).max() < 1e-10 and np.abs(Hxd[b] - Hxo).max() < 1e-10, (b, np.abs(Hxd[b] - Hxo).max())


# ---------------------------------------------------------------- AbsorbError
@pytest.mark.parametrize("name", _cases("absorb_error"))
def test_absorb_error_edges(built, name):
    """xivo_hip_absorb_error after a gated update at state widths 256 | 257 and 400: the retracted pose, groups and features
    against the oracle's AbsorbError, err zeroed across the whole width. Filter 2's covariance is indefinite and the context
    keeps it (NO_LDLT_FALLBACK): its status is non-zero, nothing is absorbed and its err comes back zero. No gating, so that
    every filter stacks every feature."""
    case = CASES[name]
    B, ng, F, N = case[5]["B"], case[5]["ng"], case[5]["F"], case[5]["N"]
    cam = synth.RADTAN
    sc, lay, ctx, poses, groups, feats, xp = make(ng, F, F, B, N, cam=cam, N=N, flags=FLAG_NO_LDLT_FALLBACK)
    P = np.array([spd(N, 70 + b) * 1e-4 for b in range(B)])
    P[2] = -spd(N, 72) * 1e-2
    poses["Rsg"] = np.eye(3).reshape(-1)
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        try:
            ctx.filter_update(R_VIS, MH, MULT, MIN_INL, False)
        except XivoHipError as e:                   # (the call may report the filter it could not factor)
            assert e.status == -3
        st = ctx.get_status(check=False)
        mask = ctx.get_gate(F)[0].copy()
        err0 = ctx.get_err()
        ctx.absorb_error()
        assert stage(ctx, "other")[0] == "absorb_error_kernel"
        err1 = ctx.get_err()
        pose_d, group_d, feat_d = ctx.get_scene()
    assert st[2] != 0 and (np.delete(st, 2) == 0).all(), st
    assert not err1.any()
    assert err1.shape[1] >= N
    assert np.array_equal(pose_d[2], poses[2]) and np.array_equal(group_d[2], groups[2]) and np.array_equal(feat_d[2]["x"], feats[2]["x"])
    for b in range(B):
        if b == 2:
            continue
        Js, inns, _ = oracle_jacobians(sc, cam, lay, xp, b)
        m = np.ones(F, dtype=bool)
        assert np.array_equal(mask[b], m)
        H, inn, dR = orc.stack_measurements(Js[m], inns[m], sc["ref"][b][m], sc["sind"][b][m], lay, R_VIS)
        dx, _, _ = orc.update_joseph(H, P[b], inn, dR)
        assert rel_fro(err0[b][:N], dx) < TOL_DX
        s = dict(Rsb=sc["Rsb"][b].copy(), Tsb=sc["Tsb"][b].copy(), Rbc=sc["Rbc"][b].copy(), Tbc=sc["Tbc"][b].copy(),
                 Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), Rsg=np.eye(3),
                 gR=sc["gR"][b].copy(), gT=sc["gT"][b].copy(), x=sc["x"][b].copy(), sind=sc["sind"][b], ref=sc["ref"][b])
        orc.absorb_error(s, dx, lay, range(ng), np.nonzero(m)[0])
        cmT = lambda v: np.asarray(v).reshape(3, 3).T
        for k in ("Rsb", "Rbc", "Rsg"):
            assert np.abs(cmT(pose_d[b][k]) - s[k]).max() < 1e-9, (b, k)
        for k in ("Tsb", "Tbc", "Vsb", "bg", "ba"):
            assert np.abs(pose_d[b][k] - s[k]).max() < 1e-9, (b, k)
        for g in range(ng):
            assert np.abs(cmT(group_d[b, g]["Rsb"]) - s["gR"][g]).max() < 1e-9
            assert np.abs(group_d[b, g]["Tsb"] - s["gT"][g]).max() < 1e-9
        assert np.abs(feat_d[b]["x"] - s["x"]).max() < 1e-9
