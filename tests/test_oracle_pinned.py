"""Pins the numpy oracle (oracle/xivo_oracle.py) BEFORE it is trusted as the checker:
 1. the reference's own known-answer test GivensSub (src/test/unittest_givens.cpp:15-37);
 2. the reference's finite-difference Jacobian checks, re-run on the restatement
    (src/test/unittest_jacobians_instate.cpp:28-29 tol 9e-4, ..._oos.cpp tol 1e-5);
 3. committed golden vectors generated from oracle/_ref - the reference's own Eigen /
    Sophus / helpers.cpp / camera arithmetic (tests/golden/make_golden.py);
 4. comparison against oracle/_ref - live where the library is built, else against the calls it answered on the same
    inputs, stored in tests/golden/ref_calls.npz (tests/ref_replay.py, tests/golden/make_ref_calls.py)."""
import math
import os

import numpy as np
import pytest

import xivo_oracle as orc
from ref_replay import reference
from xivo_amd import synth

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v1.npz"))
CAMS = {"pinhole": synth.PINHOLE, "equi": synth.EQUI, "radtan": synth.RADTAN, "atan": synth.ATAN}


def lay_from(a):
    N, gb, ng, fb, nf = [int(v) for v in a]
    lay = orc.Layout(ng, nf, N=N, group_begin=gb)
    assert lay.feature_begin == fb
    return lay


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300)


# ---- 1. reference KAT -------------------------------------------------------------
def test_givens_sub_kat():
    tol = 5e-4
    v1 = np.array([0.9134, 0.6324]); G1 = orc.givens(*v1); y1 = G1.T @ v1
    assert abs(abs(y1[0]) - 1.1110) < tol and abs(y1[1]) < tol
    assert abs(abs(G1[0, 0]) - 0.8222) < tol and abs(abs(G1[0, 1]) - 0.5692) < tol
    assert abs(abs(G1[1, 0]) - 0.5692) < tol and abs(abs(G1[1, 1]) - 0.8222) < tol
    v2 = np.array([0.1270, 1.1109]); G2 = orc.givens(*v2); y2 = G2.T @ v2
    assert abs(abs(y2[0]) - 1.1181) < tol and abs(y2[1]) < tol
    assert abs(abs(G2[0, 0]) - 0.1136) < tol and abs(abs(G2[0, 1]) - 0.9935) < tol


# ---- 2. finite-difference checks of the Jacobian chain ------------------------------
def _scene(seed=0, cam=synth.PINHOLE):
    sc = synth.g_level(3, 4, 4, 1, seed=seed, cam=cam)
    lay = orc.Layout(3, 4)
    i = 1
    r = int(sc["ref"][0, i])
    return dict(x=sc["x"][0, i].copy(), Rsbr=sc["gR"][0, r].copy(), Tsbr=sc["gT"][0, r].copy(), Rsb=sc["Rsb"][0].copy(),
                Tsb=sc["Tsb"][0].copy(), Rbc=sc["Rbc"][0].copy(), Tbc=sc["Tbc"][0].copy(), lay=lay, ref=r, sind=i)


def _xcn(s):
    _, _, _, c = orc.compute_jacobian(s["x"], [0, 0], s["Rsbr"], s["Tsbr"], s["Rsb"], s["Tsb"], s["Rbc"], s["Tbc"],
                                      synth.PINHOLE, s["lay"], s["ref"], s["sind"], return_cache=True)
    return c


@pytest.mark.parametrize("which", ["Wsb", "Tsb", "Wbc", "Tbc", "Wsbr", "Tsbr", "x"])
def test_instate_chain_finite_difference(which):
    """As unittest_jacobians_instate.cpp: forward differences (delta 1e-6) of Xcn
    w.r.t. each error-state block vs the analytic cache entry, tol 9e-4."""
    s = _scene(3)
    c0 = _xcn(s)
    ana = c0["dXcn_d" + which]
    delta = 1e-6
    num = np.zeros((3, 3))
    for j in range(3):
        p = dict(s)
        d = np.zeros(3); d[j] = delta
        if which == "Wsb": p["Rsb"] = s["Rsb"] @ orc.so3_exp(d)
        elif which == "Wbc": p["Rbc"] = s["Rbc"] @ orc.so3_exp(d)
        elif which == "Wsbr": p["Rsbr"] = s["Rsbr"] @ orc.so3_exp(d)
        elif which == "Tsb": p["Tsb"] = s["Tsb"] + d
        elif which == "Tbc": p["Tbc"] = s["Tbc"] + d
        elif which == "Tsbr": p["Tsbr"] = s["Tsbr"] + d
        else: p["x"] = s["x"] + d
        num[:, j] = (_xcn(p)["Xcn"] - c0["Xcn"]) / delta
    assert np.abs(num - ana).max() < 9e-4


def test_oos_chain_finite_difference():
    """As unittest_jacobians_oos.cpp: d(xp)/d(group pose, Wbc, Tbc, Xs), tol 1e-5 (relative here)."""
    s = _scene(4)
    lay = s["lay"]; cam = synth.PINHOLE
    Xs = _xcn(s)["Xs"]
    f = lambda Xs_, R, T, Rbc, Tbc: orc.oos_jacobian_internal(Xs_, R, T, Rbc, Tbc, [0, 0], cam, lay, 1)
    Hf, Hx, inn0 = f(Xs, s["Rsb"], s["Tsb"], s["Rbc"], s["Tbc"])
    delta = 1e-7
    goff = lay.group_begin + 6
    for j in range(3):
        d = np.zeros(3); d[j] = delta
        num = -(f(Xs + d, s["Rsb"], s["Tsb"], s["Rbc"], s["Tbc"])[2] - inn0) / delta
        assert np.abs(num - Hf[:, j]).max() < 1e-5 * max(1, np.abs(Hf).max())
        num = -(f(Xs, s["Rsb"] @ orc.so3_exp(d), s["Tsb"], s["Rbc"], s["Tbc"])[2] - inn0) / delta
        assert np.abs(num - Hx[:, goff + j]).max() < 1e-4 * max(1, np.abs(Hx).max())
        num = -(f(Xs, s["Rsb"], s["Tsb"] + d, s["Rbc"], s["Tbc"])[2] - inn0) / delta
        assert np.abs(num - Hx[:, goff + 3 + j]).max() < 1e-4 * max(1, np.abs(Hx).max())
        num = -(f(Xs, s["Rsb"], s["Tsb"], s["Rbc"], s["Tbc"] + d)[2] - inn0) / delta
        assert np.abs(num - Hx[:, orc.TBC + j]).max() < 1e-4 * max(1, np.abs(Hx).max())


# ---- 3. golden vectors from the Eigen-built reference driver -------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_golden_update_joseph(tag):
    err, Pn, _ = orc.update_joseph(G[f"uj_{tag}_H"], G[f"uj_{tag}_P"], G[f"uj_{tag}_inn"], G[f"uj_{tag}_dR"])
    assert rel(err, G[f"uj_{tag}_err"]) < 1e-10
    assert rel(Pn, G[f"uj_{tag}_Pn"]) < 1e-10


@pytest.mark.parametrize("name", list(CAMS))
def test_golden_cameras(name):
    for i, xc in enumerate(G["cam_xc"]):
        xp, J = orc.camera_project(CAMS[name], xc)
        assert rel(xp, G[f"cam_{name}_xp"][i]) < 1e-13
        assert np.abs(J - G[f"cam_{name}_J"][i]).max() < 1e-10 * max(1.0, np.abs(J).max())


@pytest.mark.parametrize("name", list(CAMS))
def test_golden_jacobian_fill_and_gating(name):
    lay = lay_from(G["lay"])
    k = lambda s: G[f"jac_{name}_{s}"]
    Js, inns = [], []
    for i in range(10):
        r, s = int(k("ref")[i]), int(k("sind")[i])
        J, inn, _ = orc.compute_jacobian(k("x")[i], k("xp")[i], k("gR")[r], k("gT")[r], k("Rsb"), k("Tsb"), k("Rbc"),
                                         k("Tbc"), CAMS[name], lay, r, s)
        assert rel(J, k("J")[i]) < 1e-12 and np.abs(inn - k("inn")[i]).max() < 1e-9
        Js.append(J); inns.append(inn)
    H, inn, dR = orc.stack_measurements(Js, inns, k("ref"), k("sind"), lay, 2.25)
    assert rel(H, k("H")) < 1e-12          # includes the FillJacobianBlock quirk (feature.cpp:675-676)
    goff = lay.group_begin + 6 * int(k("ref")[0])
    assert np.all(H[0:2, goff + 3:goff + 6] == 0) and np.any(Js[0][:, goff + 3:goff + 6] != 0)
    d = orc.mh_distances(np.array(Js), k("P"), np.array(inns), 2.25)
    assert rel(d, k("dist")) < 1e-9


def test_golden_oos_and_slow_givens():
    lay = lay_from(G["oos_lay"])
    obs = [(c, G["oos_xp"][c]) for c in range(5)]
    for c in range(5):
        hf, hx, inn = orc.oos_jacobian_internal(G["oos_Xs"], G["oos_gR"][c], G["oos_gT"][c], G["oos_Rbc"], G["oos_Tbc"],
                                                G["oos_xp"][c], synth.PINHOLE, lay, c)
        assert rel(hf, G["oos_Hf"][2 * c:2 * c + 2]) < 1e-12
        assert rel(hx, G["oos_Hx"][2 * c:2 * c + 2]) < 1e-12
        assert np.abs(inn - G["oos_r"][2 * c:2 * c + 2]).max() < 1e-9
    Hxp, rp, A = orc.oos_jacobian(G["oos_Xs"], obs, G["oos_gR"], G["oos_gT"], G["oos_Rbc"], G["oos_Tbc"], synth.PINHOLE, lay)
    assert A.shape == G["oos_A"].shape == (10, 7)
    assert rel(A, G["oos_A"]) < 1e-11       # the SAME (non-orthonormal) basis as Eigen's FullPivLU::kernel
    assert rel(Hxp, G["oos_Hxp"]) < 1e-11 and rel(rp, G["oos_rp"]) < 1e-11
    assert np.abs(A.T @ G["oos_Hf"]).max() < 1e-9 * np.abs(G["oos_Hf"]).max()


@pytest.mark.parametrize("tag", ["full", "def"])
def test_golden_fullpivlu_kernel(tag):
    ker, rank = orc.fullpivlu_kernel(G[f"lu_{tag}_A"])
    assert rank == int(G[f"lu_{tag}_rank"]) and ker.shape == G[f"lu_{tag}_ker"].shape
    assert np.abs(ker - G[f"lu_{tag}_ker"]).max() < 1e-12


def test_golden_givens_elimination():
    rows, x, Hx, Hf = orc.givens_eliminate(G["giv_x"], G["giv_Hx"], G["giv_Hf"])
    assert rows == int(G["giv_rows"])
    assert rel(x, G["giv_xo"]) < 1e-12 and rel(Hx, G["giv_Hxo"]) < 1e-12
    assert np.abs(Hf - G["giv_Hfo"]).max() < 1e-12   # eliminated block: ~0, compare absolutely


def test_golden_propagation_tail_and_so3():
    Pn, _ = orc.rk4_cov_tail(G["prop_P"], G["prop_FK"], G["prop_PK"], float(G["prop_dt"]), G["prop_Q"])
    assert rel(Pn, G["prop_Pn"]) < 1e-13
    for w, R in zip(G["so3_w"], G["so3_R"]):
        assert np.abs(orc.so3_exp(w) - R).max() < 1e-12


# ---- 4. against oracle/_ref: live where it is built, its stored calls elsewhere (tests/ref_replay.py) ---------------
def _ref(stored=True):
    import ref_binding
    return reference("ref", ref_binding.load, stored)


@pytest.mark.parametrize("N,F", [(150, 50), (250, 80), (203, 30)])
def test_live_update_joseph_vs_ref(N, F):
    ref = _ref(stored=False)     # (library only: without it, test_golden_update_joseph / _at_baseline_sizes make this comparison)
    P, H, inn, dR = synth.s_level(N, F, 1, seed=N + F)
    e1, P1 = ref.update_joseph(H[0], P[0], inn[0], dR[0])
    e2, P2, _ = orc.update_joseph(H[0], P[0], inn[0], dR[0])
    assert rel(e2, e1) < 1e-9 and rel(P2, P1) < 1e-11


@pytest.mark.parametrize("case", ["spd", "indefinite", "negative_definite", "zero_pivots", "asymmetric_P"])
def test_ldlt_restatement_vs_eigen_ldlt(case):
    """orc.ldlt_eigen / ldlt_solve_eigen (Eigen 3.3.9 LDLT.h:291-404, :561-600 restated) inside UpdateJosephForm against the
    real `S_.ldlt().solve(H_ * P_)` of oracle/_ref: positive definite, indefinite and negative definite S, an S with exactly
    zero pivots (two all-zero measurement rows with R = 0: Eigen leaves a zero pivot undivided and its solve drops the
    component - the update equals the one without those rows), and a P_ that is not symmetric (the reference never
    re-symmetrises; it reads P_ as stored)."""
    ref = _ref(stored=False)     # (library only: five 100 x 100 covariances of the reference's rounding are not kept)
    N, F = 100, 20
    P, H, inn, dR = synth.s_level(N, F, 1, seed=41)
    P, H, inn, dR = P[0], H[0], inn[0], dR[0]
    if case == "indefinite":
        w, Q = np.linalg.eigh(P); w[-3:] *= -1.0; P = (Q * w) @ Q.T; P = 0.5 * (P + P.T)
    elif case == "negative_definite":
        P = -P
    elif case == "zero_pivots":
        H[6:8] = 0.0; dR[6:8] = 0.0
    elif case == "asymmetric_P":
        rng = np.random.default_rng(3)
        P = P + 1e-3 * np.triu(rng.standard_normal((N, N)), 1) * np.abs(P).mean()
    S = (H @ P) @ H.T + np.diag(dR)
    if case == "indefinite":
        assert np.linalg.eigvalsh(0.5 * (S + S.T)).min() < 0 < np.linalg.eigvalsh(0.5 * (S + S.T)).max()
    e1, P1 = ref.update_joseph(H, P, inn, dR)[:2]
    e2, P2, _ = orc.update_joseph(H, P, inn, dR, solver="ldlt")
    assert rel(e2, e1) < 1e-11 and rel(P2, P1) < 1e-12
    if case == "zero_pivots":
        mat, tr = orc.ldlt_eigen(S)
        assert (np.diag(mat) == 0.0).sum() == 2
        keep = np.ones(2 * F, dtype=bool); keep[6:8] = False
        e3, P3, _ = orc.update_joseph(H[keep], P, inn[keep], dR[keep])
        assert rel(e1, e3) < 1e-11 and rel(P1, P3) < 1e-12
    elif case != "asymmetric_P":   # (an asymmetric P_ makes S asymmetric: Eigen's L D L^T reads its lower triangle, LU all of it)
        e3, P3, _ = orc.update_joseph(H, P, inn, dR)          # the LAPACK-LU oracle the parity tests use
        assert rel(e3, e1) < 1e-10 and rel(P3, P1) < 1e-11


def test_live_fullpivlu_random_shapes():
    ref = _ref()
    rng = np.random.default_rng(5)
    for k in range(2, 9):
        A = rng.normal(size=(3, 2 * k))
        k1, r1 = ref.fullpivlu_kernel(A)
        k2, r2 = orc.fullpivlu_kernel(A)
        assert r1 == r2 and np.abs(k1 - k2).max() < 1e-11


def test_mh_gate_loop_semantics():
    d = np.array([1.0, 7.0, 3.0, 9.0, 100.0, 6.5])
    m, rej, th = orc.mh_gate(d, 5.991, 1.1, 2)
    assert m.tolist() == [True, False, True, False, False, False] and rej == 4 and th == 5.991
    # needs two relaxations to reach 4 inliers: 5.991 -> 6.59 -> 7.25
    m, rej, th = orc.mh_gate(d, 5.991, 1.1, 4)
    assert m.sum() == 4 and rej == 4 + 3 + 2 and abs(th - 5.991 * 1.1 * 1.1) < 1e-12
    assert orc.mh_gate(d, 5.991, 1.1, 0)[0].sum() == 0   # loop never entered (update.cpp:73)


# ---- propagation (a11-a14) ------------------------------------------------------------
def _rk4_inputs():
    X = orc.MotionState(G["rk4_Rsb"], G["rk4_Tsb"], G["rk4_Vsb"], G["rk4_bg"], G["rk4_ba"], G["rk4_Rsg"])
    return X, G["rk4_P"], G["rk4_gyro"], G["rk4_accel"], G["rk4_sg"], G["rk4_sa"], float(G["rk4_dt"]), G["rk4_Qimu"], G["rk4_g"]


def test_golden_rk4_step():
    """Tableau form of the oracle == line-by-line RK4Step on Sophus/Eigen (rk4.cpp:35-103)."""
    X, P, gy, ac, sg, sa, dt, Qi, gv = _rk4_inputs()
    Xn, Pn = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, orc.RK4_TABLEAU)
    assert np.abs(Xn.Rsb - G["rk4_Rn"]).max() < 1e-14 and np.abs(Xn.Tsb - G["rk4_Tn"]).max() < 1e-15
    assert np.abs(Xn.Vsb - G["rk4_Vn"]).max() < 1e-15 and rel(Pn, G["rk4_Pn"]) < 1e-14


def test_prince_dormand_consistent_with_rk4():
    """Both integrators solve the same ODE: on one 2 ms step they agree to O(h^4)."""
    X, P, gy, ac, sg, sa, dt, Qi, gv = _rk4_inputs()
    Xa, Pa = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, orc.RK4_TABLEAU)
    Xb, Pb = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, orc.PD_TABLEAU)
    assert np.abs(Xa.Rsb - Xb.Rsb).max() < 1e-8 and np.abs(Xa.Vsb - Xb.Vsb).max() < 1e-6
    assert rel(Pb, Pa) < 1e-3
    # Dormand-Prince weights of princedormand.cpp:195-200 sum to 1 (to the 4 printed digits)
    assert abs(sum(orc.PD_TABLEAU["b"]) - 1.0) < 1e-3 and abs(sum(orc.RK4_TABLEAU["b"]) - 1.0) < 1e-15


def test_substepping_half_step_trick():
    """rk4.cpp:19-31: dt = 5 ms at stepsize 2 ms -> steps 2, 2, 1 ms; 4.5 ms -> 2, 1 (half), 1.5 ms."""
    X, P, gy, ac, sg, sa, _, Qi, gv = _rk4_inputs()
    calls = []
    real = orc.integrator_step

    def spy(X_, P_, g_, a_, sg_, sa_, h, *rest):
        calls.append(round(h, 6))
        return real(X_, P_, g_, a_, sg_, sa_, h, *rest)
    orc.integrator_step = spy
    try:
        orc.integrate(X, P, gy, ac, sg, sa, 0.005, Qi, gv, orc.RK4_TABLEAU, 0.002)
        assert calls == [0.002, 0.002, 0.001]
        calls.clear()
        orc.integrate(X, P, gy, ac, sg, sa, 0.0045, Qi, gv, orc.RK4_TABLEAU, 0.002)
        assert calls == [0.002, 0.001, 0.0015]
    finally:
        orc.integrator_step = real


# ---- depth sub-filter (Feature::SubfilterUpdate, src/feature.cpp:246-297) ----
SUB_CAMS = {"pinhole": synth.PINHOLE, "equi": synth.EQUI, "radtan": synth.RADTAN, "atan": synth.ATAN}


@pytest.mark.parametrize("name", list(SUB_CAMS))
def test_golden_subfilter_update(name):
    """numpy restatement vs the Eigen/Sophus driver of the reference expression sequence: three consecutive frames,
    three features, incl. the ratio > 1 (inflated S, outlier counter) branch and the INITIALIZING -> READY switch."""
    cam = SUB_CAMS[name]
    k = lambda s: G[f"sub_{name}_{s}"]
    x = k("x0").copy(); P = np.array([np.diag([1e-4, 1e-4, 0.25]) for _ in range(3)])
    ic = [0, 0, 0]; oc = [0.0, 0.0, 0.0]
    saw_outlier = False
    for fr in range(3):
        for i in range(3):
            r = int(k("ref")[i])
            x[i], P[i], st, ic[i], oc[i] = orc.subfilter_update(x[i], P[i], k("xp")[fr, i], k("Rsb"), k("Tsb"), k("Rbc"), k("Tbc"),
                                                                k("gR")[r], k("gT")[r], cam, 3.5, 5.991, 1, ic[i], oc[i])
            assert st == k("status")[fr, i] and ic[i] == k("ic")[fr, i]
            assert abs(oc[i] - k("oc")[fr, i]) < 1e-9 * max(1.0, oc[i])
            saw_outlier |= oc[i] > 0
        assert np.abs(x - k("x")[fr]).max() < 1e-11 and rel(P, k("P")[fr]) < 1e-9
    assert saw_outlier and k("status")[0].max() == 0 and k("status")[2].min() == 1


def test_candidate_flags_and_score():
    """Criteria::Candidate / CandidateStrict (src/options.cpp:10-33), Feature::score (src/feature.cpp:133-142)."""
    x = np.array([0.1, -0.2, math.log(2.0)])
    assert orc.candidate_flags(x, orc.FEAT_INITIALIZING, 0.0) == (True, False)
    assert orc.candidate_flags(x, orc.FEAT_READY, 0.0) == (True, True)
    assert orc.candidate_flags(x, orc.FEAT_READY, 0.02) == (False, False)              # outlier counter too high
    assert orc.candidate_flags(np.array([0, 0, math.log(6.0)]), orc.FEAT_READY, 0.0) == (False, False)   # beyond max_depth
    assert orc.candidate_flags(np.array([0, 0, math.log(0.01)]), orc.FEAT_READY, 0.0) == (False, False)  # below min_depth
    assert orc.feature_score(np.diag([1.0, 2.0, 0.3])) == -0.3


@pytest.mark.parametrize("rows,cols,eff", [(12, 5, -1), (40, 21, -1), (30, 7, 20)])
def test_live_qr_compress_vs_ref(rows, cols, eff):
    """xivo::QR (src/helpers.cpp:78-101) of the reference itself (helpers.cpp compiled verbatim) vs the restatement;
    the result is upper-trapezoidal and the rotations are orthonormal (norms preserved)."""
    rng = np.random.default_rng(rows * 100 + cols)
    x = rng.normal(size=rows); Hx = rng.normal(size=(rows, cols))
    r0, x0, H0 = _ref().QR(x, Hx, eff)
    r1, x1, H1 = orc.qr_compress(x, Hx, eff)
    assert r0 == r1 == (rows if eff == -1 else eff)
    assert np.abs(x0 - x1).max() < 1e-12 and np.abs(H0 - H1).max() < 1e-12
    n = r1
    assert np.abs(np.tril(H1[:n], -1)).max() < 1e-12
    assert abs(np.linalg.norm(H1[:n]) - np.linalg.norm(Hx[:n])) < 1e-10 and abs(np.linalg.norm(x1[:n]) - np.linalg.norm(x[:n])) < 1e-10


# ---- round 2 pins: golden_v2.npz (tests/golden/make_golden_v2.py) ------------------------------------------------
G2 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v2.npz"))


def _pd_inputs(tag):
    g = lambda k: G2[f"pd_{tag}_{k}"]
    X = orc.MotionState(g("Rsb"), g("Tsb"), g("Vsb"), g("bg"), g("ba"), g("Rsg"))
    return X, g("P"), g("gyro"), g("accel"), g("sg"), g("sa"), float(g("dt")), g("Qimu"), g("g")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_prince_dormand_step(tag):
    """Tableau form of the oracle == line-by-line PrinceDormandStep on Sophus / Eigen (src/princedormand.cpp:85-221):
    the 7 stages, the printed 4-digit combination weights (:195-200), ComposeMotion incl. normalize(), the covariance tail."""
    X, P, gy, ac, sg, sa, dt, Qi, gv = _pd_inputs(tag)
    Xn, Pn = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, orc.PD_TABLEAU)
    g = lambda k: G2[f"pd_{tag}_{k}"]
    assert np.abs(Xn.Rsb - g("Rn")).max() < 1e-14 and np.abs(Xn.Tsb - g("Tn")).max() < 1e-15
    assert np.abs(Xn.Vsb - g("Vn")).max() < 1e-15 and rel(Pn, g("Pn")) < 1e-14


def test_live_prince_dormand_and_rk4_steps_vs_ref():
    ref = _ref()
    rng = np.random.default_rng(9)
    for k in range(4):
        N = 29 + 6 * k
        A = rng.uniform(-1, 1, size=(N, N)); P = A @ A.T / N * 1e-3 + 1e-6 * np.eye(N)
        X = orc.MotionState(orc.so3_exp(rng.normal(size=3) * 0.4), rng.normal(size=3), rng.normal(size=3),
                            rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05, orc.so3_exp([0.02, -0.01, 0.0]))
        gy, ac = rng.normal(size=3) * (1 + 3 * k), np.array([0.2, -0.1, 9.7]) + rng.normal(size=3)
        sg, sa = rng.normal(size=3) * 5, rng.normal(size=3)
        Qi = np.diag(rng.uniform(1e-6, 1e-3, 12)); gv = np.array([0.0, 0.0, -9.8]); dt = 0.001 * (1 + k)
        for tab, fn in ((orc.PD_TABLEAU, ref.pd_step), (orc.RK4_TABLEAU, ref.rk4_step)):
            R1, T1, V1, P1 = fn(X, P, gy, ac, sg, sa, dt, Qi, gv)
            Xn, Pn = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, tab)
            assert np.abs(Xn.Rsb - R1).max() < 1e-13 and np.abs(Xn.Tsb - T1).max() < 1e-14 and np.abs(Xn.Vsb - V1).max() < 1e-13
            assert rel(Pn, P1) < 1e-13


def _ransac_state(tag):
    g = lambda k: G2[f"rs_{tag}_in_{k}"]
    st = dict(Rsb=g("Rsb").copy(), Tsb=g("Tsb").copy(), Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), Rbc=g("Rbc").copy(),
              Tbc=g("Tbc").copy(), Rsg=np.eye(3), gR=g("gR").copy(), gT=g("gT").copy(), x=g("x").copy(), sind=g("sind"), ref=g("ref"))
    return st, g("P"), g("xp"), lay_from(g("lay")), float(g("R")), float(g("thresh")), float(g("chi2")), int(g("gauge"))


@pytest.mark.parametrize("tag,cam", [("pin", "pinhole"), ("rad", "radtan"), ("tmp", "equi")])
def test_golden_one_point_ransac(tag, cam):
    """The oracle's OnePointRANSAC (src/update.cpp:213-393) against the flow run on the reference's arithmetic: Eigen core
    up to the partial UpdateJosephForm (low-innovation set, FindNewRefGroup, P zeroing, full-row stacking), Sophus exp in
    AbsorbError, ComputeJacobian at the updated state, 2x2 LLT chi-square rescue. 'tmp': gauge group without a
    low-innovation inlier -> temporary reference group path (:292-301)."""
    st, P, xp, lay, R, th, c2, gauge = _ransac_state(tag)
    ng = lay.n_groups
    out = orc.one_point_ransac(st, P, xp, CAMS[cam], lay, R, th, c2, gauge, range(ng))
    assert np.array_equal(out["low"], G2[f"rs_{tag}_low"]) and out["low"].sum() == int(G2[f"rs_{tag}_n_low"])
    assert rel(out["err"], G2[f"rs_{tag}_err"]) < 1e-9 and rel(out["P_partial"], G2[f"rs_{tag}_P_partial"]) < 1e-11
    chi = G2[f"rs_{tag}_chi"]
    for i, d in out["chi2"].items():
        assert abs(d - chi[i]) < 1e-7 * max(1.0, chi[i])
    assert sorted(out["chi2"]) == list(np.nonzero(~G2[f"rs_{tag}_low"])[0])
    assert out["inliers"] == list(G2[f"rs_{tag}_kept"])
    assert len(out["rejected"]) >= 1 and len(out["inliers"]) > out["low"].sum()      # something rescued, something rejected


def test_live_one_point_ransac_core_vs_ref():
    ref = _ref(stored=False)     # (library only: without it, test_golden_one_point_ransac makes this comparison)
    for seed in range(6):
        cam = [synth.PINHOLE, synth.EQUI, synth.RADTAN][seed % 3]
        ng, nf = 4, 11
        sc = synth.g_level(ng, nf, nf, 1, seed=100 + seed, cam=cam)
        lay = orc.Layout(ng, nf)
        rng = np.random.default_rng(seed)
        A = rng.uniform(-1, 1, size=(lay.N, lay.N)); P = (A @ A.T / lay.N + 1e-3 * np.eye(lay.N)) * 1e-4
        xp = np.array([orc.camera_project(cam, sc["Xcn"][0, i][:2] / sc["Xcn"][0, i][2])[0] for i in range(nf)])
        xp += rng.normal(size=xp.shape) * 1.2
        st = dict(Rsb=sc["Rsb"][0], Tsb=sc["Tsb"][0], Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), Rbc=sc["Rbc"][0],
                  Tbc=sc["Tbc"][0], Rsg=np.eye(3), gR=sc["gR"][0].copy(), gT=sc["gT"][0].copy(), x=sc["x"][0].copy(),
                  sind=sc["sind"][0], ref=sc["ref"][0])
        gauge = -1 if seed % 2 else 0
        out = orc.one_point_ransac(st, P, xp, cam, lay, 1.0, 1.8, 5.89, gauge, range(ng))
        J = []; inn = []
        for i in range(nf):
            r = int(st["ref"][i])
            Ji, ii, _ = ref.compute_jacobian(st["x"][i], xp[i], st["gR"][r], st["gT"][r], st["Rsb"], st["Tsb"], st["Rbc"], st["Tbc"],
                                             cam, lay, r, int(st["sind"][i]))
            J.append(Ji); inn.append(ii)
        n, low, err, P2 = ref.one_point_ransac_core(np.array(J), np.array(inn), P, st["sind"], st["ref"], gauge, lay, 1.0, 1.8)
        assert np.array_equal(low, out["low"])
        if n == -1:
            assert out["low"].all()
        elif n > 0:
            assert rel(out["err"], err) < 1e-9 and rel(out["P_partial"], P2) < 1e-11


@pytest.mark.parametrize("tag", ["150", "250"])
def test_golden_update_joseph_at_baseline_sizes(tag):
    """a1 at BASELINE.json's synthetic sizes (150, 50) and (250, 80) against the Eigen driver's LDLT / dense products."""
    import hashlib
    N, F, seed = [int(v) for v in G2[f"ujb_{tag}_seed"]]
    P, H, inn, dR = synth.s_level(N, F, 1, seed=seed)
    h = hashlib.sha256()
    for a in (P[0], H[0], inn[0], dR[0]):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), G2[f"ujb_{tag}_sha"]), "synthetic input generator drifted"
    err, Pn, _ = orc.update_joseph(H[0], P[0], inn[0], dR[0])
    assert rel(err, G2[f"ujb_{tag}_err"]) < 1e-9 and rel(Pn, G2[f"ujb_{tag}_Pn"]) < 1e-11


# ---- round 4 pins: the reference's OWN TEXT compiled (oracle/ref/extract_reference.py -> oracle/ref/xivo_refx.cpp) -------------
def _refx(N, stored=True):
    import ref_binding
    return reference(f"refx_{N}", lambda: ref_binding.loadx(N), stored)


def test_extracted_build_layout_constants():
    """the extracted src/core.h:40-105 computes the layout itself: default build N = 203, 8 groups / 60 features N = 251"""
    x = _refx(203)
    assert (x.N, x.group_begin, x.feature_begin) == (203, 23, 23 + 6 * 15)
    y = _refx(251)
    assert (y.N, y.group_begin, y.feature_begin) == (251, 23, 23 + 6 * 8)
    lay = orc.Layout(8, 60)
    assert (lay.N, lay.group_begin, lay.feature_begin) == (y.N, y.group_begin, y.feature_begin)


@pytest.mark.parametrize("N,F", [(203, 30), (250, 80), (150, 50), (64, 8)])
def test_extracted_update_joseph_form_equals_the_retyped_driver_bit_for_bit(N, F):
    """Estimator::UpdateJosephForm: the text of src/estimator.cpp:1257-1288 compiled as is == the line-by-line retyping
    of oracle/ref/xivo_ref.cpp, BIT FOR BIT (same Eigen expressions on the same dynamic types) - and hence the numpy
    oracle's distance to either is the same number."""
    # (library against library: only the libraries can show it; the oracle's half is test_golden_update_joseph's)
    ref, x = _ref(stored=False), _refx(203, stored=False)
    P, H, inn, dR = synth.s_level(N, F, 2, seed=5 + N)
    for b in range(2):
        e1, P1 = ref.update_joseph(H[b], P[b], inn[b], dR[b])
        e2, P2 = x.update_joseph(H[b], P[b], inn[b], dR[b])
        assert np.array_equal(e1, e2) and np.array_equal(P1, P2)
        e3, P3, _ = orc.update_joseph(H[b], P[b], inn[b], dR[b])
        assert rel(e3, e2) < 1e-9 and rel(P3, P2) < 1e-11
    # an indefinite S and zero pivots go through Eigen's pivoted L D L^T in both
    Pn = -P[0]
    assert all(np.array_equal(a, b_) for a, b_ in zip(ref.update_joseph(H[0], Pn, inn[0], dR[0]), x.update_joseph(H[0], Pn, inn[0], dR[0])))


@pytest.mark.parametrize("N,cam", [(203, "pinhole"), (251, "equi")])
def test_extracted_mh_gating_whole_function(N, cam):
    """Estimator::MHGating, src/update.cpp:50-116 as extracted (distances through the fixed-size 2 x kFullSize J of
    src/feature.h:281, the relaxation loop, the status / DestroyFeatures bookkeeping) vs the oracle: same inlier list in the
    same order, the same accumulated num_mh_rejected_ (the counting quirk of :87), REJECTED_BY_FILTER exactly on the others,
    a GAUGE feature keeps its status when it is an inlier; and the retyped distances agree to rounding."""
    x, ref = _refx(N), _ref()
    ng, nf = (15, 30) if N == 203 else (8, 60)
    lay = orc.Layout(ng, nf)
    assert lay.N == N
    from scene_util import scene_arrays, oracle_jacobians, spd
    for seed in range(3):
        sc = synth.g_level(ng, nf, nf, 1, seed=400 + seed, cam=CAMS[cam])
        poses, groups, feats, xp = scene_arrays(sc, CAMS[cam])
        if seed == 1:
            xp[0, [2, 7, 11]] += 40.0                       # three outliers
        if seed == 2:
            xp[0, 3:] += np.linspace(6, 60, nf - 3)[:, None]   # almost everything wild: the threshold has to relax
        P = spd(N, 50 + seed) * 1e-4
        Js, inns, _ = oracle_jacobians(sc, CAMS[cam], lay, xp, 0)
        d = orc.mh_distances(Js, P, inns, 2.25)
        m, nrej, _ = orc.mh_gate(d, 5.991, 1.1, 5)
        status = np.full(nf, 3, dtype=np.int32); status[0] = 7      # feature 0 fixes the gauge
        idx, st_after, nrej_x, ndes = x.mh_gating(Js, inns, P, 2.25, 5.991, 1.1, 5, status)
        assert idx.tolist() == np.nonzero(m)[0].tolist() and nrej_x == nrej and ndes == int((~m).sum())
        assert all(st_after[i] == (4 if not m[i] else (7 if i == 0 else 3)) for i in range(nf))
        assert rel(ref.mh_distances(Js, P, inns, 2.25), d) < 1e-10
    assert (~m).sum() > 0


@pytest.mark.parametrize("N", [203, 251])
def test_extracted_filter_update_stacking_quirk_update_and_absorb(N):
    """Estimator::FilterUpdate (src/update.cpp:120-153) as extracted - Feature::FillJacobianBlock (src/feature.cpp:658-684,
    incl. the :675-676 overwrite of the group block), UpdateJosephForm, AbsorbError (src/estimator.cpp:875-921 with
    State::operator+= of src/core.h:135-165 and Feature::UpdateState) - vs the oracle's stack_measurements / update_joseph /
    absorb_error: H identical entry for entry (a copy), dx 1e-9, P 1e-11, the retracted state and the features 1e-12."""
    x = _refx(N, stored=False)    # (library only: without it, test_golden_v3_filter_update makes this comparison)
    ng, nf = (15, 30) if N == 203 else (8, 60)
    lay = orc.Layout(ng, nf)
    from scene_util import scene_arrays, oracle_jacobians, spd
    sc = synth.g_level(ng, nf, nf, 1, seed=77, cam=synth.RADTAN)
    poses, groups, feats, xp = scene_arrays(sc, synth.RADTAN)
    P = spd(N, 9) * 1e-4
    Js, inns, _ = oracle_jacobians(sc, synth.RADTAN, lay, xp, 0)
    X = orc.MotionState(sc["Rsb"][0], sc["Tsb"][0], [0.1, -0.2, 0.05], [0.01, 0.0, -0.01], [0.02, 0.01, 0.0], orc.so3_exp([0.01, -0.02, 0.0]))
    Hx, err_x, Px, Rsb, Tsb, Vsb, bg, ba, Rsg, xs = x.filter_update(Js, inns, sc["ref"][0], sc["sind"][0], 2.25, P, X, sc["Rbc"][0],
                                                                     sc["Tbc"][0], sc["x"][0])
    H, inn, dR = orc.stack_measurements(Js, inns, sc["ref"][0], sc["sind"][0], lay, 2.25)
    assert np.array_equal(Hx, H)                             # the as-coded stacking incl. the overwrite quirk
    goff = lay.group_begin + 6 * int(sc["ref"][0][0])
    assert np.abs(Hx[0:2, goff:goff + 3]).max() > 0 and not Hx[0:2, goff + 3:goff + 6].any()
    e_ref, P_ref, _ = orc.update_joseph(H, P, inn, dR)
    assert rel(e_ref, err_x) < 1e-9 and rel(P_ref, Px) < 1e-11
    st = dict(Rsb=X.Rsb.copy(), Tsb=X.Tsb.copy(), Vsb=X.Vsb.copy(), bg=X.bg.copy(), ba=X.ba.copy(), Rbc=sc["Rbc"][0].copy(),
              Tbc=sc["Tbc"][0].copy(), Rsg=X.Rsg.copy(), gR=sc["gR"][0].copy(), gT=sc["gT"][0].copy(), x=sc["x"][0].copy(), sind=sc["sind"][0])
    orc.absorb_error(st, err_x, lay, [], range(nf))
    assert np.abs(st["Rsb"] - Rsb).max() < 1e-12 and np.abs(st["Tsb"] - Tsb).max() < 1e-12 and np.abs(st["Vsb"] - Vsb).max() < 1e-12
    assert np.abs(st["bg"] - bg).max() < 1e-12 and np.abs(st["ba"] - ba).max() < 1e-12 and np.abs(st["Rsg"] - Rsg).max() < 1e-12
    assert np.abs(st["x"] - xs).max() < 1e-12


@pytest.mark.parametrize("N", [203, 251])
def test_extracted_integrator_steps_vs_retyped_and_oracle(N):
    """Estimator::RK4Step (src/rk4.cpp:35-103) and PrinceDormandStep (src/princedormand.cpp:85-221) as extracted - with the
    reference's SPARSE F_ / G_ (src/estimator.h:467-470; the retyping uses dense matrices: same sums, the sparse products
    skip the structural zeros) and the compile-time block sizes - vs the retyped driver and the oracle's tableau form:
    state 1e-13, P 1e-13 relative (measured ~1e-16)."""
    # (library only: without it, test_golden_v3_integrator_steps / test_golden_rk4_step / test_golden_prince_dormand_step make
    #  the comparison with the oracle)
    x, ref = _refx(N, stored=False), _ref(stored=False)
    rng = np.random.default_rng(19 + N)
    for k in range(3):
        A = rng.uniform(-1, 1, size=(N, N)); P = A @ A.T / N * 1e-3 + 1e-6 * np.eye(N)
        X = orc.MotionState(orc.so3_exp(rng.normal(size=3) * 0.4), rng.normal(size=3), rng.normal(size=3),
                            rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05, orc.so3_exp([0.02, -0.01, 0.0]))
        gy, ac = rng.normal(size=3) * (1 + 3 * k), np.array([0.2, -0.1, 9.7]) + rng.normal(size=3)
        sg, sa = rng.normal(size=3) * 5, rng.normal(size=3)
        Qi = np.diag(rng.uniform(1e-6, 1e-3, 12)); gv = np.array([0.0, 0.0, -9.8]); dt = 0.001 * (1 + k)
        for method, tab, fn in (("PD", orc.PD_TABLEAU, ref.pd_step), ("RK4", orc.RK4_TABLEAU, ref.rk4_step)):
            Rx, Tx, Vx, Px = x.integrator_step(method, X, P, gy, ac, sg, sa, dt, Qi, gv)
            R1, T1, V1, P1 = fn(X, P, gy, ac, sg, sa, dt, Qi, gv)
            assert np.abs(Rx - R1).max() < 1e-15 and np.abs(Tx - T1).max() < 1e-15 and np.abs(Vx - V1).max() < 1e-15
            assert rel(Px, P1) < 1e-13
            Xn, Pn = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, tab)
            assert np.abs(Xn.Rsb - Rx).max() < 1e-13 and np.abs(Xn.Tsb - Tx).max() < 1e-14 and np.abs(Xn.Vsb - Vx).max() < 1e-13
            assert rel(Pn, Px) < 1e-13


# ---- golden_v3.npz: outputs of the extracted reference build (tests/golden/make_golden_v3.py); runs without oracle/_ref ----
G3 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v3.npz"))


def _g3_mod():
    """the generator's input builders (seeded scenes), so test and fixture share one definition of the inputs"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_v3", os.path.join(os.path.dirname(__file__), "golden", "make_golden_v3.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_golden_v3_mh_gating(seed):
    m = _g3_mod()
    Js, inns, P, status = m.gating_scene(seed)
    assert np.array_equal(m.digest(Js, inns, P), G3[f"gate_{seed}_in_sha"]), "input generator drifted"
    d = orc.mh_distances(Js, P, inns, 2.25)
    mask, nrej, _ = orc.mh_gate(d, 5.991, 1.1, 5)
    assert np.nonzero(mask)[0].tolist() == G3[f"gate_{seed}_inliers"].tolist()
    assert [nrej, int((~mask).sum())] == G3[f"gate_{seed}_nrej"].tolist()
    want = np.where(mask, 3, 4); want[0] = 7 if mask[0] else 4
    assert want.tolist() == G3[f"gate_{seed}_status"].tolist()


def test_golden_v3_filter_update():
    m = _g3_mod()
    sc, lay, Js, inns, P, X = m.filter_update_scene()
    assert np.array_equal(m.digest(Js, inns, P, X.Rsb, sc["x"][0]), G3["fu_in_sha"]), "input generator drifted"
    H, inn, dR = orc.stack_measurements(Js, inns, sc["ref"][0], sc["sind"][0], lay, 2.25)
    Hg = np.zeros_like(H); Hg[G3["fu_H_nz_rows"], G3["fu_H_nz_cols"]] = G3["fu_H_nz_vals"]
    assert np.array_equal(H, Hg)
    e, Pn, _ = orc.update_joseph(H, P, inn, dR)
    assert rel(e, G3["fu_err"]) < 1e-9 and rel(Pn, G3["fu_P"]) < 1e-11
    st = dict(Rsb=X.Rsb.copy(), Tsb=X.Tsb.copy(), Vsb=X.Vsb.copy(), bg=X.bg.copy(), ba=X.ba.copy(), Rbc=sc["Rbc"][0].copy(),
              Tbc=sc["Tbc"][0].copy(), Rsg=X.Rsg.copy(), gR=sc["gR"][0].copy(), gT=sc["gT"][0].copy(), x=sc["x"][0].copy(), sind=sc["sind"][0])
    orc.absorb_error(st, G3["fu_err"], lay, [], range(m.NF))
    got = np.concatenate([st["Rsb"].reshape(-1), st["Tsb"], st["Vsb"], st["bg"], st["ba"], st["Rsg"].reshape(-1)])
    assert np.abs(got - G3["fu_state"]).max() < 1e-12 and np.abs(st["x"] - G3["fu_x"]).max() < 1e-12


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("method", ["RK4", "PD"])
def test_golden_v3_integrator_steps(k, method):
    m = _g3_mod()
    X, P, gy, ac, sg, sa, dt, Qi, gv = m.step_inputs(k)
    assert np.array_equal(m.digest(P, X.Rsb, X.Tsb, gy, ac, sg, sa, Qi), G3[f"step_{k}_in_sha"]), "input generator drifted"
    Xn, Pn = orc.integrator_step(X, P, gy, ac, sg, sa, dt, Qi, gv, orc.RK4_TABLEAU if method == "RK4" else orc.PD_TABLEAU)
    got = np.concatenate([Xn.Rsb.reshape(-1), Xn.Tsb, Xn.Vsb])
    assert np.abs(got - G3[f"step_{k}_{method}_state"]).max() < 1e-13
    assert rel(Pn[:23, :], G3[f"step_{k}_{method}_Prows"]) < 1e-13 and np.array_equal(Pn[23:, 23:], P[23:, 23:])


# ---- Feature::ComputeJacobian as extracted: default build and the three online-calibration defines ---------------------------
CAM_DIM = {"pinhole": 4, "atan": 5, "radtan": 9, "equi": 8}


def _calib_case(cam, seed, i):
    """one in-state feature of a 15-group / 30-feature scene + the quantities the calibration blocks need"""
    sc = synth.g_level(15, 30, 30, 1, seed=seed, cam=cam)
    rng = np.random.default_rng(1000 * seed + i)
    r = int(sc["ref"][0][i])
    cal = dict(gyro=rng.normal(size=3) * 0.5, Cg=np.eye(3) + 0.01 * rng.normal(size=(3, 3)), bg=rng.normal(size=3) * 0.01,
               Vsb=rng.normal(size=3), td=0.013)
    xp = np.array([300.0, 200.0]) + rng.normal(size=2) * 20
    args = (sc["x"][0][i], xp, sc["gR"][0][r], sc["gT"][0][r], sc["Rsb"][0], sc["Tsb"][0], sc["Rbc"][0], sc["Tbc"][0])
    return args, r, int(sc["sind"][0][i]), cal


@pytest.mark.parametrize("name", list(CAMS))
def test_extracted_compute_jacobian_default_build(name):
    """Feature::ComputeJacobian + FillJacobianBlock, the TEXT of src/feature.cpp:542-684 compiled in the default build, vs
    the oracle: J, inn and the stacked rows (incl. the :675-676 overwrite) - this pins a4 to the reference itself."""
    x = _refx(203)
    lay = orc.Layout(15, 30)
    worst = 0.0
    for i in range(0, 30, 3):
        args, r, sind, cal = _calib_case(CAMS[name], 5, i)
        J, inn, _ = orc.compute_jacobian(*args, CAMS[name], lay, r, sind)
        Jx, innx, Hx = x.compute_jacobian(*args, CAMS[name], r, sind, gyro=cal["gyro"], Cg=cal["Cg"], bg=cal["bg"], Vsb=cal["Vsb"], td=cal["td"])
        H = np.zeros((2, lay.N)); orc.fill_jacobian_block(H, 0, J, lay, r, sind)
        worst = max(worst, np.abs(J - Jx).max() / np.abs(Jx).max(), np.abs(inn - innx).max(), np.abs(H - Hx).max() / np.abs(Hx).max())
    assert worst < 1e-12


@pytest.mark.parametrize("name", list(CAMS))
def test_extracted_compute_jacobian_online_calibration_build(name):
    """The same text compiled with -DUSE_ONLINE_TEMPORAL_CALIB -DUSE_ONLINE_IMU_CALIB -DUSE_ONLINE_CAMERA_CALIB
    (src/CMakeLists.txt:13-15): kMotionSize 39, N = 228; the extracted enum Index gives the slots, the oracle's calib_layout
    derives the same ones; the td / Cg / bg / intrinsics blocks of J and of the stacked rows agree to 1e-12."""
    x = _refx("calib")
    lay = orc.calib_layout(15, 30, True, True, CAM_DIM[name])
    td, Cg, cam_begin, max_cam, motion = x.calib_slots()
    assert (lay.N, lay.group_begin, lay.feature_begin, lay.td, lay.Cg, lay.cam_begin) == (x.N, x.group_begin, x.feature_begin, td, Cg, cam_begin)
    assert (max_cam, motion) == (9, 39)
    worst = 0.0
    for i in range(0, 30, 3):
        args, r, sind, cal = _calib_case(CAMS[name], 7, i)
        J, inn, _, Jc = orc.compute_jacobian(*args, CAMS[name], lay, r, sind, calib=cal)
        Jx, innx, Hx = x.compute_jacobian(*args, CAMS[name], r, sind, gyro=cal["gyro"], Cg=cal["Cg"], bg=cal["bg"], Vsb=cal["Vsb"], td=cal["td"])
        H = np.zeros((2, lay.N)); orc.fill_jacobian_block(H, 0, J, lay, r, sind)
        worst = max(worst, np.abs(J - Jx).max() / np.abs(Jx).max(), np.abs(inn - innx).max(), np.abs(H - Hx).max() / np.abs(Hx).max())
        assert np.abs(Jx[:, td]).max() > 0 and np.abs(Jx[:, Cg:Cg + 9]).max() > 0 and np.abs(Jx[:, 9:12]).max() > 0
        assert (np.abs(Jx[:, cam_begin:cam_begin + 9]).sum(0) > 0).sum() == CAM_DIM[name]
        assert np.array_equal(Jc[:, 0], J[:, td]) and np.array_equal(Jc[:, 13:13 + CAM_DIM[name]], J[:, cam_begin:cam_begin + CAM_DIM[name]])
    assert worst < 1e-12


# ---- golden_v4.npz: ComputeJacobian / FillJacobianBlock of the extracted builds (default + online calibration) ----------------
G4 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v4.npz"))


@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("build", ["default", "calib"])
def test_golden_v4_compute_jacobian(build, name):
    """the oracle against stored outputs of the reference's own text (runs without oracle/_ref)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_v4", os.path.join(os.path.dirname(__file__), "golden", "make_golden_v4.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    lay = orc.calib_layout(15, 30, True, True, CAM_DIM[name]) if build == "calib" else orc.Layout(15, 30)
    L = G4[f"{build}_layout"]
    assert [lay.N, lay.group_begin, lay.feature_begin] == L[:3].tolist()
    if build == "calib":
        assert [lay.td, lay.Cg, lay.cam_begin] == L[3:6].tolist() and L[6:8].tolist() == [9, 39]
    for i in (0, 11, 29):
        args, r, sind, cal = m.case(CAMS[name], 7, i)
        res = orc.compute_jacobian(*args, CAMS[name], lay, r, sind, calib=cal if build == "calib" else None)
        J, inn = res[0], res[1]
        H = np.zeros((2, lay.N)); orc.fill_jacobian_block(H, 0, J, lay, r, sind)
        k = f"{build}_{name}_{i}"
        for M_, cols, vals in ((J, G4[k + "_Jcols"], G4[k + "_J"]), (H, G4[k + "_Hcols"], G4[k + "_H"])):
            assert np.nonzero(np.abs(M_).sum(0))[0].tolist() == cols.tolist()
            assert np.abs(M_[:, cols] - vals).max() / np.abs(vals).max() < 1e-12
        assert np.abs(inn - G4[k + "_inn"]).max() < 1e-10


# ---- motion side of the online-calibration builds: golden_v5.npz + the extracted build live ------------------------------------
G5 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v5.npz"))


def _v5():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_v5", os.path.join(os.path.dirname(__file__), "golden", "make_golden_v5.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _oracle_calib_step(c, method, lay):
    tab = orc.RK4_TABLEAU if method == "RK4" else orc.PD_TABLEAU
    return orc.integrator_step(c["X"].copy(), c["P"], c["gy"], c["ac"], c["sg"], c["sa"], 0.004, c["Qimu"], c["g"], tab, c["Cg"], c["Ca"], lay)


def _oracle_calib_absorb(c, m, lay):
    X = c["X"]
    st = dict(Rsb=X.Rsb.copy(), Tsb=X.Tsb.copy(), Vsb=X.Vsb.copy(), bg=X.bg.copy(), ba=X.ba.copy(), Rbc=c["Rbc"].copy(), Tbc=c["Tbc"].copy(),
              Rsg=X.Rsg.copy(), td=c["td"], Cg=c["Cg"].copy(), Ca=c["Ca"].copy(), cam=dict(m.CAM, d=list(m.CAM["d"])),
              gR=np.zeros((0, 3, 3)), gT=np.zeros((0, 3)), x=np.zeros((0, 3)), sind=[])
    orc.absorb_error(st, c["err"], lay, [], [])
    return st


@pytest.mark.parametrize("seed", [1, 2])
def test_golden_v5_calibration_motion_side(seed):
    """the oracle's 39-dimensional integrator step and calibration absorb against stored outputs of the reference's own text
    compiled with the three online-calibration defines (runs without oracle/_ref)"""
    m = _v5()
    lay = orc.calib_layout(15, 30, True, True, 9)
    assert (lay.N, lay.motion_size, lay.Ca) == (m.N, m.NM, 33)
    c = m.case(seed)
    for method in ("RK4", "PrinceDormand"):
        Xo, Po = _oracle_calib_step(c, method, lay)
        k = f"s{seed}_{method}"
        assert np.abs(Xo.Rsb - G5[k + "_Rsb"]).max() < 1e-14 and np.abs(Xo.Tsb - G5[k + "_Tsb"]).max() < 1e-14
        assert np.abs(Xo.Vsb - G5[k + "_Vsb"]).max() < 1e-14
        assert np.linalg.norm(Po[:m.NM] - G5[k + "_Ptop"]) / np.linalg.norm(G5[k + "_Ptop"]) < 1e-14
        assert np.abs(c["w"] @ Po[m.NM:, :m.NM] - G5[k + "_Pleft_w"]).max() / np.abs(G5[k + "_Pleft_w"]).max() < 1e-13
        # the Cg / Ca columns matter: the same step without them (default-build Jacobian in the 39 slots) is measurably different
        lay0 = orc.calib_layout(15, 30, True, False, 9); lay0.motion_size = lay.motion_size
        _, P0 = _oracle_calib_step(c, method, lay0)
        assert np.linalg.norm(P0[:m.NM] - G5[k + "_Ptop"]) / np.linalg.norm(G5[k + "_Ptop"]) > 1e-9
    st = _oracle_calib_absorb(c, m, lay)
    k = f"s{seed}_absorb"
    for name in ("Rsb", "Tsb", "Vsb", "bg", "ba", "Rsg", "Rbc", "Tbc", "Cg", "Ca"):
        assert np.abs(st[name] - G5[f"{k}_{name}"]).max() < 1e-15, name
    assert abs(st["td"] - G5[k + "_td"][0]) < 1e-17
    intr = np.array([st["cam"]["fx"], st["cam"]["fy"], st["cam"]["cx"], st["cam"]["cy"]] + list(st["cam"]["d"]))
    assert np.abs(intr - G5[k + "_intr"]).max() < 1e-13


def test_extracted_calibration_build_motion_side_live():
    """the same against the library itself when it is here (a fresh seed)"""
    x = _refx("calib")
    m = _v5()
    lay = orc.calib_layout(15, 30, True, True, 9)
    assert x.index_Ca() == lay.Ca and x.calib_slots()[4] == lay.motion_size
    c = m.case(9)
    for method in ("RK4", "PrinceDormand"):
        R, T, V, Pn = x.integrator_step(method, c["X"], c["P"], c["gy"], c["ac"], c["sg"], c["sa"], 0.004, c["Qimu"], c["g"], c["Cg"], c["Ca"])
        Xo, Po = _oracle_calib_step(c, method, lay)
        assert np.abs(R - Xo.Rsb).max() < 1e-14 and np.abs(T - Xo.Tsb).max() < 1e-14 and np.abs(V - Xo.Vsb).max() < 1e-14
        assert np.linalg.norm(Pn - Po) / np.linalg.norm(Pn) < 1e-14
    o = x.absorb_motion_calib(c["X"], c["Rbc"], c["Tbc"], c["td"], c["Cg"], c["Ca"], m.CAM, c["err"])
    st = _oracle_calib_absorb(c, m, lay)
    for name in ("Rsb", "Tsb", "Vsb", "bg", "ba", "Rsg", "Rbc", "Tbc", "Cg", "Ca"):
        assert np.abs(st[name] - o[name]).max() < 1e-15, name
    assert st["td"] == o["td"]


# ---- round 5: the rest of the path on the reference's own text (golden_v6.npz; tests/golden/make_golden_v6.py) --------------------
G6 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v6.npz"))


def _v6():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_v6", os.path.join(os.path.dirname(__file__), "golden", "make_golden_v6.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _lay_of(build, name):
    if build == "calib":
        return orc.calib_layout(15, 30, True, True, CAM_DIM[name])
    return orc.Layout(8, 60)


@pytest.mark.parametrize("name", list(CAMS))
@pytest.mark.parametrize("build", ["n251", "calib", "invdepth"])
def test_golden_v6_loop_closure_rows(build, name):
    """oracle lc_jacobian_rows against stored rows of the extracted Feature::ComputeLCJacobian (src/oos.cpp:92-145) in three
    builds: default, online calibration (the intrinsics block of :140-143), USE_INVDEPTH (Xs through unproject_invz)"""
    m = _v6()
    sc, _, matches, _ = m.lc_case(build, CAMS[name], 3)
    lay = _lay_of(build, name)
    assert lay.N == int(G6[f"lc_{build}_{name}_N"][0])
    H, inn = orc.lc_jacobian_rows(matches, sc["Rbc"][0], sc["Tbc"][0], CAMS[name], lay, invdepth=(build == "invdepth"))
    cols = G6[f"lc_{build}_{name}_cols"]
    assert np.nonzero(np.abs(H).sum(0))[0].tolist() == cols.tolist()
    assert np.abs(H[:, cols] - G6[f"lc_{build}_{name}_H"]).max() / np.abs(H).max() < 1e-12
    assert np.abs(inn - G6[f"lc_{build}_{name}_inn"]).max() < 1e-10
    if build == "calib":       # the intrinsics block is there, and only the slots of this camera model
        cb = lay.cam_begin
        assert set(range(cb, cb + CAM_DIM[name])) >= {c for c in cols.tolist() if cb <= c < cb + 9} != set()


def test_extracted_loop_closure_rows_live():
    m = _v6()
    for build in ("n251", "calib", "invdepth"):
        lib = _refx({"n251": 251}.get(build, build))
        for name in CAMS:
            for seed in (4, 5):
                sc, _, matches, _ = m.lc_case(build, CAMS[name], seed, n=5)
                H, inn = lib.compute_lc_jacobian([q["x"] for q in matches], [q["Rsbr"] for q in matches], [q["Tsbr"] for q in matches],
                                                 [q["Rsb"] for q in matches], [q["Tsb"] for q in matches], [q["g_sind"] for q in matches],
                                                 [q["xp"] for q in matches], sc["Rbc"][0], sc["Tbc"][0], CAMS[name])
                Ho, io = orc.lc_jacobian_rows(matches, sc["Rbc"][0], sc["Tbc"][0], CAMS[name], _lay_of(build, name), invdepth=(build == "invdepth"))
                assert np.abs(H - Ho).max() / np.abs(H).max() < 1e-12 and np.abs(inn - io).max() < 1e-10


@pytest.mark.parametrize("name", list(CAMS))
def test_golden_v6_invdepth_jacobian_and_subfilter(name):
    """USE_INVDEPTH build (src/feature.cpp:98-105): ComputeJacobian + FillJacobianBlock, SubfilterUpdate, Feature::z"""
    m = _v6()
    cam = CAMS[name]; lay = orc.Layout(8, 60)
    sc = synth.g_level(8, 60, 60, 1, seed=9, cam=cam)
    for i in (0, 17, 59):
        r = int(sc["ref"][0, i]); x = m.to_invdepth(sc["x"][0, i])
        xp = np.array([cam["cx"], cam["cy"]]) + np.array([13.0 * (i % 5) - 20, 9.0 * (i % 7) - 25])
        J, inn, _ = orc.compute_jacobian(x, xp, sc["gR"][0, r], sc["gT"][0, r], sc["Rsb"][0], sc["Tsb"][0], sc["Rbc"][0], sc["Tbc"][0], cam, lay,
                                         r, int(sc["sind"][0, i]), invdepth=True)
        k = f"inv_jac_{name}_{i}"
        cols = G6[k + "_cols"]
        assert np.nonzero(np.abs(J).sum(0))[0].tolist() == cols.tolist()
        assert np.abs(J[:, cols] - G6[k + "_J"]).max() / np.abs(J).max() < 1e-12 and np.abs(inn - G6[k + "_inn"]).max() < 1e-10
        H = np.zeros((2, lay.N)); orc.fill_jacobian_block(H, 0, J, lay, r, int(sc["sind"][0, i]))
        assert np.abs(H[:, G6[k + "_Hcols"]] - G6[k + "_H"]).max() / np.abs(H).max() < 1e-12
        # the same point in the log-depth parametrisation: every block but d/dx is unchanged, d/dx differs by the chain rule
        Jl, _, _ = orc.compute_jacobian(sc["x"][0, i], xp, sc["gR"][0, r], sc["gT"][0, r], sc["Rsb"][0], sc["Tsb"][0], sc["Rbc"][0], sc["Tbc"][0],
                                        cam, lay, r, int(sc["sind"][0, i]))
        fo = lay.feature_begin + 3 * int(sc["sind"][0, i])
        assert np.abs(np.delete(J - Jl, np.s_[fo:fo + 3], axis=1)).max() < 1e-9 * np.abs(J).max()
        assert np.abs(J[:, fo:fo + 2] - Jl[:, fo:fo + 2]).max() < 1e-9 * np.abs(J).max()
        assert np.abs(J[:, fo + 2] * (-x[2]) - Jl[:, fo + 2]).max() < 1e-9 * np.abs(J).max()      # d(1/Z)/d(log Z) = -1/Z
    c = m.sub_case(cam, 4, invdepth=True)
    xs, Ps, st, ic, oc = orc.subfilter_update(c["x"], c["P"], c["xp"], c["Rsb"], c["Tsb"], c["Rbc"], c["Tbc"], c["Rsbr"], c["Tsbr"], cam,
                                              3.5, 5.991, 5, c["init_counter"], c["outlier_counter"], invdepth=True)
    g = G6[f"inv_sub_{name}"]
    assert rel(xs, g[:3]) < 1e-10 and rel(Ps.reshape(-1), g[3:12]) < 1e-9 and [st, ic] == [int(g[12]), int(g[13])] and abs(oc - g[14]) < 1e-9 * max(1, g[14])
    assert abs(orc.feature_z(c["x"], True) - 1.0 / c["x"][2]) == 0.0


@pytest.mark.parametrize("name", list(CAMS))
def test_golden_v6_oos_rows_and_subfilter_of_the_extracted_text(name):
    """Feature::ComputeOOSJacobian (+Internal, SlowGivens) and Feature::SubfilterUpdate as extracted. The reference hands
    SlowGivens the WHOLE 2 * kMaxGroup-row buffers (src/oos.cpp:28): its result = the rows this repo (and the oracle) compute
    from the 2k live rows + exactly-zero rows, one per unused buffer row."""
    m = _v6()
    cam = CAMS[name]; lay = orc.Layout(8, 60)
    sc, i, r, obs = m.oos_case(cam, 2)
    Xs = orc.feature_xs(sc["x"][0, i], sc["gR"][0, r], sc["gT"][0, r], sc["Rbc"][0], sc["Tbc"][0])
    assert rel(Xs, G6[f"oos_{name}_Xs"]) < 1e-14
    Hx, rp, _ = orc.oos_jacobian(Xs, obs, sc["gR"][0], sc["gT"][0], sc["Rbc"][0], sc["Tbc"][0], cam, lay)
    k = len(obs)
    assert Hx.shape[0] == 2 * k - 3
    assert int(G6[f"oos_{name}_rows"][0]) == 2 * 8 - 3                     # whole buffer: 16 rows, rank 3
    nz, cols = G6[f"oos_{name}_nzrows"], G6[f"oos_{name}_cols"]
    assert len(nz) == 2 * k - 3                                            # ... of which 2k - 3 are not exactly zero
    assert np.nonzero(np.abs(Hx).sum(0))[0].tolist() == cols.tolist()
    assert np.abs(Hx[:, cols] - G6[f"oos_{name}_Hx"]).max() / np.abs(Hx).max() < 1e-10
    inn = G6[f"oos_{name}_inn"]
    assert np.abs(rp - inn[nz]).max() < 1e-9 * max(1.0, np.abs(rp).max()) and np.abs(np.delete(inn, nz)).max() == 0.0
    c = m.sub_case(cam, 4)
    xs, Ps, st, ic, oc = orc.subfilter_update(c["x"], c["P"], c["xp"], c["Rsb"], c["Tsb"], c["Rbc"], c["Tbc"], c["Rsbr"], c["Tsbr"], cam,
                                              3.5, 5.991, 5, c["init_counter"], c["outlier_counter"])
    g = G6[f"sub_{name}"]
    assert rel(xs, g[:3]) < 1e-10 and rel(Ps.reshape(-1), g[3:12]) < 1e-9 and [st, ic] == [int(g[12]), int(g[13])] and abs(oc - g[14]) < 1e-9 * max(1, g[14])


def test_extracted_oos_and_subfilter_equal_the_retyped_driver_live():
    """extracted text == retyped driver (oracle/ref/xivo_ref.cpp) on the same inputs: the retyping of rounds 1-4 was faithful"""
    m = _v6()
    ref = _ref()
    x251 = _refx(251)
    lay = orc.Layout(8, 60)
    for name, cam in CAMS.items():
        for seed in (2, 3):
            sc, i, r, obs = m.oos_case(cam, seed, k=5 + seed % 2)
            rows, Hx, inn, Xs = x251.compute_oos_jacobian(sc["x"][0, i], sc["gR"][0, r], sc["gT"][0, r], obs, sc["gR"][0], sc["gT"][0],
                                                          sc["Rbc"][0], sc["Tbc"][0], cam)
            k = len(obs)
            Hf = np.zeros((2 * k, 3)); Hxr = np.zeros((2 * k, lay.N)); rr = np.zeros(2 * k)
            for c_, (g, xp) in enumerate(obs):
                hf, hx, ii = ref.oos_internal(Xs, sc["gR"][0, g], sc["gT"][0, g], sc["Rbc"][0], sc["Tbc"][0], xp, cam, lay, g)
                Hf[2 * c_:2 * c_ + 2] = hf; Hxr[2 * c_:2 * c_ + 2] = hx; rr[2 * c_:2 * c_ + 2] = ii
            Hxp, rp = ref.slow_givens(Hf, Hxr, rr)[:2]
            nz = np.nonzero(np.abs(Hx).sum(1))[0]
            assert len(nz) == 2 * k - 3 and np.abs(Hx[nz] - Hxp).max() <= 1e-13 * np.abs(Hxp).max() and np.abs(inn[nz] - rp).max() <= 1e-12 * max(1, np.abs(rp).max())
            # below the minimum number of in-state observations: no rows (src/oos.cpp:15, :32-34)
            assert x251.compute_oos_jacobian(sc["x"][0, i], sc["gR"][0, r], sc["gT"][0, r], obs, sc["gR"][0], sc["gT"][0], sc["Rbc"][0],
                                             sc["Tbc"][0], cam, min_obs=k + 1)[0] == 0
        c = m.sub_case(cam, 4)
        a = x251.subfilter_update(c["x"], c["P"], c["xp"], c["Rsb"], c["Tsb"], c["Rbc"], c["Tbc"], c["Rsbr"], c["Tsbr"], cam, 3.5, 5.991, 5,
                                  c["init_counter"], c["outlier_counter"])
        b = ref.subfilter_update(c["x"], c["P"], c["xp"], c["Rsb"], c["Tsb"], c["Rbc"], c["Tbc"], c["Rsbr"], c["Tsbr"], cam, 3.5, 5.991, 5,
                                 c["init_counter"], c["outlier_counter"])
        # (the two drivers build their SE3 objects from the same matrices along different routes: equal to rounding, not bitwise)
        assert rel(a[0], b[0]) < 1e-13 and rel(a[1], b[1]) < 1e-12 and list(a[2:4]) == list(b[2:4]) and abs(a[4] - b[4]) <= 1e-12 * max(1.0, b[4])


@pytest.mark.parametrize("dt_ns", [2500000, 7000000])
@pytest.mark.parametrize("method", ["RK4", "PrinceDormand"])
@pytest.mark.parametrize("seed", [1, 2])
def test_golden_v6_propagate_with_the_integrators_outer_loops(seed, method, dt_ns):
    """oracle.propagate against stored outputs of the extracted Estimator::Propagate -> Estimator::RK4 / PrinceDormand
    (sub-stepping with the half-step trick, src/rk4.cpp:13-32) -> RK4Step / PrinceDormandStep, P_mm += Qmodel (:590)"""
    m = _v6()
    c = m.prop_case(seed)
    X = orc.MotionState(c["X"].Rsb.copy(), c["X"].Tsb.copy(), c["X"].Vsb.copy(), c["X"].bg.copy(), c["X"].ba.copy(), c["X"].Rsg.copy())
    X2, P2 = orc.propagate(X, c["P"], c["gy"], c["ac"], c["sg"], c["sa"], dt_ns * 1e-9, c["Qimu"], c["Qmodel"], c["g"], method=method,
                           stepsize=0.002)[:2]
    k = f"prop_s{seed}_{method}_{dt_ns}"
    assert rel(X2.Rsb, G6[k + "_Rsb"]) < 1e-12 and rel(X2.Tsb, G6[k + "_Tsb"]) < 1e-12 and rel(X2.Vsb, G6[k + "_Vsb"]) < 1e-12
    assert rel(P2[:23, :23], G6[k + "_Pmm"]) < 1e-11 and rel(P2[:23, 23:] @ c["w"], G6[k + "_Pms_w"]) < 1e-11
    assert rel(c["w"] @ P2[23:, :23], G6[k + "_Pleft_w"]) < 1e-11
    last = G6[k + "_last"]        # a visual message: last_gyro_ / last_accel_ advanced along the slopes (:569-575)
    assert rel(c["gy"] + c["sg"] * (dt_ns * 1e-9), last[:3]) < 1e-14 and rel(c["ac"] + c["sa"] * (dt_ns * 1e-9), last[3:]) < 1e-14


@pytest.mark.parametrize("tag,cam", [("pin", "pinhole"), ("rad", "radtan"), ("tmp", "equi")])
def test_golden_v6_one_point_ransac_whole_function(tag, cam):
    """oracle.one_point_ransac against the extracted Estimator::OnePointRANSAC (hypothesis loop on rng_, BackupState,
    FindNewRefGroup, P zeroing, partial update + AbsorbError, Jacobians at the updated state, chi-square rescue, RestoreState,
    Jacobians at the original state): the kept set, the rejected set (status 4 = REJECTED_BY_FILTER), the count"""
    m = _v6()
    c = m.ransac_case(tag)
    sc = c["sc"]; lay = orc.Layout(c["ng"], c["nf"])
    xp = G6[f"ransac_{tag}_xp"]
    assert np.abs(xp - m.ransac_pixels(c, lambda cam_, xcn: orc.camera_project(cam_, xcn)[0])).max() < 1e-9
    st = dict(Rsb=sc["Rsb"][0], Tsb=sc["Tsb"][0], Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), Rbc=sc["Rbc"][0], Tbc=sc["Tbc"][0],
              Rsg=np.eye(3), gR=sc["gR"][0].copy(), gT=sc["gT"][0].copy(), x=sc["x"][0].copy(), sind=sc["sind"][0], ref=sc["ref"][0])
    out = orc.one_point_ransac(st, c["P"], xp, CAMS[cam], lay, c["R"], c["thresh"], c["chi2"], c["gauge"], range(c["ng"]))
    keep = G6[f"ransac_{tag}_keep"]
    assert out["inliers"] == np.nonzero(keep)[0].tolist()
    assert sorted(out["rejected"]) == np.nonzero(G6[f"ransac_{tag}_status"] == 4)[0].tolist() and len(out["rejected"]) == int(G6[f"ransac_{tag}_nrej"][0])
    assert 0 < out["low"].sum() < c["nf"] and len(out["rejected"]) >= 1 and len(out["inliers"]) > out["low"].sum()
    if tag == "tmp":
        assert c["gauge"] not in set(int(sc["ref"][0, i]) for i in range(c["nf"]) if out["low"][i])
    r = int(sc["ref"][0, 3])
    J3 = orc.compute_jacobian(sc["x"][0, 3], xp[3], sc["gR"][0, r], sc["gT"][0, r], sc["Rsb"][0], sc["Tsb"][0], sc["Rbc"][0], sc["Tbc"][0],
                              CAMS[cam], lay, r, int(sc["sind"][0, 3]))[0]
    assert np.abs(J3[:, G6[f"ransac_{tag}_J3cols"]] - G6[f"ransac_{tag}_J3"]).max() / np.abs(J3).max() < 1e-12


def test_extracted_one_point_ransac_calibration_build_live():
    """The whole OnePointRANSAC of the extracted build compiled with the three online-calibration defines (N = 228): the partial
    update runs on the whole rows J() with their td / Cg / bg / intrinsics blocks, AbsorbError moves td / Cg / Ca / the
    intrinsics, Backup / RestoreState carry them - the oracle's calibration branch of one_point_ransac against it."""
    x = _refx("calib")
    m = _v6()
    for tag, camname in (("rad", "radtan"), ("tmp", "equi"), ("pin", "pinhole")):
        c = m.ransac_case(tag)
        sc = c["sc"]; cam = CAMS[camname]
        lay = orc.calib_layout(c["ng"], c["nf"], True, True, CAM_DIM[camname])
        assert lay.N == x.N
        rng = np.random.default_rng(11)
        A = rng.uniform(-1, 1, size=(lay.N, lay.N)); P = (A @ A.T / lay.N + 1e-3 * np.eye(lay.N)) * 1e-4
        xp = m.ransac_pixels(c, lambda cam_, xcn: orc.camera_project(cam_, xcn)[0])
        X = orc.MotionState(sc["Rsb"][0], sc["Tsb"][0], np.zeros(3), np.zeros(3), np.zeros(3), np.eye(3))
        o = x.one_point_ransac(X, sc["Rbc"][0], sc["Tbc"][0], P, sc["x"][0], xp, sc["ref"][0], sc["sind"][0], sc["gR"][0], sc["gT"][0],
                               cam, c["R"], c["thresh"], c["chi2"], gauge_sind=c["gauge"])
        st = dict(Rsb=sc["Rsb"][0], Tsb=sc["Tsb"][0], Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), Rbc=sc["Rbc"][0], Tbc=sc["Tbc"][0],
                  Rsg=np.eye(3), gR=sc["gR"][0].copy(), gT=sc["gT"][0].copy(), x=sc["x"][0].copy(), sind=sc["sind"][0], ref=sc["ref"][0],
                  td=0.0, Cg=np.eye(3), Ca=np.eye(3), cam=dict(cam, d=list(cam.get("d", []))))
        out = orc.one_point_ransac(st, P, xp, cam, lay, c["R"], c["thresh"], c["chi2"], c["gauge"], range(c["ng"]), calib_gyro=np.zeros(3))
        assert out["inliers"] == np.nonzero(o["keep"])[0].tolist(), tag
        assert sorted(out["rejected"]) == np.nonzero(o["status"] == 4)[0].tolist() and len(out["rejected"]) == o["n_rejected"]
        assert np.array_equal(o["P"], P) and 0 < out["low"].sum() < c["nf"]
        # the partial update really moved the calibration columns
        assert np.abs(out["err"][lay.td]) > 0 and np.abs(out["err"][lay.cam_begin:lay.cam_begin + 4]).max() > 0


# ---- round 6 pin: golden_v7.npz (tests/golden/make_golden_v7.py) - the step-size-controlled branch of Estimator::PrinceDormand ----
G7 = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v7.npz"))


def _v7():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_v7", os.path.join(os.path.dirname(__file__), "golden", "make_golden_v7.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def pd_control_chain_oracle(seed):
    """The chain of make_golden_v7 through the oracle: (case, [(X, P) after every call], the step lengths taken)"""
    m7 = _v7(); c = _v6().prop_case(seed)
    ctl = orc.PDControl(stepsize=0.002, **m7.PD_CTL)
    X = orc.MotionState(c["X"].Rsb.copy(), c["X"].Tsb.copy(), c["X"].Vsb.copy(), c["X"].bg.copy(), c["X"].ba.copy(), c["X"].Rsg.copy())
    P = c["P"]
    outs = []
    for dt_ns in m7.CHAIN_NS:
        X, P = orc.propagate(X, P, c["gy"], c["ac"], c["sg"], c["sa"], dt_ns * 1e-9, c["Qimu"], c["Qmodel"], c["g"], method="PrinceDormand",
                             stepsize=0.002, pd_control=ctl)[:2]
        outs.append((X, P))
    return c, outs, ctl.steps


@pytest.mark.parametrize("seed", [1, 2])
def test_golden_v7_prince_dormand_step_size_control_as_coded(seed):
    """oracle.integrate_pd_controlled against stored outputs of the extracted Estimator::PrinceDormand with control_stepsize = true
    (src/princedormand.cpp:26-60): five Propagate calls in a row - the step the branch carries in a function-local static grows
    4 x per step (PrinceDormandStep returns 0, :216-220) and is clipped / halved at the end of a sample (:53-58)."""
    c, outs, steps = pd_control_chain_oracle(seed)
    # (what the reference prints, :49)
    assert np.allclose(steps, [0.002, 0.0005, 0.002, 0.005, 0.0025, 0.01, 0.002, 0.001], rtol=1e-12)
    for i, (X, P) in enumerate(outs):
        k = f"pdc_s{seed}_{i}"
        assert rel(X.Rsb, G7[k + "_Rsb"]) < 1e-12 and rel(X.Tsb, G7[k + "_Tsb"]) < 1e-12 and rel(X.Vsb, G7[k + "_Vsb"]) < 1e-12
        assert rel(P[:23, :23], G7[k + "_Pmm"]) < 1e-11 and rel(P[:23, 23:] @ c["w"], G7[k + "_Pms_w"]) < 1e-11


def test_live_prince_dormand_step_size_control_vs_ref():
    """The same chain on a private copy of the extracted library (fresh function-local statics), live"""
    m7 = _v7()
    rx = reference("refx_private_203", lambda: m7.private_refx(203))
    if not hasattr(rx.lib, "refx_pd_control"):
        pytest.skip("oracle/_ref predates refx_pd_control")
    c, ref_outs = m7.run_chain(rx, 2)
    _, outs, _ = pd_control_chain_oracle(2)
    for (X, P), o in zip(outs, ref_outs):
        assert rel(X.Rsb, o["Rsb"]) < 1e-12 and rel(X.Vsb, o["Vsb"]) < 1e-12 and rel(P[:23, :], o["P"][:23, :]) < 1e-11
