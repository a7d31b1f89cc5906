"""The measurement update (Estimator::UpdateJosephForm, src/estimator.cpp:1257-1288) on every route of plan_update
(xivo_amd/csrc/capi_update.hip) against the extended-precision reference of tests/precise_ref.py, within fp64 bounds
C u (kappa_2(S) + N) - helpers.TOL_P / TOL_DX leave eight decades of room above the kernels and see neither a float leak nor an
error confined to the states of small variance:
  - a filter and its twin in power-of-two units (P -> D P D, H -> H D^-1, variances from 2^-40 to 2^4) in one launch: the
    twin's P+, dx, gate are the filter's to the bit (every correct sum combines terms of one scale), and within the bound in
    units of the prior correlation;
  - an innovation covariance with kappa_2(S) from ~5e3 to ~5e8 (tests/joseph_forms_accuracy.py's cases) under every flag set
    of test_update_gpu.py::test_every_route_of_the_plan;
  - XIVO_HIP_FLAG_FP32_WHITENED: what it may change (beyond one workgroup) and what not (within one);
  - rows that are not plain compressed pairs: the leading calibration block, OOS rows behind the in-state rows, QR-compressed
    OOS rows - read back as staged (xivo_hip_get_H) and updated;
  - XIVO_HIP_CHUNK: the batch walked in ranges is the unchunked batch, bit for bit, the L D L^T fallback included."""
import numpy as np
import pytest

import precise_ref as pr
import xivo_oracle as orc
from helpers import rel_fro, TOL_P
from scene_util import spd
from xivo_amd import synth
from xivo_amd.lib import (Context, oos_dtype, FLAG_PROFILE, FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_DENSE_H,
                          FLAG_SYMMETRIC_FORM, FLAG_STANDALONE_TAIL, FLAG_FP32_WHITENED)
import test_update_edges_gpu as edges
from test_update_edges_gpu import GATE, R

pytestmark = pytest.mark.gpu
TP, MT, SYM, TAIL, DH, F32 = (FLAG_THROUGHPUT_ROUTE, FLAG_MULTI_KERNEL, FLAG_SYMMETRIC_FORM, FLAG_STANDALONE_TAIL,
                              FLAG_DENSE_H, FLAG_FP32_WHITENED)
TOL_P_FP32 = 5e-5     # the stated tolerance of XIVO_HIP_FLAG_FP32_WHITENED (test_update_gpu.py)


def _case(name, N, M, src="gen", B=3):
    """an EDGE_CASES-shaped tuple for edge_inputs (only name, N, M, nc, pw, B and the source are read)"""
    return (name, N, M, (M + 15) // 16, (N + 15) // 16, 12, 6, B, 0, None, None, "j", src)


def _run(P, H, inn, dR, flags, gated, profile=False):
    B, M, N = H.shape
    F = M // 2
    out = {}
    with Context(N, M, B, flags=flags | (FLAG_PROFILE if profile else 0)) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn, dR)
        if gated:
            ctx.update_dense_gated(F, R, *GATE)
            out["mask"], out["dist"] = ctx.get_gate(F, B)
        else:
            ctx.update_joseph()
        out["P"], out["dx"] = ctx.download_P(), ctx.get_err()
        out["status"], out["ldlt"] = ctx.get_status(check=False), ctx.get_ldlt_used()
        out["route"] = ctx.last_route()
        if profile:
            out["kernel"] = ctx.profile_get()["trsm_gain"]["kernel"]
    return out


# ---------------------------------------------------------------- b. scaled states, bit for bit
# label, shape (an EDGE_CASES name or a tuple), flags, route, entry points
TWINS = [
    ("fused_six_slot", "m64_150", 0, "fused", "jg"),
    ("fused_nine_slot", "pw9_m60", 0, "fused", "jg"),
    ("sparse_in_solve", "formsT_nb11", TP, "sparse_in_solve", "j"),
    ("whitened_latency", "m114_150", 0, "sparse_whitened", "jg"),
    ("whitened_stream8", "stream8_nb8", TP, "sparse_whitened", "j"),
    ("whitened_nb24", "factor_nb24", 0, "sparse_whitened", "j"),
    ("sparse_symmetric", "m64_150", SYM, "sparse_symmetric", "jg"),
    ("sparse_tail", "m64_150", TAIL, "sparse_tail", "jg"),
    ("dense_ascoded", "m64_150", DH, "dense_ascoded", "jg"),
    ("dense_whitened", _case("dense_64_40", 64, 40, "dense"), 0, "dense_whitened", "jg"),
    ("fp32_whitened", _case("f32_300_120", 300, 120), F32, "sparse_whitened", "j"),
]


def _twin_params():
    return [pytest.param(t[0], e, id="%s-%s" % (t[0], e)) for t in TWINS for e in t[4]]


@pytest.mark.parametrize("label,entry", _twin_params())
def test_power_of_two_units_bit_for_bit(built, label, entry):
    """Filters b and their twins in other units (P -> D P D, H -> H D^-1, same innovation and R; D = 2^e, e in [-20, 2], a
    whole 16-column block below 2^-15) in one launch. S of the twin is the filter's S to the bit, and no value leaves the
    normal range, so a correct kernel returns D P+ D, D dx, the same gate - an absolute constant or a sum mixing units would
    not. The twins' P+ within the bound in units of the prior correlation (the float operands of FP32_WHITENED: TOL_P_FP32)."""
    _, shape, flags, route, _ = next(t for t in TWINS if t[0] == label)
    case = edges.CASES[shape] if isinstance(shape, str) else shape
    P, H, inn, dR = edges.edge_inputs(case)
    B, N = P.shape[0], P.shape[1]
    gated = entry == "g"
    if gated:
        inn[:, 4:8] *= 1e4                                          # features 2 and 3 of every filter fail the gate
    D = pr.pow2_scales(N, seed=N + H.shape[1])
    Ps, Hs = pr.scale(D, P, H)
    o = _run(np.concatenate([P, Ps]), np.concatenate([H, Hs]), np.concatenate([inn, inn]), np.concatenate([dR, dR]), flags, gated)
    assert o["route"] == route, (o["route"], route)
    assert (o["status"] == 0).all() and not o["ldlt"].any()
    for b in range(B):
        assert np.array_equal(o["P"][B + b], o["P"][b] * np.outer(D, D)), (label, b, np.abs(o["P"][B + b] / np.outer(D, D) - o["P"][b]).max())
        assert np.array_equal(o["dx"][B + b], o["dx"][b] * D), (label, b)
        if gated:
            assert np.array_equal(o["mask"][B + b], o["mask"][b]) and np.array_equal(o["dist"][B + b], o["dist"][b])
            assert not o["mask"][b][2:4].any()
    keep = np.repeat(o["mask"][B], 2) if gated else None
    ref = pr.extended(Hs[0], Ps[0], inn[0], dR[0], keep)
    if flags & F32:
        assert rel_fro(o["P"][B], ref.P.astype(np.float64)) < TOL_P_FP32
        return
    rel, corr, dx = pr.check(ref, o["P"][B], o["dx"][B], what=label)
    print("accuracy %s twin %s-%s: rel %.3f corr %.3f dx %.3f x u (kappa + N)" % (route, label, entry, rel, corr, dx))


# ---------------------------------------------------------------- c. ill-conditioned S on every route
ROUTE_FLAGS = [0, TP, MT, MT | TP, SYM, TAIL, DH]     # the flag sets of test_every_route_of_the_plan


@pytest.mark.parametrize("flags", ROUTE_FLAGS)
def test_ill_conditioned_S_on_every_route(built, flags):
    """kappa_2(S) from ~5e3 to ~5e8 (tests/joseph_forms_accuracy.py: P with 2 .. 11 decades of eigenvalues, small R): P+ and dx
    within C u (kappa_2(S) + N) of the extended-precision reference on whatever route the flags select."""
    import joseph_forms_accuracy as jfa
    for ci, (P, H, inn, dR) in enumerate(jfa.cases()):
        o = _run(P, H, inn, dR, flags, False)
        assert (o["status"] == 0).all() and not o["ldlt"].any(), (ci, o["status"], o["ldlt"])
        for b in range(P.shape[0]):
            ref = pr.extended(H[b], P[b], inn[b], dR[b])
            assert ref.kappa > 1e3
            rel, _, dx = pr.check(ref, o["P"][b], o["dx"][b], what=(flags, ci, b), corr=False)
            print("accuracy %s ill-conditioned flags %d case %d kappa %.1e: rel %.3f dx %.3f x u (kappa + N)"
                  % (o["route"], flags, ci, ref.kappa, rel, dx))


# ---------------------------------------------------------------- d. what the fp32 flag may and may not do
def test_fp32_flag_beyond_one_workgroup_is_seen_by_the_fp64_bound(built):
    """N = 300, M = 120: the whitened operands leave the solve as float. P+ within the flag's stated 5e-5, and outside the
    fp64 bound - the check this file adds sees what TOL_P does not."""
    P, H, inn, dR = synth.s_level(300, 60, 3, seed=31)
    o = _run(P, H, inn, dR, F32, False)
    assert (o["status"] == 0).all()
    for b in range(3):
        ref = pr.extended(H[b], P[b], inn[b], dR[b])
        rel, _, _ = pr.metrics(ref, o["P"][b])
        assert rel < TOL_P_FP32 and rel_fro(o["P"][b], ref.P.astype(np.float64)) < TOL_P_FP32
        assert rel > pr.tol(ref), (rel, pr.tol(ref))


@pytest.mark.parametrize("flags", [0, TP])
def test_fp32_flag_within_one_workgroup_changes_nothing(built, flags):
    """N = 200, M = 120: one workgroup holds the factor and every column of the state (trsm_forms_T), plan.f32_whitened is
    false, and the flag must not change a bit of P+ or dx."""
    P, H, inn, dR = synth.s_level(200, 60, 3, seed=32)
    a = _run(P, H, inn, dR, flags, False)
    b = _run(P, H, inn, dR, flags | F32, False)
    assert a["route"] == b["route"] and a["route"] != "fused"
    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["dx"], b["dx"])


# ---------------------------------------------------------------- e. rows that are not plain compressed pairs
def _oos_list(sc, lay, cam, B, n_oos, ks, seed):
    rng = np.random.default_rng(seed)
    oos = np.zeros((B, n_oos), dtype=oos_dtype)
    ng = sc["gR"].shape[1]
    for b in range(B):
        for o in range(n_oos):
            k = ks[o % len(ks)]
            Xs = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3, 6)])
            gs = rng.permutation(ng)[:k]
            oos[b, o]["Xs"] = Xs; oos[b, o]["n_obs"] = k
            for q, g in enumerate(gs):
                _, _, r = orc.oos_jacobian_internal(Xs, sc["gR"][b, g], sc["gT"][b, g], sc["Rbc"][b], sc["Tbc"][b], [0, 0], cam, lay, int(g))
                oos[b, o]["group_sind"][q] = g; oos[b, o]["xp"][q] = -r + rng.normal(0, 1.0, 2)
    return oos


def _staged_update_check(stage, what):
    """The rows as staged (get_H of every filter), then the update of the same staging in a second context, against the
    extended-precision reference on those rows. (Two contexts: reading the rows back builds their dense copy, and a calibration
    stacking read back is re-stacked densely - the update would no longer take the route under test.)"""
    ctx, P = stage()
    B = P.shape[0]
    with ctx:
        rows = [ctx.get_H(b) for b in range(B)]
    ctx, _ = stage()
    with ctx:
        ctx.update_joseph()
        assert (ctx.get_status() == 0).all() and not ctx.get_ldlt_used().any()
        Pn, err, route, path = ctx.download_P(), ctx.get_err(), ctx.last_route(), ctx.last_path()
    for b in range(B):
        H, inn, dR = rows[b]
        ref = pr.extended(H, P[b], inn, dR)
        rel, corr, dx = pr.check(ref, Pn[b], err[b], what=(what, b))
        print("accuracy %s %s: rel %.3f corr %.3f dx %.3f x u (kappa + N)" % (route, what, rel, corr, dx))
    return route, path


def test_calibration_lead_block_rows(built):
    """An online-calibration stacking: compressed in-state rows + the leading dense block of the td / Cg / bg / intrinsics
    columns (sparse pipeline)."""
    import test_calib_gpu as cal

    def stage():
        cam, lay, sc, poses, groups, feats, xp, calib, cals, ctx = cal.setup("radtan", True, True, True, B=3, ng=6, nf=14, seed=8)
        P = np.array([spd(lay.N, 120 + b) * 1e-4 for b in range(3)])
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats); ctx.set_calib_state(calib)
        ctx.jacobians_instate(); ctx.mh_gate(R, cal.MH, cal.MULT, 5); ctx.stack(R)
        return ctx, P
    route, path = _staged_update_check(stage, "calibration lead block")
    assert path == 1, route


@pytest.mark.parametrize("compress", [False, True])
def test_oos_rows_behind_the_in_state_rows(built, compress):
    """OOS rows appended by oos_project (the mixed-row route: compressed in-state rows, dense OOS block - it needs room for the
    16-row-padded block behind the in-state rows, hence M_max), and the same rows QR-compressed by compress_oos."""
    import test_glevel_gpu as gl
    ng, nf, F, B, n_oos = 4, 10, 10, 3, 12

    def stage():
        sc, lay, ctx, poses, groups, feats, xp = gl.make(ng, nf, F, B, 12, synth.PINHOLE, M_max=2 * F + n_oos * 5 + 32)
        oos = _oos_list(sc, lay, synth.PINHOLE, B, n_oos, [4, 3], 5)
        P = np.array([spd(lay.N, 140 + b) * 1e-4 for b in range(B)])
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.jacobians_instate(); ctx.mh_gate(R, gl.MH, gl.MULT, 5); ctx.stack(R)
        nrows = ctx.oos_project(oos, 3.5 ** 2)
        assert (nrows > 0).all()
        if compress:
            crow = ctx.compress_oos(1.0)
            assert (crow < nrows).all(), (crow, nrows)
        return ctx, P
    route, path = _staged_update_check(stage, "oos qr-compressed" if compress else "oos mixed rows")
    assert path == 1, route


# ---------------------------------------------------------------- f. XIVO_HIP_CHUNK
CHUNK_SHAPES = [
    ("fused", 150, 32, False, 0, "fused"),
    ("throughput_in_solve", 200, 88, False, TP, "sparse_in_solve"),
    ("dense_whitened", 64, 20, True, 0, "dense_whitened"),
]


def _not_spd(P, H, dR, seed):
    """P - a z z^T with a random z, a large enough that S = H P H^T + R is indefinite while every feature's 2 x 2 block of S
    stays positive definite (the gate's distances stay finite)."""
    z = np.random.default_rng(seed).normal(size=P.shape[0])
    w = H @ z
    S = H @ P @ H.T + np.diag(dR)
    a = 2.0 / (w @ np.linalg.solve(S, w))
    Pb = P - a * np.outer(z, z)
    Sb = H @ Pb @ H.T + np.diag(dR)
    assert np.linalg.eigvalsh(Sb).min() < 0
    for f in range(H.shape[0] // 2):
        assert np.linalg.eigvalsh(Sb[2 * f:2 * f + 2, 2 * f:2 * f + 2]).min() > 0
    return Pb


@pytest.mark.parametrize("chunk", [64, 7])
@pytest.mark.parametrize("entry", ["j", "g"])
@pytest.mark.parametrize("shape", [s[0] for s in CHUNK_SHAPES])
def test_chunked_batch_is_the_unchunked_batch(built, monkeypatch, shape, entry, chunk):
    """XIVO_HIP_CHUNK walks the batch in ranges (update_chunks): the b0 offsets of every per-filter buffer (range_view,
    ell_range), the few-filter decision taken on the whole call's batch (call_batch), the L D L^T fallback per range. 200
    distinct filters - below every batch-size class boundary (256) - one of them in the third range with an indefinite S:
    per filter P+, dx, gate, status and ldlt_used the unchunked run's bits, the same route and solve kernel, the fallback
    flag at that filter only."""
    _, N, F, dense, flags, route = next(s for s in CHUNK_SHAPES if s[0] == shape)
    B = 200
    P, H, inn, dR = synth.s_level(N, F, B, seed=N + F + (7 if dense else 0), dense=dense)
    bad = 2 * chunk + 3
    P[bad] = _not_spd(P[bad], H[bad], dR[bad], bad)
    monkeypatch.delenv("XIVO_HIP_CHUNK", raising=False)
    whole = _run(P, H, inn, dR, flags, entry == "g", profile=True)
    monkeypatch.setenv("XIVO_HIP_CHUNK", str(chunk))
    part = _run(P, H, inn, dR, flags, entry == "g", profile=True)
    assert whole["route"] == part["route"] == route, (whole["route"], part["route"])
    assert whole["kernel"] == part["kernel"], (whole["kernel"], part["kernel"])
    assert np.nonzero(whole["ldlt"])[0].tolist() == [bad] and (whole["status"] == 0).all()
    keys = ("P", "dx", "status", "ldlt") + (("mask", "dist") if entry == "g" else ())
    for k in keys:
        diff = [b for b in range(B) if not np.array_equal(whole[k][b], part[k][b])]
        assert not diff, (k, diff[:10])
