"""Innovation log on the device (xivo_hip_innov_*): every record against the longdouble restatement of tests/innov_restate.py
from the rows and the dx the context returns after the update (bound 1), against inn^T S^-1 inn from the prior P in longdouble
(bound 2), and the ordering prefit >= nis >= postfit >= 0 (3) - on every representation of the staged rows and every update
route; the guards, the allocation accounting, the statistics and the drivers. Each test prints its worst error / bound."""
import numpy as np
import pytest

import innov_restate as ir
from xivo_amd import pcw, sequence, synth
from xivo_amd import lib as L
from xivo_amd.lib import (Context, XivoHipError, FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_DENSE_H, FLAG_SYMMETRIC_FORM,
                          FLAG_STANDALONE_TAIL, FLAG_FP32_WHITENED, FLAG_NO_LDLT_FALLBACK)

pytestmark = pytest.mark.gpu
MT, TP, SYM, TAIL, DH, F32 = (FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_SYMMETRIC_FORM, FLAG_STANDALONE_TAIL, FLAG_DENSE_H,
                              FLAG_FP32_WHITENED)
W_PAIR, W_LEAD = ir.W_PAIR, ir.W_PAIR + ir.W_LEAD
R_VIS, MH, MULT = 2.25, 5.991, 1.1


def _check_records(ctx, rec, P0, w, what, truth_for=(), expect_flags=0):
    """rec [B]: the frame just recorded. Reads dx, status and the rows as staged (get_H builds the dense copy - after the
    record) and holds every filter to the bounds. -> (worst ratio to bound 1, worst ratio to bound 2)"""
    B = rec.shape[0]
    dx, st, ld = ctx.get_err(), ctx.get_status(check=False), ctx.get_ldlt_used()
    rows = [ctx.get_H(b) for b in range(B)]
    w1 = w2 = 0.0
    for b in range(B):
        H, inn, dR = rows[b]
        ref = ir.restate(H, inn, dR, dx[b], st[b], ld[b], w=w)
        w1 = max(w1, ir.check(rec[b], ref, (what, b)))
        assert int(rec[b]["flags"]) == expect_flags, (what, b, int(rec[b]["flags"]))
        if rec[b]["flags"] == 0:
            ir.ordering_slack(rec[b], ref, (what, b))
        if b in truth_for:
            t, bound = ir.truth(H, P0[b], inn, dR, dx[b], w=w)
            err = abs(float(ir.LD(float(rec[b]["nis"])) - t))
            assert err <= bound, (what, b, float(rec[b]["nis"]), float(t), err, bound)
            w2 = max(w2, err / bound)
    return w1, w2, rows, dx


# ---------------------------------------------------------------- S-level, compressed rows
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("N,M", [(59, 2), (59, 14), (59, 16), (59, 18), (64, 130)])
def test_compressed_rows_from_a_hand_over(built, N, M, B):
    """XIVO-structured rows (layout 23 + 6 * 3 + 3 * 6, or N = 64) through xivo_hip_set_measurements: row counts on both sides
    of the padding to 16 and more than 64 pairs; one filter, a few, more than a wave of them. Full log and a slice."""
    nd = min(B, 4)
    P, H, inn, dR = synth.s_level(N, M // 2, nd, seed=N + M, G=3)
    idx = np.arange(B) % nd
    P, H, inn, dR = P[idx], H[idx], inn[idx], dR[idx]
    with Context(N, M, B) as ctx:
        ctx.innov_config(3)
        ctx.upload_P(P); ctx.set_measurements(H, inn, dR); ctx.update_joseph()
        assert ctx.last_path() == 1
        assert ctx.innov_record(ts_ns=77) == 0
        recs, ts = ctx.innov_read()
        assert recs.shape == (1, B) and ts.tolist() == [77] and ctx.innov_count() == 1
        w1, w2, rows, dx = _check_records(ctx, recs[0], P, W_PAIR, ("hand-over", N, M, B), truth_for=range(nd))
        assert (recs[0]["dof"] == M).all() and (recs[0]["rows"] == M).all()
        for b in range(B):                                      # equal filters, equal bits - whatever workgroup took them
            assert recs[0][b].tobytes() == recs[0][idx[b]].tobytes()
        # the dense copy is alive now (get_H): the same rows, one thread per row - within both bounds of the same restatement
        assert ctx.innov_record(ts_ns=78) == 1
        again, _ = ctx.innov_read(t0=1)
        for b in range(min(B, nd)):
            ref = ir.restate(*rows[b], dx[b], w=N)
            w1 = max(w1, ir.check(again[0][b], ref, ("dense copy", b)))
        if B >= 3:
            part, pts = ctx.innov_read(b0=1, nb=2)
            assert part.shape == (2, 2) and part.tobytes() == np.ascontiguousarray(np.concatenate([recs, again])[:, 1:3]).tobytes()
            assert pts.tolist() == [77, 78]
    print("innov hand-over N %d M %d B %d: worst error / bound (1) %.3f, (2) %.4f" % (N, M, B, w1, w2))


# ---------------------------------------------------------------- every route
ROUTES = [(0, "fused"), (MT, "sparse_whitened"), (MT | TP, "sparse_in_solve"), (TP, "fused"), (SYM, "sparse_symmetric"),
          (TAIL, "sparse_tail"), (DH, "dense_ascoded"), (MT | F32, "sparse_whitened")]


def _route_params():
    shapes = [(N, M, f, r) for (N, M) in ((59, 12), (203, 60)) for f, r in ROUTES]
    return shapes + [(300, 120, F32, "sparse_whitened")]        # beyond one workgroup: the flag's float operands are in use


@pytest.mark.parametrize("N,M,flags,route", _route_params())
def test_every_route_leaves_a_dx_the_record_can_use(built, N, M, flags, route):
    """the routes of plan_update at two shapes (and XIVO_HIP_FLAG_FP32_WHITENED where it applies: N = 300, M = 120, beyond one
    workgroup - dx stays fp64): the intended route ran, no route consumed inn or diagR, same bounds"""
    B = 3
    P, H, inn, dR = synth.s_level(N, M // 2, B, seed=N + M + 1, G=3 if N == 59 else 8)
    with Context(N, M, B, flags=flags) as ctx:
        ctx.innov_config(1)
        ctx.upload_P(P); ctx.set_measurements(H, inn, dR); ctx.update_joseph()
        assert ctx.last_route() == route, (ctx.last_route(), route)
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w = N if flags & DH else W_PAIR
        w1, w2, rows, _ = _check_records(ctx, recs[0], P, w, (route, N, M), truth_for=(0,))
        for b in range(B):                                      # what was handed over is what is staged
            assert np.array_equal(rows[b][1], inn[b]) and np.array_equal(rows[b][2], dR[b]) and np.array_equal(rows[b][0], H[b])
    print("innov route %s N %d M %d: worst error / bound (1) %.3f, (2) %.4f" % (route, N, M, w1, w2))


def test_symmetric_form_on_dense_rows(built):
    """XIVO_HIP_FLAG_SYMMETRIC_FORM on rows that do not compress: the dense_symmetric route"""
    N, F, B = 64, 8, 3
    P, H, inn, dR = synth.s_level(N, F, B, seed=9, dense=True)
    with Context(N, 2 * F, B, flags=SYM) as ctx:
        ctx.innov_config(1)
        ctx.upload_P(P); ctx.set_measurements(H, inn, dR); ctx.update_joseph()
        assert ctx.last_route() == "dense_symmetric"
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w1, w2, _, _ = _check_records(ctx, recs[0], P, N, "dense_symmetric", truth_for=range(B))
    print("innov route dense_symmetric: worst error / bound (1) %.3f, (2) %.4f" % (w1, w2))


# ---------------------------------------------------------------- rows that do not fit
def test_dense_rows_and_a_batch_that_mixes_both(built):
    N, F, B = 64, 8, 4
    P, H, inn, dR = synth.s_level(N, F, B, seed=5, G=3)
    Hd = synth.s_level(N, F, B, seed=6, dense=True)[1]
    for which in ([0, 1, 2, 3], [1, 3]):                        # every filter dense; fitting and non-fitting filters mixed
        Hm = H.copy(); Hm[which] = Hd[which]
        with Context(N, 2 * F, B) as ctx:
            ctx.innov_config(1)
            ctx.upload_P(P); ctx.set_measurements(Hm, inn, dR); ctx.update_joseph()
            assert ctx.last_path() == 0 and ctx.last_route() == "dense_whitened"
            ctx.innov_record()
            recs, _ = ctx.innov_read()
            w1, w2, _, _ = _check_records(ctx, recs[0], P, N, ("over", tuple(which)), truth_for=range(B))
            assert (recs[0]["dof"] == 2 * F).all()
        print("innov dense rows %s: worst error / bound (1) %.3f, (2) %.4f" % (which, w1, w2))


# ---------------------------------------------------------------- G-level with a gate
@pytest.mark.parametrize("ransac", [False, True])
def test_filter_update_with_a_rejected_and_an_absent_feature(built, ransac):
    import test_glevel_gpu as gl
    from scene_util import spd
    ng, F, B = 3, 6, 3
    sc, lay, ctx, poses, groups, feats, xp = gl.make(ng, F, F, B, 9, synth.PINHOLE)
    feats["xp"][:, 2] += 60.0                                   # MH gating rejects feature 2 of every filter
    feats["sind"][:, 4] = -1                                    # feature 4 is absent
    P = np.array([spd(lay.N, 50 + b) * 1e-4 for b in range(B)])
    with ctx:
        ctx.innov_config(1)
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        if ransac:
            ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, 3, want=False)
            ctx.one_point_ransac(R_VIS, 5.0, 5.89, want=False)
            with pytest.raises(XivoHipError):                   # the partial update inside RANSAC is absorbed there
                ctx.innov_record()
            ctx.stack(R_VIS); ctx.update_joseph()
        else:
            ctx.filter_update(R_VIS, MH, MULT, 3, use_gating=True)
        mask, _ = ctx.get_gate(F)
        assert not mask[:, 2].any() and not mask[:, 4].any()
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w1, w2, rows, _ = _check_records(ctx, recs[0], P, W_PAIR, ("filter_update", ransac), truth_for=range(B))
        for b in range(B):
            assert recs[0][b]["rows"] == 2 * F and recs[0][b]["dof"] == 2 * int(mask[b].sum()) and mask[b].sum() <= 4
            assert not rows[b][0][4:6].any() and not rows[b][1][4:6].any()      # the rejected pair: empty rows, no innovation
    print("innov filter_update ransac %s: worst error / bound (1) %.3f, (2) %.4f" % (ransac, w1, w2))


def test_gate_inside_the_update_neutralises_in_place(built):
    """xivo_hip_update_dense_gated on handed-over rows: the gate neutralises rejected pairs where they are staged (values 0,
    inn 0, diagR 1); the record counts what is left, on the one-kernel route and on the dense pipeline"""
    N, F, B = 96, 12, 3
    P, H, inn, dR = synth.s_level(N, F, B, seed=23)
    inn[:, 4:8] *= 1e4
    for flags in (0, MT, DH):
        with Context(N, 2 * F, B, flags=flags) as ctx:
            ctx.innov_config(1)
            ctx.upload_P(P); ctx.set_measurements(H, inn, dR)
            ctx.update_dense_gated(F, R_VIS, MH, MULT, 5)
            mask, _ = ctx.get_gate(F, B)
            assert not mask[:, 2:4].any()
            ctx.innov_record()
            recs, _ = ctx.innov_read()
            w1, w2, _, _ = _check_records(ctx, recs[0], P, N if flags & DH else W_PAIR, ("gated", flags), truth_for=(0,))
            assert (recs[0]["dof"] == 2 * mask.sum(axis=1)).all() and (recs[0]["rows"] == 2 * F).all()
        print("innov gated update flags %d (%s): worst error / bound (1) %.3f, (2) %.4f" % (flags, ctx.last_route(), w1, w2))


# ---------------------------------------------------------------- mixed and lead stagings, loop closure
@pytest.mark.parametrize("compress", [False, True])
def test_oos_rows_behind_the_compressed_rows(built, compress):
    import test_staging_gpu as sg
    ctx, P, F, _ = sg._stacked(0, False, M_extra=92, oos=12, compress=compress)
    B = P.shape[0]
    with ctx:
        ctx.innov_config(1)
        with pytest.raises(XivoHipError):                       # staged, not updated
            ctx.innov_record()
        ctx.update_joseph()
        assert ctx.last_path() == 1                             # the mixed-row route: the in-state rows stayed compressed
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w1, w2, rows, _ = _check_records(ctx, recs[0], P, ctx.N, ("oos", compress), truth_for=range(B))
        assert (recs[0]["rows"] > 2 * F).all() and (recs[0]["dof"] > 2 * F - 4).all()
    print("innov mixed stacking compress %s rows %d: worst error / bound (1) %.3f, (2) %.4f" % (compress, recs[0][0]["rows"], w1, w2))


def test_calibration_lead_block(built):
    import test_staging_gpu as sg
    ctx, P, F, _ = sg._stacked(0, True)
    B = P.shape[0]
    with ctx:
        ctx.innov_config(1)
        ctx.update_joseph()
        assert ctx.last_path() == 1                             # compressed rows + the leading block of calibration columns
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w1, w2, rows, _ = _check_records(ctx, recs[0], P, W_LEAD, "lead", truth_for=range(B))
        assert any(np.abs(r[0][:, 23:48]).max() > 0 for r in rows)     # the calibration columns are live
    print("innov lead block: worst error / bound (1) %.3f, (2) %.4f" % (w1, w2))


def test_loop_closure_rows(built):
    import test_staging_gpu as sg
    ctx, P, F, _ = sg._stacked(0, False, M_extra=92, oos=12)
    B, n = P.shape[0], 4
    mt = np.zeros((B, n), dtype=L.lc_dtype)
    with ctx:
        ctx.innov_config(1)
        feats = ctx.get_scene()[2]
        for b in range(B):
            for i in range(n):
                mt[b, i]["feat"], mt[b, i]["group_sind"], mt[b, i]["xp"] = i, feats["ref_sind"][b, i], feats["xp"][b, i] + 0.5
        ctx.close_loop_stack(mt, 1.5 ** 2); ctx.update_joseph()
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        w = W_PAIR if ctx.last_path() == 1 else ctx.N
        w1, w2, _, _ = _check_records(ctx, recs[0], P, w, "loop closure", truth_for=range(B))
        assert (recs[0]["rows"] == 2 * n).all() and (recs[0]["dof"] == 2 * n).all()
    print("innov loop closure: worst error / bound (1) %.3f, (2) %.4f" % (w1, w2))


# ---------------------------------------------------------------- status
@pytest.mark.parametrize("fallback", [False, True])
def test_indefinite_S(built, fallback):
    from test_update_accuracy_gpu import _not_spd
    N, F, B, bad = 96, 12, 4, 2
    P, H, inn, dR = synth.s_level(N, F, B, seed=41)
    P[bad] = _not_spd(P[bad], H[bad], dR[bad], 7)
    with Context(N, 2 * F, B, flags=0 if fallback else FLAG_NO_LDLT_FALLBACK) as ctx:
        ctx.innov_config(1)
        ctx.upload_P(P); ctx.set_measurements(H, inn, dR); ctx.update_joseph()
        ctx.innov_record()
        recs, _ = ctx.innov_read()
        st = ctx.innov_stats()
        rec = recs[0]
        good = [b for b in range(B) if b != bad]
        dx, status, ld = ctx.get_err(), ctx.get_status(check=False), ctx.get_ldlt_used()
        for b in range(B):
            Hb, ib, Rb = ctx.get_H(b)
            ir.check(rec[b], ir.restate(Hb, ib, Rb, dx[b], status[b], ld[b], w=W_PAIR), ("indefinite", b))
        if fallback:
            assert rec[bad]["flags"] == L.INNOV_LDLT and np.isfinite([rec[bad]["nis"], rec[bad]["prefit"], rec[bad]["postfit"]]).all()
        else:
            assert rec[bad]["flags"] == L.INNOV_FAILED and np.isnan([rec[bad]["nis"], rec[bad]["prefit"], rec[bad]["postfit"]]).all()
            assert rec[bad]["dx_max"] == 0.0
        assert (rec[good]["flags"] == 0).all()
        assert st["frame_used"].tolist() == [B - 1] and st["filt_used"].tolist() == [int(b != bad) for b in range(B)]
        assert st["frame_dof"][0] == rec[good]["dof"].sum() and st["filt_nis"][bad] == 0.0


# ---------------------------------------------------------------- guards
def _status(fn, *a, **k):
    try:
        fn(*a, **k)
    except XivoHipError as e:
        return e.status
    return 0


def test_guards_and_allocation_accounting(built):
    import test_glevel_gpu as gl
    from scene_util import spd
    ng, F, B = 3, 6, 2
    sc, lay, ctx, poses, groups, feats, xp = gl.make(ng, F, F, B, 9, synth.PINHOLE)
    P = np.array([spd(lay.N, 50 + b) * 1e-4 for b in range(B)])
    with ctx:
        ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
        ctx.filter_update(R_VIS, MH, MULT, 3, use_gating=True)
        assert _status(ctx.innov_record) == -1 and _status(ctx.innov_count) == -1 and _status(ctx.innov_reset) == -1   # not configured
        assert _status(ctx.innov_read, nt=0) == -1 and _status(ctx.innov_stats, nt=0) == -1
        ctx.snapshot_P()                                        # (allocates the snapshot: before the accounting below)
        live0, bytes0 = ctx.ctx_allocs()
        ctx.innov_config(2)
        live1, bytes1 = ctx.ctx_allocs()
        assert live1 == live0 + 2 and bytes1 - bytes0 == 2 * B * 64 + (2 + B) * 32
        assert ctx.innov_record(ts_ns=5) == 0                   # the update above is still current: configuring changes nothing
        ctx.absorb_error()
        assert _status(ctx.innov_record) == -1                  # dx is consumed
        ctx.filter_update(R_VIS, MH, MULT, 3, use_gating=True)
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, 3, want=False); ctx.stack(R_VIS)
        assert _status(ctx.innov_record) == -1                  # new rows staged, not updated
        ctx.update_joseph()
        ctx.restore_P()
        assert _status(ctx.innov_record) == -1                  # the covariance is no longer the update's
        ctx.update_joseph()
        assert ctx.innov_record(ts_ns=6) == 1
        assert _status(ctx.innov_record) == L.ERR_FULL and ctx.innov_count() == 2
        assert _status(ctx.innov_record, B=B + 1) == -1 and _status(ctx.innov_read, t0=1, nt=2) == -1
        assert ctx.ctx_allocs() == (live1, bytes1)              # nothing but innov_config allocates for the log
        recs, ts = ctx.innov_read()
        st = ctx.innov_stats()
        assert ts.tolist() == [5, 6] and (recs["flags"] == 0).all() and st["frame_used"].tolist() == [B, B]
        assert ctx.ctx_allocs() == (live1, bytes1)
        ctx.innov_reset()
        assert ctx.innov_count() == 0 and ctx.innov_record(ts_ns=9) == 0
        ctx.innov_config(0)                                     # releases the log
        assert ctx.ctx_allocs() == (live0, bytes0) and _status(ctx.innov_record) == -1 and _status(ctx.innov_count) == -1


def test_new_measurements_without_an_update_and_the_one_filter_call(built):
    N, F, B = 59, 6, 2
    P, H, inn, dR = synth.s_level(N, F, B, seed=3, G=3)
    with Context(N, 2 * F, B) as ctx:
        ctx.innov_config(4)
        ctx.upload_P(P)
        assert _status(ctx.innov_record) == -1                  # before any update
        ctx.set_measurements(H, inn, dR); ctx.update_joseph(); ctx.innov_record()
        ctx.set_measurements(H, inn * 2, dR)
        assert _status(ctx.innov_record) == -1 and ctx.innov_count() == 1
        # xivo_hip_update_joseph_host, the one-filter drop-in call, vouches for its own filter only
        Pcm = np.asfortranarray(P[1].copy())
        ctx.update_joseph_host(H[1], inn[1], dR[1], Pcm, b=1, mode=0)
        assert _status(ctx.innov_record, B=B) == -1             # filter 0 holds new rows and a stale dx
        ctx.upload_P(P[:1])
        ctx.update_joseph_host(H[0], inn[0], dR[0], None, b=0, mode=L.HOST_P_RESIDENT | L.HOST_KEEP_P)   # P stays on the device
        assert ctx.innov_record(B=B) == 1
        recs, _ = ctx.innov_read()
        dx = ctx.get_err()
        for b in range(B):
            Hb, ib, Rb = ctx.get_H(b)
            assert np.array_equal(ib, inn[b])
            ir.check(recs[1][b], ir.restate(Hb, ib, Rb, dx[b], w=W_PAIR), ("one-filter call", b))
            assert recs[1][b]["dof"] == 2 * F and recs[1][b]["flags"] == 0
        # an update of fewer filters than the record asks for
        ctx.set_measurements(H, inn, dR); ctx.update_joseph(B=1)
        assert _status(ctx.innov_record, B=B) == -1 and ctx.innov_record(B=1) == 2


# ---------------------------------------------------------------- statistics
def test_stats_are_fixed_order_sums_of_the_records(built):
    from test_update_accuracy_gpu import _not_spd
    N, F, B, T = 59, 6, 65, 5
    nd = 8
    P, H, inn, dR = synth.s_level(N, F, nd, seed=13, G=3)
    idx = np.arange(B) % nd
    P, H, dR = P[idx], H[idx], dR[idx]
    Pbad = P.copy(); Pbad[11] = _not_spd(P[11], H[11], dR[11], 3)
    rng = np.random.default_rng(2)
    with Context(N, 2 * F, B) as ctx:
        ctx.innov_config(T)
        for t in range(T):
            ctx.upload_P(Pbad if t in (1, 3) else P)
            ctx.set_measurements(H, rng.normal(0, 1.5, size=(B, 2 * F)), dR); ctx.update_joseph()
            ctx.innov_record(ts_ns=t)
        recs, _ = ctx.innov_read()
        assert sorted(zip(*np.nonzero(recs["flags"]))) == [(1, 11), (3, 11)] and (recs["flags"][[1, 3], 11] == L.INNOV_LDLT).all()
        a, b = ctx.innov_stats(), ctx.innov_stats()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k          # two calls, the same bits
        ok = (recs["flags"] == 0) & np.isfinite(recs["nis"])
        nis = np.where(ok, recs["nis"], 0.0).astype(ir.LD)
        dof = np.where(ok, recs["dof"], 0).astype(np.int64)
        worst = 0.0
        for name, axis, n in (("frame", 1, B), ("filt", 0, T)):
            s = -(-n // 256) + 8                                # the longest chain: a thread's strided sum + the tree
            bound = (s + 4) * ir.U * np.abs(nis).sum(axis=axis).astype(np.float64)
            err = np.abs((a[name + "_nis"].astype(ir.LD) - nis.sum(axis=axis)).astype(np.float64))
            assert (err <= bound).all(), (name, err.max(), bound.min())
            worst = max(worst, float((err / bound).max()))
            assert np.array_equal(a[name + "_dof"], dof.sum(axis=axis)) and np.array_equal(a[name + "_used"], ok.sum(axis=axis))
        assert a["frame_used"].tolist() == [B, B - 1, B, B - 1, B] and a["filt_used"][11] == T - 2
        # a slice: its filters' sums are the full call's bits; its frame sums are sums over the slice
        part = ctx.innov_stats(b0=7, nb=9, t0=0, nt=T)
        for k in ("filt_nis", "filt_dof", "filt_used"):
            assert part[k].tobytes() == np.ascontiguousarray(a[k][7:16]).tobytes(), k
        assert np.array_equal(part["frame_dof"], dof[:, 7:16].sum(axis=1))
        late = ctx.innov_stats(b0=0, nb=B, t0=2, nt=3)
        assert late["frame_nis"].tobytes() == np.ascontiguousarray(a["frame_nis"][2:]).tobytes()
        ratio = a["frame_nis"] / a["frame_dof"]
        assert np.isfinite(ratio).all() and (ratio > 0).all()
    print("innov stats: worst error / bound %.3f; nis per dof per frame %s" % (worst, " ".join("%.2e" % r for r in ratio)))


# ---------------------------------------------------------------- drivers
class _Probe(sequence.HipBackend):
    """HipBackend whose record is followed by a read of what the record used: dx, status and the staged rows of every filter"""

    def enable_innovation_log(self, T_max):
        super().enable_innovation_log(T_max)
        self.seen = []
        record = self.ctx.innov_record

        def probed(ts_ns=0, B=None):
            k = record(ts_ns, B)
            self.seen.append((self.ctx.get_err(), self.ctx.get_status(check=False), self.ctx.get_ldlt_used(),
                              [self.ctx.get_H(b) for b in range(self.B)]))
            return k
        self.ctx.innov_record = probed


def _check_report(out, recs):
    """what a driver returns next to the records follows from the records: the ratios of the fixed-order sums, to the
    (s + 4) u rounding of a sum of non-negative terms and one division"""
    used = (recs["flags"] == 0) & np.isfinite(recs["nis"])
    assert np.array_equal(out["nis_used"], used.sum(axis=1)) and out["nis_records_left_out"] == int((~used).sum())
    nis, dof = np.where(used, recs["nis"], 0.0).astype(ir.LD), np.where(used, recs["dof"], 0)
    for key, axis in (("nis_per_dof", 1), ("nis_per_dof_seq", 0)):
        d = dof.sum(axis=axis)
        want = np.where(d > 0, (nis.sum(axis=axis) / np.maximum(d, 1)).astype(np.float64), np.nan)
        got = out[key]
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), key
        ok = ~np.isnan(want)
        tol = (ir.chain(recs.shape[axis]) + 5) * ir.U * np.abs(np.where(used, recs["nis"], 0.0)).sum(axis=axis) / np.maximum(d, 1)
        assert (np.abs(got[ok] - want[ok]) <= tol[ok]).all(), key


def test_drivers_record_every_frame_and_leave_the_filter_alone(built):
    B, total = 2, 0.4                                           # 10 camera frames
    cfg = sequence.SequenceConfig()
    runs = {}
    for key, factory, on in (("off", sequence.HipBackend, False), ("on", sequence.HipBackend, True), ("probe", _Probe, True)):
        worlds = [pcw.RandomPCW(seed=10 + b) for b in range(B)]
        sims = [pcw.TrajectorySim("trefoil" if b == 1 else "lissajous", seed=200 + b) for b in range(B)]
        runs[key] = sequence.run_pcw(factory, cfg, worlds, sims, total_time=total, innovation_log=on)
    off, on, probe = runs["off"], runs["on"], runs["probe"]
    assert "nis_per_dof" not in off and "innovation" not in off
    for r in (on, probe):                                       # the log does not perturb the filter
        assert np.array_equal(r["Tsb"], off["Tsb"]) and np.array_equal(r["Wsb"], off["Wsb"]) and np.array_equal(r["ts"], off["ts"])
    recs = on["innovation"]["recs"]
    assert recs.shape == (10, B) and np.array_equal(on["innovation"]["ts"], on["ts"])
    assert recs.tobytes() == probe["innovation"]["recs"].tobytes()
    worst = 0.0
    for t, (dx, st, ld, rows) in enumerate(probe["backend"].seen):
        for b in range(B):
            ref = ir.restate(*rows[b], dx[b], st[b], ld[b], w=W_PAIR)
            worst = max(worst, ir.check(recs[t][b], ref, ("run_pcw", t, b)))
            if recs[t][b]["flags"] == 0:
                ir.ordering_slack(recs[t][b], ref, ("run_pcw", t, b))
    assert on["nis_per_dof"].shape == (10,) and on["nis_per_dof_seq"].shape == (B,) and on["nis_used"].shape == (10,)
    _check_report(on, recs)
    print("innov run_pcw: worst error / bound (1) %.3f; nis per dof per frame %s" % (worst, np.round(on["nis_per_dof"], 3)))
    # the C++ frame (BatchEstimator::EnableInnovationLog) on the same worlds and simulators: its records against the
    # restatement of the probed python frame. The two hosts agree on the state within 1e-9 (tests/test_sequence_gpu.py); a state
    # that far off moves inn_i by at most 1e-9 sum_j |H_ij|, and each sum by at most
    #   PAR = 2e-9 sum_i (|inn_i| + (|H||dx|)_i) (sum_j |H_ij|) / R_i
    # to first order (|r_i| <= |inn_i| + (|H||dx|)_i) - on top of bound (1)
    worlds = [pcw.RandomPCW(seed=10 + b) for b in range(B)]
    sims = [pcw.TrajectorySim("trefoil" if b == 1 else "lissajous", seed=200 + b) for b in range(B)]
    cp = sequence.run_pcw_cpp(cfg, worlds, sims, total_time=total, innovation_log=True)
    cr = cp["innovation"]["recs"]
    assert cr.shape == (10, B) and np.array_equal(cp["innovation"]["ts"], on["ts"])      # one record per frame, stamped t * 1e9
    assert np.abs(cp["Tsb"] - on["Tsb"]).max() < 1e-9
    worst_c = 0.0
    for t, (dx, st, ld, rows) in enumerate(probe["backend"].seen):
        for b in range(B):
            Hb, ib, Rb = rows[b]
            ref = ir.restate(Hb, ib, Rb, dx[b], st[b], ld[b], w=W_PAIR)
            for k in ("dof", "rows", "flags"):
                assert int(cr[t][b][k]) == ref[k], ("run_pcw_cpp", t, b, k)
            par = 2e-9 * float(np.sum((np.abs(ib) + np.abs(Hb) @ np.abs(dx[b])) * np.abs(Hb).sum(axis=1) / Rb))
            for k in ("nis", "prefit", "postfit"):
                err, bound = abs(float(ir.LD(float(cr[t][b][k])) - ref[k])), ref["b_" + k] + par
                assert err <= bound, ("run_pcw_cpp", t, b, k, err, bound)
                worst_c = max(worst_c, err / bound if bound > 0 else 0.0)
            if cr[t][b]["flags"] == 0:
                wide = dict(ref, b_nis=ref["b_nis"] + par, b_prefit=ref["b_prefit"] + par, b_postfit=ref["b_postfit"] + par)
                ir.ordering_slack(cr[t][b], wide, ("run_pcw_cpp", t, b))
    _check_report(cp, cr)
    print("innov run_pcw_cpp: worst error / (bound (1) + parity) %.3g; bit-identical to the python frame's records: %s" % (
        worst_c, cr.tobytes() == recs.tobytes()))
    cp["estimator"].close()
    for r in runs.values():
        r["backend"].close()
    # the C++ frame (BatchEstimator::EnableInnovationLog) records at the same point
    nseq = 4
    batch = {}
    for flag in (False, True):
        batch[flag] = sequence.run_pcw_batch(cfg, nseq, total_time=total, innovation_log=flag)
    assert np.array_equal(batch[True]["Tsb"], batch[False]["Tsb"]) and "nis_per_dof" not in batch[False]
    br = batch[True]["innovation"]["recs"]
    assert br.shape == (10, nseq) and np.array_equal(batch[True]["innovation"]["ts"], batch[True]["ts"])
    assert (br["rows"] == 2 * cfg.n_features).all() and (br["dof"] % 2 == 0).all() and (br["dof"] <= br["rows"]).all()
    live = br["flags"] == 0
    assert (br["postfit"][live] >= 0).all() and (br["dof"][live].sum() > 0)
    # (3) without the rows at hand: the slack of (1) with (|H||dx|)_i taken as at most 63 |inn_i| - a correction 63 times the
    # innovation it answers is not an update of this simulator -, i.e. 64 (w + s + 8) u prefit
    slack = 64 * (W_PAIR + ir.chain(2 * cfg.n_features) + 8) * ir.U * br["prefit"][live]
    assert (br["prefit"][live] >= br["nis"][live] - slack).all() and (br["nis"][live] >= br["postfit"][live] - slack).all()
    assert (br["dof"][1:] > 0).all()                            # every frame after the first updates on in-state features
    _check_report(batch[True], br)
    for r in batch.values():
        r["estimator"].close()
    print("innov run_pcw_batch: nis per dof per frame %s" % np.round(batch[True]["nis_per_dof"], 3))
