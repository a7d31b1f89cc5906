"""The landmark map's two options through the C ABI on the GPU (xivo_hip_lcmap_cov_config): the covariance an added point is
stored with, its weight in the gate and in the rows, the update on the whitened rows, and one use per visit - held against
tests/lcmap_cov_restate.py, tests/lcmap_restate.py (the rows) and tests/map_restate.py (Sigma = J Pcc J^T in 80-bit arithmetic).
Shapes (tests/lcmap_cases.py): B = 3, 4 groups, 8 features (N = 71), Context(N, 16, 3), map_max 8, lc_max 6, min_matches 5."""
import numpy as np
import pytest

import lcmap_cases as LC
import lcmap_cov_cases as CC
import lcmap_cov_restate as CR
import lcmap_restate as R
import map_restate as mr
from helpers import rel_fro, TOL_P, TOL_DX
from test_lcmap_gpu import _adds, _config, _fill, _open, _P, _queries, _status, ERR_INVALID
from xivo_amd import synth
from xivo_amd.lib import lc_dtype, lcmap_cov_opts_dtype, lcmap_entry_dtype

pytestmark = pytest.mark.gpu
B, NG, NF = LC.B, LC.NG, LC.NF


def _cov_of(sig_by_entry):
    """{(b, entry): Sigma [3, 3]} -> [B, MAP_MAX, 6]"""
    cov = np.zeros((B, LC.MAP_MAX, 6))
    for (b, e), S in sig_by_entry.items():
        cov[b, e] = CR.pack6(S)
    return cov


def _perturb(ctx, c, scene):
    poses, groups, feats = scene
    for b in range(B):
        poses[b]["Rsb"] = c["Rsb_p"][b].T.reshape(-1); poses[b]["Tsb"] = c["Tsb_p"][b]
    ctx.set_scene(poses, groups, feats)


# ---------------------------------------------------------------- 1. add stores Sigma
@pytest.mark.parametrize("inv", [False, True])
def test_add_stores_the_covariance_of_the_world_point(built, inv):
    cam = synth.PINHOLE
    sc, x, Xs = LC.scene(cam, invdepth=inv)
    lay, P = LC.layout(), _P()
    ctx, (poses, groups, feats) = _open(cam, sc, x, P, inv)
    with ctx:
        assert _status(ctx.lcmap_get_cov) == ERR_INVALID and _status(ctx.lcmap_set_cov, np.zeros((B, LC.MAP_MAX, 6))) == ERR_INVALID
        assert _status(ctx.lcmap_cov_stats) == ERR_INVALID                    # all three: only with an option on
        ctx.lcmap_cov_config(point_cov=True)
        feats["sind"][1, 5] = -1                                              # a free slot of a ragged batch
        ctx.set_scene(poses, groups, feats)
        # filter 0: six features in a scrambled order, then a key stored already (dup: the first Sigma stays) under another
        # feature; filter 1: a free slot (skipped) between two records; filter 2: one record, in a second call
        order0 = [3, 0, 7, 1, 6, 2]
        recs = [(0, j, LC.key(0, j)) for j in order0] + [(0, 5, LC.key(0, 3))] + [(1, 4, 50), (1, 5, 51), (1, 2, 52)]
        ctx.lcmap_add(_adds(recs))
        ctx.lcmap_add(_adds([(2, 1, 7)]))
        (ent, cnt), cov = ctx.lcmap_get(), ctx.lcmap_get_cov()
        assert cnt.tolist() == [6, 2, 1] and ctx.lcmap_stats()["dup"].tolist() == [1, 0, 0]
        stored = {0: order0, 1: [4, 2], 2: [1]}
        ml = dict(group_begin=lay.group_begin, n_groups=NG, feature_begin=lay.feature_begin, n_features=NF)
        worst = 0.0
        for b in range(B):
            ref = {e["pos"]: e for e in mr.record(poses[b], groups[b], feats[b], P[b], ml, NF, invdepth=inv)}
            for pos, j in enumerate(stored[b]):
                d = np.abs(mr.LD(1) * cov[b, pos] - ref[j]["cov_world"]) / (mr.EPS * ref[j]["cov_world_mag"])
                worst = max(worst, float(d.max()))
            assert not cov[b, cnt[b]:].any()                                   # behind count: zero
            assert rel_fro(ent["Xs"][b, :cnt[b]], np.array([Xs[b, j] for j in stored[b]])) < 1e-12
        print("add inv=%d: worst |dSigma| / (eps |J||Pcc||J|^T) = %.2f (bound 64)" % (inv, worst))
        assert worst <= 64.0
        assert all(np.linalg.eigvalsh(CR.unpack6(cov[0, e])).min() > 0 for e in range(6))
        # set_cov / get_cov: every bit, also from b0 > 0; what set_cov refuses changes nothing
        new = np.random.default_rng(2).normal(size=(B, LC.MAP_MAX, 6)); new[..., (0, 3, 5)] = np.abs(new[..., (0, 3, 5)])
        ctx.lcmap_set_cov(new)
        assert ctx.lcmap_get_cov().tobytes() == new.tobytes()
        ctx.lcmap_set_cov(2 * new[2:3], b0=1)
        got = ctx.lcmap_get_cov()
        assert got[1].tobytes() == (2 * new[2]).tobytes() and got[0].tobytes() == new[0].tobytes() and got[2].tobytes() == new[2].tobytes()
        assert ctx.lcmap_get_cov(1, 2).tobytes() == got[1:].tobytes()
        for k, v in ((1, np.nan), (4, np.inf), (0, -1e-30), (3, -1.0), (5, -np.inf)):
            bad = new.copy(); bad[1, 3, k] = v
            assert _status(ctx.lcmap_set_cov, bad) == ERR_INVALID, (k, v)
        assert ctx.lcmap_get_cov().tobytes() == got.tobytes()
        # a loaded map has exact points until set_cov
        ent2 = np.zeros((1, LC.MAP_MAX), dtype=lcmap_entry_dtype); ent2["key"] = np.arange(LC.MAP_MAX) + 900
        ctx.lcmap_set(ent2, [4], b0=1)
        g2 = ctx.lcmap_get_cov()
        assert not g2[1].any() and g2[0].tobytes() == got[0].tobytes() and g2[2].tobytes() == got[2].tobytes()
        # the refusals of cov_config; then both options off: released
        o = np.zeros(1, dtype=lcmap_cov_opts_dtype)
        for size, pc, gap in ((12, 1, 0), (16, 2, 0), (16, -1, 0), (16, 1, -1)):
            o["struct_size"], o["point_cov"], o["revisit_gap"] = size, pc, gap
            assert ctx.lib.xivo_hip_lcmap_cov_config(ctx.h, o.ctypes.data) == ERR_INVALID, (size, pc, gap)
        assert ctx.lcmap_get_cov().tobytes() == g2.tobytes()
        ctx.lcmap_cov_config(revisit_gap=3)                                    # the options are independent: no Sigma with this one
        assert _status(ctx.lcmap_get_cov) == ERR_INVALID and not ctx.lcmap_cov_stats()["resting"].any()
        ctx.lcmap_cov_config()
        assert _status(ctx.lcmap_cov_stats) == ERR_INVALID and ctx.lcmap_get()[1].tolist() == [6, 4, 1]
        _config(ctx, map_max=0)
        assert _status(ctx.lcmap_cov_config, True, 0) == ERR_INVALID           # no configured map


# ---------------------------------------------------------------- 2. rows
@pytest.mark.parametrize("name", list(LC.CAMS))
def test_rows_are_whitened_and_gamma_is_the_gate_on_the_unwhitened_pair(built, name):
    cam = LC.CAMS[name]
    sc, x, Xs = LC.scene(cam)
    lay, P = LC.layout(), _P()
    rng = np.random.default_rng(3)
    js, gs = [1, 6, 3], [2, 0, 1]                                        # filter b: stored feature js[b], observing group gs[b]
    for b in range(B):                                                   # group slot gs[b] holds the body's own pose: the point is in view
        sc["gR"][b, gs[b]], sc["gT"][b, gs[b]] = sc["Rsb"][b], sc["Tsb"][b]
    assert all(sc["ref"][b, js[b]] != gs[b] for b in range(B))           # (the stored feature's own anchor stays what it was)
    xps = [LC.pixel(cam, Xs[b, js[b]], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b]) + rng.normal(0, 1.5, 2) for b in range(B)]
    xpb = xps
    ctx, _ = _open(cam, sc, x, P, min_matches=1, chi2=0.0)
    with ctx:
        ctx.lcmap_cov_config(point_cov=True)
        ctx.lcmap_add(_adds([(b, js[b], LC.key(b, js[b])) for b in range(B)]))
        ctx.lcmap_set_cov(_cov_of({(b, 0): CC.sigma(b) for b in range(B)}))
        got = {}
        for kind, g_of, xp_of in (("group", lambda b: gs[b], xps), ("body", lambda b: -1, xpb)):
            assert ctx.lcmap_close(_queries([(b, g_of(b), LC.key(b, js[b]), xp_of[b]) for b in range(B)])) == B
            got[kind] = ([ctx.get_H(b) for b in range(B)], ctx.lcmap_matches())
    worst = 0.0
    for kind in ("group", "body"):
        rows, mt = got[kind]
        for b in range(B):
            grp = kind == "group"
            pose = (sc["gR"][b, gs[b]], sc["gT"][b, gs[b]]) if grp else (sc["Rsb"][b], sc["Tsb"][b])
            m = dict(Xs=Xs[b, js[b]], Rsb=pose[0], Tsb=pose[1], g_sind=gs[b] if grp else -1, xp=(xps if grp else xpb)[b])
            Ho, io, dRo = R.rows([m], sc["Rbc"][b], sc["Tbc"][b], cam, lay, LC.LC_MAX, LC.RLC)
            Re = CR.r_eff(Ho[0:2], CC.sigma(b), LC.RLC, lay.group_begin + 6 * gs[b] if grp else 0)
            Hw, iw, dw = CR.whiten(Ho, io, dRo, [Re], [False] + [True] * (LC.LC_MAX - 1))
            H, inn, dR = rows[b]
            assert rel_fro(H, Hw) < 1e-12 and np.abs(inn - iw).max() < 1e-9 and (dR == 1.0).all()
            g = CR.gamma(Ho[0:2], P[b], io[0:2], Re)
            worst = max(worst, abs(mt["gamma"][b, 0] / g - 1))
            assert mt["kept"][b, 0] == 1 and mt["reserved"][b, 0] == 0
            assert not np.allclose(Hw[0:2], Ho[0:2])                     # (the whitening is no identity here)
    print("rows %s: worst rel. error of gamma %.2e" % (name, worst))
    assert worst < 1e-9


# ---------------------------------------------------------------- 3. / 5. update
def _update(cam, c, point_cov, sig=None, **kw):
    """fill, perturb the poses, close with c's queries, update, absorb -> dict of what the tests read"""
    ctx, scene = _open(cam, c["sc"], c["x"], c["P"], **kw)
    with ctx:
        _fill(ctx)                                                        # the points, stored from the unperturbed scene
        if point_cov:
            ctx.lcmap_cov_config(point_cov=True)                          # entries already in the map: Sigma = 0
            assert not ctx.lcmap_get_cov().any()
            if sig is not None:
                ctx.lcmap_set_cov(sig)
        _perturb(ctx, c, scene)
        before = (ctx.download_P(), ) + tuple(a.copy() for a in ctx.get_scene())
        n = ctx.lcmap_close(_queries([(b, -1, k, xp) for b, k, xp in c["queries"]]))
        out = dict(n=n, mt=ctx.lcmap_matches(), st=ctx.lcmap_stats(), cst=ctx.lcmap_cov_stats() if point_cov else None, before=before)
        if n:
            out["rows"] = ctx.get_H(0)
            ctx.update_joseph()
            assert (ctx.get_status() == 0).all()
            out["dx"] = ctx.get_err()
            ctx.absorb_error()
        out["after"] = (ctx.download_P(), ) + tuple(ctx.get_scene())
    return out


def test_zero_covariance_is_the_exact_point_update(built):
    cam = synth.EQUI
    c = LC.update_case(cam)
    off, on = _update(cam, c, False), _update(cam, c, True)
    assert off["n"] == on["n"] == 1 and np.array_equal(on["mt"]["kept"], off["mt"]["kept"])
    print("Sigma = 0: rel. diff P %.2e dx %.2e gamma %.2e" % (rel_fro(on["after"][0][0], off["after"][0][0]), rel_fro(on["dx"][0], off["dx"][0]),
                                                              np.abs(on["mt"]["gamma"][0] / off["mt"]["gamma"][0] - 1).max()))
    assert rel_fro(on["after"][0][0], off["after"][0][0]) < TOL_P and rel_fro(on["dx"][0], off["dx"][0]) < TOL_DX
    assert np.abs(on["mt"]["gamma"][0] / off["mt"]["gamma"][0] - 1).max() < 1e-9
    assert (on["rows"][2] == 1.0).all() and (off["rows"][2][:12] == LC.RLC).all()      # whitened with L = sqrt(Rlc) I
    assert rel_fro(on["rows"][0] * np.sqrt(LC.RLC), off["rows"][0]) < 1e-14


def test_update_with_point_covariance_is_the_full_R_joseph_form(built):
    cam = synth.EQUI
    c = CC.gate_case(cam)
    sig = _cov_of({(0, m): CC.sigma(m) for m in range(6)})
    r = _update(cam, c, True, sig)
    assert r["n"] == 1 and r["mt"]["kept"][0].tolist() == [1] * 6
    assert (r["st"]["closed_frames"].tolist(), r["st"]["short_frames"].tolist(), r["st"]["matched"].tolist()) == ([1, 0, 0], [0, 1, 0], [6, 4, 0])
    assert not r["cst"]["bad_cov"].any() and not r["cst"]["resting"].any()
    H, inn, dR, Res = CC.rows0(c, cam)
    e_ref, P_ref = CR.joseph_full_R(H, c["P"][0], inn, CR.block_R(Res, [False] * 6, LC.LC_MAX))
    print("update with Sigma: rel. error P %.2e dx %.2e" % (rel_fro(r["after"][0][0], P_ref), rel_fro(r["dx"][0], e_ref)))
    assert rel_fro(r["after"][0][0], P_ref) < TOL_P and rel_fro(r["dx"][0], e_ref) < TOL_DX
    assert not np.array_equal(r["after"][1][0], r["before"][1][0])        # the closing filter's pose moved
    for b in (1, 2):                                                      # short / no match: nothing changed by a bit
        assert np.array_equal(r["after"][0][b], r["before"][0][b]) and not r["dx"][b].any()
        for k in (1, 2, 3):
            assert r["after"][k][b].tobytes() == r["before"][k][b].tobytes(), (b, k)


# ---------------------------------------------------------------- 4. gate
def test_gate_weighs_the_point_and_refuses_an_indefinite_R(built):
    cam = synth.EQUI
    c = CC.gate_case(cam)
    P = c["P"]
    H, inn, dR, Res = CC.rows0(c, cam)
    sig = _cov_of({(0, m): CC.sigma(m) for m in range(6)})
    qs = _queries([(b, -1, k, xp) for b, k, xp in c["queries"]])
    ctx, scene = _open(cam, c["sc"], c["x"], P)
    with ctx:
        _fill(ctx); _perturb(ctx, c, scene)
        ctx.lcmap_close(qs, wait=False)
        m0 = ctx.lcmap_matches()
        assert m0["kept"][0].tolist() == [1, 1, 0, 1, 1, 1]               # exact points: the moved pair is gated
        ctx.lcmap_cov_config(point_cov=True); ctx.lcmap_set_cov(sig)
        ctx.lcmap_close(qs, wait=False)
        m1 = ctx.lcmap_matches()
        assert m1["kept"][0].tolist() == [1] * 6
        g = np.array([CR.gamma(H[2 * m:2 * m + 2], P[0], inn[2 * m:2 * m + 2], Res[m]) for m in range(6)])
        print("gate: gamma exact %s with Sigma %s, rel. error %.2e" % (np.round(m0["gamma"][0], 3), np.round(m1["gamma"][0], 3),
                                                                        np.abs(m1["gamma"][0] / g - 1).max()))
        assert np.abs(m1["gamma"][0] / g - 1).max() < 1e-9
        # tie: chi2 equal to a gamma read back keeps that match, one ulp below gates it
        g2 = float(m1["gamma"][0, CC.MOVED])
        for chi2, kept in ((g2, 1), (float(np.nextafter(g2, 0.0)), 0)):
            _config(ctx, chi2=chi2, min_matches=1); _fill(ctx)            # (a new configuration drops the options too)
            assert _status(ctx.lcmap_get_cov) == ERR_INVALID
            ctx.lcmap_cov_config(point_cov=True); ctx.lcmap_set_cov(sig)
            ctx.lcmap_close(qs, wait=False)
            m2 = ctx.lcmap_matches()
            assert m2["gamma"][0, CC.MOVED] == g2 and m2["kept"][0, CC.MOVED] == kept, chi2
        # a Sigma that passes set_cov (zero diagonal) and makes R_e of pair 4 indefinite: signed on the host from H_T
        a0 = H[8, 3:6]
        S = np.zeros((3, 3))
        for i, j in ((0, 1), (0, 2), (1, 2)):
            S[i, j] = S[j, i] = -1.0 if a0[i] * a0[j] > 0 else 1.0
        assert not CR.pivots_ok(CR.r_eff(H[8:10], S, LC.RLC))
        bad = sig.copy(); bad[0, 4] = CR.pack6(S)
        _config(ctx); _fill(ctx); ctx.lcmap_cov_config(point_cov=True); ctx.lcmap_set_cov(bad)
        assert ctx.lcmap_close(qs) == 1                                   # five kept: the filter still closes
        m3, st, cst = ctx.lcmap_matches(), ctx.lcmap_stats(), ctx.lcmap_cov_stats()
        assert m3["kept"][0].tolist() == [1, 1, 1, 1, 0, 1] and m3["gamma"][0, 4] == -1.0
        assert cst["bad_cov"].tolist() == [1, 0, 0] and st["gated"][0] == 1
        rows = ctx.get_H(0)
        assert not rows[0][8:10].any() and not rows[1][8:10].any() and np.isfinite(rows[0]).all()


# ---------------------------------------------------------------- 6. one use per visit
def test_visit_rule_on_the_device(built):
    cam = synth.EQUI
    c = LC.update_case(cam)
    sc, Xs, gap = c["sc"], c["Xs"], 2
    xp = lambda b, j: LC.pixel(cam, Xs[b, j], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b])
    q = lambda b, js: [(b, -1, LC.key(b, j), xp(b, j)) for j in js]
    calls = [q(0, range(6)),                                  # 1: six fresh matches close
             q(0, range(6)) + q(1, range(6)),                 # 2: filter 0 rests (filter 1 closes, so the rows are staged)
             q(0, [0, 1, 2, 3, 4, 6]),                        # 3: five resting and a new key: one pair takes part
             q(0, [7]), [], q(1, [0]),                        # 4 - 6: gap + 1 calls without filter 0's keys (one of them empty)
             q(0, range(6)),                                  # 7: fresh again
             q(0, [0, 1, 2, 3]) + [(0, -1, 12345, xp(0, 0))] + q(0, [7, 7]),   # 8: a key twice, next to resting matches
             q(0, [7])]                                       # 9: ... which has been used
    want_frames0 = [CR.CLOSED, CR.RESTED, CR.CLOSED, CR.SHORT, CR.NONE, CR.NONE, CR.CLOSED, CR.CLOSED, CR.SHORT]
    rs = [CR.VisitRestate(LC.MAP_MAX, LC.LC_MAX, LC.MIN_MATCHES, gap) for _ in range(B)]
    for b in range(B):
        rs[b].add([LC.key(b, j) for j in range(NF)])
    ctx, scene = _open(cam, sc, c["x"], c["P"])
    with ctx:
        _fill(ctx); _perturb(ctx, c, scene)
        ctx.lcmap_cov_config(revisit_gap=gap)
        for t, qs in enumerate(calls):
            n = ctx.lcmap_close(_queries(qs))
            mt = ctx.lcmap_matches()
            res = [rs[b].close([k for bb, _, k, _ in qs if bb == b], list(mt["kept"][b])) for b in range(B)]
            assert n == sum(r["frame"] == CR.CLOSED for r in res), t
            assert res[0]["frame"] == want_frames0[t], (t, res[0])
            for b in range(B):
                k = len(res[b]["entries"])
                assert mt["entry"][b].tolist() == res[b]["entries"] + [-1] * (LC.LC_MAX - k), (t, b)
                assert mt["reserved"][b].tolist() == res[b]["resting"] + [0] * (LC.LC_MAX - k), (t, b)
                assert mt["kept"][b, :k].all(), (t, b)                     # (inside the covariance: the gate keeps them all)
                if n:                                                      # staged: zero exactly where the restatement says neutral
                    H, inn, dR = ctx.get_H(b)
                    got = [int(not H[2 * m:2 * m + 2].any() and not inn[2 * m:2 * m + 2].any() and (dR[2 * m:2 * m + 2] == 1.0).all())
                           for m in range(LC.LC_MAX)]
                    assert got == res[b]["neutral"], (t, b)
            if t == 1:                                                     # the rested frame: closing 0 (only filter 1 closes)
                assert n == 1 and res[1]["frame"] == CR.CLOSED and res[0]["neutral"] == [1] * 6 and res[0]["resting"] == [1] * 6
            if t == 2:
                assert res[0]["neutral"] == [1, 1, 1, 1, 1, 0]
            if t == 7:
                assert res[0]["entries"] == [0, 1, 2, 3, 7, 7] and res[0]["neutral"] == [1, 1, 1, 1, 0, 0]
            if t == 8:
                assert res[0]["resting"] == [1]
            st, cst = ctx.lcmap_stats(), ctx.lcmap_cov_stats()
            for b in range(B):
                for k in ("gated", "short_frames", "closed_frames"):
                    assert st[k][b] == rs[b].stats[k], (t, b, k)
                for k in ("resting", "rested_frames"):
                    assert cst[k][b] == rs[b].stats[k], (t, b, k)
        assert cst["rested_frames"].tolist() == [1, 0, 0] and cst["resting"][0] == 6 + 5 + 4 + 1
        # a new cov_config starts over: t = 1, nothing seen
        ctx.lcmap_cov_config(revisit_gap=gap)
        assert ctx.lcmap_close(_queries(calls[0])) == 1 and not ctx.lcmap_matches()["reserved"].any()
        assert not ctx.lcmap_cov_stats()["resting"].any()


# ---------------------------------------------------------------- 7. options off
def test_options_off_are_the_rows_of_close_loop_stack_bit_for_bit(built):
    cam = synth.EQUI
    sc, x, Xs = LC.scene(cam)
    lay, P = LC.layout(), _P()
    rng = np.random.default_rng(3)
    js, gs = [1, 6, 3], [2, 0, 1]
    for b in range(B):
        sc["gR"][b, gs[b]], sc["gT"][b, gs[b]] = sc["Rsb"][b], sc["Tsb"][b]
    xps = [LC.pixel(cam, Xs[b, js[b]], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b]) + rng.normal(0, 1.5, 2) for b in range(B)]
    qs = _queries([(b, gs[b], LC.key(b, js[b]), xps[b]) for b in range(B)])
    ctx, _ = _open(cam, sc, x, P, min_matches=1, chi2=0.0)
    with ctx:
        ctx.lcmap_cov_config(point_cov=True, revisit_gap=4)
        ctx.lcmap_add(_adds([(b, js[b], LC.key(b, js[b])) for b in range(B)]))
        ctx.lcmap_close(qs, wait=False)
        on = [ctx.get_H(b) for b in range(B)]
        ctx.lcmap_cov_config()                                            # both off
        ctx.lcmap_close(qs, wait=False)
        off = [ctx.get_H(b) for b in range(B)]
        assert not ctx.lcmap_matches()["reserved"].any()
        mt = np.zeros((B, LC.LC_MAX), dtype=lc_dtype); mt["feat"] = -1
        for b in range(B):
            mt[b, 0]["feat"], mt[b, 0]["group_sind"], mt[b, 0]["xp"] = js[b], gs[b], xps[b]
        ctx.close_loop_stack(mt, LC.RLC)
        ref = [ctx.get_H(b) for b in range(B)]
        for b in range(B):
            for k in range(3):
                assert np.array_equal(off[b][k], ref[b][k]), (b, k)       # H, inn, diagR: the same bits
            assert not np.array_equal(on[b][0], ref[b][0]) and (on[b][2] == 1.0).all()
        ctx.lcmap_cov_config(point_cov=True)
        assert ctx.lcmap_get_cov().shape == (B, LC.MAP_MAX, 6)
        _config(ctx)                                                      # a new map configuration releases the arrays
        assert _status(ctx.lcmap_get_cov) == ERR_INVALID and _status(ctx.lcmap_cov_stats) == ERR_INVALID
