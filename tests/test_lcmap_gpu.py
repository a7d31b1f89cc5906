"""The resident landmark map through the C ABI on the GPU (xivo_hip_lcmap_*): add, the rows, the verification, the update that
closes a loop, and the call that closes none - held against tests/lcmap_restate.py (whose rows are the oracle's
lc_jacobian_rows) and, for the rows, against xivo_hip_close_loop_stack bit for bit.
Shapes (tests/lcmap_cases.py): B = 3, 4 groups, 8 features (N = 71), Context(N, 16, 3), map_max 8, lc_max 6, min_matches 5."""
import numpy as np
import pytest

import lcmap_cases as LC
import lcmap_restate as R
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import scene_arrays, spd
from xivo_amd import synth
from xivo_amd.lib import (Context, FLAG_INVDEPTH, XivoHipError, lc_dtype, lcmap_add_dtype, lcmap_entry_dtype, lcmap_opts_dtype,
                          lcmap_query_dtype)

pytestmark = pytest.mark.gpu
B, NG, NF = LC.B, LC.NG, LC.NF
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def _open(cam, sc, x, P, inv=False, **kw):
    lay = LC.layout()
    poses, groups, feats, _ = scene_arrays(sc, cam, xp=np.zeros((B, NF, 2)))
    feats["x"] = x
    ctx = Context(lay.N, 16, B, flags=FLAG_INVDEPTH if inv else 0)
    ctx.set_layout(lay.N, lay.group_begin, NG, lay.feature_begin, NF, cam)
    ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
    _config(ctx, **kw)
    return ctx, (poses, groups, feats)


def _config(ctx, **kw):
    o = dict(lc_max=LC.LC_MAX, min_matches=LC.MIN_MATCHES, Rlc=LC.RLC, chi2=LC.CHI2, max_depth_var=0.0)
    o.update(kw)
    ctx.lcmap_config(o.pop("map_max", LC.MAP_MAX), **o)


def _adds(recs):
    a = np.zeros(len(recs), dtype=lcmap_add_dtype)
    for i, (b, j, k) in enumerate(recs):
        a[i]["b"], a[i]["feat"], a[i]["key"] = b, j, k
    return a


def _queries(qs):
    a = np.zeros(len(qs), dtype=lcmap_query_dtype)
    for i, (b, g, k, xp) in enumerate(qs):
        a[i]["b"], a[i]["group_sind"], a[i]["key"], a[i]["xp"] = b, g, k, xp
    return a


def _fill(ctx, n=NF):
    """every filter's first n features become map entries, key(b, j) each"""
    ctx.lcmap_add(_adds([(b, j, LC.key(b, j)) for b in range(B) for j in range(n)]))


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except XivoHipError as e:
        return e.status
    return 0


def _P(seed=40):
    return np.array([spd(LC.layout().N, seed + b) * 1e-4 for b in range(B)])


# ---------------------------------------------------------------- 1. add
@pytest.mark.parametrize("inv", [False, True])
def test_add_stores_the_world_point_in_record_order_and_counts(built, inv):
    cam = synth.PINHOLE
    sc, x, Xs = LC.scene(cam, invdepth=inv)
    lay, P = LC.layout(), _P()
    ctx, (poses, groups, feats) = _open(cam, sc, x, P, inv)
    with ctx:
        feats["sind"][1, 5] = -1                                         # a free slot of a ragged batch
        ctx.set_scene(poses, groups, feats)
        # filter 0: its eight features in a scrambled order fill the map exactly; one more is `full`, a stored key is `dup` even then
        # filter 1: a key twice in one call, a free slot, a negative key; filter 2: nothing in this call
        order0 = [3, 0, 7, 1, 6, 2, 5, 4]
        recs = [(0, j, LC.key(0, j)) for j in order0] + [(0, 2, 999), (0, 1, LC.key(0, 3))]
        recs += [(1, 3, 50), (1, 4, 50), (1, 5, 51), (1, 6, -7), (1, 0, 52)]
        ctx.lcmap_add(_adds(recs))
        ctx.lcmap_add(_adds([(1, 3, 52), (2, 1, 7)]))                    # a key stored by an earlier call; filter 2's first entry
        ent, cnt = ctx.lcmap_get()
        st = ctx.lcmap_stats()
        want = [R.MapRestate(LC.MAP_MAX, LC.LC_MAX, LC.MIN_MATCHES) for _ in range(B)]
        for b, j, k in recs + [(1, 3, 52), (2, 1, 7)]:
            want[b].add([(k, not (b == 1 and j == 5), False, Xs[b, j])])
        assert cnt.tolist() == [8, 2, 1] == [len(w.keys) for w in want]
        for b in range(B):
            assert ent["key"][b, :cnt[b]].tolist() == want[b].keys       # positions count, count + 1, ... in record order
            got, ref = ent["Xs"][b, :cnt[b]], np.array(want[b].Xs)
            print("add inv=%d filter %d: rel. error of Xs %.2e" % (inv, b, rel_fro(got, ref)))
            assert rel_fro(got, ref) < 1e-12
            for k in ("added", "dup", "full", "poor", "skipped"):
                assert st[k][b] == want[b].stats[k], (b, k)
        assert (st["added"].tolist(), st["dup"].tolist(), st["full"].tolist(), st["skipped"].tolist()) == ([8, 2, 1], [1, 2, 0], [1, 0, 0], [0, 2, 0])
        # set / get: whole maps round-trip, and a loaded map is matched like an added one
        ent2 = np.zeros((B, LC.MAP_MAX), dtype=lcmap_entry_dtype)
        ent2["key"] = np.arange(B * LC.MAP_MAX).reshape(B, -1) + 500; ent2["Xs"] = np.random.default_rng(1).normal(size=(B, LC.MAP_MAX, 3))
        ctx.lcmap_set(ent2, [8, 0, 3])
        e3, c3 = ctx.lcmap_get()
        assert c3.tolist() == [8, 0, 3] and np.array_equal(e3, ent2)
        ctx.lcmap_set(ent2[1:2], [5], b0=1)
        assert ctx.lcmap_get()[1].tolist() == [8, 5, 3]
        bad = ent2.copy(); bad["key"][0, 1] = bad["key"][0, 0]
        assert _status(ctx.lcmap_set, bad, [8, 0, 3]) == ERR_INVALID     # a key twice in one filter
        assert _status(ctx.lcmap_set, ent2, [9, 0, 3]) == ERR_INVALID


def test_add_depth_variance_at_the_bound_and_one_ulp_below(built):
    cam = synth.PINHOLE
    sc, x, _ = LC.scene(cam)
    lay, P = LC.layout(), _P()
    j = 4
    var = P[0][lay.feature_begin + 3 * j + 2, lay.feature_begin + 3 * j + 2]
    ctx, _ = _open(cam, sc, x, P, max_depth_var=var)
    with ctx:
        ctx.lcmap_add(_adds([(0, j, 1)]))
        assert ctx.lcmap_get()[1][0] == 1 and ctx.lcmap_stats()["poor"][0] == 0      # equal to the bound: kept
        _config(ctx, max_depth_var=float(np.nextafter(var, 0.0)))                    # (a new configuration empties the map)
        ctx.lcmap_add(_adds([(0, j, 1)]))
        st = ctx.lcmap_stats()
        assert ctx.lcmap_get()[1][0] == 0 and (st["poor"][0], st["added"][0]) == (1, 0)


# ---------------------------------------------------------------- 2. rows
@pytest.mark.parametrize("inv", [False, True])
@pytest.mark.parametrize("name", list(LC.CAMS))
def test_rows_equal_close_loop_stack_bit_for_bit_and_the_oracle(built, name, inv):
    cam = LC.CAMS[name]
    sc, x, Xs = LC.scene(cam, invdepth=inv)
    lay, P = LC.layout(), _P()
    rng = np.random.default_rng(3)
    js, gs = [1, 6, 3], [2, 0, 1]                                        # filter b: old feature js[b], observing group gs[b]
    # group slot gs[b] holds the body's own pose: the body-observed pair must equal the group-observed one, blocks moved
    for b in range(B):
        sc["gR"][b, gs[b]], sc["gT"][b, gs[b]] = sc["Rsb"][b], sc["Tsb"][b]
    assert all(sc["ref"][b, js[b]] != gs[b] for b in range(B))           # (the old feature's own anchor stays what it was)
    xps = [LC.pixel(cam, Xs[b, js[b]], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b]) + rng.normal(0, 1.5, 2) for b in range(B)]
    ctx, _ = _open(cam, sc, x, P, inv, min_matches=1, chi2=0.0)
    with ctx:
        ctx.lcmap_add(_adds([(b, js[b], LC.key(b, js[b])) for b in range(B)]))
        ctx.lcmap_close(_queries([(b, gs[b], LC.key(b, js[b]), xps[b]) for b in range(B)]), wait=False)
        grp = [ctx.get_H(b) for b in range(B)]
        assert ctx.lcmap_close(_queries([(b, -1, LC.key(b, js[b]), xps[b]) for b in range(B)])) == B
        body = [ctx.get_H(b) for b in range(B)]
        mt = np.zeros((B, LC.LC_MAX), dtype=lc_dtype); mt["feat"] = -1
        for b in range(B):
            mt[b, 0]["feat"], mt[b, 0]["group_sind"], mt[b, 0]["xp"] = js[b], gs[b], xps[b]
        ctx.close_loop_stack(mt, LC.RLC)
        ref = [ctx.get_H(b) for b in range(B)]
    for b in range(B):
        for k in range(3):
            assert np.array_equal(grp[b][k], ref[b][k]), (b, k)          # H, inn, diagR: the same bits
        go = lay.group_begin + 6 * gs[b]
        moved = grp[b][0].copy()
        moved[:, 0:6] = grp[b][0][:, go:go + 6]; moved[:, go:go + 6] = 0.0
        assert np.array_equal(body[b][0], moved) and np.array_equal(body[b][1], grp[b][1]) and np.array_equal(body[b][2], grp[b][2])
        for g_sind, got in ((gs[b], grp[b]), (-1, body[b])):
            m = dict(Xs=Xs[b, js[b]], Rsb=sc["Rsb"][b], Tsb=sc["Tsb"][b], g_sind=g_sind, xp=xps[b])
            Ho, io, dRo = R.rows([m], sc["Rbc"][b], sc["Tbc"][b], cam, lay, LC.LC_MAX, LC.RLC)
            assert got[0].shape == Ho.shape and rel_fro(got[0], Ho) < 1e-12 and np.abs(got[1] - io).max() < 1e-9
            assert np.array_equal(got[2], dRo)


# ---------------------------------------------------------------- 3. verify
def _verify_case(cam, seed=5):
    """filter 0: six matches, pixel 2 moved by 60 px; filter 1: six, pixels 1 and 4 moved; filter 2: six keys no map holds"""
    sc, x, Xs = LC.scene(cam)
    rng = np.random.default_rng(seed)
    qs = []
    for b in range(B):
        for j in range(6):
            xp = LC.pixel(cam, Xs[b, j], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b]) + rng.normal(0, 0.3, 2)
            if (b, j) in ((0, 2), (1, 1), (1, 4)):
                xp = xp + 60.0
            qs.append((b, -1, LC.key(b, j) if b < 2 else 7000 + j, xp))
    return sc, x, Xs, qs


def test_verify_gates_counts_and_decides(built):
    cam = synth.EQUI
    sc, x, Xs, qs = _verify_case(cam)
    lay, P = LC.layout(), _P(60)
    ctx, _ = _open(cam, sc, x, P)
    with ctx:
        _fill(ctx)
        assert ctx.lcmap_close(_queries(qs)) == 1
        mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
        rows = [ctx.get_H(b) for b in range(B)]
        assert mt["entry"].tolist() == [list(range(6)), list(range(6)), [-1] * 6]
        assert mt["kept"][0].tolist() == [1, 1, 0, 1, 1, 1] and mt["kept"][1].tolist() == [1, 0, 1, 1, 0, 1]
        for k, want in (("queries", [6, 6, 6]), ("matched", [6, 6, 0]), ("surplus", [0, 0, 0]), ("gated", [1, 2, 0]),
                        ("short_frames", [0, 1, 0]), ("closed_frames", [1, 0, 0])):
            assert st[k].tolist() == want, k
        worst = 0.0
        for b in range(2):
            ms = [dict(Xs=Xs[b, j], Rsb=sc["Rsb"][b], Tsb=sc["Tsb"][b], g_sind=-1, xp=qs[6 * b + j][3]) for j in range(6)]
            Ho, io, dRo = R.rows(ms, sc["Rbc"][b], sc["Tbc"][b], cam, lay, LC.LC_MAX, LC.RLC)
            g = np.array([R.gamma(Ho[2 * m:2 * m + 2], P[b], io[2 * m:2 * m + 2], LC.RLC) for m in range(6)])
            worst = max(worst, np.abs(mt["gamma"][b] / g - 1).max())
            assert np.array_equal(mt["kept"][b] != 0, g <= LC.CHI2)
            m = R.MapRestate(LC.MAP_MAX, LC.LC_MAX, LC.MIN_MATCHES); m.keys = list(range(6))
            frame, neutral = m.decide(list(g <= LC.CHI2))
            Hn, inn_n, dRn = R.neutralise(Ho, io, dRo, neutral)
            assert rel_fro(rows[b][0], Hn) < 1e-12 and np.abs(rows[b][1] - inn_n).max() < 1e-9 and np.array_equal(rows[b][2], dRn)
            # neutral means exactly zero: the moved pair of filter 0, every pair of the short filter
            for p in np.nonzero(neutral)[0]:
                assert not rows[b][0][2 * p:2 * p + 2].any() and not rows[b][1][2 * p:2 * p + 2].any()
        print("verify: worst rel. error of gamma %.2e" % worst)
        assert worst < 1e-9                                               # (the bound the MH-distance tests hold dist to)
        assert not rows[2][0].any() and not rows[2][1].any() and (rows[2][2] == 1.0).all()
        # tie: chi2 equal to a gamma read back keeps that match, one ulp below gates it
        g3 = float(mt["gamma"][0, 3])
        for chi2, kept in ((g3, 1), (float(np.nextafter(g3, 0.0)), 0)):
            _config(ctx, chi2=chi2, min_matches=1); _fill(ctx)
            ctx.lcmap_close(_queries(qs))
            m2 = ctx.lcmap_matches()
            assert m2["gamma"][0, 3] == g3 and m2["kept"][0, 3] == kept, chi2
        # eight matching queries: the first six in query order, two surplus
        _config(ctx, chi2=0.0, min_matches=1); _fill(ctx)
        q8 = [(0, -1, LC.key(0, j), qs[0][3]) for j in (5, 7, 0, 6, 2, 1, 4, 3)]
        ctx.lcmap_close(_queries(q8 + [(1, -1, 12345, qs[6][3])]))
        m3, s3 = ctx.lcmap_matches(), ctx.lcmap_stats()
        assert m3["entry"][0].tolist() == [5, 7, 0, 6, 2, 1] and (s3["surplus"][0], s3["matched"][0], s3["queries"][0]) == (2, 6, 8)
        assert m3["entry"][1].tolist() == [-1] * 6 and s3["queries"][1] == 1


# ---------------------------------------------------------------- 4. update
@pytest.mark.parametrize("name", ["pinhole", "equi"])
def test_update_closes_one_filter_and_leaves_the_others_alone(built, name):
    cam = LC.CAMS[name]
    c = LC.update_case(cam)
    sc, lay, P = c["sc"], LC.layout(), c["P"]
    ctx, (poses, groups, feats) = _open(cam, sc, c["x"], P)
    with ctx:
        _fill(ctx)                                                        # the points, stored from the unperturbed scene
        for b in range(B):
            poses[b]["Rsb"] = c["Rsb_p"][b].T.reshape(-1); poses[b]["Tsb"] = c["Tsb_p"][b]
        ctx.set_scene(poses, groups, feats)
        before = (ctx.download_P(), ) + tuple(a.copy() for a in ctx.get_scene())
        assert ctx.lcmap_close(_queries([(b, -1, k, xp) for b, k, xp in c["queries"]])) == 1
        st = ctx.lcmap_stats()
        assert (st["closed_frames"].tolist(), st["short_frames"].tolist(), st["matched"].tolist()) == ([1, 0, 0], [0, 1, 0], [6, 4, 0])
        ctx.update_joseph()
        assert (ctx.get_status() == 0).all()
        dx = ctx.get_err()
        ctx.absorb_error()
        after = (ctx.download_P(), ) + tuple(ctx.get_scene())
    ms = [dict(Xs=c["Xs"][0, j], Rsb=c["Rsb_p"][0], Tsb=c["Tsb_p"][0], g_sind=-1, xp=c["queries"][j][2]) for j in range(6)]
    Ho, io, dRo = R.rows(ms, sc["Rbc"][0], sc["Tbc"][0], cam, lay, LC.LC_MAX, LC.RLC)
    e_ref, P_ref, _ = orc.update_joseph(Ho, P[0], io, dRo)
    print("update %s: rel. error P %.2e dx %.2e" % (name, rel_fro(after[0][0], P_ref), rel_fro(dx[0], e_ref)))
    assert rel_fro(after[0][0], P_ref) < TOL_P and rel_fro(dx[0], e_ref) < TOL_DX
    assert not np.array_equal(after[1][0], before[1][0])                  # the closing filter's pose moved
    for b in (1, 2):                                                      # short / no match: nothing changed by a bit
        assert np.array_equal(after[0][b], before[0][b]) and not dx[b].any()
        for k in (1, 2, 3):
            assert after[k][b].tobytes() == before[k][b].tobytes(), (b, k)


# ---------------------------------------------------------------- 5. no closing filter, refusals
def test_no_closing_filter_stages_nothing_and_config_refuses(built):
    cam = synth.PINHOLE
    sc, x, Xs, qs = _verify_case(cam)
    lay = LC.layout()
    Ps, H, inn, dR = synth.s_level(lay.N, 8, B, seed=2)
    ctx, _ = _open(cam, sc, x, Ps)
    with ctx:
        _fill(ctx)
        ctx.set_measurements(H, inn, dR)
        rows = [ctx.get_H(b) for b in range(B)]
        short = [q for q in qs if q[0] == 1][:4] + [q for q in qs if q[0] == 2]     # four matches: short; no match
        assert ctx.lcmap_close(_queries(short)) == 0
        for b in range(B):
            got = ctx.get_H(b)
            assert all(np.array_equal(got[k], rows[b][k]) for k in range(3))       # the frame's rows as before
        assert ctx.lcmap_stats()["short_frames"].tolist() == [0, 1, 0]
        ctx.lcmap_close(_queries(short), wait=False)                                # without the count: always stages
        assert ctx.get_H(0)[0].shape[0] == 2 * LC.LC_MAX and not ctx.get_H(1)[0].any()
        # refusals of config, each with its status; the map stays as it was through all of them
        for kw, want in ((dict(map_max=4097), ERR_UNSUPPORTED), (dict(lc_max=65), ERR_UNSUPPORTED), (dict(lc_max=9), ERR_INVALID),
                         (dict(Rlc=0.0), ERR_INVALID), (dict(Rlc=-1.0), ERR_INVALID), (dict(min_matches=0), ERR_INVALID)):
            assert _status(_config, ctx, **kw) == want, kw
        assert ctx.lcmap_get()[1].tolist() == [8, 8, 8]
        o = np.zeros(1, dtype=lcmap_opts_dtype)                                    # a struct of another size
        o["struct_size"] = lcmap_opts_dtype.itemsize - 8; o["map_max"] = 8; o["lc_max"] = 6; o["min_matches"] = 5; o["Rlc"] = 1.0
        assert ctx.lib.xivo_hip_lcmap_config(ctx.h, o.ctypes.data) == ERR_INVALID
        _config(ctx, map_max=0)                                                     # releases: every other entry point is INVALID again
        assert _status(ctx.lcmap_add, _adds([(0, 0, 1)])) == ERR_INVALID and _status(ctx.lcmap_close, _queries(short)) == ERR_INVALID
        assert _status(ctx.lcmap_stats) == ERR_INVALID and _status(ctx.lcmap_get) == ERR_INVALID and _status(ctx.lcmap_matches) == ERR_INVALID
    cl = orc.calib_layout(NG, NF, True, True, 4)                                    # a context with online calibration
    with Context(cl.N, 16, B) as c2:
        c2.set_layout(cl.N, cl.group_begin, NG, cl.feature_begin, NF, cam)
        c2.set_calib(cl.td, cl.Cg, cl.cam_begin, cl.cam_dim)
        assert _status(_config, c2) == ERR_UNSUPPORTED
        assert _status(c2.lcmap_stats) == ERR_INVALID                               # before any configuration
