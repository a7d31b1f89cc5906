"""The resident landmark map on the GPU at its limits (tests/lcmap_edge_cases.py has the inputs, the 80-bit restatement and the
derived bounds; tests/test_lcmap_edges_cpu.py checks them on the host):
  A  capacity and launch shapes against MapRestate / VisitRestate, exact: the add kernel's duplicate search past one pass, the
     match kernel's chunks, all 64 lanes of the close kernel busy, the largest map
  B  Xs, Sigma, the row pairs, the innovation and gamma against the 80-bit restatement, under bounds()
  C  chi2, max_depth_var and min_matches straddled at value (1 -+ 1e-6), the two pivots of the plain kernel at their sign change
  D  pixels and stored points that are not finite: never kept, shown as a failed pivot, the frame and the update finite
Shapes: 4 groups, 8 features (N = 71), Context(N, 128, B), B <= 48."""
import numpy as np
import pytest

import lcmap_cov_restate as CR
import lcmap_edge_cases as E
import lcmap_restate as R
import map_restate as mr
import precise_ref as pr
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import scene_arrays
from test_lcmap_gpu import _adds, _queries
from xivo_amd import synth
from xivo_amd.lib import Context, FLAG_INVDEPTH, lcmap_entry_dtype

pytestmark = pytest.mark.gpu
LD = E.LD
NG, NF = E.NG, E.NF


def _open(sc, cam, P, inv=False, x=None, **cfg):
    lay = E.layout()
    B = sc["x"].shape[0]
    poses, groups, feats, _ = scene_arrays(sc, cam, xp=np.zeros((B, NF, 2)))
    if x is not None:
        feats["x"] = x
    ctx = Context(lay.N, E.M_MAX, B, flags=FLAG_INVDEPTH if inv else 0)
    ctx.set_layout(lay.N, lay.group_begin, NG, lay.feature_begin, NF, cam)
    ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
    _config(ctx, **cfg)
    return ctx


def _config(ctx, **kw):
    o = dict(map_max=8, lc_max=6, min_matches=1, Rlc=E.RLC, chi2=0.0, max_depth_var=0.0)
    o.update(kw)
    ctx.lcmap_config(o.pop("map_max"), **o)


def _load(ctx, keys, Xs, map_max, cov=None):
    """keys [B, n], Xs [B, n, 3] -> lcmap_set (and set_cov of Sigma [B, n, 3, 3])"""
    B, n = keys.shape
    ent = np.zeros((B, map_max), dtype=lcmap_entry_dtype)
    ent["key"][:, :n] = keys; ent["Xs"][:, :n] = Xs
    ctx.lcmap_set(ent, [n] * B)
    if cov is not None:
        c6 = np.zeros((B, map_max, 6))
        for b in range(B):
            for m in range(n):
                c6[b, m] = CR.pack6(cov[b, m])
        ctx.lcmap_set_cov(c6)


def _fam_queries(fam, xp=None, take=None):
    """every filter's pairs in order (take: {filter: how many})"""
    xp = fam["xp"] if xp is None else xp
    B, n = fam["keys"].shape
    return _queries([(b, int(fam["g"][b, m]), int(fam["keys"][b, m]), xp[b, m]) for b in range(B)
                     for m in range(n if take is None else take.get(b, n))])


def _rows(ctx, B):
    got = [ctx.get_H(b) for b in range(B)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got]), np.array([g[2] for g in got])


def _neutral(H, inn, dR, m):
    return not H[2 * m:2 * m + 2].any() and not inn[2 * m:2 * m + 2].any() and (dR[2 * m:2 * m + 2] == 1.0).all()


# ================================================================ A. capacity and launch shapes
@pytest.mark.parametrize("inv", [False, True])
@pytest.mark.parametrize("map_max", E.ADD_MAP_MAX)
def test_add_beyond_one_pass_of_the_duplicate_search(built, map_max, inv):
    import lcmap_cases as LC
    cam = synth.PINHOLE
    sc, x, _ = LC.scene(cam, invdepth=inv)
    B = LC.B
    P = np.array([E.spd(E.layout().N, 40 + b) * 1e-4 for b in range(B)])
    X80 = np.array([[mr.world_point(sc["Rbc"][b], sc["Tbc"][b], sc["gR"][b, sc["ref"][b, j]], sc["gT"][b, sc["ref"][b, j]], x[b, j], inv)
                     for j in range(NF)] for b in range(B)])
    want = [R.MapRestate(map_max, 6, 1) for _ in range(B)]
    with _open(sc, cam, P, inv, x=x, map_max=map_max) as ctx:
        for call in (0, 1):
            recs, dec = [], []
            for b in range(B):
                script = E.add_script(map_max, b)[call]
                recs += [(b, j, k) for j, k in script]
                dec.append(want[b].add([(k, True, False, j) for j, k in script]))
            ctx.lcmap_add(_adds(recs))
            if call == 1:
                assert all(d[:-1] == [R.DUP] * (len(d) - 1) and d[-1] == R.FULL for d in dec)      # stored keys on a full map; a new one
        ent, cnt = ctx.lcmap_get()
        st = ctx.lcmap_stats()
    assert cnt.tolist() == [map_max] * B
    worst = 0.0
    for b in range(B):
        assert ent["key"][b].tolist() == want[b].keys, b                   # keys in record order
        for k in ("added", "dup", "full", "poor", "skipped"):
            assert st[k][b] == want[b].stats[k], (b, k, int(st[k][b]), want[b].stats[k])
        js = [int(j) for j in want[b].Xs]                                  # (MapRestate keeps what add was given: the feature)
        worst = max(worst, E.xs_error(ent["Xs"][b], X80[b, js]))
    assert st["dup"].tolist() == [len(E.add_script(map_max, 0)[1]) - 1 + (2 if map_max == 130 else 0)] * B and st["full"].tolist() == [3] * B
    print("add map_max=%d inv=%d: worst |dXs| / |Xs| %.2e (bound %.2e)" % (map_max, inv, worst, E.bounds()["added"]["xs"]))
    assert worst <= E.bounds()["added"]["xs"]


@pytest.mark.parametrize("lc_max", E.MATCH_LC_MAX)
def test_match_across_chunks_of_64_queries(built, lc_max):
    cam = synth.PINHOLE
    B = len(E.MATCH_COUNTS)
    sc = E.base_scene(cam, B, 31)
    P = np.array([E.pose_prior(60 + b, 0.02, 0.05) for b in range(B)])
    keys = np.array([E.match_map_keys(b) for b in range(B)])
    rng = np.random.default_rng(5)
    Xs = np.zeros((B, E.MATCH_ENTRIES, 3))
    for b in range(B):
        for e in range(E.MATCH_ENTRIES):
            Xs[b, e], _ = E.place(sc, cam, b, -1, tuple(rng.uniform(-0.4, 0.4, 2)), rng.uniform(2, 8), 0.0)
    want = [R.MapRestate(E.MATCH_ENTRIES, lc_max, 1) for _ in range(B)]
    for b in range(B):
        want[b].keys = list(keys[b])
    with _open(sc, cam, P, map_max=E.MATCH_ENTRIES, lc_max=lc_max) as ctx:
        _load(ctx, keys, Xs, E.MATCH_ENTRIES)
        # first every list is filled to the last position, so that the second call has a tail to clear
        fill = [[int(keys[b, e]) for e in range(64)] for b in range(B)]
        script = [E.match_queries(lc_max, b) for b in range(B)]
        for call in (fill, script):
            qs = [(b, (i % (NG + 1)) - 1, k, (100.0 + i, 50.0 + b)) for b in range(B) for i, k in enumerate(call[b])]
            ctx.lcmap_close(_queries(qs), wait=False)
            mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
            for b in range(B):
                slots, lst = want[b].match(call[b])
                n = len(lst)
                assert mt["entry"][b].tolist() == [e for _, e in lst] + [-1] * (lc_max - n), (b, len(call[b]))
                assert mt["group_sind"][b, :n].tolist() == [(q % (NG + 1)) - 1 for q, _ in lst], b          # the query's own
                assert mt["xp"][b, :n].tolist() == [[100.0 + q, 50.0 + b] for q, _ in lst], b
                assert not mt["xp"][b, n:].any() and not mt["kept"][b, n:].any() and not mt["gamma"][b, n:].any(), b
                for k in ("queries", "matched", "surplus"):
                    assert st[k][b] == want[b].stats[k], (b, k, int(st[k][b]), want[b].stats[k])
        assert st["queries"].tolist() == [64 + n for n in E.MATCH_COUNTS]
        assert st["surplus"].sum() > 0 and (mt["entry"][1] == -1).all()     # the filter without a query, between two with 200


def _staged_update(stage, B, what):
    """test_update_accuracy_gpu._staged_update_check: the rows as staged, then the update of the same staging in a second
    context, against the extended-precision update on those rows"""
    ctx, P = stage()
    with ctx:
        rows = [ctx.get_H(b) for b in range(B)]
        mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
    ctx, _ = stage()
    with ctx:
        ctx.update_joseph()
        assert (ctx.get_status() == 0).all()
        Pn, err = ctx.download_P(), ctx.get_err()
    for b in range(B):
        H, inn, dR = rows[b]
        assert np.isfinite(H).all() and np.isfinite(inn).all()
        ref = pr.extended(H, P[b], inn, dR)
        rel, corr, dx = pr.check(ref, Pn[b], err[b], what=(what, b))
        print("staged update %s filter %d: rel %.3f corr %.3f dx %.3f x u (kappa + N), kappa %.1e" % (what, b, rel, corr, dx, ref.kappa))
    return rows, mt, st


def test_close_with_all_64_lanes_holding_a_pair(built):
    cam = synth.EQUI
    fam = E.family("nominal", "equi", nb=2, npairs=64)
    B = 2
    assert (fam["g"][:, 0::2] == -1).all() and (fam["g"][:, 1::2] >= 0).all()      # body pose and group slots alternate

    def stage(xp=None, wait=True, want_n=2):
        ctx = _open(fam["sc"], cam, fam["P"], map_max=130, lc_max=64, min_matches=64, chi2=E.CHI2)
        _load(ctx, fam["keys"], fam["Xs"], 130)
        n = ctx.lcmap_close(_fam_queries(fam, xp), wait=wait)
        assert n == (want_n if wait else None)
        return ctx, fam["P"]
    rows, mt, st = _staged_update(stage, B, "64 pairs")
    assert mt["kept"].all() and mt["entry"].tolist() == [list(range(64))] * 2 and st["closed_frames"].tolist() == [1, 1]
    for b in range(B):
        H, inn, dR = rows[b]
        assert H.shape == (128, E.layout().N) and (dR == E.RLC).all() and all(H[2 * m:2 * m + 2].any() for m in range(64))
        Ho, io, _ = R.rows(E.matches_of(fam, b), fam["sc"]["Rbc"][b], fam["sc"]["Tbc"][b], cam, E.layout(), 64, E.RLC)
        assert rel_fro(H, Ho) < 1e-12 and np.abs(inn - io).max() < 1e-9
    # one pixel of filter 0 out of the gate: 63 kept of 64 wanted - short, and every pair exactly neutral; filter 1 still closes
    xp = fam["xp"].copy(); xp[0, 37] += 400.0
    ctx, _ = stage(xp, want_n=1)
    with ctx:
        mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
        H, inn, dR = ctx.get_H(0)
        assert mt["kept"][0].sum() == 63 and mt["kept"][0, 37] == 0 and mt["gamma"][0, 37] > E.CHI2
        assert (st["short_frames"].tolist(), st["closed_frames"].tolist(), st["gated"].tolist()) == ([1, 0], [0, 1], [1, 0])
        assert not H.any() and not inn.any() and (dR == 1.0).all()
        assert ctx.get_H(1)[0].any()
        before = (ctx.download_P(), ) + tuple(a.copy() for a in ctx.get_scene())
        ctx.update_joseph(); ctx.absorb_error()
        after = (ctx.download_P(), ) + tuple(ctx.get_scene())
        assert np.array_equal(after[0][0], before[0][0]) and all(after[k][0].tobytes() == before[k][0].tobytes() for k in (1, 2, 3))
        assert not np.array_equal(after[0][1], before[0][1])
        # min_matches = 63: the same 63 kept close
        _config(ctx, map_max=130, lc_max=64, min_matches=63, chi2=E.CHI2); _load(ctx, fam["keys"], fam["Xs"], 130)
        assert ctx.lcmap_close(_fam_queries(fam, xp)) == 2
        H, inn, dR = ctx.get_H(0)
        assert [_neutral(H, inn, dR, m) for m in range(64)] == [m == 37 for m in range(64)]


def test_close_with_64_lanes_both_options_and_a_key_at_three_positions(built):
    cam = synth.EQUI
    fam = E.family("nominal", "equi", nb=2, npairs=64)
    B, gap = 2, 2
    rng = np.random.default_rng(9)
    Sg = np.array([[E.sigma_blob(rng) for _ in range(64)] for _ in range(B)])
    order = [list(range(61)) + [61, 61, 61],                       # 1: 64 positions, entry 61 at three of them: all fresh
             list(range(61)) + [61, 61, 61],                       # 2: all resting: rested
             [61, 62, 63, 61] + list(range(60))]                   # 3: entries 62 and 63 are new to the visit: two pairs take part
    rs = [CR.VisitRestate(130, 64, 64, gap) for _ in range(B)]
    for b in range(B):
        rs[b].add([int(k) for k in fam["keys"][b]])
    with _open(fam["sc"], cam, fam["P"], map_max=130, lc_max=64, min_matches=64, chi2=E.CHI2) as ctx:
        _load(ctx, fam["keys"], fam["Xs"], 130)
        ctx.lcmap_cov_config(point_cov=True, revisit_gap=gap)
        _load(ctx, fam["keys"], fam["Xs"], 130, cov=Sg)
        frames = []
        for t, ms in enumerate(order):
            qs = _queries([(b, int(fam["g"][b, m]), int(fam["keys"][b, m]), fam["xp"][b, m]) for b in range(B) for m in ms])
            ctx.lcmap_close(qs, wait=False)
            mt = ctx.lcmap_matches()
            assert mt["kept"].all(), t                                                # (inside the covariance)
            for b in range(B):
                res = rs[b].close([int(fam["keys"][b, m]) for m in ms], list(mt["kept"][b]))
                assert mt["entry"][b].tolist() == res["entries"] == ms, (t, b)
                assert mt["reserved"][b].tolist() == res["resting"], (t, b)
                H, inn, dR = ctx.get_H(b)
                assert [int(_neutral(H, inn, dR, m)) for m in range(64)] == res["neutral"], (t, b)
                assert (dR == 1.0).all() and np.isfinite(H).all()
                if b == 0:
                    frames.append(res["frame"])
            st, cst = ctx.lcmap_stats(), ctx.lcmap_cov_stats()
            for b in range(B):
                for k in ("gated", "short_frames", "closed_frames"):
                    assert st[k][b] == rs[b].stats[k], (t, b, k)
                for k in ("resting", "rested_frames"):
                    assert cst[k][b] == rs[b].stats[k], (t, b, k)
        assert frames == [CR.CLOSED, CR.RESTED, CR.CLOSED]
        assert cst["resting"].tolist() == [64 + 62] * 2 and cst["rested_frames"].tolist() == [1, 1] and not cst["bad_cov"].any()
        assert sum(1 - v for v in res["neutral"]) == 2


def test_the_largest_map(built):
    cam = synth.PINHOLE
    B, MM = 2, 4096
    sc = E.base_scene(cam, B, 33)
    P = np.array([E.pose_prior(70 + b, 0.02, 0.05) for b in range(B)])
    keys = np.array([[10 + 3 * e + b for e in range(MM)] for b in range(B)])
    Xs = np.zeros((B, MM, 3))
    for b in range(B):
        Xs[b] = E.place(sc, cam, b, -1, (0.1, -0.2), 4.0, 0.0)[0] + 1e-3 * np.arange(MM)[:, None]
    with _open(sc, cam, P, map_max=MM) as ctx:
        _load(ctx, keys, Xs, MM)
        qk = [lambda b: int(keys[b, 0]), lambda b: int(keys[b, 63]), lambda b: 5, lambda b: int(keys[b, 64]), lambda b: int(keys[b, MM - 1])]
        ctx.lcmap_close(_queries([(b, -1, f(b), (300.0, 200.0)) for b in range(B) for f in qk]), wait=False)
        mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
        assert mt["entry"].tolist() == [[0, 63, 64, MM - 1, -1, -1]] * B
        assert (st["queries"].tolist(), st["matched"].tolist(), st["surplus"].tolist()) == ([5] * B, [4] * B, [0] * B)
        ctx.lcmap_add(_adds([(b, j, k) for b in range(B) for j, k in ((0, int(keys[b, MM - 1])), (1, 7), (2, int(keys[b, 64])))]))
        ent, cnt = ctx.lcmap_get()
        st = ctx.lcmap_stats()
        assert cnt.tolist() == [MM] * B and (st["dup"].tolist(), st["full"].tolist(), st["added"].tolist()) == ([2] * B, [1] * B, [0] * B)
        assert np.array_equal(ent["key"], keys) and np.array_equal(ent["Xs"], Xs)


# ================================================================ B. accuracy against the 80-bit restatement
@pytest.mark.parametrize("inv", [False, True])
def test_added_points_and_covariances_within_the_derived_bounds(built, inv):
    c = E.xs_case(inv)
    s80 = E.sigma_case(inv)["S80"]
    b = E.bounds()["added"]
    with _open(c["sc"], synth.PINHOLE, c["P"], inv, x=c["x"]) as ctx:
        ctx.lcmap_cov_config(point_cov=True)
        ctx.lcmap_add(_adds([(f, j, 100 * f + j) for f in range(E.NB) for j in range(NF)]))
        (ent, cnt), cov = ctx.lcmap_get(), ctx.lcmap_get_cov()
    assert cnt.tolist() == [NF] * E.NB
    ex, es = E.xs_error(ent["Xs"], c["Xs80"]), E.sigma_error(cov, s80)
    print("added inv=%d: |dXs| / |Xs| %.2e (bound %.2e), Sigma %.2e (bound %.2e)" % (inv, ex, b["xs"], es, b["sigma"]))
    assert ex <= b["xs"] and es <= b["sigma"]


@pytest.mark.parametrize("inv", [False, True])
@pytest.mark.parametrize("camname", list(E.CAMS))
@pytest.mark.parametrize("name", E.FAMILIES)
def test_rows_innovation_and_gamma_within_the_derived_bounds(built, name, camname, inv):
    """aniso on the equidistant camera is the case that found the plain sums in R_e's entries: with them gamma on R_e of filter
    16, pair 5 (kappa_2(R_e) 2.5e5) was 5.48e-11 against the bound 4.26e-11; with lcmap_quad3 it is 3.8e-12."""
    fam, ref, bnd = E.family(name, camname), E.reference(name, camname), E.bounds()[name]
    cov = fam["Sigma"]
    with _open(fam["sc"], fam["cam"], fam["P"], inv) as ctx:
        def close(chi2):
            _config(ctx, chi2=chi2)
            _load(ctx, fam["keys"], fam["Xs"], 8)
            if cov is not None:
                ctx.lcmap_cov_config(point_cov=True)
                _load(ctx, fam["keys"], fam["Xs"], 8, cov=cov)
            ctx.lcmap_close(_fam_queries(fam), wait=False)
            return ctx.lcmap_matches()
        mt = close(0.0)
        H, inn, dR = _rows(ctx, E.NB)
        assert mt["kept"].all() and (mt["entry"] == np.arange(E.NP)).all()
        assert (dR == (1.0 if cov is not None else E.RLC)).all()
        err = E.errors(fam, ref, H, inn, mt["gamma"])
        print("device %s %s inv=%d: " % (name, camname, inv) + " ".join("%s %.2e (bound %.2e)" % (q, err[q], bnd[q]) for q in E.QUANTITIES))
        for q in E.QUANTITIES:
            assert err[q] <= bnd[q], (q, err[q], bnd[q])
        # the gate's decision at chi2: that of the 80-bit gamma (no gamma within 1e-6 of it: the CPU test)
        mt = close(E.CHI2)
        assert np.array_equal(mt["kept"] != 0, ref["gamma"].astype(np.float64) <= E.CHI2)
        assert ctx.lcmap_stats()["gated"].sum() == (mt["kept"] == 0).sum()


# ================================================================ C. thresholds and pivots
@pytest.mark.parametrize("camname", list(E.CAMS))
def test_chi2_just_above_and_just_below_a_gamma(built, camname):
    fam, ref = E.family("nominal", camname), E.reference("nominal", camname)
    with _open(fam["sc"], fam["cam"], fam["P"]) as ctx:
        for b, m in ((0, 2), (17, 5), (40, 1)):
            g80 = ref["gamma"][b, m]
            for chi2, kept in ((float(g80 * (1 + LD(E.OFF))), 1), (float(g80 * (1 - LD(E.OFF))), 0)):
                _config(ctx, chi2=chi2); _load(ctx, fam["keys"], fam["Xs"], 8)
                ctx.lcmap_close(_fam_queries(fam), wait=False)
                mt = ctx.lcmap_matches()
                assert mt["kept"][b, m] == kept and mt["gamma"][b, m] > 0, (b, m, chi2, mt["gamma"][b, m])
                assert np.array_equal(mt["kept"] != 0, ref["gamma"].astype(np.float64) <= chi2)       # every other match of the call too
            # the exact tie on this match: chi2 equal to the gamma read back keeps it, one ulp below gates it
            gd = float(mt["gamma"][b, m])
            for chi2, kept in ((gd, 1), (float(np.nextafter(gd, 0.0)), 0)):
                _config(ctx, chi2=chi2); _load(ctx, fam["keys"], fam["Xs"], 8)
                ctx.lcmap_close(_fam_queries(fam), wait=False)
                m2 = ctx.lcmap_matches()
                assert m2["gamma"][b, m] == gd and m2["kept"][b, m] == kept, (b, m, chi2)


def test_max_depth_var_just_above_and_just_below_a_variance(built):
    c = E.xs_case(False)
    lay = E.layout()
    j = 4
    with _open(c["sc"], synth.PINHOLE, c["P"], x=c["x"]) as ctx:
        for f, (bound, poor) in enumerate(((1 + E.OFF, 0), (1 - E.OFF, 1))):
            var = c["P"][f][lay.feature_begin + 3 * j + 2, lay.feature_begin + 3 * j + 2]
            _config(ctx, max_depth_var=var * bound)
            ctx.lcmap_add(_adds([(f, j, 1)]))
            st = ctx.lcmap_stats()
            assert (ctx.lcmap_get()[1][f], st["poor"][f], st["added"][f]) == (1 - poor, poor, 1 - poor), bound


def test_pivots_of_the_plain_kernel_at_their_sign_change(built):
    f = E.pivot_case()
    lay, cols = E.layout(), E.pair_cols(-1)
    N = lay.N
    with _open(f["sc"], f["cam"], np.array([np.eye(N) * 1e-6] * 2)) as ctx:
        def close(cs, chi2=0.0):
            _config(ctx, chi2=chi2); _load(ctx, f["keys"], f["Xs"], 8)
            ctx.upload_P(np.array([-c * np.eye(N) for c in cs]))
            ctx.lcmap_close(_fam_queries(f), wait=False)
            return ctx.lcmap_matches(), ctx.lcmap_stats()
        close((0.0, 0.0))
        H, inn, _ = _rows(ctx, 2)                                        # h0, h1 from the rows the device staged
        h = [H[b][0:2][:, cols] for b in range(2)]
        assert not np.delete(H[0][0:2], cols, axis=1).any()
        c_pos, c_neg, _ = E.pivot_cs(h[0])
        _, _, mid = E.pivot_cs(h[1])
        safe = 0.5 * E.RLC / float(h[1][1] @ h[1][1])
        assert mid is not None and E.pivots_ld(h[0], c_pos)[:2] == (True, True) and E.pivots_ld(h[0], c_neg)[:2] == (False, False)
        assert E.pivots_ld(h[1], mid)[:2] == (True, False) and E.pivots_ld(h[1], safe)[:2] == (True, True)
        # the non-positive side of either pivot: gamma = -1, not kept, counted
        mt, st = close((c_neg, mid))
        assert mt["gamma"][:, 0].tolist() == [-1.0, -1.0] and mt["kept"][:, 0].tolist() == [0, 0] and st["gated"].tolist() == [1, 1]
        assert st["short_frames"].tolist() == [1, 1]
        # the positive side: the pivots pass and gamma alone decides
        mt, st = close((c_pos, safe))
        g80 = [E.gamma_ld(E.pivots_ld(h[b], c)[2], inn[b][0:2].astype(LD)) for b, c in ((0, c_pos), (1, safe))]
        assert mt["kept"][:, 0].tolist() == [1, 1] and st["gated"].tolist() == [0, 0]
        for b in range(2):
            # S = Rlc I - c h h^T loses kappa_2(S) <= 1 / 1e-3 times the 2^-53 of its entries; a wide margin on top
            print("pivot filter %d: gamma %.6g, 80-bit %.6g" % (b, mt["gamma"][b, 0], float(g80[b])))
            assert abs(mt["gamma"][b, 0] / float(g80[b]) - 1) < 1e-9
        for side, kept in ((1 + E.OFF, 1), (1 - E.OFF, 0)):
            mt, st = close((c_pos, safe), chi2=float(g80[0] * LD(side)))
            assert mt["kept"][0, 0] == kept and mt["gamma"][0, 0] > 0 and st["gated"][0] == 1 - kept


@pytest.mark.parametrize("lc_max", [6, 64])
def test_one_fewer_than_min_matches_and_exactly_min_matches(built, lc_max):
    cam = synth.PINHOLE
    fam = E.family("nominal", "pinhole", nb=2, npairs=lc_max)
    xp = fam["xp"].copy(); xp[0, lc_max // 2] += 400.0                   # filter 0: lc_max - 1 kept; filter 1: lc_max kept
    with _open(fam["sc"], cam, fam["P"]) as ctx:
        for mm, closing in ((lc_max, [0, 1]), (lc_max - 1, [1, 1])):
            _config(ctx, map_max=lc_max, lc_max=lc_max, min_matches=mm, chi2=E.CHI2); _load(ctx, fam["keys"], fam["Xs"], lc_max)
            assert ctx.lcmap_close(_fam_queries(fam, xp)) == sum(closing)
            mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
            assert mt["kept"].sum(axis=1).tolist() == [lc_max - 1, lc_max]
            assert st["closed_frames"].tolist() == closing and st["short_frames"].tolist() == [1 - c for c in closing]
            for b in range(2):
                H, inn, dR = ctx.get_H(b)
                assert [_neutral(H, inn, dR, m) for m in range(lc_max)] == [not closing[b] or (b == 0 and m == lc_max // 2) for m in range(lc_max)]


# ================================================================ D. inputs that are not finite
BAD_PIXELS = ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0))             # one component replaced, the other kept (factor 1)


@pytest.mark.parametrize("chi2", [5.99, 0.0])
def test_a_match_that_is_not_finite_is_gated_and_the_update_stays_finite(built, chi2):
    """filters 0 - 2: six queries, the pixel of position 2 is (NaN, v), (u, NaN), (inf, v): the other five close; filters 3 - 5:
    the same with five queries: four kept, short; filter 6: the stored point of entry 1 has a NaN coordinate (closes on five);
    filter 7: entry 3 has an inf coordinate, five queries (short)"""
    cam = synth.EQUI
    fam = E.family("nominal", "equi", nb=8, npairs=6, seed=3)
    B, lay = 8, E.layout()
    xp, Xs = fam["xp"].copy(), fam["Xs"].copy()
    bad = {}
    for b in range(6):
        for k in range(2):
            if not np.isfinite(BAD_PIXELS[b % 3][k]):
                xp[b, 2, k] = BAD_PIXELS[b % 3][k]
        bad[b] = 2
    Xs[6, 1, 1] = np.nan; Xs[7, 3, 0] = np.inf
    bad[6], bad[7] = 1, 3
    take = {3: 5, 4: 5, 5: 5, 7: 5}
    closes = [b not in take for b in range(B)]

    def stage():
        ctx = _open(fam["sc"], cam, fam["P"], min_matches=5, chi2=chi2)
        _load(ctx, fam["keys"], Xs, 8)
        assert ctx.lcmap_close(_fam_queries(fam, xp, take)) == sum(closes)
        return ctx
    with stage() as ctx:
        mt, st = ctx.lcmap_matches(), ctx.lcmap_stats()
        rows = [ctx.get_H(b) for b in range(B)]
    for b in range(B):
        n = take.get(b, 6)
        want_kept = [int(m != bad[b]) for m in range(n)] + [0] * (6 - n)
        assert mt["kept"][b].tolist() == want_kept, (b, mt["kept"][b], mt["gamma"][b])
        assert mt["gamma"][b, bad[b]] == -1.0, (b, mt["gamma"][b])                  # as for a failed pivot
        assert (mt["gamma"][b, :n][np.arange(n) != bad[b]] > 0).all()
        assert st["gated"][b] == 1 and st["closed_frames"][b] == closes[b] and st["short_frames"][b] == 1 - closes[b]
        H, inn, dR = rows[b]
        assert np.isfinite(H).all() and np.isfinite(inn).all() and np.isfinite(dR).all(), b
        assert [_neutral(H, inn, dR, m) for m in range(6)] == [not closes[b] or m == bad[b] or m >= n for m in range(6)], b
    # the update, in a second context staged the same way
    with stage() as ctx:
        before = (ctx.download_P(), ) + tuple(a.copy() for a in ctx.get_scene())
        ctx.update_joseph()
        assert (ctx.get_status() == 0).all()
        dx = ctx.get_err()
        ctx.absorb_error()
        after = (ctx.download_P(), ) + tuple(ctx.get_scene())
    assert np.isfinite(after[0]).all() and np.isfinite(dx).all()
    xq = xp.copy(); xq[~np.isfinite(xq)] = 0.0                                        # (the oracle's rows of the bad pair are dropped below)
    fq = dict(fam, Xs=np.where(np.isfinite(Xs), Xs, fam["Xs"]))
    for b in range(B):
        if closes[b]:
            Ho, io, dRo = R.rows(E.matches_of(fq, b, xq), fam["sc"]["Rbc"][b], fam["sc"]["Tbc"][b], cam, lay, 6, E.RLC)
            Hn, in_n, dRn = R.neutralise(Ho, io, dRo, [m == bad[b] for m in range(6)])
            e_ref, P_ref, _ = orc.update_joseph(Hn, fam["P"][b], in_n, dRn)
            print("non-finite chi2=%.2f filter %d: rel. error P %.2e dx %.2e" % (chi2, b, rel_fro(after[0][b], P_ref), rel_fro(dx[b], e_ref)))
            assert rel_fro(after[0][b], P_ref) < TOL_P and rel_fro(dx[b], e_ref) < TOL_DX
            assert not np.array_equal(after[1][b], before[1][b])
        else:                                                                         # short: no bit of P or the scene changes
            assert np.array_equal(after[0][b], before[0][b]) and not dx[b].any()
            for k in (1, 2, 3):
                assert after[k][b].tobytes() == before[k][b].tobytes(), (b, k)
