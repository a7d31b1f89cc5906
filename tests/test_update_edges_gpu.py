"""The measurement update (Estimator::UpdateJosephForm, src/estimator.cpp:1257-1288) on both sides of every admission limit
of the route table (plan_update in xivo_amd/csrc/capi_update.hip) and of the one-kernel update's instantiations (fused_pick /
fused_variant in xivo_amd/csrc/fused_update.hip), against the oracle.

Each case names the shape it means - block rows of the factor nb = round16(M) / 16, column blocks of the state
nwl = round16(N) / 16, common columns nc and private columns per row pair pw of the row-pair compressed H - and the test
first checks that the compressed form of its generated H really has those values (xivo_hip_selftest_host_compress), so a
case cannot drift onto another route unnoticed. Then: status 0, no L D L^T fallback, the route the table names, for the
one-kernel route the exact kernel label (the FLAG_PROFILE stage record), P+ within TOL_P, dx within TOL_DX, P+ exactly
symmetric; and in addition P+ (relative and in units of the prior correlation) and dx against the extended-precision reference
of tests/precise_ref.py within 8 u (kappa_2(S) + N). tests/test_dropin_cpu.py checks on the host that EDGE_CASES reaches every
instantiation the admission test can pick, and that every fused case's label is the one the library would launch."""
import zlib

import ctypes as C
import numpy as np
import pytest

import precise_ref as pr
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd import synth
from xivo_amd.lib import (Context, XivoHipError, FLAG_PROFILE, FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE)

pytestmark = pytest.mark.gpu

FU = "fused_update_f64_kernel<%s>"
LAT = "trsm_stream_f64_kernel<%d,1,4>"          # latency route (<= 64 filters, <= 14 block rows): streamed solve, four waves
MT, TP = FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE

# name, N, M, nb, nwl, nc, pw (an int, or one per filter), B, flags, route, trsm_gain kernel, entry points, source of H.
# Entry points: "j" xivo_hip_update_joseph, "g" xivo_hip_update_dense_gated (F = M / 2, two features pushed out of the gate),
# "h" xivo_hip_update_joseph_host (the drop-in, one filter). Source: "gen" the generator below, "slevel" synth.s_level (its
# rows: 12 common + 6 private columns per pair), "dense" a dense U(-1, 1) H (every column common).
EDGE_CASES = [
    # ---- factor vs state: the in-LDS Cholesky gives block row i to wave i, so the one-kernel route needs nb <= nwl
    ("slevel_48_64",     48,  64, 4, 3, 12, 6, 3, 0, "sparse_whitened", LAT % 4, "jgh", "slevel"),
    ("slevel_80_112",    80, 112, 7, 5, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "jg", "slevel"),
    ("slevel_96_112",    96, 112, 7, 6, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "jg", "slevel"),
    ("dense_12_32",      12,  32, 2, 1, 12, 0, 3, 0, "sparse_whitened", LAT % 4, "jg", "dense"),
    ("dense_12_64",      12,  64, 4, 1, 12, 0, 3, 0, "sparse_whitened", LAT % 4, "jg", "dense"),
    ("nb_eq_nwl_64_64",  64,  64, 4, 4, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "jgh", "gen"),
    ("nb_gt_nwl_64_80",  64,  80, 5, 4, 12, 6, 3, 0, "sparse_whitened", LAT % 6, "jg", "gen"),
    ("nb_eq_nwl_112_112", 112, 112, 7, 7, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "jg", "gen"),
    ("nb_eq_nwl_97_112",  97, 112, 7, 7, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("nb_gt_nwl_96_112",  96, 112, 7, 6, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "j", "gen"),
    ("nb_gt_nwl_16_32",   16,  32, 2, 1, 12, 2, 3, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    # ---- the instantiations: factor height 64 | 66 (nb 4 -> 5) and 112 | 114 (nb 7 -> 8)
    ("m64_150",         150,  64, 4, 10, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "jg", "gen"),
    ("m66_150",         150,  66, 5, 10, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "jg", "gen"),
    ("m112_150",        150, 112, 7, 10, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("m114_150",        150, 114, 8, 10, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "j", "gen"),
    # state width 192 | 193 at nb 5..7 (nwl 12 -> 13)
    ("n192_m80_pw9",    192,  80, 5, 12, 12, 9, 3, 0, "fused", FU % "7,12,48,1,9", "jg", "gen"),
    ("n193_m80_pw9",    193,  80, 5, 13, 12, 9, 3, 0, "sparse_whitened", LAT % 6, "j", "gen"),
    ("n192_m96",        192,  96, 6, 12, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("n192_m112",       192, 112, 7, 12, 12, 6, 3, 0, "fused", FU % "7,12,32,2,9", "jg", "gen"),
    ("n193_m112",       193, 112, 7, 13, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "j", "gen"),
    # state width 256 | 257 at nb <= 4
    ("n256_m64",        256,  64, 4, 16, 12, 6, 3, 0, "fused", FU % "4,16,32,1,9", "jg", "gen"),
    ("n257_m64",        257,  64, 4, 17, 12, 6, 3, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    ("n256_m32_pw9",    256,  32, 2, 16, 12, 9, 3, 0, "fused", FU % "4,16,64,1,9", "jg", "gen"),
    ("n257_m32_pw9",    257,  32, 2, 17, 12, 9, 3, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    # common columns 12 | 13
    ("nc12",            150,  60, 4, 10, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "j", "gen"),
    ("nc13",            150,  60, 4, 10, 13, 6, 3, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    # private columns 9 | 10 (the kernel's slots), 6 | 7 (six- vs nine-slot instantiation)
    ("pw9_m100",        150, 100, 7, 10, 12, 9, 3, 0, "fused", FU % "7,12,48,2,9", "jg", "gen"),
    ("pw10_m100",       150, 100, 7, 10, 12, 10, 3, 0, "sparse_whitened", LAT % 8, "j", "gen"),
    ("pw9_m60",         150,  60, 4, 10, 12, 9, 3, 0, "fused", FU % "4,16,64,2,9", "jg", "gen"),
    ("pw10_m60",        150,  60, 4, 10, 12, 10, 3, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    ("pw6_m100",        150, 100, 7, 10, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("pw7_m100",        150, 100, 7, 10, 12, 7, 3, 0, "fused", FU % "7,12,48,2,9", "j", "gen"),
    ("pw6_m60",         203,  60, 4, 13, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "j", "gen"),
    ("pw7_m60",         203,  60, 4, 13, 12, 7, 3, 0, "fused", FU % "4,16,64,2,9", "j", "gen"),
    # the LDS fallbacks: the 64-wide slab -> 32 (M 64: Np 224 | 240), the 48-wide -> 32 (M 112: Np 160 | 176)
    ("xc64_n224",       224,  64, 4, 14, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "j", "gen"),
    ("xc32_n225",       225,  64, 4, 15, 12, 6, 3, 0, "fused", FU % "4,16,32,1,9", "j", "gen"),
    ("xc48_n160",       160, 112, 7, 10, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("xc32_n161",       161, 112, 7, 11, 12, 6, 3, 0, "fused", FU % "7,12,32,2,9", "jg", "gen"),
    # the gather staging: two units per wave -> one (nine slots: M 48 at Np 144 | 160, M 80 at Np 160 | 176, M 16 at 32 | 48)
    ("gd2_n144_m48",    144,  48, 3, 9, 12, 9, 3, 0, "fused", FU % "4,16,64,2,9", "j", "gen"),
    ("gd1_n145_m48",    145,  48, 3, 10, 12, 9, 3, 0, "fused", FU % "4,16,64,1,9", "jg", "gen"),
    ("gd2_n160_m80",    160,  80, 5, 10, 12, 9, 3, 0, "fused", FU % "7,12,48,2,9", "j", "gen"),
    ("gd1_n161_m80",    161,  80, 5, 11, 12, 9, 3, 0, "fused", FU % "7,12,48,1,9", "j", "gen"),
    ("gd2_n32_m16",      32,  16, 1, 2, 4, 7, 3, 0, "fused", FU % "4,16,64,2,9", "j", "gen"),
    ("gd1_n33_m16",      33,  16, 1, 3, 4, 7, 3, 0, "fused", FU % "4,16,64,1,9", "j", "gen"),
    # odd M: the last pair has one row
    ("odd_m61",         150,  61, 4, 10, 12, 6, 3, 0, "fused", FU % "4,16,64,2,6", "j", "gen"),
    ("odd_m65",         150,  65, 5, 10, 12, 6, 3, 0, "fused", FU % "7,12,48,2,6", "j", "gen"),
    ("odd_m111_pw9",    150, 111, 7, 10, 12, 9, 3, 0, "fused", FU % "7,12,48,2,9", "j", "gen"),
    ("odd_m113",        150, 113, 8, 10, 12, 6, 3, 0, "sparse_whitened", LAT % 8, "j", "gen"),
    # ---- the route table behind the one-kernel route
    # trsm_forms_T: the update inside the solve kernel up to nb 11 and Np 256 (more than 64 filters, or THROUGHPUT_ROUTE)
    ("formsT_nb11",     200, 176, 11, 13, 12, 6, 3, TP, "sparse_in_solve", "trsm_lds_f64_kernel<11,4>", "j", "gen"),
    ("formsT_nb12",     200, 192, 12, 13, 12, 6, 3, TP, "sparse_whitened", "trsm_stream_f64_kernel<14,1>", "j", "gen"),
    ("formsT_np256",    256, 144, 9, 16, 12, 6, 3, TP, "sparse_in_solve", "trsm_lds_f64_kernel<10,4>", "j", "gen"),
    ("formsT_np272",    257, 144, 9, 17, 12, 6, 3, TP, "sparse_whitened", "trsm_lds_f64_kernel<10,5>", "j", "gen"),
    # trsm_latency_route: nb 14 | 15 at few filters, and a call batch of 64 | 65 filters
    ("latency_nb14",    256, 224, 14, 16, 12, 6, 3, 0, "sparse_whitened", LAT % 14, "j", "gen"),
    ("latency_nb15",    256, 240, 15, 16, 12, 6, 3, 0, "sparse_whitened", "trsm_stream_f64_kernel<19,1>", "j", "gen"),
    ("latency_b64",     200, 144, 9, 13, 12, 6, 64, 0, "sparse_whitened", LAT % 14, "j", "gen"),
    ("latency_b65",     200, 144, 9, 13, 12, 6, 65, 0, "sparse_in_solve", "trsm_lds_f64_kernel<10,4>", "j", "gen"),
    # stream8: a state wider than 256 with at most eight block rows takes the eight-wave streamed solve
    ("stream8_nb8",     300, 128, 8, 19, 12, 6, 3, TP, "sparse_whitened", "trsm_stream_f64_kernel<8,1>", "j", "gen"),
    ("stream8_nb9",     300, 144, 9, 19, 12, 6, 3, TP, "sparse_whitened", "trsm_lds_f64_kernel<10,5>", "j", "gen"),
    # the narrow seven-block solve (trsm_narrow_supported): ten waves to Np 160, twelve to 192, the general kernel beyond
    ("narrow_np160",    160, 112, 7, 10, 12, 6, 3, MT | TP, "sparse_in_solve", "trsm_lds_f64_kernel<7,4,10,3>", "j", "gen"),
    ("narrow_np176",    161, 112, 7, 11, 12, 6, 3, MT | TP, "sparse_in_solve", "trsm_lds_f64_kernel<7,4,12,3>", "j", "gen"),
    ("narrow_np192",    192, 112, 7, 12, 12, 6, 3, MT | TP, "sparse_in_solve", "trsm_lds_f64_kernel<7,4,12,3>", "j", "gen"),
    ("narrow_np208",    193, 112, 7, 13, 12, 6, 3, MT | TP, "sparse_in_solve", "trsm_lds_f64_kernel<10,4>", "j", "gen"),
    # the largest factor a context is built for: round16(M_max) / 16 = 24 (test_create_factor_limit: 25 is refused)
    ("factor_nb24",      64, 384, 24, 4, 12, 6, 2, 0, "sparse_whitened", "trsm_stream_f64_kernel<24,1>", "j", "gen"),
    # ---- batches: one filter, and one filter across a boundary that takes the whole batch with it
    ("b1_fused",        203,  60, 4, 13, 12, 6, 1, 0, "fused", FU % "4,16,64,2,6", "jg", "gen"),
    ("b1_nb_gt_nwl",     64,  80, 5, 4, 12, 6, 1, 0, "sparse_whitened", LAT % 6, "j", "gen"),
    ("batch_one_pw10",  150, 100, 7, 10, 12, (9, 9, 10, 9, 6), 5, 0, "sparse_whitened", LAT % 8, "jg", "gen"),
    ("batch_one_nc13",  150,  60, 4, 10, (12, 12, 12, 13), 6, 4, 0, "sparse_whitened", LAT % 4, "j", "gen"),
    ("batch_one_pw7",   150, 100, 7, 10, 12, (6, 6, 7, 6), 4, 0, "fused", FU % "7,12,48,2,9", "jg", "gen"),
    ("batch_one_pw10_b8", 203, 60, 4, 13, 12, (6, 9, 6, 6, 6, 6, 10, 6), 8, 0, "sparse_whitened", LAT % 4, "j", "gen"),
]
CASES = {c[0]: c for c in EDGE_CASES}
_REFS = {}                    # (case, gated) -> the extended-precision references of its distinct filters
GATE = (5.991, 1.1, 5)        # MH threshold, relaxation, min inliers (src/update.cpp:60-96)
R = 2.25


def _per_filter(v, B):
    return list(v) if isinstance(v, tuple) else [v] * B


def edge_inputs(case):
    """P [B, N, N], H [B, M, N], inn [B, M], dR [B, M] of a case. The generator's rows: every pair names the first nc
    columns, and pw private columns of its own, taken cyclically from the rest (so no private column is named by more than
    half of the pairs); entries N(0, 3^2). Batches above eight filters repeat eight distinct ones."""
    name, N, M, nb, nwl, nc, pw, B, flags, route, kern, entries, src = case
    seed = zlib.crc32(name.encode())
    nd = min(B, 8)
    if src == "slevel":
        P, H, inn, dR = synth.s_level(N, M // 2, nd, seed=seed)
    else:
        rng = np.random.default_rng(seed)
        A = rng.uniform(-1, 1, size=(nd, N, N))
        P = A @ np.transpose(A, (0, 2, 1)) / N + 1e-3 * np.eye(N)[None]
        H = np.zeros((nd, M, N))
        ncs, pws = _per_filter(nc, nd), _per_filter(pw, nd)
        for b in range(nd):
            if src == "dense":
                H[b] = rng.uniform(-1, 1, size=(M, N))
                continue
            pool = np.arange(ncs[b], N)
            for p in range((M + 1) // 2):
                cols = list(range(ncs[b])) + [int(pool[(p * pws[b] + t) % len(pool)]) for t in range(pws[b])]
                rows = slice(2 * p, min(2 * p + 2, M))
                H[b][rows, cols] = rng.normal(0, 3.0, size=(H[b][rows].shape[0], len(cols)))
        inn = rng.normal(0, 1.5, size=(nd, M))
        dR = np.full((nd, M), R)
    idx = np.arange(B) % nd
    return P[idx].copy(), H[idx].copy(), inn[idx].copy(), dR[idx].copy()


def compressed_form(lib, Hb, M_max=None):
    """(nc, pw, over) of one filter's H [M, N] under the library's own host compressor (the format of ell.h)"""
    M, N = Hb.shape
    pairs_clear = (M if M_max is None else M_max) // 2 + 8
    Hc = np.asfortranarray(Hb)
    idx = np.zeros((pairs_clear, 28), dtype=np.int32)
    val = np.zeros((pairs_clear, 28, 2))
    nc, pw = C.c_int(-1), C.c_int(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    over = lib.xivo_hip_selftest_host_compress(p(Hc), M, M, N, pairs_clear, p(idx), p(val), C.byref(nc), C.byref(pw))
    return nc.value, pw.value, over


def check_intent(lib, case, H):
    """The shape really is the one the case names: nb, nwl from the sizes, nc, pw per filter from the compressed rows."""
    name, N, M, nb, nwl, nc, pw, B, *_ = case
    assert ((M + 15) // 16, (N + 15) // 16) == (nb, nwl), name
    ncs, pws = _per_filter(nc, B), _per_filter(pw, B)
    for b in range(B):
        assert compressed_form(lib, H[b]) == (ncs[b], pws[b], 0), (name, b, compressed_form(lib, H[b]), ncs[b], pws[b])


def _expand():
    return [pytest.param(c[0], e, id="%s-%s" % (c[0], e)) for c in EDGE_CASES for e in c[11]]


@pytest.mark.parametrize("name,entry", _expand())
def test_update_at_the_edges(built, name, entry):
    case = CASES[name]
    _, N, M, nb, nwl, nc, pw, B, flags, route, kern, _, _ = case
    P, H, inn, dR = edge_inputs(case)
    gated = entry == "g"
    if entry == "h":
        B = 1
    from xivo_amd.lib import load_library
    check_intent(load_library(), case, H)
    F = M // 2
    if gated:
        assert M % 2 == 0 and F > GATE[2]
        inn[:, 4:8] *= 1e4                                      # features 2 and 3 of every filter fail the gate
    Pn = np.empty((B, N, N))
    with Context(N, M, B, flags=flags | FLAG_PROFILE) as ctx:
        if entry == "h":
            Pio = np.asfortranarray(P[0].copy())
            err, rc = ctx.update_joseph_host(H[0], inn[0], dR[0], Pio)
            assert rc == 0
            Pn[0], err = Pio, err[None]
        else:
            ctx.upload_P(P)
            ctx.set_measurements(H, inn, dR)
            if gated:
                ctx.update_dense_gated(F, R, *GATE)
                mask, dist = ctx.get_gate(F, B)
            else:
                ctx.update_joseph()
            Pn, err = ctx.download_P(), ctx.get_err()
        got_route, got_kern = ctx.last_route(), ctx.profile_get()["trsm_gain"]["kernel"]
        st, used = ctx.get_status(0, B, check=False), ctx.get_ldlt_used(0, B)
    print("%s-%s: route %s, kernel %s" % (name, entry, got_route, got_kern))
    assert (st == 0).all() and not used.any(), (st, used)
    assert got_route == route, (got_route, route)
    assert got_kern == kern, (got_kern, kern)
    for b in range(B):
        if gated:
            d_ref = orc.mh_distances(H[b].reshape(F, 2, N), P[b], inn[b].reshape(F, 2), R)
            m_ref = np.asarray(orc.mh_gate(d_ref, *GATE)[0]).astype(bool)
            assert np.array_equal(mask[b].astype(bool), m_ref) and not m_ref[2:4].any()
            assert np.allclose(dist[b], d_ref, rtol=1e-9, atol=0)
            keep = np.repeat(m_ref, 2)
            e_ref, P_ref, _ = orc.update_joseph(H[b][keep], P[b], inn[b][keep], dR[b][keep])
        else:
            e_ref, P_ref, _ = orc.update_joseph(H[b], P[b], inn[b], dR[b])
        assert rel_fro(Pn[b], P_ref) < TOL_P, (b, rel_fro(Pn[b], P_ref))
        assert rel_fro(err[b], e_ref) < TOL_DX, (b, rel_fro(err[b], e_ref))
        assert np.array_equal(Pn[b], Pn[b].T)
    # the same results against the extended-precision reference (filters b and b + 8 of a batch are the same filter)
    nd = min(B, 8)
    key = (name, gated)
    if key not in _REFS or len(_REFS[key]) < nd:
        keep = [np.repeat(mask[b].astype(bool), 2) for b in range(nd)] if gated else None
        _REFS[key] = pr.extended_batch(H[:nd], P[:nd], inn[:nd], dR[:nd], keep)
    worst = np.zeros(3)
    for b in range(B):
        r = pr.check(_REFS[key][b % nd], Pn[b], err[b], what=(name, entry, b))
        worst = np.maximum(worst, r)
    print("accuracy %s %s-%s: rel %.3f corr %.3f dx %.3f x u (kappa + N)" % (route, name, entry, *worst))


def test_create_factor_limit(built):
    """xivo_hip_create: round16(M_max) / 16 = 24 block rows is the largest factor the solver is built for (factor_nb24
    updates at it); 25 is refused with XIVO_HIP_ERR_UNSUPPORTED, before anything is allocated."""
    with Context(64, 384, 1) as ctx:
        assert ctx.h
    with Context(64, 369, 1) as ctx:                            # M_max 369 rounds to 384 as well
        assert ctx.h
    with pytest.raises(XivoHipError) as e:
        Context(64, 385, 1)
    assert e.value.status == -5
