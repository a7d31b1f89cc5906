"""The in-solve whitened update off the stash (trsm_lds_f64_kernel<10,4> / <11,4>, whitened_tiles_from_stash in
xivo_amd/csrc/trsm_lds_kernel.h): the backward substitution keeps D in the registers, the stash of W is read once - by the DMA
of the product - and a wave forms V = W - D and Y = W + D when its own block arrives in LDS, in phase group(w) = w / jbp;
a pair of blocks from two groups is formed by the wave of the earlier group, the pairs inside a group by the cyclic rule.

The shapes are the smallest at which that schedule can go wrong (nb block rows of the factor, jbp column blocks per phase):
  (250, 160)  nb 10, jbp 4: four full groups, 16 live waves - the flagship shape
  (256, 128)  nb  8, jbp 5: groups 5, 5, 5, 1 - the last group is one block whose only tile is its diagonal
  (200, 104)  nb  7, jbp 5: groups 5, 5, 3, 13 live waves of 16 - dead waves behind the last group
  (100, 160)  nb 10, jbp 4: groups 4, 3, seven live waves
  (251, 174)  nb 11, jbp 3: groups 3, 3, 3, 3, 3, 1 - the packed-diagonal instantiation <11,4>
Every case: the route and the kernel label, status 0, P+ and dx against the oracle at TOL_P / TOL_DX, P+ exactly symmetric.
Batches of 70 filters repeat eight distinct ones (more than one workgroup per XCD, filters b and b + 8 must agree bit for bit)."""
import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd import synth
from xivo_amd.lib import (Context, FLAG_PROFILE, FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_NO_LDLT_FALLBACK)

pytestmark = pytest.mark.gpu

FLAGS = FLAG_THROUGHPUT_ROUTE | FLAG_MULTI_KERNEL | FLAG_PROFILE
B, ND = 70, 8
GATE = (5.991, 1.1, 5)        # MH threshold, relaxation, min inliers (src/update.cpp:60-96)
R = 2.25
K10, K11 = "trsm_lds_f64_kernel<10,4>", "trsm_lds_f64_kernel<11,4>"
SHAPES = [(250, 160, K10), (256, 128, K10), (200, 104, K10), (100, 160, K10), (251, 174, K11)]
_INPUTS = {}


def inputs(N, M, seed=None):
    """P, H, inn, dR of B filters - eight distinct synth.s_level filters, repeated - and the oracle's (dx, P+) of the eight"""
    key = (N, M, seed)
    if key not in _INPUTS:
        P, H, inn, dR = synth.s_level(N, M // 2, ND, seed=1000 + N + M if seed is None else seed)
        ref = [orc.update_joseph(H[b], P[b], inn[b], dR[b])[:2] for b in range(ND)]
        _INPUTS[key] = (P, H, inn, dR, ref)
    P, H, inn, dR, ref = _INPUTS[key]
    idx = np.arange(B) % ND
    return P[idx].copy(), H[idx].copy(), inn[idx].copy(), dR[idx].copy(), ref


def check_route(ctx, kern):
    route, got = ctx.last_route(), ctx.profile_get()["trsm_gain"]["kernel"]
    assert route == "sparse_in_solve", route
    assert got == kern, (got, kern)


def check_filter(Pn, err, e_ref, P_ref, what):
    rp, re = rel_fro(Pn, P_ref), rel_fro(err, e_ref)
    assert rp < TOL_P, (what, rp)
    assert re < TOL_DX, (what, re)
    assert np.array_equal(Pn, Pn.T), what


@pytest.mark.parametrize("N,M,kern", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_in_solve_update_reads_the_stash_once(built, N, M, kern):
    P, H, inn, dR, ref = inputs(N, M)
    with Context(N, M, B, flags=FLAGS) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn, dR)
        ctx.update_joseph()
        Pn, err = ctx.download_P(), ctx.get_err()
        check_route(ctx, kern)
        st = ctx.get_status(check=False)
    assert (st == 0).all(), st
    worst = np.zeros(2)
    for b in range(B):
        e_ref, P_ref = ref[b % ND]
        worst = np.maximum(worst, (rel_fro(Pn[b], P_ref), rel_fro(err[b], e_ref)))
        check_filter(Pn[b], err[b], e_ref, P_ref, (N, M, b))
        if b >= ND:   # the same filter on another workgroup: the same bits
            assert np.array_equal(Pn[b], Pn[b % ND]) and np.array_equal(err[b], err[b % ND]), b
    print("(%d, %d) %s: worst rel err P %.2e dx %.2e" % (N, M, kern, *worst))


def test_gated_rows_inside_the_factor(built):
    """Two features of ONE filter fail the gate: neutral rows inside that filter's factor, its neighbours see none."""
    N, M = 250, 160
    F = M // 2
    P, H, inn, dR, _ = inputs(N, M)
    gb = 11
    inn[gb, 4:8] *= 1e4                                         # features 2 and 3 of filter gb
    with Context(N, M, B, flags=FLAGS) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn, dR)
        ctx.update_dense_gated(F, R, *GATE)
        mask, dist = ctx.get_gate(F, B)
        Pn, err = ctx.download_P(), ctx.get_err()
        check_route(ctx, K10)
        st = ctx.get_status(check=False)
    assert (st == 0).all(), st
    refs = {}
    for b in range(B):
        key = gb if b == gb else b % ND
        if key not in refs:
            d_ref = orc.mh_distances(H[b].reshape(F, 2, N), P[b], inn[b].reshape(F, 2), R)
            m_ref = np.asarray(orc.mh_gate(d_ref, *GATE)[0]).astype(bool)
            keep = np.repeat(m_ref, 2)
            refs[key] = (d_ref, m_ref) + tuple(orc.update_joseph(H[b][keep], P[b], inn[b][keep], dR[b][keep])[:2])
        d_ref, m_ref, e_ref, P_ref = refs[key]
        assert np.array_equal(mask[b].astype(bool), m_ref), b
        assert np.allclose(dist[b], d_ref, rtol=1e-9, atol=0), b
        check_filter(Pn[b], err[b], e_ref, P_ref, ("gated", b))
    assert not refs[gb][1][2:4].any() and refs[gb % ND][1][2:4].all()


def test_not_spd_filter_leaves_before_the_product(built):
    """One filter whose S is not positive definite (P negated), no L D L^T fallback: its whole workgroup returns before the
    product - its P is the prior bit for bit, its status is set - and the other filters are updated."""
    N, M = 250, 160
    P, H, inn, dR, ref = inputs(N, M)
    bad = 21
    P[bad] = -P[bad]
    with Context(N, M, B, flags=FLAGS | FLAG_NO_LDLT_FALLBACK) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn, dR)
        ctx.update_joseph()
        Pn, err = ctx.download_P(), ctx.get_err()
        check_route(ctx, K10)
        st = ctx.get_status(check=False)
        assert not ctx.get_ldlt_used().any()
    assert st[bad] != 0 and (np.delete(st, bad) == 0).all(), st
    assert np.array_equal(Pn[bad], P[bad])
    for b in range(B):
        if b != bad:
            check_filter(Pn[b], err[b], *ref[b % ND], ("not_spd", b))


def test_chain_of_updates(built):
    """Five updates in a row, new measurements each time, P carried on the device: against the oracle's own chain."""
    N, M, steps = 250, 160, 5
    P, H, inn, dR, _ = inputs(N, M)
    P_ref = [P[b].copy() for b in range(ND)]
    idx = np.arange(B) % ND
    with Context(N, M, B, flags=FLAGS) as ctx:
        ctx.upload_P(P)
        for s in range(steps):
            _, Hs, inns, dRs = synth.s_level(N, M // 2, ND, seed=7000 + s)
            ctx.set_measurements(Hs[idx], inns[idx], dRs[idx])
            ctx.update_joseph()
            Pn, err = ctx.download_P(), ctx.get_err()
            check_route(ctx, K10)
            assert (ctx.get_status(check=False) == 0).all()
            out = [orc.update_joseph(Hs[b], P_ref[b], inns[b], dRs[b])[:2] for b in range(ND)]
            P_ref = [o[1] for o in out]
            for b in range(B):
                check_filter(Pn[b], err[b], out[b % ND][0], P_ref[b % ND], ("chain", s, b))
