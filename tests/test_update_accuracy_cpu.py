"""The yardsticks of tests/precise_ref.py checked on the host, on the first filter of every case of
tests/test_update_edges_gpu.py::EDGE_CASES: the fp64 oracle passes them with room to spare, and the two kinds of error that
helpers.TOL_P cannot see fail them - a float rounding of P+ (what a float leak on an fp64 route would leave) and an error
confined to the states with the smallest variances. Also: the oracle is bit-exactly equivariant under a power-of-two change of
units (P -> D P D, H -> H D^-1), the exactness tests/test_update_accuracy_gpu.py asks of the device routes. No GPU."""
import numpy as np
import pytest

import precise_ref as pr
import xivo_oracle as orc
from helpers import rel_fro, TOL_P
import test_update_edges_gpu as edges


def _first(case):
    P, H, inn, dR = edges.edge_inputs(case)
    return P[0], H[0], inn[0], dR[0]


@pytest.mark.parametrize("name", [c[0] for c in edges.EDGE_CASES])
def test_oracle_float_rounding_and_equivariance(name):
    P, H, inn, dR = _first(edges.CASES[name])
    ref = pr.extended(H, P, inn, dR)
    e, Pn, _ = orc.update_joseph(H, P, inn, dR)
    t = pr.tol(ref)
    rel, corr, rdx = pr.metrics(ref, Pn, e)
    assert max(rel, corr, rdx) < t / 10, (rel, corr, rdx, t, ref.kappa)       # the fp64 oracle: ten times inside the bound
    # P+ rounded to float: what TOL_P lets through, and the bound does not
    P32 = Pn.astype(np.float32).astype(np.float64)
    assert rel_fro(P32, Pn) < TOL_P
    rel32, corr32, _ = pr.metrics(ref, P32)
    assert rel32 > t and corr32 > t, (rel32, corr32, t)
    # power-of-two units: the oracle's every sum combines terms of one scale, so the twin's result is D P+ D, D dx to the bit
    D = pr.pow2_scales(P.shape[0], seed=len(name))
    Ps, Hs = pr.scale(D, P, H)
    es, Pns, _ = orc.update_joseph(Hs, Ps, inn, dR)
    assert np.array_equal(Pns, Pn * np.outer(D, D))
    assert np.array_equal(es, e * D)


def test_small_variance_tile_error_passes_tol_p_but_not_corr():
    """m64_150 in units where the variances span 2^-40 .. 2^4: one 16 x 16 tile of P+ over the sixteen states of smallest
    variance off by 0.1 %. The relative Frobenius norm of TOL_P moves by ~1e-16; in units of the prior correlation the error
    is ~1e-3, far outside the bound."""
    P, H, inn, dR = _first(edges.CASES["m64_150"])
    D = pr.pow2_scales(P.shape[0], seed=1)
    P, H = pr.scale(D, P, H)
    assert (D[16:32] < 2.0 ** -15).all()
    ref = pr.extended(H, P, inn, dR)
    _, Pn, _ = orc.update_joseph(H, P, inn, dR)
    assert max(pr.metrics(ref, Pn)[:2]) < pr.tol(ref) / 10
    idx = np.argsort(np.diag(P))[:16]
    Pm = Pn.copy()
    Pm[np.ix_(idx, idx)] *= 1.001
    assert rel_fro(Pm, Pn) < 1e-12 and rel_fro(Pm, Pn) < TOL_P
    rel, corr, _ = pr.metrics(ref, Pm)
    assert rel < pr.tol(ref) and corr > 1e3 * pr.tol(ref), (rel, corr, pr.tol(ref))


def test_extended_reference_keeps_only_the_kept_rows():
    """keep= drops the rows the gate rejected before anything else: the same answer as the update of the kept rows alone."""
    P, H, inn, dR = _first(edges.CASES["m64_150"])
    keep = np.ones(H.shape[0], dtype=bool)
    keep[4:8] = False
    a = pr.extended(H, P, inn, dR, keep=keep)
    b = pr.extended(H[keep], P, inn[keep], dR[keep])
    assert np.array_equal(a.P, b.P) and np.array_equal(a.dx, b.dx) and a.kappa == b.kappa
    assert np.finfo(np.longdouble).nmant >= 63                   # (an 80-bit longdouble: this reference means nothing in fp64)
