"""The many-factors instantiations of the register Cholesky (chol_reg_la_f64_kernel, chol_f64.hip: batch >= 512) deal the
block rows from the bottom, land the blocks of S in the registers of L one column ahead and factor the next diagonal block
while the current column's panel is still being formed (one barrier per column, double-buffered LDS). Every block of L is
still the same operations on the same operands, so everything must be the same BITS as the few-factors instantiations
(batch < 512, unchanged) produce - at the block-row counts where the ownership table and the look-ahead change shape:

    F = 8   one block row: no successor column            F = 72  nine block rows: the three-per-CU cut starts
    F = 16  two: one look-ahead step, the last has none   F = 80  ten: the benchmark's instantiation
    F = 36  five (M = 72 padded to 80): second row per    F = 88  eleven: the <12, 3> instantiation, partly filled
            wave, ragged last block

B = 512 is the smallest batch that selects them (chol_reg_mode), N = 100 keeps a case to milliseconds; the inputs repeat
with period 16, so the oracle is evaluated sixteen times per case and filter b must equal filter b mod 16 bit for bit."""
import functools

import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd import synth
from xivo_amd.lib import Context, FLAG_MULTI_KERNEL, FLAG_PROFILE

pytestmark = pytest.mark.gpu

N, B, UNIQ = 100, 512, 16
FS = [8, 16, 36, 72, 80, 88]
GATE = (5.991, 1.1, 5)


def _rejected(F):
    """filter -> the pairs whose innovations are blown up: the first and the last pair of the first and of the last 16-row
    block, in several filters, never so many that the threshold is relaxed"""
    last = 8 * ((F - 1) // 8)
    every = sorted({0, 7, last, F - 1})
    return {1: every, 5: [0], 14: sorted({7, F - 1}), 15: [last]}


def _inputs(F):
    P, H, inn, dR = synth.s_level(N, F, UNIQ, seed=1000 + F)
    for b, fs in _rejected(F).items():
        for f in fs:
            inn[b, 2 * f:2 * f + 2] *= 1e4
    return P, H, inn, dR


def _run(F, nfilt, gated, P, H, inn, dR):
    idx = np.arange(nfilt) % UNIQ
    with Context(N, 2 * F, nfilt, flags=FLAG_MULTI_KERNEL | FLAG_PROFILE) as ctx:
        ctx.upload_P(P[idx])
        dH = ctx.device_array(np.ascontiguousarray(np.transpose(H[idx], (0, 2, 1))))
        dinn = ctx.device_array(inn[idx]); dRd = ctx.device_array(dR[idx])
        ctx.set_measurements_device(dH, dinn, dRd, 2 * F, nfilt)
        if gated:
            ctx.update_dense_gated(F, float(dR[0, 0]), *GATE, nfilt)
            mask, dist = ctx.get_gate(F, nfilt)
        else:
            ctx.update_joseph()
            mask, dist = np.ones((nfilt, F), np.uint8), np.zeros((nfilt, F))
        prof = ctx.profile_get()
        return dict(P=ctx.download_P(), dx=ctx.get_err(), mask=mask.copy(), dist=dist.copy(), status=ctx.get_status(check=False),
                    ldlt=ctx.get_ldlt_used(), kernel=prof["chol_S"]["kernel"], gate_launches=prof.get("mh_gate", {}).get("launches", 0))


@functools.lru_cache(maxsize=None)
def _runs(F, gated):
    """the same inputs as 512 filters (many-factors kernel) and as their 511 leading filters (few-factors kernel, stand-alone
    gate), computed once per case and shared by the tests below, which only read it"""
    inp = _inputs(F)
    return inp, _run(F, B, gated, *inp), _run(F, B - 1, gated, *inp)


@functools.lru_cache(maxsize=None)
def _oracle(F, gated):
    P, H, inn, dR = _inputs(F)
    out = []
    for b in range(UNIQ):
        m = np.ones(F, bool)
        d = np.zeros(F)
        if gated:
            d = orc.mh_distances(H[b].reshape(F, 2, -1), P[b], inn[b].reshape(F, 2), float(dR[0, 0]))
            m = np.asarray(orc.mh_gate(d, *GATE)[0]).astype(bool)
        rows = np.repeat(m, 2)
        e_ref, P_ref, _ = orc.update_joseph(H[b][rows], P[b], inn[b][rows], dR[b][rows])
        out.append((m, d, e_ref, P_ref))
    return out


CASES = [(F, True) for F in FS] + [(80, False)]


@pytest.mark.parametrize("F,gated", CASES)
def test_the_instantiations_under_test_ran(built, F, gated):
    _, many, few = _runs(F, gated)
    assert many["kernel"].startswith("chol_reg_la_f64_kernel") and few["kernel"].startswith("chol_reg_f64_kernel"), (many["kernel"], few["kernel"])
    if gated:
        assert "+gate" in many["kernel"] and many["gate_launches"] == 0 and few["gate_launches"] > 0


@pytest.mark.parametrize("F,gated", CASES)
def test_many_factors_update_matches_oracle(built, F, gated):
    _, many, _ = _runs(F, gated)
    ref = _oracle(F, gated)
    assert (many["status"] == 0).all() and not many["ldlt"].any()
    for b in list(range(UNIQ)) + [B - 1]:
        m, d, e_ref, P_ref = ref[b % UNIQ]
        if gated:
            assert np.array_equal(many["mask"][b].astype(bool), m) and rel_fro(many["dist"][b], d) < 1e-9
        assert rel_fro(many["P"][b], P_ref) < TOL_P, (b, rel_fro(many["P"][b], P_ref))
        assert rel_fro(many["dx"][b], e_ref) < TOL_DX, (b, rel_fro(many["dx"][b], e_ref))
    if gated:
        for b, fs in _rejected(F).items():      # exactly the chosen pairs are thrown out: some, not all, block edges included
            assert sorted(np.flatnonzero(ref[b][0] == 0).tolist()) == fs, (b, fs, np.flatnonzero(ref[b][0] == 0))


@pytest.mark.parametrize("F,gated", CASES)
def test_many_factors_bits_equal_the_few_factors_kernel(built, F, gated):
    _, many, few = _runs(F, gated)
    for key in ("status", "mask", "dist", "dx", "P", "ldlt"):
        assert np.array_equal(many[key][:B - 1], few[key]), key


@pytest.mark.parametrize("F,gated", CASES)
def test_every_filter_equals_its_twin_bitwise(built, F, gated):
    _, many, _ = _runs(F, gated)
    idx = np.arange(B) % UNIQ
    for key in ("status", "mask", "dist", "dx", "P"):
        assert np.array_equal(many[key], many[key][idx]), key


def test_a_filter_whose_S_is_not_positive_definite(built):
    """An indefinite covariance (three eigenvalues flipped, tests/test_robustness_gpu.py) in one filter of the ten-block-row
    case: the factorisation flags it, the pivoted L D L^T fallback answers it, and status, fallback flag and every result -
    its own and its neighbours' - are the bits of the few-factors run."""
    F = 80
    P, H, inn, dR = _inputs(F)
    P = P.copy()
    w, Q = np.linalg.eigh(P[6])
    w[-3:] *= -1.0
    P[6] = (Q * w) @ Q.T
    P[6] = 0.5 * (P[6] + P[6].T)
    many, few = _run(F, B, True, P, H, inn, dR), _run(F, B - 1, True, P, H, inn, dR)
    assert many["kernel"].startswith("chol_reg_la_f64_kernel")
    assert many["ldlt"][:UNIQ].tolist() == [int(b == 6) for b in range(UNIQ)] and (many["status"] == 0).all()
    for key in ("status", "ldlt", "mask", "dist", "dx", "P"):
        assert np.array_equal(many[key][:B - 1], few[key]), key
