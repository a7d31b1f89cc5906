"""`ell<S>` (S = H (P H^T) + diag(R), `ell_tile_kernel<1,12,64,9>`) forms only the sixteen-column blocks of a slab that
somebody reads - those left of the padding and on or below the block diagonal - deals them to its eight waves in runs that
may cut a row-pair block in two, and requests the next slab while the current one is parked. Everything behind S (the
gate's compact diagonal blocks, factorisation, solve, covariance update) must be what it was:

 * dx, P+, status, inlier mask and distances against the numpy oracle, at the tolerances of tests/test_update_gpu.py;
 * 1032 filters (persistent form: all slabs of a filter in one workgroup, the last stride over the batch not full) against
   the first 1031 of them as a batch of their own, and against 200 of them (one slab per workgroup, not persistent): bit
   for bit - a tile's bits do not depend on which wave formed it, in which piece, or on how its slab arrived;
 * M = 160 and then M = 80 on one context: the tiles above the block diagonal still hold the factor of the first update and
   the rows beyond the smaller M its S - bit for bit the outputs of a context that only ever saw M = 80.

Shapes: M = 16 one live block; 48 a single partial slab; 64 exactly one slab; 80 one live block in the second slab; 128 two
full slabs; 160 two and a half (the benchmark's); 176 eleven block rows (the twelve-row factorisation with its mirror, the
largest factor the solve kernel holds). The state is the smallest that gives every feature a slot of its own in
`synth.s_level` (23 + 6 * 8 group columns + 3 F), capped at the benchmark's 250; XIVO_HIP_FLAG_MULTI_KERNEL keeps the
small shapes off the one-kernel update."""
import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd import synth
from xivo_amd.lib import Context, FLAG_MULTI_KERNEL, FLAG_PROFILE

pytestmark = pytest.mark.gpu

U = 7                       # distinct filters; filter b of a batch is source filter b % U
GATE = (2.25, 5.991, 1.1, 5)
S_KERNEL = "ell_tile_kernel<1,12,64,9>"


def _state(F):
    return min(250, 23 + 6 * 8 + 3 * F)


def _case(F, gated, seed, N=None):
    N = _state(F) if N is None else N
    P, H, inn, dR = synth.s_level(N, F, U, seed=seed)
    if gated:   # rows small enough that S_f ~ R, and a few wild innovations per filter (as tests/test_update_gpu.py)
        H *= 0.01
        rng = np.random.default_rng(seed)
        for b in range(U):
            bad = rng.choice(F, size=min(2 + b % 3, F // 4), replace=False)
            inn[b].reshape(F, 2)[bad] += rng.choice([-1, 1], size=(len(bad), 2)) * rng.uniform(8, 30, size=(len(bad), 2))
    return N, P, H, inn, dR


def _run(ctx, F, gated, P, H, inn, dR):
    ctx.upload_P(P); ctx.set_measurements(H, inn, dR)
    if gated:
        ctx.update_dense_gated(F, *GATE)
    else:
        ctx.update_joseph()
    assert ctx.last_route() == "sparse_in_solve", ctx.last_route()
    assert ctx.profile_get()["gemm_S"]["kernel"] == S_KERNEL
    out = dict(dx=ctx.get_err(), P=ctx.download_P(), status=ctx.get_status(check=False))
    if gated:
        mask, dist = ctx.get_gate(F)
        out.update(mask=mask, dist=dist)
    return out


def _update(F, gated, src, B):
    N, P, H, inn, dR = src
    idx = np.arange(B) % U
    with Context(N, 2 * F, B, flags=FLAG_MULTI_KERNEL | FLAG_PROFILE) as ctx:
        return _run(ctx, F, gated, P[idx], H[idx], inn[idx], dR[idx])


def _same(a, b, n):
    for k in a:
        assert np.array_equal(a[k][:n], b[k][:n]), k


def _against_oracle(F, gated, src, out):
    _, P, H, inn, dR = src
    assert (out["status"] == 0).all()
    for b in range(U):
        rows = slice(None)
        if gated:
            d = orc.mh_distances(H[b].reshape(F, 2, -1), P[b], inn[b].reshape(F, 2), GATE[0])
            m = orc.mh_gate(d, *GATE[1:])[0]
            assert rel_fro(out["dist"][b], d) < 1e-9 and np.array_equal(out["mask"][b].astype(bool), m)
            assert not m.all()
            rows = np.repeat(m, 2)
        e_ref, P_ref, _ = orc.update_joseph(H[b][rows], P[b], inn[b][rows], dR[b][rows])
        assert rel_fro(out["P"][b], P_ref) < TOL_P and rel_fro(out["dx"][b], e_ref) < TOL_DX
        assert np.array_equal(out["P"][b], out["P"][b].T)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("M", [16, 48, 64, 80, 128, 160, 176])
def test_live_tiles_only(built, M, gated):
    F = M // 2
    src = _case(F, gated, seed=300 + M + int(gated))
    big = _update(F, gated, src, 1032)
    _against_oracle(F, gated, src, big)
    _same(big, {k: v[np.arange(1032) % U] for k, v in big.items()}, 1032)      # every filter equals its twins
    _same(big, _update(F, gated, src, 1031), 1031)
    few = _update(F, gated, src, 200)
    _against_oracle(F, gated, src, few)
    _same(big, few, 200)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("B", [1032, 200])
def test_smaller_M_after_larger_M(built, B, gated):
    N = 250
    first = _case(80, gated, seed=411)
    second = (N, first[1]) + _case(40, gated, seed=412, N=N)[2:]     # the same P, 80 rows
    idx = np.arange(B) % U
    with Context(N, 160, B, flags=FLAG_MULTI_KERNEL | FLAG_PROFILE) as ctx:
        _run(ctx, 80, gated, *(x[idx] for x in first[1:]))
        after = _run(ctx, 40, gated, *(x[idx] for x in second[1:]))
    _against_oracle(40, gated, second, after)
    with Context(N, 160, B, flags=FLAG_MULTI_KERNEL | FLAG_PROFILE) as ctx:
        alone = _run(ctx, 40, gated, *(x[idx] for x in second[1:]))
    _same(after, alone, B)
