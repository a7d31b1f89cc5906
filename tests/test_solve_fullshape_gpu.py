"""The full-shape instantiation of the in-solve update (trsm_lds_f64_kernel<10,4> / <11,4> with a compile-time block-row
count, xivo_amd/csrc/trsm_lds_kernel.h) against the general one (XIVO_HIP_SOLVE_GENERIC, read once per process): the same
operations on the same operands in the same order, so P+, dx, status and gate masks come out bit for bit the same - and both
within TOL_P / TOL_DX of the oracle.

Each shape runs in a process of its own kind twice, with the knob and without (nine filters: one sits beyond an XCD group of
eight):
  (250, 80)  ten full block rows: the full-shape <10,4>
  (250, 88)  eleven full block rows: the full-shape <11,4> (packed diagonal slots)
  (250, 72)  nine block rows on <10,4>: the general form either way (it shares the negated factor with the full-shape one)
  (100, 80)  ten full block rows on a narrow state: seven live waves, nine dead ones
and twice per shape: a gated update in which two features of filter 5 fail the gate (neutral rows inside its factor), and a
plain one in which S of filter 7 is not positive definite (no L D L^T fallback: its product is skipped, its prior kept)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd import synth

pytestmark = pytest.mark.gpu

KNOB = "XIVO_HIP_SOLVE_GENERIC"
B, BAD, GATED = 9, 7, 5
GATE = (5.991, 1.1, 5)        # MH threshold, relaxation, min inliers (src/update.cpp:60-96)
SHAPES = [(250, 80, "trsm_lds_f64_kernel<10,4>"), (250, 88, "trsm_lds_f64_kernel<11,4>"),
          (250, 72, "trsm_lds_f64_kernel<10,4>"), (100, 80, "trsm_lds_f64_kernel<10,4>")]

_SNIPPET = """
import sys, json, hashlib
sys.path[:0] = [{root!r}, {root!r} + "/tests", {root!r} + "/oracle"]
import numpy as np
import test_solve_fullshape_gpu as t
out = {{}}
for (N, F, _) in t.SHAPES:
    res = t.run_shape(N, F)
    np.savez({dump!r} + "/%d_%d.npz" % (N, F), **{{k: v for k, v in res.items() if isinstance(v, np.ndarray)}})
    out["%d,%d" % (N, F)] = {{k: (hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() if isinstance(v, np.ndarray) else v)
                             for k, v in res.items()}}
print(json.dumps(out))
"""


def shape_inputs(N, F):
    P, H, inn, dR = synth.s_level(N, F, B, seed=500 + N + F)
    inn_g = inn.copy()
    inn_g[GATED, 4:8] *= 1e4                                   # features 2 and 3 of filter 5 fail the gate
    P_bad = P.copy()
    P_bad[BAD] = -P_bad[BAD]                                   # S of filter 7 is not positive definite
    return P, H, inn, dR, inn_g, P_bad


def run_shape(N, F):
    """Both updates of a shape on the device: arrays, and the route / kernel label of each"""
    from xivo_amd.lib import (Context, FLAG_PROFILE, FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_NO_LDLT_FALLBACK)
    flags = FLAG_THROUGHPUT_ROUTE | FLAG_MULTI_KERNEL | FLAG_PROFILE
    P, H, inn, dR, inn_g, P_bad = shape_inputs(N, F)
    res = {}
    with Context(N, 2 * F, B, flags=flags) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn_g, dR)
        ctx.update_dense_gated(F, float(dR[0, 0]), *GATE)
        mask, dist = ctx.get_gate(F, B)
        res.update(g_P=ctx.download_P(), g_dx=ctx.get_err(), g_status=np.asarray(ctx.get_status(check=False)),
                   g_mask=np.asarray(mask), g_dist=np.asarray(dist),
                   g_route=ctx.last_route(), g_kernel=ctx.profile_get()["trsm_gain"]["kernel"])
    with Context(N, 2 * F, B, flags=flags | FLAG_NO_LDLT_FALLBACK) as ctx:
        ctx.upload_P(P_bad)
        ctx.set_measurements(H, inn, dR)
        ctx.update_joseph()
        res.update(b_P=ctx.download_P(), b_dx=ctx.get_err(), b_status=np.asarray(ctx.get_status(check=False)),
                   b_ldlt=np.asarray(ctx.get_ldlt_used()),
                   b_route=ctx.last_route(), b_kernel=ctx.profile_get()["trsm_gain"]["kernel"])
    return res


@pytest.fixture(scope="module")
def both_runs(built, tmp_path_factory):
    """[without the knob, with it]: per shape the sha256 of every array and the labels; the arrays of each run on disk"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for knob in (False, True):
        dump = str(tmp_path_factory.mktemp("generic" if knob else "fullshape"))
        env = dict(os.environ)
        env.pop(KNOB, None)
        if knob:
            env[KNOB] = "1"
        r = subprocess.run([sys.executable, "-c", _SNIPPET.format(root=root, dump=dump)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append((json.loads(r.stdout.strip().splitlines()[-1]), dump))
    return runs


@pytest.mark.parametrize("N,F,kern", SHAPES, ids=["%dx%d" % (s[0], 2 * s[1]) for s in SHAPES])
def test_full_shape_and_general_solve_are_bit_identical(both_runs, N, F, kern):
    (full, _), (generic, _) = both_runs
    a, b = full["%d,%d" % (N, F)], generic["%d,%d" % (N, F)]
    for k in ("g_route", "b_route"):
        assert a[k] == b[k] == "sparse_in_solve", (k, a[k], b[k])
    for k in ("g_kernel", "b_kernel"):                       # the label names the instantiation by its first two parameters
        assert a[k] == b[k] == kern, (k, a[k], b[k])
    for k in ("g_P", "g_dx", "g_status", "g_mask", "g_dist", "b_P", "b_dx", "b_status", "b_ldlt"):
        assert a[k] == b[k], (N, F, k)


@pytest.mark.parametrize("which", [0, 1], ids=["fullshape", "generic"])
@pytest.mark.parametrize("N,F,kern", SHAPES, ids=["%dx%d" % (s[0], 2 * s[1]) for s in SHAPES])
def test_both_solves_match_the_oracle(both_runs, N, F, kern, which):
    d = np.load(both_runs[which][1] + "/%d_%d.npz" % (N, F))
    P, H, inn, dR, inn_g, P_bad = shape_inputs(N, F)
    R = float(dR[0, 0])
    worst = np.zeros(2)
    # the gated update: the oracle's gate, then its update on the rows that passed
    assert (d["g_status"] == 0).all(), d["g_status"]
    for b in range(B):
        d_ref = orc.mh_distances(H[b].reshape(F, 2, N), P[b], inn_g[b].reshape(F, 2), R)
        m_ref = np.asarray(orc.mh_gate(d_ref, *GATE)[0]).astype(bool)
        assert np.array_equal(d["g_mask"][b].astype(bool), m_ref), b
        assert b != GATED or not m_ref[2:4].any()
        keep = np.repeat(m_ref, 2)
        e_ref, P_ref, _ = orc.update_joseph(H[b][keep], P[b], inn_g[b][keep], dR[b][keep])
        rp, re = rel_fro(d["g_P"][b], P_ref), rel_fro(d["g_dx"][b], e_ref)
        worst = np.maximum(worst, (rp, re))
        assert rp < TOL_P and re < TOL_DX, ("gated", b, rp, re)
        assert np.array_equal(d["g_P"][b], d["g_P"][b].T), b
    # the plain update with one breakdown: prior kept bit for bit, status set, the others updated
    st = d["b_status"]
    assert st[BAD] != 0 and (np.delete(st, BAD) == 0).all() and not d["b_ldlt"].any(), st
    assert np.array_equal(d["b_P"][BAD], P_bad[BAD])
    for b in range(B):
        if b == BAD:
            continue
        e_ref, P_ref, _ = orc.update_joseph(H[b], P[b], inn[b], dR[b])
        rp, re = rel_fro(d["b_P"][b], P_ref), rel_fro(d["b_dx"][b], e_ref)
        worst = np.maximum(worst, (rp, re))
        assert rp < TOL_P and re < TOL_DX, ("plain", b, rp, re)
        assert np.array_equal(d["b_P"][b], d["b_P"][b].T), b
    print("(%d, %d) %s %s: worst rel err P %.2e dx %.2e" % (N, 2 * F, kern, ("fullshape", "generic")[which], *worst))
