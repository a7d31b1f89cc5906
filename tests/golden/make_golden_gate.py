#!/usr/bin/env python
"""Generates tests/golden/gate_ties.npz: what the EXTRACTED Estimator::OnePointRANSAC (oracle/_ref/libxivo_refx_n203_{v3,v4}.so,
the reference's own text compiled for both ISA levels) decides for a feature whose innovation norm sits exactly on
ransac_thresh_ - the low-innovation test `res.norm() < ransac_thresh_` of src/update.cpp:245-249.

A compiler may contract r0 * r0 + r1 * r1 to one fused multiply-add, in either order; the three forms (tests/gate_restate.py:
norm_unfused, norm_fused, and the fused form with the other product exact) differ by one ulp on a few percent of innovations.
For innovations on which they differ the generator runs the extracted function with ransac_thresh = the unfused norm U and with
nextafter(U), and chi2 = 0 (nothing is rescued, so with one clearly high-innovation feature in the frame the returned inlier
set IS the low-innovation set). tests/test_gate_edges_cpu.py reads from the record which form each build computes.

The generator takes the prediction from the extracted ComputeJacobian with xp = 0, so its xp - prediction is one IEEE
subtraction of two known doubles: the innovation of the Jacobian pass, which is what the device tests. The reference's loop
calls f->Predict(gsb(), gbc()) once more instead (src/update.cpp:248), a second evaluation with its own rounding; norm_v3 /
norm_v4 record the norm each build actually compares (found by bisection on the threshold). What came out: the two builds agree
in every bit, and their norm lies 0 .. 1351 ulp from the Jacobian pass's - two to three decades more than the one ulp between
the fused and the unfused form. On the device's inputs the reference therefore does not define the decision at a one-ulp tie;
the project pins the explicit unfused form.
Run in the authoring container only:  python tests/golden/make_golden_gate.py"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from xivo_amd import synth  # noqa: E402

NG, NF = 15, 30                     # the default build's kMaxGroup / kMaxFeature (N = 203)
CAM = synth.RADTAN
R_VIS = 1.0
HIGH = 7                            # the feature moved 6 px: never low-innovation, keeps the frame in the partial-update branch
KINDS = ("a_below", "a_above", "b_below", "b_above")
PER_KIND = 2


def norm_fused_b(r0, r1):
    """sqrt(fma(r0, r0, r1 * r1)): the other order of tests/gate_restate.py::norm_fused"""
    b = float(r1) * float(r1)
    return math.sqrt(float(Fraction(float(r0)) * Fraction(float(r0)) + Fraction(b)))


def tie_case():
    sc = synth.g_level(NG, NF, NF, 1, seed=411, cam=CAM)
    rng = np.random.default_rng(412)
    N = 23 + 6 * NG + 3 * NF
    A = rng.uniform(-1, 1, size=(N, N)); P = (A @ A.T / N + 1e-3 * np.eye(N)) * 1e-4
    noise = rng.normal(size=(NF, 2)) * 0.3
    noise[HIGH] = [6.0, -6.0]
    return dict(sc=sc, P=P, noise=noise, N=N)


def kind_of(r):
    import gate_restate as gr
    u, a, b = gr.norm_unfused(r[0], r[1]), gr.norm_fused(r[0], r[1]), norm_fused_b(r[0], r[1])
    out = []
    if a < u: out.append("a_below")
    if a > u: out.append("a_above")
    if b < u: out.append("b_below")
    if b > u: out.append("b_above")
    return u, out


def generate():
    """the arrays of gate_ties.npz (tests/test_gate_edges_cpu.py regenerates them where oracle/_ref is built and compares every bit)"""
    import ref_binding
    import xivo_oracle as orc
    import gate_edge_cases as gc
    libs = {v: ref_binding.RefX(os.path.join(ROOT, "oracle", "_ref", "libxivo_refx_n203_%s.so" % v)) for v in ("v3", "v4")}
    c = tie_case(); sc = c["sc"]
    pred = {}
    for v, lib in libs.items():
        pred[v] = np.array([-lib.compute_jacobian(sc["x"][0, i], np.zeros(2), sc["gR"][0, sc["ref"][0, i]], sc["gT"][0, sc["ref"][0, i]], sc["Rsb"][0],
                                                  sc["Tsb"][0], sc["Rbc"][0], sc["Tbc"][0], CAM, sc["ref"][0, i], sc["sind"][0, i])[1] for i in range(NF)])
    assert np.array_equal(pred["v3"], pred["v4"]), "the two builds predict different pixels: record them per build"
    pred = pred["v3"]
    base_xp = pred + c["noise"]
    recs, count = [], dict.fromkeys(KINDS, 0)
    for f in range(NF):
        if f == HIGH or all(count[k] >= PER_KIND for k in KINDS):
            continue
        xps, rs = gc.tie_innovations(pred[f], 500 + f, n=200, scale=0.8)
        for xp, r in zip(xps, rs):
            u, kinds = kind_of(r)
            want = [k for k in kinds if count[k] < PER_KIND]
            if want:
                for k in kinds:
                    count[k] += 1
                recs.append((f, xp, r, u, "+".join(kinds)))
                break
    assert all(count[k] >= PER_KIND for k in KINDS), count
    X = orc.MotionState(sc["Rsb"][0], sc["Tsb"][0], np.zeros(3), np.zeros(3), np.zeros(3), np.eye(3))
    out = dict(feature=np.array([r[0] for r in recs], dtype=np.int32), xp=np.array([r[1] for r in recs]), r=np.array([r[2] for r in recs]),
               U=np.array([r[3] for r in recs]), kinds=np.array([r[4] for r in recs]), pred=pred)
    for v, lib in libs.items():
        keep = np.zeros((len(recs), 2, NF), dtype=bool)
        for k, (f, xp_f, r, u, _) in enumerate(recs):
            xp = base_xp.copy(); xp[f] = xp_f
            assert np.array_equal(xp[f] - pred[f], r)
            for t, th in enumerate((u, np.nextafter(u, np.inf))):
                o = lib.one_point_ransac(X, sc["Rbc"][0], sc["Tbc"][0], c["P"], sc["x"][0], xp, sc["ref"][0], sc["sind"][0], sc["gR"][0], sc["gT"][0],
                                         CAM, R_VIS, float(th), 0.0, gauge_sind=0)
                keep[k, t] = o["keep"]
        out["keep_" + v] = keep
        # the norm the build itself compares: the decision is monotone in the threshold, so bisection over the doubles finds
        # the largest threshold at which the feature is NOT low-innovation - its norm, to the bit
        nref = np.zeros(len(recs))
        for k, (f, xp_f, r, u, _) in enumerate(recs):
            xp = base_xp.copy(); xp[f] = xp_f
            lo, hi = 0.0, 16.0
            while np.nextafter(lo, np.inf) < hi:
                mid = 0.5 * (lo + hi)
                o = lib.one_point_ransac(X, sc["Rbc"][0], sc["Tbc"][0], c["P"], sc["x"][0], xp, sc["ref"][0], sc["sind"][0], sc["gR"][0], sc["gT"][0],
                                         CAM, R_VIS, mid, 0.0, gauge_sind=0)
                lo, hi = (lo, mid) if o["keep"][f] else (mid, hi)
            nref[k] = lo
        out["norm_" + v] = nref
    return out


def main():
    out = generate()
    path = os.path.join(ROOT, "tests", "golden", "gate_ties.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out["feature"]), "records")


if __name__ == "__main__":
    main()
