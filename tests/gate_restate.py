"""Estimator::MHGating (src/update.cpp:60-96) and the decisions of Estimator::OnePointRANSAC (src/update.cpp:213-393) restated in
plain numpy / Python on the host, with no project kernel code: what tests/test_gate_edges_cpu.py and tests/test_gate_edges_gpu.py
hold the five gate copies and the RANSAC kernels against.

  distances_80   S = J P J^T + R I2 and d = r^T S^-1 r in np.longdouble (80-bit on x86) from the fp64 inputs the device reads: the
                 whole row J (21 columns of a default build scattered over the N state columns, 43 of a calibration build), the
                 whole P, the innovation the Jacobian pass left (the Jacobian pass is tested elsewhere and is an input here).
                 Returns kappa_2(S) with it.
  relax          the threshold-relaxation loop, update.cpp:72-96, on fp64 distances, decided in fp64.
  low_unfused    |r| < thresh as Eigen's res.norm() forms it: two rounded products, one rounded add, sqrt.
  low_fused      the same with r0 * r0 + r1 * r1 contracted to one fused multiply-add - only the case builder uses it, to find
                 innovations on which the two differ.
  find_new_ref_group   Estimator::FindNewRefGroup, estimator.cpp:1394-1407.
  ransac_decisions     frame state, groups and feature rows to zero; `rescue` the strict chi-square test.
The partial update and AbsorbError are the oracle's (oracle/xivo_oracle.py: one_point_ransac with the low-innovation set handed in).

Two guards of the relaxation loop are the PROJECT's, not the reference's (which loops until it has min_inliers, for ever if it
must): GUARD_ALL_IN - stop when every present entry is an inlier - and GUARD_PASSES - stop after 4096 passes. `relax` names
the reason it stopped so a case can say which one it rests on.

FindNewRefGroup walks an unordered_set of group pointers: among groups whose summed variances are equal in every bit the
reference's choice is unspecified (hash order). "The lowest slot wins" is the project's choice, pinned here as coded."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
MAX_PASSES = 4096
STOP_MIN_INLIERS, GUARD_ALL_IN, GUARD_PASSES, NO_LOOP = "min_inliers", "guard_all_in", "guard_passes", "no_loop"


# ---------------------------------------------------------------- distance
def distance_80(J, P, r, R):
    """J [2, N], P [N, N], r [2] fp64 -> (d, kappa_2(S)) in 80 bits. S is symmetrised from its lower triangle, as Eigen's LLT reads
    it (update.cpp:68); the 2 x 2 solve is written out (Cramer) - no factorisation whose order could matter at 80 bits."""
    Jl, Pl, rl = np.asarray(J, dtype=LD), np.asarray(P, dtype=LD), np.asarray(r, dtype=LD)
    PJ = Pl @ Jl.T                                  # [N, 2]
    s00 = Jl[0] @ PJ[:, 0] + LD(R)
    s10 = Jl[1] @ PJ[:, 0]
    s11 = Jl[1] @ PJ[:, 1] + LD(R)
    det = s00 * s11 - s10 * s10
    d = (rl[0] * rl[0] * s11 - LD(2) * rl[0] * rl[1] * s10 + rl[1] * rl[1] * s00) / det
    tr = s00 + s11
    disc = np.sqrt((s00 - s11) * (s00 - s11) + LD(4) * s10 * s10)
    lmax = (tr + disc) / LD(2)
    lmin = det / lmax                               # (no cancellation: the small eigenvalue from the determinant)
    return d, float(lmax / lmin)


def distances_80(J, P, inn, R):
    """J [F, 2, N], inn [F, 2] -> (d [F] longdouble, kappa [F])"""
    out = [distance_80(J[f], P, inn[f], R) for f in range(len(J))]
    return np.array([o[0] for o in out], dtype=LD), np.array([o[1] for o in out])


# ---------------------------------------------------------------- relaxation loop
def relax(dist, thresh, mult, min_inliers, present=None):
    """update.cpp:72-96 on the distances of one filter. dist: fp64, +inf for an absent entry (never an inlier). present: how many
    entries can become inliers (None: all of them - the update-level gates' rule; the feature-level gates count sind >= 0).
      `dist < thresh` is strict (:84); `thresh *= mult` comes after the pass (:94); the loop ends at inliers >= min_inliers (:73).
    Returns dict(mask, thresh = the threshold of the last pass, relaxations = passes - 1, stop, visited = every threshold tried)."""
    dist = np.asarray(dist, dtype=np.float64)
    F = len(dist)
    present = F if present is None else present
    th = float(thresh)
    if min_inliers <= 0:                            # :73 never true: inliers stays empty
        return dict(mask=np.zeros(F, dtype=bool), thresh=-1.0, relaxations=0, stop=NO_LOOP, visited=[])
    visited = []
    for it in range(MAX_PASSES):
        mask = dist < th                            # :84
        visited.append(th)
        cnt = int(mask.sum())
        if cnt >= min_inliers:                      # :73
            return dict(mask=mask, thresh=th, relaxations=it, stop=STOP_MIN_INLIERS, visited=visited)
        if cnt >= present:                          # NOT the reference's: it would multiply on for ever
            return dict(mask=mask, thresh=th, relaxations=it, stop=GUARD_ALL_IN, visited=visited)
        th = float(np.float64(th) * np.float64(mult))   # :94
    # NOT the reference's: after 4096 passes the project gates once more on the threshold the last multiplication left
    return dict(mask=dist < th, thresh=th, relaxations=MAX_PASSES, stop=GUARD_PASSES, visited=visited + [th])


def gate(dist, here, thresh, mult, min_inliers, counts_present):
    """One filter through a gate as the project codes it. here [F] bool: the entry is present (sind >= 0).
    counts_present: the feature-level rule (gate_sparse_kernel, gate_dense_kernel with the scene's entries) - gate only when
    more than min_inliers entries are present (src/manager.cpp:635), otherwise the mask is the present entries and dist is 0;
    the update-level gates take present = F and the caller has decided F > min_inliers.
    Returns (mask, dist as reported, relax record or None)."""
    here = np.asarray(here, dtype=bool)
    d = np.where(here, np.asarray(dist, dtype=np.float64), np.inf)
    present = int(here.sum()) if counts_present else len(d)
    if counts_present and not present > min_inliers:
        return here.copy(), np.zeros(len(d)), None
    rec = relax(d, thresh, mult, min_inliers, present)
    return rec["mask"], np.where(here, d, 0.0), rec


# ---------------------------------------------------------------- low-innovation test
def norm_unfused(r0, r1):
    """Eigen's res.norm() of a 2-vector in explicit fp64 steps (Python floats: no BLAS, nothing a compiler could contract)"""
    a = float(r0) * float(r0)
    b = float(r1) * float(r1)
    return math.sqrt(a + b)


def _round_fraction(q):
    """the fp64 nearest (ties to even) to the rational q >= 0: float(Fraction) is correctly rounded by the language definition"""
    return float(q)


def norm_fused(r0, r1):
    """sqrt(fma(r1, r1, r0 * r0)): the first product rounded, the second exact inside the fused operation (exact rationals)"""
    a = float(r0) * float(r0)
    s = _round_fraction(Fraction(float(r1)) * Fraction(float(r1)) + Fraction(a))
    return math.sqrt(s)


def low_unfused(r, thresh):
    return norm_unfused(r[0], r[1]) < thresh        # update.cpp:245-249, strict


def low_fused(r, thresh):
    return norm_fused(r[0], r[1]) < thresh


# ---------------------------------------------------------------- FindNewRefGroup
def group_cov(P, group_begin, g):
    """the six diagonal entries of group slot g summed in ascending order (estimator.cpp:1398-1401), in fp64"""
    off = group_begin + 6 * g
    s = 0.0
    for i in range(6):
        s = s + float(P[off + i, off + i])
    return s


def find_new_ref_group(P, group_begin, candidates):
    """estimator.cpp:1394-1407 over the candidate slots: the first minimum in ascending slot order (`cov < best`, strict). Among
    equal sums the reference's order is its unordered_set's; lowest slot is the project's choice."""
    best, arg = math.inf, -1
    for g in sorted(candidates):
        c = group_cov(P, group_begin, g)
        if c < best:
            best, arg = c, g
    return arg


# ---------------------------------------------------------------- RANSAC decisions
def ransac_decisions(mh, sind, ref, low, P, group_begin, n_groups, gauge):
    """mh [F]: the MH mask handed in; an entry with sind < 0 is no inlier whatever the mask says. low [F]: the low-innovation test
    of every entry. Returns dict(state, low (among the MH inliers), tmpref (-1 none), zero_groups, zero_feats (slots)).
      state 0: no MH inlier, or all of them low (update.cpp:263-265); 2: none low (:287); 1 otherwise."""
    mh = np.asarray(mh, dtype=bool) & (np.asarray(sind) >= 0)
    low = np.asarray(low, dtype=bool) & mh
    n_mh, n_low = int(mh.sum()), int(low.sum())
    state = 0 if (n_mh == 0 or n_low == n_mh) else (2 if n_low == 0 else 1)
    out = dict(state=state, low=low, mh=mh, tmpref=-1, zero_groups=[], zero_feats=[])
    if state != 1:
        return out
    active = sorted(set(int(ref[f]) for f in np.nonzero(mh)[0]))
    withlow = sorted(set(int(ref[f]) for f in np.nonzero(low)[0]))
    zg = set()
    if not (0 <= gauge < n_groups and gauge in withlow):        # :292-301
        out["tmpref"] = find_new_ref_group(P, group_begin, withlow)
        zg.add(out["tmpref"])
    zg |= set(active) - set(withlow)                            # :311-317
    out["zero_groups"] = sorted(zg)
    out["zero_feats"] = sorted(int(sind[f]) for f in np.nonzero(mh & ~low)[0])   # :304-310
    return out


def rescue(d, chi2):
    return d < chi2                                             # update.cpp:356, strict
