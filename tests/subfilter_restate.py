"""Feature::SubfilterUpdate (src/feature.cpp:246-297 of the reference) and Criteria::Candidate(Strict) (src/options.cpp:10-33)
in a dtype, line for line as oracle/xivo_oracle.py::subfilter_update states them. np.longdouble (on x86-64 an 80-bit float with
eleven more mantissa bits) stands for the exact answer next to an fp64 result, as in tests/precise_ref.py and
tests/geometry_edge_cases.py; the cameras and their Jacobians are geometry_edge_cases.project in the same dtype.

Besides the new state the restatement returns what decides a branch: q = inn . S^-1 inn, ratio = q / MH_thresh, whether the
outlier branch was taken, the posterior depth z and the 2-norm condition number of S."""
import numpy as np

import geometry_edge_cases as gc

LD = np.longdouble
FEAT_INITIALIZING, FEAT_READY = 0, 1


def _m(a, T):
    return np.asarray(a, dtype=T)


def feature_xc(x, invdepth, T=LD):
    """Feature::Xc(&dXc_dx) (feature.cpp:98-105): unproject_logz (project.h:79-95) or unproject_invz (:52-56) -> (Xc, J)"""
    zero = T(0)
    if invdepth:
        r = x[2]
        return (np.array([x[0] / r, x[1] / r, T(1) / r], dtype=T),
                np.array([[T(1) / r, zero, -x[0] / (r * r)], [zero, T(1) / r, -x[1] / (r * r)], [zero, zero, -T(1) / (r * r)]], dtype=T))
    z = np.exp(x[2])
    return (np.array([x[0] * z, x[1] * z, z], dtype=T),
            np.array([[z, zero, x[0] * z], [zero, z, x[1] * z], [zero, zero, z]], dtype=T))


def feature_z(x2, invdepth, T=LD):
    """Feature::z (feature.cpp:120-126)"""
    with np.errstate(all="ignore"):
        return T(1) / T(x2) if invdepth else np.exp(T(x2))


def subfilter_update(x, P, xp_meas, Rsb, Tsb, Rbc, Tbc, Rsbr, Tsbr, cam, Rtri=3.5, MH_thresh=5.991, ready_steps=5,
                     init_counter=0, outlier_counter=0.0, invdepth=False, T=LD):
    """-> dict(x [3], P [3, 3] row-major, status, init_counter, outlier_counter, q, ratio, outlier (the branch of :279),
    z (Feature::z of the new x), kappa (cond_2 of S before the inflation of :280-281), inn [2])"""
    x = _m(x, T); P = _m(P, T)
    Rsb, Tsb, Rbc, Tbc, Rsbr, Tsbr = (_m(a, T) for a in (Rsb, Tsb, Rbc, Tbc, Rsbr, Tsbr))
    Rtri, MH_thresh = T(Rtri), T(MH_thresh)
    init_counter = int(init_counter) + 1                           # :255
    Xc, dXc_dx = feature_xc(x, invdepth, T)                        # :258
    Rsc, Tsc = Rsb @ Rbc, Rsb @ Tbc + Tsb                          # :259 gtot = (gsb * gbc)^-1 * ref.gsb * gbc
    Rrc, Trc = Rsbr @ Rbc, Rsbr @ Tbc + Tsbr
    Rtot, Ttot = Rsc.T @ Rrc, Rsc.T @ (Trc - Tsc)
    Xcn = Rtot @ Xc + Ttot                                         # :260
    zero = T(0)
    dxcn_dXcn = np.array([[T(1) / Xcn[2], zero, -Xcn[0] / (Xcn[2] * Xcn[2])],
                          [zero, T(1) / Xcn[2], -Xcn[1] / (Xcn[2] * Xcn[2])]], dtype=T)   # :263 project(Xcn, &dxcn_dXcn)
    xp, dxp_dxcn = gc.project(cam, Xcn[0] / Xcn[2], Xcn[1] / Xcn[2], T=T)[:2]             # :266
    H = ((dxp_dxcn @ dxcn_dXcn) @ Rtot) @ dXc_dx                   # :268
    inn = _m(xp_meas, T) - xp                                      # :269
    S = H @ P @ H.T                                                # :271
    S[0, 0] += Rtri; S[1, 1] += Rtri                               # :273-274
    tr, dt = S[0, 0] + S[1, 1], S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    disc = np.sqrt(((S[0, 0] - S[1, 1]) / 2) ** 2 + S[0, 1] * S[1, 0])
    kappa = float((tr / 2 + disc) / (dt / (tr / 2 + disc)))        # lambda_max / lambda_min, lambda_min = det / lambda_max
    sol = np.array([S[1, 1] * inn[0] - S[0, 1] * inn[1], S[0, 0] * inn[1] - S[1, 0] * inn[0]], dtype=T) / dt
    q = inn @ sol
    ratio = q / MH_thresh                                          # :276
    outlier_counter = T(outlier_counter)
    outlier = bool(ratio > 1)
    if outlier:                                                    # :278-284
        S[0, 0] += Rtri * (ratio - 1); S[1, 1] += Rtri * (ratio - 1)
        outlier_counter = outlier_counter + np.sqrt(ratio)
    else:
        outlier_counter = T(0)
    dt = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    Sinv = np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]], dtype=T) / dt
    K = P @ H.T @ Sinv                                             # :286
    xn = x + K @ inn                                               # :288
    I_KH = np.eye(3, dtype=T) - K @ H
    Pn = I_KH @ P @ I_KH.T + K * Rtri @ K.T                        # :290
    status = FEAT_READY if init_counter > ready_steps else FEAT_INITIALIZING   # :292-296
    return dict(x=xn, P=Pn, status=status, init_counter=init_counter, outlier_counter=outlier_counter, q=q, ratio=ratio,
                outlier=outlier, z=feature_z(xn[2], invdepth, T), kappa=kappa, inn=inn)


def candidate_bits(outlier_counter, z, status, min_depth, max_depth, max_subfilter_outlier):
    """bit 0: Criteria::Candidate, bit 1: Criteria::CandidateStrict (options.cpp:10-33), on values of any dtype"""
    ok = bool(outlier_counter < max_subfilter_outlier) and bool(z > min_depth) and bool(z < max_depth)
    return (1 if ok else 0) | (2 if ok and status == FEAT_READY else 0)
