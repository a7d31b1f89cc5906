"""An extended-precision reference of the measurement update and the metrics its accuracy is judged by.

extended() evaluates the reference's expression (Estimator::UpdateJosephForm, src/estimator.cpp:1257-1288) in numpy
longdouble: on x86-64 an 80-bit float with a 64-bit mantissa, eleven bits more than fp64, so next to an fp64 result it is
the exact answer. The metrics are measured against it:
  rel   ||E||_F / ||P+_ref||_F                          E = P+ - P+_ref (the yardstick of helpers.TOL_P, but exact)
  corr  max |E_ij| / (d_i d_j)                          d = sqrt(diag(P prior)): the error in units of the prior correlation,
                                                        blind to how many decades the variances of the states span
  dx    ||(dx - dx_ref) / d|| / ||dx_ref / d||          the correction in units of the prior standard deviations
and bounded by tol = C u (kappa_2(S) + N), u = 2^-53: what a backward-stable evaluation of the update can promise. A float
leak (2.5e-8 on these shapes) or an error confined to the states with the smallest variances is many times over it, while
helpers.TOL_P (1e-6, relative Frobenius) sees neither."""
import numpy as np

U = 2.0 ** -53
C_DEFAULT = 8.0
LD = np.longdouble


class Ref:
    """The extended-precision update of one filter: P (P+), dx, kappa (kappa_2(S)), and d (the prior's standard deviations)."""
    __slots__ = ("P", "dx", "kappa", "d", "N")

    def __init__(self, P, dx, kappa, d):
        self.P, self.dx, self.kappa, self.d, self.N = P, dx, kappa, d, P.shape[0]


def _chol(S):
    M = S.shape[0]
    L = np.zeros_like(S)
    for j in range(M):
        L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def extended(H, P, inn, R, keep=None):
    """The Joseph update of estimator.cpp:1257-1288 in longdouble: S = H P H^T + R, K = P H^T S^-1 (extended-precision
    Cholesky and two substitutions: numpy.linalg has no longdouble solve), dx = K inn, P+ = (I - K H) P (I - K H)^T + K R K^T.
    keep: a boolean mask of the rows that take part (the rows the gate kept); the others are dropped before anything else.
    kappa_2(S) comes from the fp64 rounding of S (it only sizes a bound)."""
    H, inn, R = np.asarray(H), np.asarray(inn), np.asarray(R)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        H, inn, R = H[keep], inn[keep], R[keep]
    Hl, Pl, Rl = H.astype(LD), np.asarray(P).astype(LD), R.astype(LD)
    HP = Hl @ Pl
    S = HP @ Hl.T + np.diag(Rl)
    L = _chol(S)
    M = S.shape[0]
    Y = np.zeros_like(HP)
    for i in range(M):
        Y[i] = (HP[i] - L[i, :i] @ Y[:i]) / L[i, i]
    Kt = np.zeros_like(Y)
    for i in range(M - 1, -1, -1):
        Kt[i] = (Y[i] - L[i + 1:, i] @ Kt[i + 1:]) / L[i, i]
    K = Kt.T
    A = np.eye(Pl.shape[0], dtype=LD) - K @ Hl
    Pn = A @ Pl @ A.T + (K * Rl) @ K.T
    dx = K @ inn.astype(LD)
    d = np.sqrt(np.diag(np.asarray(P, dtype=np.float64)))
    return Ref(Pn, dx, float(np.linalg.cond(S.astype(np.float64))), d)


def extended_batch(H, P, inn, R, keep=None):
    """extended() of every filter of a batch, each distinct filter evaluated once (edge batches repeat a few)."""
    out, seen = [], {}
    for b in range(len(P)):
        key = (H[b].tobytes(), P[b].tobytes(), inn[b].tobytes(), R[b].tobytes(),
               None if keep is None else np.asarray(keep[b], dtype=bool).tobytes())
        if key not in seen:
            seen[key] = extended(H[b], P[b], inn[b], R[b], None if keep is None else keep[b])
        out.append(seen[key])
    return out


def metrics(ref, P_new, dx=None):
    """(rel, corr, dx) of an fp64 result against the extended-precision reference (dx None: not measured)."""
    E = np.asarray(P_new).astype(LD) - ref.P
    rel = float(np.linalg.norm(E.astype(np.float64)) / np.linalg.norm(ref.P.astype(np.float64)))
    dd = ref.d.astype(LD)
    corr = float(np.max(np.abs(E) / np.outer(dd, dd)))
    rdx = None
    if dx is not None:
        ed = ((np.asarray(dx).astype(LD) - ref.dx) / dd).astype(np.float64)
        rdx = float(np.linalg.norm(ed) / np.linalg.norm((ref.dx / dd).astype(np.float64)))
    return rel, corr, rdx


def pow2_scales(N, seed):
    """D = 2^e per state, e in [-20, 2], one exponent per 3-column block (XIVO's states come in 3-vectors); the blocks over
    columns 16..31 (0..15 for N < 32, all of them for N < 16) all below 2^-15. Variances then span 2^-40 .. 2^4 with a whole
    16-column block of the smallest, as biases, calibration and td sit next to pose and features in XIVO's state."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-20, 3, size=(N + 2) // 3)
    lo = 16 if N >= 32 else 0
    low = slice(lo // 3, (lo + 16 + 2) // 3)
    e[low] = rng.integers(-20, -15, size=len(e[low]))
    return np.ldexp(1.0, np.repeat(e, 3)[:N])


def scale(D, P, H):
    """The same filter in other units: P -> D P D, H -> H D^-1 (exact for powers of two that keep every value normal)"""
    return P * np.outer(D, D), H / D


def tol(ref, C=C_DEFAULT):
    """C u (kappa_2(S) + N)"""
    return C * U * (ref.kappa + ref.N)


def check(ref, P_new, dx=None, C=C_DEFAULT, what="", corr=True):
    """Assert rel, corr (unless corr=False) and dx (when given) within tol(ref, C); returns the three ratios
    metric / (u (kappa + N))."""
    rel, cr, rdx = metrics(ref, P_new, dx)
    t = tol(ref, C)
    assert rel < t, ("rel", what, rel, t, ref.kappa)
    assert not corr or cr < t, ("corr", what, cr, t, ref.kappa)
    if dx is not None:
        assert rdx < t, ("dx", what, rdx, t, ref.kappa)
    unit = U * (ref.kappa + ref.N)
    return rel / unit, cr / unit, (rdx / unit if rdx is not None else None)
