"""Test-side numpy restatement of the trajectory log (TEST INFRASTRUCTURE ONLY): the packed index of the recorded covariance
block, the pose error in the filter's error coordinates and its NEES - in longdouble (on x86-64 an 80-bit float, eleven
mantissa bits more than fp64), so that next to an fp64 device result its own rounding does not show.

numpy.linalg has no longdouble solve: `solve_ld` is Gaussian elimination with partial pivoting written out here, and
tests/test_traj_log_cpu.py pins it to numpy.linalg.solve where fp64 is enough to tell."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def pack_index(i, j):
    """position of the entry of list positions (i, j), i >= j, in the packed lower triangle (row by row)"""
    assert i >= j >= 0
    return i * (i + 1) // 2 + j


def pack_lower(P, cols):
    """what the record keeps of P [N, N] for the column list `cols`: entry (i, j) from the LOWER triangle of P"""
    n = len(cols)
    out = np.zeros(n * (n + 1) // 2, dtype=P.dtype)
    for i in range(n):
        for j in range(i + 1):
            out[pack_index(i, j)] = P[max(cols[i], cols[j]), min(cols[i], cols[j])]
    return out


def unpack_block(packed, pos):
    """the symmetric block on the list positions `pos` of one packed record"""
    S = np.zeros((len(pos), len(pos)), dtype=packed.dtype)
    for a, pa in enumerate(pos):
        for b, pb in enumerate(pos):
            S[a, b] = packed[pack_index(max(pa, pb), min(pa, pb))]
    return S


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)


def so3_exp(w):
    """Rodrigues in longdouble (angles well away from 0 and pi only: the tests' range)"""
    w = np.asarray(w, dtype=LD)
    th = np.sqrt(w @ w)
    W = hat(w)
    return np.eye(3, dtype=LD) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


def so3_log(R):
    """rotation vector of R in longdouble, angle in (0, pi)"""
    R = np.asarray(R, dtype=LD)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=LD) / 2       # sin(th) axis
    s = np.sqrt(v @ v)
    th = np.arctan2(s, (np.trace(R) - 1) / 2)
    return v * (th / s)


def retract(R, T, e):
    """the pose absorb_error_kernel makes of (R, T) and the error-state segment e: R exp(e[:3]), T + e[3:]"""
    e = np.asarray(e, dtype=LD)
    return np.asarray(R, dtype=LD) @ so3_exp(e[:3]), np.asarray(T, dtype=LD) + e[3:]


def pose_error(R_est, T_est, R_gt, T_gt):
    """e with retract(est, e) = gt"""
    R_est = np.asarray(R_est, dtype=LD)
    return np.concatenate([so3_log(R_est.T @ np.asarray(R_gt, dtype=LD)), np.asarray(T_gt, dtype=LD) - np.asarray(T_est, dtype=LD)])


def solve_ld(A, b):
    """A x = b in longdouble, Gaussian elimination with partial pivoting"""
    A = np.array(A, dtype=LD); b = np.array(b, dtype=LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]; b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]; b[i] -= f * b[k]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def nees_solve(S, e):
    """e^T S^-1 e through the general solve"""
    e = np.asarray(e, dtype=LD)
    return e @ solve_ld(S, e)


def nees_cholesky(S, e, dtype=LD):
    """The device's expression: S = L L^T un-pivoted, |L^-1 e|^2; NaN when a pivot is not positive"""
    S = np.array(S, dtype=dtype); e = np.array(e, dtype=dtype)
    n = len(e)
    L = np.zeros((n, n), dtype=dtype); y = np.zeros(n, dtype=dtype)
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return dtype(np.nan)
        L[j, j] = np.sqrt(d)
        y[j] = (e[j] - L[j, :j] @ y[:j]) / L[j, j]
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return y @ y


def spd_with_spectrum(rng, eig):
    """a symmetric matrix with the eigenvalues `eig` on a random orthogonal basis (fp64, symmetric bit for bit)"""
    Q, _ = np.linalg.qr(rng.normal(size=(len(eig), len(eig))))
    S = (Q * np.asarray(eig)) @ Q.T
    return np.tril(S) + np.tril(S, -1).T


def frame_mean_tree(values):
    """The device's mean of the finite values of one frame (frame_anees_kernel), addition for addition in fp64: thread tid of 256
    adds the finite entries tid, tid + 256, ... in ascending order, a halving tree adds the 256 partial sums and counts, one
    division -> (mean, number of finite values); (NaN, 0) when nothing is finite"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    s = np.zeros(256, dtype=np.float64)
    c = np.zeros(256, dtype=np.int64)
    for tid in range(256):
        for x in v[tid::256]:
            if np.isfinite(x):
                s[tid] = s[tid] + x
                c[tid] += 1
    h = 128
    while h > 0:
        s[:h] = s[:h] + s[h:2 * h]
        c[:h] = c[:h] + c[h:2 * h]
        h //= 2
    return (s[0] / np.float64(c[0]) if c[0] > 0 else np.float64(np.nan)), int(c[0])
