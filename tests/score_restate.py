"""Test-side numpy restatement of the trajectory score (TEST INFRASTRUCTURE ONLY), in the role traj_restate.py has for the
log: the same three passes as the device - centroids, centred cross-covariance, residuals - accumulated in longdouble (on
x86-64 an 80-bit float), the closed-form alignment through numpy.linalg.svd of the longdouble H cast to double, and the RPE
of src/metrics.cpp:110-113 in longdouble. Next to every score it returns the magnitudes the tests' bounds are made of."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
RANK_TOL = 1e-12


def so3_log(R):
    """rotation vector of R in longdouble, angle in [0, pi); the identity gives zero"""
    R = np.asarray(R, dtype=LD)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=LD) / 2       # sin(th) axis
    s = np.sqrt(v @ v)
    if s < LD(1e-12):                                     # th / sin(th) = 1 + th^2 / 6 + ...: 1 to longdouble rounding
        return v * (1 + s * s / 6)
    return v * (np.arctan2(s, (np.trace(R) - 1) / 2) / s)


def kabsch(H):
    """H [3, 3] (any float type) -> (R double: U diag(1, 1, det(U V^T)) V^T of numpy's SVD of H in double, sv)"""
    U, s, Vt = np.linalg.svd(np.asarray(H, dtype=np.float64))
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(U) * np.linalg.det(Vt))) or 1.0])
    return U @ D @ Vt, s


def pack_gt(R, T):
    """[nt, nb, 3, 3], [nt, nb, 3] -> the [nt, nb, 12] the C ABI takes (R column-major, then T)"""
    R = np.asarray(R, dtype=np.float64); nt, nb = R.shape[:2]
    g = np.empty((nt, nb, 12))
    g[:, :, :9] = np.transpose(R, (0, 1, 3, 2)).reshape(nt, nb, 9)
    g[:, :, 9:] = np.asarray(T, dtype=np.float64)
    return g


def score(est_R, est_T, gt_R, gt_T, align=True, rpe_lag=0):
    """One filter: est_R / gt_R [nt, 3, 3], est_T / gt_T [nt, 3] (double, NaN / inf: the frame is left out).
    -> dict with ate, ate_raw, rpe_pos, rpe_rot (longdouble; -1: nothing to average), R [3, 3], T [3] (gt -> est), sv,
    n_used, n_pairs, flags, and the magnitudes of the bounds: rho = rms |x - xbar| + rms |y - ybar|, xbar_norm, ybar_norm,
    kappa = sv0 / (sv1 + sv2), max_T = the largest |Tsb| entry of a used frame, max_rot = the largest |log rot E| of a pair."""
    est_R = np.asarray(est_R, dtype=np.float64); est_T = np.asarray(est_T, dtype=np.float64)
    gt_R = np.asarray(gt_R, dtype=np.float64); gt_T = np.asarray(gt_T, dtype=np.float64)
    nt = est_T.shape[0]
    used = np.array([np.isfinite(est_R[t]).all() and np.isfinite(est_T[t]).all() and np.isfinite(gt_R[t]).all() and
                     np.isfinite(gt_T[t]).all() for t in range(nt)], dtype=bool)
    n = int(used.sum())
    out = dict(n_used=n, n_pairs=0, ate=LD(-1), ate_raw=LD(-1), rpe_pos=LD(-1), rpe_rot=LD(-1), R=np.eye(3), T=np.zeros(3),
               sv=np.zeros(3), flags=1, rho=0.0, xbar_norm=0.0, ybar_norm=0.0, kappa=np.inf, max_T=0.0, max_rot=0.0)
    if n > 0:
        x = gt_T[used].astype(LD); y = est_T[used].astype(LD)
        xb = x.sum(0) / n; yb = y.sum(0) / n                                   # pass 1
        xc = x - xb; yc = y - yb
        H = yc.T @ xc                                                          # pass 2: sum (y - ybar)(x - xbar)^T
        Rk, sv = kabsch(H)
        out["sv"] = sv
        out["flags"] = int(sv[1] <= RANK_TOL * sv[0] or n < 3)
        out["kappa"] = float(sv[0] / (sv[1] + sv[2])) if sv[1] + sv[2] > 0 else np.inf
        if align:
            R = Rk.astype(LD); T = yb - R @ xb
        else:
            R = np.eye(3, dtype=LD); T = np.zeros(3, dtype=LD)
        out["R"], out["T"] = R.astype(np.float64), T.astype(np.float64)
        r = y - (x @ R.T + T)                                                  # pass 3
        out["ate"] = np.sqrt((r * r).sum() / n)
        out["ate_raw"] = np.sqrt(((y - x) ** 2).sum() / n)
        out["rho"] = float(np.sqrt((xc * xc).sum() / n) + np.sqrt((yc * yc).sum() / n))
        out["xbar_norm"] = float(np.sqrt(xb @ xb)); out["ybar_norm"] = float(np.sqrt(yb @ yb))
        out["max_T"] = float(max(np.abs(x).max(), np.abs(y).max()))
    if rpe_lag > 0:
        sp = LD(0); sr = LD(0); k = 0
        for t in range(nt - rpe_lag):
            u = t + rpe_lag
            if not (used[t] and used[u]):
                continue
            RX = gt_R[t].astype(LD).T @ gt_R[u].astype(LD); pX = gt_R[t].astype(LD).T @ (gt_T[u].astype(LD) - gt_T[t].astype(LD))
            RY = est_R[t].astype(LD).T @ est_R[u].astype(LD); pY = est_R[t].astype(LD).T @ (est_T[u].astype(LD) - est_T[t].astype(LD))
            w = so3_log(RX.T @ RY); p = RX.T @ (pY - pX)                       # E = dgX^-1 dgY
            sp += p @ p; sr += w @ w; k += 1
            out["max_rot"] = max(out["max_rot"], float(np.sqrt(w @ w)))
        out["n_pairs"] = k
        if k > 0:
            out["rpe_pos"], out["rpe_rot"] = np.sqrt(sp / k), np.sqrt(sr / k)
    return out


def bounds(ref):
    """the derived fp64 bounds of the device's record against `ref` (a dict of `score`), eps = 2^-52"""
    k = ref["kappa"]
    return dict(ate=64 * EPS * (ref["rho"] + ref["xbar_norm"] + ref["ybar_norm"]),
                R=64 * EPS * k,
                T=64 * EPS * k * ref["xbar_norm"] + 16 * EPS * (ref["xbar_norm"] + ref["ybar_norm"]),
                sv=32 * EPS * float(ref["sv"][0]),
                rpe_pos=64 * EPS * ref["max_T"],
                rpe_rot=64 * EPS + 64 * EPS * max(1.0, ref["max_rot"]))


# ---- generators shared by the CPU and the GPU tests

def rot(w):
    """Rodrigues in double, any angle"""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


def smooth_trajectory(rng, nt, offset=0.0, size=1.0):
    """a smooth random pose trajectory: a few random sinusoids per coordinate; positions about a point at distance `offset`"""
    s = np.linspace(0.0, 0.9, nt) if nt > 1 else np.zeros(1)      # (not a whole period: the last point is not the first)
    c = rng.normal(size=3); c *= offset / np.linalg.norm(c)
    T = np.zeros((nt, 3)); W = np.zeros((nt, 3))
    for k in range(1, 4):
        T += size * rng.normal(size=3) / k * np.sin(2 * np.pi * k * s[:, None] + rng.uniform(0, 2 * np.pi, size=3))
        W += 0.5 * rng.normal(size=3) / k * np.sin(2 * np.pi * k * s[:, None] + rng.uniform(0, 2 * np.pi, size=3))
    return np.array([rot(w) for w in W]), T + c


def moved(rng, R, T, g_R, g_T, noise):
    """est = g * gt with position noise and a small rotation noise: R_est = g_R R exp(n), T_est = g_R T + g_T + n"""
    Re = np.array([g_R @ r @ rot(noise * rng.normal(size=3)) for r in R])
    Te = T @ g_R.T + g_T + noise * rng.normal(size=T.shape)
    return Re, Te
