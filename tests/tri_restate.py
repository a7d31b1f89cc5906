"""Test-side numpy restatement of the reference's two-view triangulation (TEST INFRASTRUCTURE ONLY).

Feature::Triangulate (src/feature.cpp:686-751) and the five triangulators of src/helpers.cpp:103-371, vectorised over n
problems. Each problem is (R12, t12, xc1, xc2): g12 maps frame-2 points into frame 1, xc1 / xc2 are normalised image
coordinates. The reference's float narrowing is restated with np.float32 at the same points: a0 / a1 (:184-185),
lambda0 / lambda1 (:331-332), theta0 / theta1 (:347-348), max_theta (:350), beta (:362) and the float thresholds of the
*Angular functions (:161, :231, :282). Everything else is fp64 in Eigen's association order.
"""
import numpy as np

METHODS = ("direct_linear_transform_svd", "direct_linear_transform_avg", "l1_angular", "l2_angular", "linf_angular")
ANGULAR = ("l1_angular", "l2_angular", "linf_angular")
DEG = np.pi / 180


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm(a):
    return np.sqrt(dot(a, a))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def mulv(R, x):
    """R [n, 3, 3] times x [n, 3], each row summed left to right"""
    return np.stack([(R[:, i, 0] * x[:, 0] + R[:, i, 1] * x[:, 1]) + R[:, i, 2] * x[:, 2] for i in range(3)], axis=-1)


def mulvt(R, x):
    return mulv(np.transpose(R, (0, 2, 1)), x)


def normalized(a):
    """Eigen normalize() (divide by sqrt of the squared norm when it is > 0)"""
    z = dot(a, a)
    s = np.where(z > 0, np.sqrt(z), 1.0)
    return a / s[:, None]


def homog(xc):
    return np.concatenate([np.asarray(xc, dtype=np.float64), np.ones((len(xc), 1))], axis=1)


def _f32(x):
    with np.errstate(invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def _acos(x):
    with np.errstate(invalid="ignore"):
        return np.arccos(x)


def check_cheirality(z, t, f1p, Rf0p):
    """helpers.cpp:327-341"""
    zn = norm(z)
    zz = zn * zn
    with np.errstate(invalid="ignore", divide="ignore"):
        lam0 = _f32(dot(z, cross(t, f1p)) / zz)
        lam1 = _f32(dot(z, cross(t, Rf0p)) / zz)
        return ~((lam0 <= 0) | (lam1 <= 0))


def check_angular_reprojection(Rf0, Rf0p, f1, f1p, thresh):
    """helpers.cpp:344-357; std::max(a, b) = a < b ? b : a (a NaN theta0 wins)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        th0 = _f32(_acos(dot(Rf0, Rf0p) / (norm(Rf0) * norm(Rf0p))))
        th1 = _f32(_acos(dot(f1, f1p) / (norm(f1) * norm(f1p))))
        mx = np.where(th0 < th1, th1, th0)
        return ~(mx > np.float32(thresh))


def check_parallax(Rf0p, f1p, thresh):
    """helpers.cpp:359-371"""
    with np.errstate(invalid="ignore", divide="ignore"):
        beta = _f32(_acos(dot(f1p, Rf0p) / (norm(f1p) * norm(Rf0p))))
        return ~(beta < np.float32(thresh))


def l2_normal(m0h, m1h, t):
    """L2Angular's n' = V.col(1) of B = A^T (I - t^ t^T): B t^ = 0, so it is the minor eigenvector of B^T B in the plane
    perpendicular to t^ (basis e1 = the longer row of B normalised, e2 = t^ x e1; sign free). Same steps as the device's."""
    th = t / norm(t)[:, None]
    M = np.eye(3)[None] - th[:, :, None] * th[:, None, :]
    b0 = (m0h[:, 0, None] * M[:, 0, :] + m0h[:, 1, None] * M[:, 1, :]) + m0h[:, 2, None] * M[:, 2, :]
    b1 = (m1h[:, 0, None] * M[:, 0, :] + m1h[:, 1, None] * M[:, 1, :]) + m1h[:, 2, None] * M[:, 2, :]
    n0, n1 = norm(b0), norm(b1)
    use0 = (n0 >= n1) & (n0 > 0)
    e1 = np.where(use0[:, None], b0 / n0[:, None], b1 / n1[:, None])
    zero = ~use0 & ~(n1 > 0)
    if zero.any():   # B = 0: any vector perpendicular to t^
        a = np.abs(th[zero])
        i = np.where(a[:, 0] <= a[:, 1], np.where(a[:, 0] <= a[:, 2], 0, 2), np.where(a[:, 1] <= a[:, 2], 1, 2))
        u = np.zeros_like(a)
        u[np.arange(len(i)), i] = 1.0
        e1[zero] = normalized(cross(th[zero], u))
    e2 = normalized(cross(th, e1))
    c01, c02, c11, c12 = dot(b0, e1), dot(b0, e2), dot(b1, e1), dot(b1, e2)
    p, q, r = c01 * c01 + c11 * c11, c01 * c02 + c11 * c12, c02 * c02 + c12 * c12
    ang = 0.5 * np.arctan2(2.0 * q, p - r)
    return -np.sin(ang)[:, None] * e1 + np.cos(ang)[:, None] * e2


def l2_sigma_ratio(R12, t12, xc1, xc2):
    """sigma_2 / sigma_1 of L2Angular's B: where it is tiny, B is rank one and V.col(1) of the reference's SVD is any unit
    vector of a two-dimensional null space (the comparison with the compiled reference is then meaningless)"""
    R12 = np.asarray(R12, dtype=np.float64).reshape(-1, 3, 3)
    f0, f1 = normalized(homog(np.reshape(xc1, (-1, 2)))), normalized(homog(np.reshape(xc2, (-1, 2))))
    t10 = -mulvt(R12, np.reshape(t12, (-1, 3)))
    m0 = mulvt(R12, f0)
    th = t10 / norm(t10)[:, None]
    M = np.eye(3)[None] - th[:, :, None] * th[:, None, :]
    B = np.stack([m0 / norm(m0)[:, None], f1 / norm(f1)[:, None]], axis=1) @ M
    out = np.zeros(len(B))
    ok = np.isfinite(B).all(axis=(1, 2))
    if ok.any():
        s = np.linalg.svd(B[ok], compute_uv=False)
        out[ok] = s[:, 1] / s[:, 0]
    return out


def triangulate(method, R12, t12, xc1, xc2, max_theta_thresh=0.1 * DEG, beta_thresh=0.25 * DEG, details=False):
    """-> (X [n, 3], ret [n] bool); details=True adds a dict of the float quantities the branches compare"""
    R12 = np.asarray(R12, dtype=np.float64).reshape(-1, 3, 3)
    t12 = np.asarray(t12, dtype=np.float64).reshape(-1, 3)
    f0, f1 = normalized(homog(np.reshape(xc1, (-1, 2)))), normalized(homog(np.reshape(xc2, (-1, 2))))
    n = len(R12)
    info = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        if method == "direct_linear_transform_svd":          # :103-131
            A = np.zeros((n, 4, 4))
            A[:, 0, 0], A[:, 0, 2] = -f0[:, 2], f0[:, 0]
            A[:, 1, 1], A[:, 1, 2] = -f0[:, 2], f0[:, 1]
            P2 = np.zeros((n, 3, 4))
            P2[:, :, :3] = np.transpose(R12, (0, 2, 1))
            P2[:, :, 3] = -mulvt(R12, t12)
            A[:, 2, :] = f1[:, 0, None] * P2[:, 2, :] - f1[:, 2, None] * P2[:, 0, :]
            A[:, 3, :] = f1[:, 1, None] * P2[:, 2, :] - f1[:, 2, None] * P2[:, 1, :]
            ok = np.isfinite(A).all(axis=(1, 2))
            X = np.full((n, 3), np.nan)
            s = np.full((n, 4), np.nan)
            if ok.any():
                _, s[ok], Vt = np.linalg.svd(A[ok])
                v = Vt[:, 3, :]
                X[ok] = v[:, :3] / v[:, 3:4]
            info["sigma"] = s
            return (X, np.ones(n, bool), info) if details else (X, np.ones(n, bool))
        if method == "direct_linear_transform_avg":          # :133-158
            f2u = mulv(R12, f1)
            b0, b1 = dot(t12, f0), dot(t12, f2u)
            a00, a10 = dot(f0, f0), dot(f0, f2u)
            a01, a11 = -a10, -dot(f2u, f2u)
            idet = 1.0 / (a00 * a11 - a10 * a01)
            i00, i10, i01, i11 = a11 * idet, -a10 * idet, -a01 * idet, a00 * idet
            l0, l1 = i00 * b0 + i01 * b1, i10 * b0 + i11 * b1
            X = ((l0[:, None] * f0) + (t12 + l1[:, None] * f2u)) / 2.0
            return (X, np.ones(n, bool), info) if details else (X, np.ones(n, bool))
        t10 = -mulvt(R12, t12)
        m0, m1 = mulvt(R12, f0), f1
        if method == "l1_angular":                           # :161-222
            a0 = _f32(norm(cross(m0 / norm(m0)[:, None], t10)))
            a1 = _f32(norm(cross(m1 / norm(m1)[:, None], t10)))
            first = a0 <= a1
            n1 = cross(m1, t10); n1h = n1 / norm(n1)[:, None]
            n0 = cross(m0, t10); n0h = n0 / norm(n0)[:, None]
            m0p = np.where(first[:, None], m0 - dot(m0, n1h)[:, None] * n1h, m0)
            m1p = np.where(first[:, None], m1, m1 - dot(m1, n0h)[:, None] * n0h)
            info.update(a0=a0, a1=a1)
        else:
            m0h, m1h = m0 / norm(m0)[:, None], m1 / norm(m1)[:, None]
            if method == "l2_angular":                       # :226-274: V.col(1) of B = A^T (I - t^ t^T)
                np_ = l2_normal(m0h, m1h, t10)
            elif method == "linf_angular":                   # :277-325: n' NOT normalised, as coded
                na, nb = cross(m0h + m1h, t10), cross(m0h - m1h, t10)
                np_ = np.where((norm(na) >= norm(nb))[:, None], na, nb)
            else:
                raise ValueError(method)
            m0p = m0 - dot(m0, np_)[:, None] * np_
            m1p = m1 - dot(m1, np_)[:, None] * np_
        z = cross(m1p, m0p)
        zn = norm(z)
        X = (dot(z, cross(t10, m0p)) / (zn * zn))[:, None] * m1p
        X = mulv(R12, X) + t12
        c1 = check_cheirality(z, t10, m1p, m0p)
        c2 = check_angular_reprojection(m0, m0p, m1, m1p, max_theta_thresh)
        c3 = check_parallax(m0p, m1p, beta_thresh)
        ret = c1 & c2 & c3
        if details:
            zz = zn * zn
            info.update(lam0=dot(z, cross(t10, m1p)) / zz, lam1=dot(z, cross(t10, m0p)) / zz,
                        th0=_acos(dot(m0, m0p) / (norm(m0) * norm(m0p))), th1=_acos(dot(m1, m1p) / (norm(m1) * norm(m1p))),
                        beta=_acos(dot(m1p, m0p) / (norm(m1p) * norm(m0p))),
                        arg0=dot(m0, m0p) / (norm(m0) * norm(m0p)), argb=dot(m1p, m0p) / (norm(m1p) * norm(m0p)))
            return X, ret, info
        return X, ret


def near_threshold(method, info, n, max_theta_thresh, beta_thresh, rel=1e-6):
    """problems whose branch quantity lies within rel of a float threshold (or of 0 for the cheirality lambdas, of each
    other for L1's a0 / a1): a last-bit difference may flip their return value"""
    if method not in ANGULAR:
        return np.zeros(n, bool)
    tt, bt = float(np.float32(max_theta_thresh)), float(np.float32(beta_thresh))
    with np.errstate(invalid="ignore"):
        near = (np.abs(info["th0"] - tt) <= rel * tt) | (np.abs(info["th1"] - tt) <= rel * tt)
        # acos at the edge of its domain: an unmodified ray gives acos(1 +- 1 ulp) = NaN or 0; a NaN theta0 (the first
        # operand of std::max) or beta passes its check, a 0 does not
        near |= (np.abs(info["arg0"] - 1) <= 8e-16) & ~(np.float32(info["th1"]) <= np.float32(tt))
        near |= np.abs(info["argb"] - 1) <= 8e-16
        near |= np.abs(info["beta"] - bt) <= rel * bt
        scale = np.maximum(np.abs(info["lam0"]), np.abs(info["lam1"]))
        near |= (np.abs(info["lam0"]) <= 1e-12 * scale) | (np.abs(info["lam1"]) <= 1e-12 * scale)
        if method == "l1_angular":
            a0, a1 = info["a0"].astype(np.float64), info["a1"].astype(np.float64)
            near |= np.abs(a0 - a1) <= rel * np.maximum(a0, a1)
    return near


def good(ret, X, zmin, zmax):
    """Feature::Triangulate's acceptance (feature.cpp:733-747) as the device states it: zmin <= z <= zmax"""
    with np.errstate(invalid="ignore"):
        return ret & (X[:, 2] >= zmin) & (X[:, 2] <= zmax)


def fit_to_so3(R):
    """SE3::fitToSE3's rotation: the SVD projection onto SO(3) (Sophus so3.hpp fitToSO3)"""
    U, _, Vt = np.linalg.svd(R)
    d = np.sign(np.linalg.det(U @ Vt))
    return U @ np.diag([1.0, 1.0, d]) @ Vt


# The reference's own unit-test cases, src/test/unittest_triangulation.cpp: (name, xc1, z1, g21 [4x4], pixel noise on xc2,
# the three angular methods' expected return). g12 = fitToSE3(g21^-1); xc2 = projection of (xc1 z1, z1) by g21 (+ noise).
UNIT_CASES = [
    ("Normal_Inputs", (0.4, 0.6), 5.0,                                             # :18-61
     [[0.9849082, 0, 0.1731, -9.8490], [0, 1, 0, 0], [-0.17310, 0, 0.98490, 1.73101], [0, 0, 0, 1]], 0.0, True),
    ("Parallax", (2.2, 0.7), 5.0,                                                  # :64-95
     [[0.9998, 0, 0.01745, -0.01], [0, 1, 0, 0], [-0.01745, 0, 0.9998, 0], [0, 0, 0, 1]], 0.0, False),
    ("Cheirality", (2.0, -0.77), 5.0,                                              # :98-130
     [[-1, 0, 0, 3], [0, 1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], 0.0, False),
    ("Angular_Reprojection_Error", (2.22216, 0.778023), 5.0,                       # :132-170
     [[1, 0, 0, 3], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], 0.7, False),
    ("Vanishing_Point", (0.2, 0.3), 6000.0,                                        # :173-208
     [[1, 0, 0, -0.1], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], 0.0, False),
]


def unit_case(case):
    """-> (R12, t12, xc1, xc2) of one UNIT_CASES entry"""
    _, xc1, z1, g21, noise, _ = case
    g21 = np.array(g21, dtype=np.float64)
    z1 = float(np.float32(z1))
    X1 = np.array([xc1[0] * z1, xc1[1] * z1, z1, 1.0])
    X2 = g21 @ X1
    xc2 = np.array([X2[0] / X2[2] + noise, X2[1] / X2[2] + noise])
    g12 = np.linalg.inv(g21)
    return fit_to_so3(g12[:3, :3]), g12[:3, 3].copy(), np.array(xc1, dtype=np.float64), xc2


def random_problems(rng, n, kind):
    """n two-view problems of one kind -> (R12, t12, xc1, xc2, Xtrue [n, 3] in frame 1, noise-free flag)
    kind: "good" well-conditioned, "lowpar" small baseline, "behind" point behind camera 2, "noisy" pixel noise,
    "degenerate" zero / ray-parallel baselines, "threshold" parallax / reprojection near the default thresholds"""
    from xivo_amd.pcw import so3_exp
    R12 = np.stack([so3_exp(rng.normal(size=3) * 0.15) for _ in range(n)])
    X1 = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(0.5, 6.0, n)], axis=1)
    t12 = rng.normal(size=(n, 3)) * 0.3
    noise = 0.0
    if kind == "lowpar":
        t12 *= 10.0 ** rng.uniform(-5, -2, (n, 1))
    elif kind == "behind":
        t12[:, 2] += X1[:, 2] + rng.uniform(0.2, 2.0, n)          # camera 2 in front of the point: it lies behind it
    elif kind == "noisy":
        noise = 10.0 ** rng.uniform(-4, -2, (n, 1))
    elif kind == "degenerate":
        t12[: n // 3] = 0.0
        ray = X1[n // 3: 2 * n // 3]
        t12[n // 3: 2 * n // 3] = ray * rng.uniform(-0.5, 0.5, (len(ray), 1))   # baseline along the ray
    elif kind == "threshold":
        # baselines whose parallax angle at the point straddles beta_thresh = 0.25 deg
        ang = np.deg2rad(rng.uniform(0.2, 0.3, n))
        d = norm(X1)
        perp = cross(X1, rng.normal(size=(n, 3)))
        perp /= norm(perp)[:, None]
        t12 = perp * (d * np.tan(ang))[:, None]
        noise = 10.0 ** rng.uniform(-7, -5, (n, 1))
    X2 = mulvt(R12, X1 - t12)                                    # frame-2 coordinates: X1 = R12 X2 + t12
    xc1 = X1[:, :2] / X1[:, 2:3]
    xc2 = X2[:, :2] / X2[:, 2:3]
    if np.any(noise):
        xc2 = xc2 + rng.normal(size=xc2.shape) * noise
    return R12, t12, xc1, xc2, X1, not np.any(noise)
