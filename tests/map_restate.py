"""Test-side numpy restatement of the landmark log (TEST INFRASTRUCTURE ONLY), written from the formulas of include/xivo_hip.h,
not from the kernel: Feature::Xs, the Jacobian of Xs in the error state under the retraction of the absorb step, the
15-column gather, cov_world = J Pcc J^T, the score, the order and the 3 x 3 NEES - in longdouble (on x86-64 an 80-bit float,
eleven mantissa bits more than fp64), so that next to an fp64 device result its own rounding does not show.

Conventions: rotation matrices are ordinary [3, 3] arrays here (the C structs store them column-major: `R(v)` converts);
P is [N, N] with P[r, c] the stored entry of row r, column c; `lay` is a dict(group_begin, n_groups, feature_begin, n_features)."""
import numpy as np

from traj_restate import EPS, LD, hat, nees_cholesky, so3_exp  # noqa: F401

WBC, TBC = 15, 18                                   # Index::Wbc, Index::Tbc of the error state (src/core.h:40-75)
SYM6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # how a symmetric 3 x 3 is packed


def R(v):
    """column-major 9 -> [3, 3]"""
    return np.asarray(v, dtype=LD).reshape(3, 3).T


def unproject(x, invdepth):
    """Feature::Xc and dXc/dx of the local state x = (X/Z, Y/Z, log Z), or (X/Z, Y/Z, 1/Z) in the USE_INVDEPTH build"""
    x = np.asarray(x, dtype=LD)
    if invdepth:
        r = x[2]
        Xc = np.array([x[0] / r, x[1] / r, 1 / r], dtype=LD)
        D = np.array([[1 / r, 0, -x[0] / (r * r)], [0, 1 / r, -x[1] / (r * r)], [0, 0, -1 / (r * r)]], dtype=LD)
    else:
        z = np.exp(x[2])
        Xc = np.array([x[0] * z, x[1] * z, z], dtype=LD)
        D = np.array([[z, 0, x[0] * z], [0, z, x[1] * z], [0, 0, z]], dtype=LD)
    return Xc, D


def world_point(Rbc, Tbc, Rg, Tg, x, invdepth):
    """Feature::Xs = Rsb_g (Rbc Xc(x) + Tbc) + Tsb_g"""
    Xc, _ = unproject(x, invdepth)
    return np.asarray(Rg, dtype=LD) @ (np.asarray(Rbc, dtype=LD) @ Xc + np.asarray(Tbc, dtype=LD)) + np.asarray(Tg, dtype=LD)


def world_point_magnitude(Rbc, Tbc, Rg, Tg, x, invdepth):
    """|Rsb_g| (|Rbc| |Xc| + |Tbc|) + |Tsb_g|, entrywise: what the rounding of an fp64 evaluation of Xs scales with"""
    Xc, _ = unproject(x, invdepth)
    return np.abs(np.asarray(Rg, dtype=LD)) @ (np.abs(np.asarray(Rbc, dtype=LD)) @ np.abs(Xc) + np.abs(np.asarray(Tbc, dtype=LD))) \
        + np.abs(np.asarray(Tg, dtype=LD))


def absorb(Rbc, Tbc, Rg, Tg, x, dx):
    """the retraction of the absorb step on what Xs depends on, dx in the order of `columns`:
    Rbc <- Rbc exp(dx[0:3]), Tbc += dx[3:6], Rsb_g <- Rsb_g exp(dx[6:9]), Tsb_g += dx[9:12], x += dx[12:15]"""
    dx = np.asarray(dx, dtype=LD)

    def rot(Rm, w):
        return np.asarray(Rm, dtype=LD) @ so3_exp(w) if np.any(w != 0) else np.asarray(Rm, dtype=LD)
    return (rot(Rbc, dx[0:3]), np.asarray(Tbc, dtype=LD) + dx[3:6], rot(Rg, dx[6:9]), np.asarray(Tg, dtype=LD) + dx[9:12],
            np.asarray(x, dtype=LD) + dx[12:15])


def jacobian(Rbc, Tbc, Rg, Tg, x, invdepth):
    """dXs / d(error state) [3, 15]. With R exp(w) v = R v + R (w x v) + O(w^2) = R v - R hat(v) w:
      Wbc: -Rsb_g Rbc hat(Xc)    Tbc: Rsb_g    Wsb_g: -Rsb_g hat(Rbc Xc + Tbc)    Tsb_g: I    x: Rsb_g Rbc dXc/dx"""
    Rbc = np.asarray(Rbc, dtype=LD); Rg = np.asarray(Rg, dtype=LD)
    Xc, D = unproject(x, invdepth)
    Xb = Rbc @ Xc + np.asarray(Tbc, dtype=LD)
    return np.hstack([-(Rg @ Rbc) @ hat(Xc), Rg, -Rg @ hat(Xb), np.eye(3, dtype=LD), (Rg @ Rbc) @ D])


def jacobian_fd(Rbc, Tbc, Rg, Tg, x, invdepth, h=1e-6):
    """central differences of Xs through the retraction"""
    J = np.zeros((3, 15), dtype=LD)
    for k in range(15):
        d = np.zeros(15, dtype=LD); d[k] = LD(h)
        J[:, k] = (world_point(*absorb(Rbc, Tbc, Rg, Tg, x, d), invdepth) - world_point(*absorb(Rbc, Tbc, Rg, Tg, x, -d), invdepth)) / (2 * LD(h))
    return J


def columns(lay, ref_sind, sind):
    """the 15 error-state columns Xs depends on"""
    g = lay["group_begin"] + 6 * ref_sind
    f = lay["feature_begin"] + 3 * sind
    return list(range(WBC, WBC + 3)) + list(range(TBC, TBC + 3)) + list(range(g, g + 6)) + list(range(f, f + 3))


def gather(P, cols):
    """P[cols, cols] from the LOWER triangle of the stored P, mirrored"""
    n = len(cols)
    out = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(n):
            out[i, j] = P[max(cols[i], cols[j]), min(cols[i], cols[j])]
    return out


def score(P, lay, sind):
    """Frobenius norm of the 3 x 3 block as stored (all nine entries)"""
    o = lay["feature_begin"] + 3 * sind
    B = np.asarray(P[o:o + 3, o:o + 3], dtype=LD)
    return np.sqrt((B * B).sum())


def order(scores, positions):
    """ascending score, ties by ascending position -> the positions in that order"""
    return [p for _, p in sorted(zip([float(s) for s in scores], positions))]


def pack6(S):
    return np.array([S[r, c] for r, c in SYM6], dtype=LD)


def unpack6(v):
    S = np.zeros((3, 3), dtype=np.asarray(v).dtype)
    for k, (r, c) in enumerate(SYM6):
        S[r, c] = S[c, r] = v[k]
    return S


def record(pose, groups, feats, P, lay, n_out, invdepth=False, world=True):
    """One filter's record from its scene (numpy records of xivo_pose_in / xivo_group_in [n_groups] / xivo_feat_in [F]) and its
    stored P [N, N]. -> list of at most n_out dicts, best first: pos, sind, ref_sind, score, Xs, Xs_mag, cov_local (fp64,
    exact copies), xp, cov_world, cov_world_mag = |J| |Pcc| |J|^T (packed six), J, cols"""
    present = [j for j in range(len(feats)) if feats[j]["sind"] >= 0]
    sc = {j: score(P, lay, int(feats[j]["sind"])) for j in present}
    out = []
    for j in order([sc[j] for j in present], present)[:n_out]:
        f = feats[j]
        sind, ref = int(f["sind"]), int(f["ref_sind"])
        geo = (R(pose["Rbc"]), pose["Tbc"], R(groups[ref]["Rsb"]), groups[ref]["Tsb"], f["x"], invdepth)
        o = lay["feature_begin"] + 3 * sind
        e = dict(pos=j, sind=sind, ref_sind=ref, score=sc[j], Xs=world_point(*geo), Xs_mag=world_point_magnitude(*geo),
                 cov_local=np.array([P[o + c, o + r] for r, c in SYM6]), xp=np.array(f["xp"]))
        if world:
            cols = columns(lay, ref, sind)
            J = jacobian(*geo); Pcc = gather(P, cols)
            e.update(J=J, cols=cols, cov_world=pack6(J @ Pcc @ J.T), cov_world_mag=pack6(np.abs(J) @ np.abs(Pcc) @ np.abs(J).T))
        else:
            e.update(cov_world=np.zeros(6, dtype=LD), cov_world_mag=np.zeros(6, dtype=LD))
        out.append(e)
    return out


def nees3(Xs, cov6, gt):
    """|L^-1 (gt - Xs)|^2 with cov = L L^T un-pivoted; NaN when a pivot is not positive"""
    return nees_cholesky(unpack6(np.asarray(cov6, dtype=LD)), np.asarray(gt, dtype=LD) - np.asarray(Xs, dtype=LD))


def anees(values):
    """mean of the finite values and their number"""
    v = np.asarray(values, dtype=LD).reshape(-1)
    fin = v[np.isfinite(v.astype(np.float64))]
    return (fin.mean() if fin.size else LD(np.nan)), int(fin.size)
