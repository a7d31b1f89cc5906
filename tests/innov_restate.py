"""The innovation log's record restated in numpy longdouble from what xivo_hip_get_H and xivo_hip_get_err return after the
update, and the bounds tests/test_innov_log_gpu.py and tests/test_innov_log_cpu.py hold the device (the row driver) to.

With r = inn - H dx over the COUNTED rows (a non-zero H entry, or inn != 0):
  nis = sum inn r / R,  prefit = sum inn^2 / R,  postfit = sum r^2 / R
A structurally zero entry of H is not multiplied (xivo_amd/csrc/innov_device.h): 0 * NaN does not reach the sums.

Bounds, u = 2^-53, w = the slots read per row (28 of a compressed pair, + 48 with a lead block, N of a dense row), s = the
longest addition chain of the reductions from rows to the filter (ceil(M / 256) per thread + the 8 levels of the tree):
  |nis - restated|      <= (w + s + 8) u sum |inn| (|inn| + (|H||dx|)) / R
  |prefit - restated|   <= (w + s + 8) u sum inn^2 / R
  |postfit - restated|  <= (w + s + 8) u sum |r| (|r| + 2 (|H||dx|)) / R
First order: (H dx)_i carries w u (|H||dx|)_i, r one more rounding, each term a product and a quotient (3 u in all on
|inn| |r| / R, |r| <= |inn| + |H||dx|), the sums s u of the sum of the magnitudes."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
W_PAIR, W_LEAD = 28, 48
THREADS, TREE_DEPTH = 256, 8


def chain(M):
    """s of a filter with M rows"""
    return -(-M // THREADS) + TREE_DEPTH


def restate(H, inn, R, dx, status=0, ldlt=0, w=None):
    """-> dict(nis, prefit, postfit, inn_max, dx_max, dof, rows, flags, b_nis, b_prefit, b_postfit); H [M, N], the vectors
    as the context holds them. w: slots per row (default: dense, N)."""
    H, inn, R, dx = (np.asarray(x, dtype=np.float64) for x in (H, inn, R, dx))
    M, N = H.shape
    w = N if w is None else w
    nzm = H != 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        Hl, dl = H.astype(LD), dx.astype(LD)
        hdx = np.array([np.sum(Hl[i, nzm[i]] * dl[nzm[i]], dtype=LD) for i in range(M)], dtype=LD)
        habs = np.array([np.sum(np.abs(Hl[i, nzm[i]] * dl[nzm[i]]), dtype=LD) for i in range(M)], dtype=LD)
        cnt = nzm.any(axis=1) | (inn != 0.0)
        il, Rl = inn.astype(LD)[cnt], R.astype(LD)[cnt]
        r = il - hdx[cnt]
        ha = habs[cnt]
        out = dict(nis=np.sum(il * r / Rl, dtype=LD), prefit=np.sum(il * il / Rl, dtype=LD), postfit=np.sum(r * r / Rl, dtype=LD))
        c = (w + chain(M) + 8) * U
        out["b_nis"] = float(c * np.sum(np.abs(il) * (np.abs(il) + ha) / Rl, dtype=LD))
        out["b_prefit"] = float(c * np.sum(il * il / Rl, dtype=LD))
        out["b_postfit"] = float(c * np.sum(np.abs(r) * (np.abs(r) + 2 * ha) / Rl, dtype=LD))
    a = np.abs(inn[cnt])
    out["inn_max"] = float("nan") if np.isnan(a).any() else float(a.max(initial=0.0))
    out["dx_max"] = float("nan") if np.isnan(dx).any() else float(np.abs(dx).max(initial=0.0))
    out["dof"], out["rows"] = int(cnt.sum()), M
    out["flags"] = (1 if status != 0 else 0) | (2 if ldlt else 0)
    if status != 0:
        out["nis"] = out["prefit"] = out["postfit"] = LD("nan")
    return out


def same_max(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def check(rec, ref, what=""):
    """assert one record (a numpy void of innov_rec_dtype, or a dict) against restate()'s; -> the worst error / bound ratio"""
    g = (lambda k: rec[k])
    for k in ("dof", "rows", "flags"):
        assert int(g(k)) == ref[k], (what, k, int(g(k)), ref[k])
    assert same_max(float(g("inn_max")), ref["inn_max"]), (what, "inn_max", float(g("inn_max")), ref["inn_max"])
    assert same_max(float(g("dx_max")), ref["dx_max"]), (what, "dx_max", float(g("dx_max")), ref["dx_max"])
    worst = 0.0
    for k in ("nis", "prefit", "postfit"):
        v, t = float(g(k)), ref[k]
        if np.isnan(t):
            assert np.isnan(v), (what, k, v)
            continue
        if not np.isfinite(float(t)):
            assert v == float(t), (what, k, v, t)
            continue
        err, b = abs(float(LD(v) - t)), ref["b_" + k]
        assert err <= b, (what, k, v, float(t), err, b)
        if b > 0:
            worst = max(worst, err / b)
    return worst


def ordering_slack(rec, ref, what=""):
    """prefit >= nis >= postfit >= 0 within the slack of the three bounds (records with flags = 0)"""
    n, p, q = float(rec["nis"]), float(rec["prefit"]), float(rec["postfit"])
    assert p >= n - (ref["b_nis"] + ref["b_prefit"]), (what, p, n)
    assert n >= q - (ref["b_nis"] + ref["b_postfit"]), (what, n, q)
    assert q >= 0.0, (what, q)


def truth(H, P, inn, R, dx, w=None):
    """inn^T S^-1 inn in longdouble from the prior P and the counted rows (precise_ref._chol), with the bound the device nis
    is held to against it: restate()'s b_nis + |D H^T R^-1 inn|_2 tol(ref) |D^-1 dx_ref|_2, D = diag(ref.d), tol(ref) =
    8 u (kappa_2(S) + N) - what the update routes' dx is held to (tests/test_update_accuracy_gpu.py). -> (nis, bound)"""
    import precise_ref as pr
    H, inn, R = np.asarray(H, dtype=np.float64), np.asarray(inn, dtype=np.float64), np.asarray(R, dtype=np.float64)
    cnt = (H != 0.0).any(axis=1) | (inn != 0.0)
    Hc, ic, Rc = H[cnt], inn[cnt], R[cnt]
    ref = pr.extended(Hc, P, ic, Rc)
    Hl, Pl, il = Hc.astype(LD), np.asarray(P).astype(LD), ic.astype(LD)
    S = Hl @ Pl @ Hl.T + np.diag(Rc.astype(LD))
    L = pr._chol(S)
    y = np.zeros(len(ic), dtype=LD)
    for i in range(len(ic)):
        y[i] = (il[i] - L[i, :i] @ y[:i]) / L[i, i]
    nis = y @ y
    d = ref.d.astype(LD)
    g = d * (Hl.T @ (il / Rc.astype(LD)))
    bound = restate(H, inn, R, dx, w=w)["b_nis"] + float(np.sqrt(g @ g)) * pr.tol(ref) * float(np.sqrt(np.sum((ref.dx / d) ** 2)))
    return nis, bound
