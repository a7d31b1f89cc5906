"""Inputs, an 80-bit restatement and derived bounds for the resident landmark map (xivo_hip_lcmap_*) at its limits.
tests/test_lcmap_edges_cpu.py checks on the host that every case sits where it claims and that the fp64 restatements
(tests/lcmap_restate.py, tests/lcmap_cov_restate.py - the oracle) stay inside the cap; tests/test_lcmap_edges_gpu.py runs the
cases on the device and holds it to bounds().

Shapes: the layout of tests/lcmap_cases.py (4 groups, 8 features, N = 71) in a Context(N, 128, B) with B <= 48, so that lc_max
may be 64. Stored points are loaded with lcmap_set or added from the eight in-state features under as many keys as needed.

The 80-bit side (np.longdouble: a 64-bit mantissa on x86-64) restates lc_row_pair, the 2 x 2 gate, R_e = Rlc I + H_T Sigma H_T^T
and the whitening from their formulas, the cameras through geometry_edge_cases.project(..., T=LD), Feature::Xs and Sigma of an
added point through tests/map_restate.py.

Families (family(name, cam): NB = 48 filters x NP = 6 pairs, pairs 0, 2, 4 observed by the body pose, 1, 3, 5 by a group slot)
  nominal     points at 2 - 8 m, pose sigma 1 - 10 cm and 1 - 3 degrees
  far         20 - 50 m
  edge        0.3 - 1 m, the pixel at 0.9 of the way from the principal point to the nearest image border
  certain     P about 1e-12: S_f is Rlc I to rounding
  illcond     P = s^2 v v^T + 1e-12 C, v over the translation blocks: S_f is rank one plus Rlc I, kappa_2(S_f) 1e5 .. KAPPA_S
  nominal_cov nominal with a point covariance of a few centimetres (both options' kernel)
  aniso       nominal with Sigma = s^2 n n^T + (1 mm)^2 I: kappa_2(R_e) 1e3 .. KAPPA_RE

Quantities and their units (errors()): "blocks" - an entry of one of the pair's four 2 x 3 blocks over the largest |entry| of
that block in the reference; "inn" - px over max(1, |xp|), xp the predicted pixel; "gamma" - relative; with a covariance the
staged rows and innovation are the whitened ones, in the same units, and gamma is that on R_e. "xs" (xs_case) - |dXs| / |Xs| of
an added record; "sigma" - the six entries of an added Sigma over sqrt(Sigma_ii Sigma_jj).

Bounds: bounds()[family][quantity] = 4 x the oracle's worst error against the 80-bit value over the family's inputs on all four
cameras, floored at 4 * 2^-53. Computed, never typed in. CAP = 1e-9 is a condition on the inputs: the CPU test asserts every
bound below it. illcond takes s^2 from the filter's pair with the largest |H v|, so that no pair passes KAPPA_S: drawn from the
median pair kappa_2(S_f) reached 1.2e7 and the oracle's own gamma left the cap (DESIGN.md section 5 has the figures)."""
import functools

import numpy as np

import geometry_edge_cases as G
import lcmap_cases as LC
import lcmap_cov_restate as CR
import lcmap_restate as R
import map_restate as mr
import xivo_oracle as orc
from gate_edge_cases import corr
from scene_util import spd
from xivo_amd import synth

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 4.0 * U
CAP = 1e-9
OFF = 1e-6                        # relative distance of a threshold from the value it straddles
NB, NP = 48, 6
NG, NF = LC.NG, LC.NF
RLC, CHI2 = LC.RLC, LC.CHI2
M_MAX = 128                       # the contexts' M_max: room for 2 x 64 rows
KAPPA_S, KAPPA_RE = 1e6, 1e6      # the ill-conditioned families' largest kappa_2
CAMS = LC.CAMS
FAMILIES = ("nominal", "far", "edge", "certain", "illcond", "nominal_cov", "aniso")
COV_FAMILIES = ("nominal_cov", "aniso")
QUANTITIES = ("blocks", "inn", "gamma")


def layout():
    return LC.layout()


def _rot(w):
    return orc.so3_exp(np.asarray(w, dtype=np.float64))


# ---------------------------------------------------------------- scenes
def base_scene(cam, nb, seed):
    """a synth.g_level scene whose group slots hold poses near the body's (5 cm, 3 degrees): a point in view of one is in view
    of all. The in-state features stay g_level's (they only fill the resident list)."""
    sc = synth.g_level(NG, NF, NF, nb, seed=seed, cam=cam)
    rng = np.random.default_rng(seed + 1000)
    for b in range(nb):
        for g in range(NG):
            sc["gR"][b, g] = sc["Rsb"][b] @ _rot(rng.uniform(-0.05, 0.05, 3))
            sc["gT"][b, g] = sc["Tsb"][b] + rng.uniform(-0.05, 0.05, 3)
    return sc


def observer(sc, b, g):
    """(Rsb, Tsb) of the pose that observes: group slot g, or the body for g = -1"""
    return (sc["Rsb"][b], sc["Tsb"][b]) if g < 0 else (sc["gR"][b, g], sc["gT"][b, g])


def edge_ray(cam, phi, frac=0.9):
    """the normalised ray whose pixel lies frac of the way from the principal point to the nearest border, at angle phi"""
    r = frac * min(cam["cx"], cam["cols"] - cam["cx"], cam["cy"], cam["rows"] - cam["cy"])
    xc, _ = G.unproject(cam, cam["cx"] + r * np.cos(phi), cam["cy"] + r * np.sin(phi))
    return float(xc[0]), float(xc[1])


def place(sc, cam, b, g, ray, Z, noise):
    """the world point on `ray` at depth Z in the camera of observer g, and its pixel there plus `noise`"""
    Ro, To = observer(sc, b, g)
    Xc = Z * np.array([ray[0], ray[1], 1.0])
    Xs = Ro @ (sc["Rbc"][b] @ Xc + sc["Tbc"][b]) + To
    return Xs, LC.pixel(cam, Xs, Ro, To, sc["Rbc"][b], sc["Tbc"][b]) + noise


def pose_prior(seed, sW, sT, rest=1e-3, scale=1.0):
    """D C D: standard deviations sW (rad) / sT (m) on the body's and every group's pose, `rest` elsewhere"""
    lay = layout()
    d = np.full(lay.N, rest)
    for o in [0] + [lay.group_begin + 6 * g for g in range(NG)]:
        d[o:o + 3] = sW; d[o + 3:o + 6] = sT
    return scale * corr(lay.N, seed) * np.outer(d, d)


def t_cols(g):
    o = 0 if g < 0 else layout().group_begin + 6 * g
    return o + 3


def _goff(g):
    return 0 if g < 0 else layout().group_begin + 6 * g


def pair_cols(g):
    """the 12 columns of a pair: the observing pose's six, then Wbc Tbc"""
    o = _goff(g)
    return list(range(o, o + 6)) + list(range(15, 21))


@functools.lru_cache(maxsize=None)
def family(name, camname, nb=NB, npairs=NP, seed=0):
    """-> dict(sc, cam, P [nb, N, N], Xs [nb, np, 3], g [nb, np] (-1: body), xp [nb, np, 2], Sigma [nb, np, 3, 3] or None,
    keys [nb, np])"""
    cam = CAMS[camname]
    sd = 7000 + 100 * FAMILIES.index(name) + 10 * list(CAMS).index(camname) + seed
    sc = base_scene(cam, nb, sd)
    rng = np.random.default_rng(sd + 1)
    lay = layout()
    Xs = np.zeros((nb, npairs, 3)); xp = np.zeros((nb, npairs, 2)); g = np.zeros((nb, npairs), dtype=np.int32)
    depth = dict(far=(20.0, 50.0), edge=(0.3, 1.0)).get(name, (2.0, 8.0))
    for b in range(nb):
        for m in range(npairs):
            g[b, m] = -1 if m % 2 == 0 else (m // 2 + b) % NG
            ray = edge_ray(cam, rng.uniform(0, 2 * np.pi)) if name == "edge" else tuple(rng.uniform(-0.45, 0.45, 2))
            Xs[b, m], xp[b, m] = place(sc, cam, b, int(g[b, m]), ray, rng.uniform(*depth), rng.normal(0, 1.5, 2))
    keys = 1000 * np.arange(nb)[:, None] + np.arange(npairs)[None, :]
    out = dict(name=name, camname=camname, sc=sc, cam=cam, Xs=Xs, g=g, xp=xp, keys=keys, Sigma=None)
    sW = np.deg2rad(rng.uniform(1.0, 3.0, nb)); sT = rng.uniform(0.01, 0.10, nb)
    if name == "certain":
        out["P"] = np.array([pose_prior(sd + b, 1e-6, 1e-6, 1e-6) for b in range(nb)])
    elif name == "illcond":
        H = oracle_rows(out, P=None)["H"]
        P = []
        for b in range(nb):
            v = np.zeros(lay.N); d = rng.normal(size=3); d /= np.linalg.norm(d)
            for gg in range(-1, NG):
                v[t_cols(gg):t_cols(gg) + 3] = d
            a2 = max(np.linalg.norm(H[b, 2 * m:2 * m + 2] @ v) ** 2 for m in range(npairs))   # the filter's largest kappa is kap
            kap = 10.0 ** rng.uniform(np.log10(2e5), np.log10(KAPPA_S))
            P.append(kap * RLC / a2 * np.outer(v, v) + 1e-12 * corr(lay.N, sd + b))
        out["P"] = np.array(P)
    else:
        out["P"] = np.array([pose_prior(sd + b, sW[b], sT[b]) for b in range(nb)])
    if name == "nominal_cov":
        out["Sigma"] = np.array([[sigma_blob(rng) for _ in range(npairs)] for _ in range(nb)])
    elif name == "aniso":
        H = oracle_rows(out, P=None)["H"]
        Sg = np.zeros((nb, npairs, 3, 3))
        for b in range(nb):
            for m in range(npairs):
                n = rng.normal(size=3); n /= np.linalg.norm(n)
                HT = H[b, 2 * m:2 * m + 2, t_cols(int(g[b, m])):t_cols(int(g[b, m])) + 3]
                kap = 10.0 ** rng.uniform(3.0, np.log10(KAPPA_RE))
                Sg[b, m] = kap * RLC / np.linalg.norm(HT @ n) ** 2 * np.outer(n, n) + 1e-6 * np.eye(3)
        out["Sigma"] = Sg
    return out


def sigma_blob(rng, s=0.05):
    A = rng.uniform(-1, 1, (3, 3))
    return s * s * (A @ A.T / 3 + 0.5 * np.eye(3))


def matches_of(fam, b, xp=None):
    """filter b's pairs as lcmap_restate.rows takes them"""
    sc = fam["sc"]
    xp = fam["xp"] if xp is None else xp
    out = []
    for m in range(fam["Xs"].shape[1]):
        Ro, To = observer(sc, b, int(fam["g"][b, m]))
        out.append(dict(Xs=fam["Xs"][b, m], Rsb=Ro, Tsb=To, g_sind=int(fam["g"][b, m]), xp=xp[b, m]))
    return out


# ---------------------------------------------------------------- the fp64 oracle on a family
def oracle_rows(fam, P="own"):
    """the oracle's side: H [nb, 2 np, N], inn [nb, 2 np] unwhitened; with P also gamma [nb, np] (NaN: no gamma), and with a
    covariance Hw, innw (whitened) and gamma on R_e"""
    sc, cam, lay = fam["sc"], fam["cam"], layout()
    nb, npairs = fam["Xs"].shape[:2]
    H = np.zeros((nb, 2 * npairs, lay.N)); inn = np.zeros((nb, 2 * npairs))
    for b in range(nb):
        H[b], inn[b], _ = R.rows(matches_of(fam, b), sc["Rbc"][b], sc["Tbc"][b], cam, lay, npairs, RLC)
    out = dict(H=H, inn=inn)
    if P is None:
        return out
    P = fam["P"]
    gam = np.full((nb, npairs), np.nan)
    Hw, iw = H.copy(), inn.copy()
    for b in range(nb):
        for m in range(npairs):
            s = slice(2 * m, 2 * m + 2)
            if fam["Sigma"] is None:
                v = R.gamma(H[b, s], P[b], inn[b, s], RLC)
            else:
                Re = CR.r_eff(H[b, s], fam["Sigma"][b, m], RLC, _goff(int(fam["g"][b, m])))
                v = CR.gamma(H[b, s], P[b], inn[b, s], Re)
                L = np.linalg.cholesky(Re)
                Hw[b, s] = np.linalg.solve(L, H[b, s]); iw[b, s] = np.linalg.solve(L, inn[b, s])
            gam[b, m] = np.nan if v is None else v
    out.update(gamma=gam, Hs=Hw, inns=iw)      # Hs / inns: as staged
    return out


# ---------------------------------------------------------------- the 80-bit restatement
def _ld(a):
    return np.asarray(a, dtype=LD)


def row_pair_ld(cam, Xs, Ro, To, Rbc, Tbc, xp_obs):
    """lc_row_pair in 80-bit: -> (blocks [4, 2, 3]: d xp / d (W, T, Wbc, Tbc), inn [2], xp [2] the predicted pixel)"""
    Xs, Ro, To, Rbc, Tbc = _ld(Xs), _ld(Ro), _ld(To), _ld(Rbc), _ld(Tbc)
    Xb = Ro.T @ (Xs - To)
    Xcn = Rbc.T @ (Xb - Tbc)
    X, Y, Z = Xcn
    xp, J, _, _, _ = G.project(cam, X / Z, Y / Z, LD)
    dn = np.array([[1 / Z, 0, -X / (Z * Z)], [0, 1 / Z, -Y / (Z * Z)]], dtype=LD)
    D = J @ dn
    blocks = np.array([D @ (Rbc.T @ G.hat(Xb)), D @ (-(Rbc.T @ Ro.T)), D @ G.hat(Xcn), D @ (-Rbc.T)], dtype=LD)
    return blocks, _ld(xp_obs) - xp, xp


def chol2_ld(s00, s10, s11):
    """the 2 x 2 Cholesky's pivots and factors: (ok, l00, l10, l11)"""
    if not s00 > 0:
        return False, None, None, None
    l00 = np.sqrt(s00); l10 = s10 / l00
    d = s11 - l10 * l10
    if not d > 0:
        return False, l00, l10, None
    return True, l00, l10, np.sqrt(d)


def gamma_ld(S, r):
    """r^T S^-1 r through mh_dist_2x2's substitutions; None where a pivot is not positive or the value is not finite"""
    ok, l00, l10, l11 = chol2_ld(S[0, 0], S[1, 0], S[1, 1])
    if not ok:
        return None
    y0 = r[0] / l00; y1 = (r[1] - l10 * y0) / l11
    x1 = y1 / l11; x0 = (y0 - l10 * x1) / l00
    g = r[0] * x0 + r[1] * x1
    return g if np.isfinite(g) else None


def S_ld(h, P12, Re):
    """h [2, 12] P12 h^T + R_e in 80-bit"""
    return _ld(h) @ _ld(P12) @ _ld(h).T + _ld(Re)


@functools.lru_cache(maxsize=None)
def reference(name, camname):
    """the 80-bit side of a family: H, inn (unwhitened), xp (predicted), gamma, Hs / inns (as staged: whitened under a
    covariance), kappa_S, kappa_Re - arrays shaped as oracle_rows'"""
    fam = family(name, camname)
    sc, cam, lay = fam["sc"], fam["cam"], layout()
    nb, npairs = fam["Xs"].shape[:2]
    H = np.zeros((nb, 2 * npairs, lay.N), dtype=LD); inn = np.zeros((nb, 2 * npairs), dtype=LD)
    xpp = np.zeros((nb, npairs, 2)); gam = np.zeros((nb, npairs), dtype=LD)
    kS = np.zeros((nb, npairs)); kR = np.ones((nb, npairs))
    for b in range(nb):
        for m in range(npairs):
            g = int(fam["g"][b, m])
            Ro, To = observer(sc, b, g)
            blocks, r, xp = row_pair_ld(cam, fam["Xs"][b, m], Ro, To, sc["Rbc"][b], sc["Tbc"][b], fam["xp"][b, m])
            cols = pair_cols(g)
            s = slice(2 * m, 2 * m + 2)
            h = np.hstack(list(blocks))                                    # [2, 12] in the order of pair_cols
            for k, c in enumerate(cols):
                H[b, s, c] = h[:, k]
            inn[b, s] = r; xpp[b, m] = xp.astype(np.float64)
    Hs, inns = H.copy(), inn.copy()
    for b in range(nb):
        for m in range(npairs):
            g = int(fam["g"][b, m]); cols = pair_cols(g); s = slice(2 * m, 2 * m + 2)
            h = H[b, s][:, cols]
            Re = LD(RLC) * np.eye(2, dtype=LD)
            if fam["Sigma"] is not None:
                HT = h[:, 3:6]
                Re = Re + HT @ _ld(fam["Sigma"][b, m]) @ HT.T
                ok, w00, w10, w11 = chol2_ld(Re[0, 0], Re[1, 0], Re[1, 1])
                assert ok
                Hs[b, 2 * m] = H[b, 2 * m] / w00; Hs[b, 2 * m + 1] = (H[b, 2 * m + 1] - w10 * Hs[b, 2 * m]) / w11
                inns[b, 2 * m] = inn[b, 2 * m] / w00; inns[b, 2 * m + 1] = (inn[b, 2 * m + 1] - w10 * inns[b, 2 * m]) / w11
                kR[b, m] = np.linalg.cond(Re.astype(np.float64))
            S = S_ld(h, fam["P"][b][np.ix_(cols, cols)], Re)
            v = gamma_ld(S, inn[b, s])
            assert v is not None
            gam[b, m] = v; kS[b, m] = np.linalg.cond(S.astype(np.float64))
    return dict(H=H, inn=inn, xp=xpp, gamma=gam, Hs=Hs, inns=inns, kappa_S=kS, kappa_Re=kR)


def errors(fam, ref, H, inn, gamma):
    """the worst error of staged rows H [nb, 2 np, N], inn and gamma against the 80-bit reference, in the units above
    -> dict(blocks, inn, gamma); everything outside a pair's 12 columns must be zero"""
    nb, npairs = fam["Xs"].shape[:2]
    w = dict(blocks=0.0, inn=0.0, gamma=0.0)
    Hr, ir = ref["Hs"], ref["inns"]
    for b in range(nb):
        for m in range(npairs):
            cols = pair_cols(int(fam["g"][b, m])); s = slice(2 * m, 2 * m + 2)
            rest = np.ones(H.shape[-1], dtype=bool); rest[cols] = False
            assert not np.asarray(H[b, s])[:, rest].any(), (b, m)
            for k in range(4):
                c = cols[3 * k:3 * k + 3]
                e = np.abs(_ld(H[b, s][:, c]) - Hr[b, s][:, c]).max() / np.abs(Hr[b, s][:, c]).max()
                w["blocks"] = max(w["blocks"], float(e))
            e = np.abs(_ld(inn[b, s]) - ir[b, s]).max() / max(1.0, float(np.linalg.norm(ref["xp"][b, m])))
            w["inn"] = max(w["inn"], float(e))
            w["gamma"] = max(w["gamma"], float(abs(LD(gamma[b, m]) - ref["gamma"][b, m]) / ref["gamma"][b, m]))
    return w


@functools.lru_cache(maxsize=None)
def oracle_worst(name):
    """{quantity: the oracle's worst error over the family's inputs on all four cameras}"""
    w = dict.fromkeys(QUANTITIES, 0.0)
    for camname in CAMS:
        fam = family(name, camname)
        o = oracle_rows(fam)
        e = errors(fam, reference(name, camname), o["Hs"], o["inns"], o["gamma"])
        w = {k: max(w[k], e[k]) for k in w}
    return w


# ---------------------------------------------------------------- added records: Xs and Sigma
@functools.lru_cache(maxsize=None)
def xs_case(inv):
    """the in-state features of NB filters in the build's parametrisation and their world points: fp64 (the oracle) and 80-bit"""
    sc = synth.g_level(NG, NF, NF, NB, seed=23, cam=synth.PINHOLE)
    x = LC.to_invdepth(sc["x"]) if inv else sc["x"].copy()
    X64 = np.zeros((NB, NF, 3)); X80 = np.zeros((NB, NF, 3), dtype=LD)
    for b in range(NB):
        for j in range(NF):
            r = int(sc["ref"][b, j])
            X64[b, j] = orc.feature_xs(x[b, j], sc["gR"][b, r], sc["gT"][b, r], sc["Rbc"][b], sc["Tbc"][b], inv)
            X80[b, j] = mr.world_point(sc["Rbc"][b], sc["Tbc"][b], sc["gR"][b, r], sc["gT"][b, r], x[b, j], inv)
    P = np.array([spd(layout().N, 500 + b) * 1e-4 for b in range(NB)])
    return dict(sc=sc, x=x, Xs64=X64, Xs80=X80, P=P)


def xs_error(got, X80):
    """|dXs| / |Xs| per point, the worst"""
    d = (_ld(got) - X80).astype(np.float64)
    return float((np.linalg.norm(d, axis=-1) / np.linalg.norm(X80.astype(np.float64), axis=-1)).max())


def _jacobian64(Rbc, Tbc, Rg, x, inv):
    """map_restate.jacobian in fp64 (the oracle of an added Sigma)"""
    Xc, D = orc.feature_xc(x, inv)
    Xb = Rbc @ Xc + Tbc
    return np.hstack([-(Rg @ Rbc) @ orc.hat(Xc), Rg, -Rg @ orc.hat(Xb), np.eye(3), (Rg @ Rbc) @ D])


@functools.lru_cache(maxsize=None)
def sigma_case(inv):
    """Sigma = J Pcc J^T of xs_case's points: fp64 and 80-bit, packed six"""
    c = xs_case(inv)
    sc, lay = c["sc"], layout()
    ml = dict(group_begin=lay.group_begin, n_groups=NG, feature_begin=lay.feature_begin, n_features=NF)
    S64 = np.zeros((NB, NF, 6)); S80 = np.zeros((NB, NF, 6), dtype=LD)
    for b in range(NB):
        for j in range(NF):
            r = int(sc["ref"][b, j])
            cols = mr.columns(ml, r, int(sc["sind"][b, j]))
            J64 = _jacobian64(sc["Rbc"][b], sc["Tbc"][b], sc["gR"][b, r], c["x"][b, j], inv)
            S64[b, j] = CR.pack6(J64 @ mr.gather(c["P"][b], cols).astype(np.float64) @ J64.T)
            J80 = mr.jacobian(sc["Rbc"][b], sc["Tbc"][b], sc["gR"][b, r], sc["gT"][b, r], c["x"][b, j], inv)
            S80[b, j] = mr.pack6(J80 @ mr.gather(c["P"][b], cols) @ J80.T)
    return dict(S64=S64, S80=S80)


def sigma_error(got, S80):
    """the six entries over sqrt(Sigma_ii Sigma_jj), the worst"""
    d = np.sqrt(S80[..., [0, 3, 5]].astype(np.float64))
    den = np.stack([d[..., i] * d[..., j] for i, j in CR.SYM6], axis=-1)
    return float((np.abs((_ld(got) - S80).astype(np.float64)) / den).max())


# ---------------------------------------------------------------- bounds
@functools.lru_cache(maxsize=None)
def bounds():
    """{family: {quantity: 4 x the oracle's worst, floored}} and {"added": {"xs", "sigma"}}"""
    out = {name: {k: max(4.0 * v, FLOOR) for k, v in oracle_worst(name).items()} for name in FAMILIES}
    out["added"] = dict(xs=max(4.0 * max(xs_error(xs_case(i)["Xs64"], xs_case(i)["Xs80"]) for i in (False, True)), FLOOR),
                        sigma=max(4.0 * max(sigma_error(sigma_case(i)["S64"], sigma_case(i)["S80"]) for i in (False, True)), FLOOR))
    return out


def table_lines():
    """family, quantity, the oracle's worst, the bound, the cap - one line each"""
    b = bounds()
    rows = []
    for name in FAMILIES:
        for q in QUANTITIES:
            rows.append("%-12s %-7s %-9.2g %-9.2g %-6.0e" % (name, q, oracle_worst(name)[q], b[name][q], CAP))
    return rows


# ---------------------------------------------------------------- A: capacity and launch shapes
ADD_MAP_MAX = (63, 64, 65, 130)


def add_script(map_max, b):
    """filter b's two add calls as (feature, key) lists: call 1 - map_max + 2 distinct keys (on the 130-entry map the keys
    accepted at positions 65 and 127 are each followed at once by themselves); call 2 - the keys stored at positions 0, 63, 64 and
    map_max - 1 (those there are) and a new one"""
    keys = [50000 * (b + 1) + 7 * i for i in range(map_max + 2)]
    c1 = []
    for i, k in enumerate(keys):
        c1.append((i % NF, k))
        if map_max == 130 and i in (65, 127):
            c1.append(((i + 3) % NF, k))
    pos = sorted({p for p in (0, 63, 64, map_max - 1) if p < map_max})
    c2 = [((p + 1) % NF, keys[p]) for p in pos] + [(2, 999999)]
    return c1, c2


MATCH_LC_MAX = (1, 6, 63, 64)
MATCH_COUNTS = (200, 0, 200, 1, 63, 64, 65, 128, 130, 200)   # queries per filter: none between two filters with many
MATCH_FILL_AT = (63, None, 130, None, None, 63, 64, 64, 128, 64)   # the query that fills the list (where the shape allows)
MATCH_ENTRIES = 130


def match_map_keys(b):
    return [3000 * (b + 1) + 11 * e for e in range(MATCH_ENTRIES)]


def match_queries(lc_max, b):
    """filter b's query keys: absent and negative keys, and matches placed so that the lc_max-th one is query MATCH_FILL_AT[b]
    (where that many queries come before it), followed by surplus; a key asked twice among the matches"""
    n, t = MATCH_COUNTS[b], MATCH_FILL_AT[b]
    rng = np.random.default_rng(100 * lc_max + b)
    mk = match_map_keys(b)
    special = [mk[0], mk[63], mk[64], mk[129]]
    q = [(-5 if i % 7 == 3 else 77 + i) for i in range(n)]              # 77 + i < 3000: in no map
    if t is not None and t < n and t >= lc_max - 1:
        idx = sorted(rng.choice(t, lc_max - 1, replace=False).tolist()) + [t] + [i for i in (t + 1, n - 1) if t < i < n]
    else:
        idx = sorted(rng.choice(n, n // 3, replace=False).tolist()) if n else []
    idx = sorted(set(idx))
    for k, i in enumerate(idx):
        q[i] = special[k] if k < 4 else mk[int(rng.integers(0, MATCH_ENTRIES))]
    if len(idx) >= 2:
        q[idx[1]] = q[idx[0]]                                           # the same key at two places, both inside the list
    return q


# ---------------------------------------------------------------- C: pivots of the plain kernel
PIVOT_RAYS = ((0.3, 0.0), (0.0, 0.3))      # filter 0: |h0| > |h1| (s00 changes sign first); filter 1: |h1| > |h0| (the Schur pivot)


@functools.lru_cache(maxsize=None)
def pivot_case():
    """two filters, one body-observed pinhole pair each, on PIVOT_RAYS at 3 m"""
    cam = synth.PINHOLE
    sc = base_scene(cam, 2, 77)
    Xs = np.zeros((2, 1, 3)); xp = np.zeros((2, 1, 2))
    for b in range(2):
        Xs[b, 0], xp[b, 0] = place(sc, cam, b, -1, PIVOT_RAYS[b], 3.0, np.array([0.7, -0.4]))
    return dict(name="pivot", sc=sc, cam=cam, Xs=Xs, xp=xp, g=np.full((2, 1), -1, dtype=np.int32), keys=np.array([[5], [6]]), Sigma=None)


def pivot_cs(h):
    """h [2, 12] of a pair -> the c of P = -c I: (s00 just positive, s00 just negative, between the two pivots or None)"""
    n0, n1 = float(h[0] @ h[0]), float(h[1] @ h[1])
    mid = 0.5 * (RLC / n1 + RLC / n0) if n1 > n0 else None
    return RLC * (1 - 1e-3) / n0, RLC * (1 + 1e-3) / n0, mid


def pivots_ld(h, c):
    """(s00 > 0, Schur pivot > 0, gamma or None) of S = Rlc I - c h h^T in 80-bit; gamma for the innovation r"""
    S = LD(RLC) * np.eye(2, dtype=LD) - LD(c) * (_ld(h) @ _ld(h).T)
    ok, l00, l10, l11 = chol2_ld(S[0, 0], S[1, 0], S[1, 1])
    return bool(S[0, 0] > 0), ok, S
