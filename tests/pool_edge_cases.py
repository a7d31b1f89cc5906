"""The cases of tests/test_pool_edges_gpu.py - the feature pool's kernels (subfilter_step, the candidate order of pool_step_kernel,
adapt_depth_kernel; xivo_amd/csrc/pool_kernels.hip) at their thresholds and ties - with the references both the GPU test and its
CPU check (tests/test_pool_edges_cpu.py) use. Nothing here needs a GPU.

A. draw(): families of sub-filter inputs; reference(): tests/subfilter_restate.py in np.longdouble and the fp64 oracle on them;
   family_bounds(): four times the oracle's worst error against the restatement, floored at 4 * 2^-53, below CAP - no typed-in
   tolerance. Errors are in units of the prior standard deviations d = sqrt(diag P_prior).
B. exact_cases(): inputs whose every intermediate is a dyadic rational, so that a comparison can sit ON its threshold;
   straddle thresholds sit at value * (1 -+ OFF).
C. order_scene(): pools full of ties (twin tracks, P = 0 entries) for the candidate order; python_order(): the sort on
   (-rank, P(2,2), entry).
D. adapt_scene(): depth sets for AdaptInitialDepth; adapt_expected(): (1 - beta) z + beta np.sort(d)[n // 2]."""
import functools
import math

import numpy as np

import geometry_edge_cases as gc
import subfilter_restate as sr
import xivo_oracle as orc
from xivo_amd import lib as L
from xivo_amd import synth

LD = np.longdouble
U = 2.0 ** -53
OFF = 1e-6                       # relative distance of a straddling threshold from the value it straddles
CAP = 1e-9                       # every bound of A must come out below this: a factor 60 under a float's rounding
EXCLUDE = 1e-6                   # cases of A whose 80-bit ratio is this close to 1 belong to B
CAMS = gc.CAMS
RBC = orc.so3_exp(np.array([-1.57079633, 0.0, 0.0]))
TBC = np.array([0.02, -0.01, 0.03])
NG, NF = 8, 4
N = 23 + 6 * NG + 3 * NF
READY = sr.FEAT_READY


def cm(R):
    """3x3 -> column-major 9 (the C ABI's layout)"""
    return np.asarray(R).T.reshape(-1)


# ---------------------------------------------------------------- A: families of sub-filter inputs
# Rtri, prior depth std (log depth; relative in inverse depth), baseline per step [m], depth range [m], pixel noise [px], the
# range of the prior's x / y std [px, log-uniform], the candidate window (so that both sides of every candidate test occur),
# steps. sxy is what puts about half of "outliers" on either side of ratio = 1 at 25 px of noise. "small_R": cond_2(S) reaches
# 2e6; the oracle's own error grows with it (adjugate inverse of S), and at 1e7 four times that error crosses CAP - the
# family is drawn below it, as the cap demands.
FAMILIES = {
    "nominal": dict(Rtri=3.5 ** 2, std=0.5, baseline=0.1, z=(0.5, 8.0), noise=3.5, sxy=(3.0, 50.0), window=(0.8, 6.0), steps=1),
    "outliers": dict(Rtri=3.5 ** 2, std=0.5, baseline=0.1, z=(0.5, 8.0), noise=25.0, sxy=(3.0, 50.0), window=(0.8, 6.0), steps=1),
    "small_R": dict(Rtri=0.04, std=0.5, baseline=1.0, z=(0.5, 3.0), noise=0.2, sxy=(0.05, 0.2), window=(0.8, 2.5), steps=1),
    "far": dict(Rtri=3.5 ** 2, std=0.5, baseline=0.01, z=(20.0, 50.0), noise=3.5, sxy=(0.5, 20.0), window=(0.05, 35.0), steps=1),
    "carried": dict(Rtri=3.5 ** 2, std=0.5, baseline=0.1, z=(0.5, 8.0), noise=3.5, sxy=(0.5, 20.0), window=(0.8, 6.0), steps=3),
}
MH_THRESH, READY_STEPS, MAX_SUB_OUTLIER = 5.991, 2, 2.0
PER_CAMERA = 128                 # cases per camera: 512 per family and depth mode
MAX_RADIUS = 0.9                 # normalised radius the drawn points stay within (every model is monotonic there)


def opts_of(family):
    f = FAMILIES[family]
    return dict(Rtri=f["Rtri"], MH_thresh=MH_THRESH, ready_steps=READY_STEPS, min_depth=f["window"][0], max_depth=f["window"][1],
                max_subfilter_outlier=MAX_SUB_OUTLIER)


def _correlation(rng):
    Lm = np.eye(3) + np.tril(rng.uniform(-0.3, 0.3, (3, 3)), -1)
    C = Lm @ Lm.T
    s = np.sqrt(np.diag(C))
    return C / np.outer(s, s)


@functools.lru_cache(maxsize=None)
def draw(family, cam_name, invdepth, n=PER_CAMERA, seed=0):
    """n cases of a family on one camera -> dict of arrays: the prior x [n, 3], P [n, 3, 3] (non-diagonal), ic / oc [n], the
    anchor pose Rsbr / Tsbr and, per step s, the sensor pose Rsb / Tsb [steps, n, ...] and the measured pixel xp [steps, n, 2]:
    the projection of the true point (the prior's depth is perturbed by the family's std) plus pixel noise. A draw whose point
    leaves MAX_RADIUS or comes closer than 0.1 m to a camera is drawn again. The result is shared: leave it unchanged."""
    f, cam = FAMILIES[family], CAMS[cam_name]
    rng = np.random.default_rng([seed, list(FAMILIES).index(family), list(CAMS).index(cam_name), int(invdepth)])
    steps = f["steps"]
    c = dict(x=np.zeros((n, 3)), P=np.zeros((n, 3, 3)), ic=np.zeros(n, dtype=np.int32), oc=np.zeros(n),
             Rsbr=np.zeros((n, 3, 3)), Tsbr=np.zeros((n, 3)), Rsb=np.zeros((steps, n, 3, 3)), Tsb=np.zeros((steps, n, 3)),
             xp=np.zeros((steps, n, 2)), z_true=np.zeros(n))
    i = 0
    while i < n:
        Rsbr, Tsbr = orc.so3_exp(rng.normal(size=3) * 0.2), rng.normal(size=3) * 0.3
        ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 0.8) * 0.5 * min(cam["rows"], cam["cols"])
        xc = gc.unproject(cam, cam["cx"] + rad * np.cos(ang), cam["cy"] + rad * np.sin(ang))[0]
        z = rng.uniform(*f["z"])
        zp = z * math.exp(float(np.clip(rng.normal() * f["std"], -2 * f["std"], 2 * f["std"])))
        Rrc, Trc = Rsbr @ RBC, Rsbr @ TBC + Tsbr
        ok = bool(np.hypot(*xc) < MAX_RADIUS)
        Rs, Ts, xps = [], [], []
        for s in range(steps):
            a = rng.uniform(0, 2 * np.pi)
            t = f["baseline"] * (s + 1) * np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2)])
            Rsc, Tsc = Rrc @ orc.so3_exp(rng.normal(size=3) * 0.02), Trc + Rrc @ t
            Rsb = Rsc @ RBC.T
            Tsb = Tsc - Rsb @ TBC
            noise = f["noise"] * (7.0 if family == "carried" and rng.random() < 0.2 else 1.0)
            for depth in (z, zp):
                Xcn = Rsc.T @ (Rrc @ (depth * np.array([xc[0], xc[1], 1.0])) + Trc - Tsc)
                ok = ok and Xcn[2] > 0.1 and np.hypot(Xcn[0], Xcn[1]) / Xcn[2] < MAX_RADIUS
                if depth == z and ok:
                    xps.append(orc.camera_project(cam, Xcn[:2] / Xcn[2])[0] + rng.normal(size=2) * noise)
            Rs.append(Rsb); Ts.append(Tsb)
        if not ok:
            continue
        sx = np.exp(rng.uniform(*np.log(f["sxy"]), 2)) / cam["fx"]
        d = np.array([sx[0], sx[1], f["std"] / zp if invdepth else f["std"]])
        c["P"][i] = _correlation(rng) * np.outer(d, d)
        c["x"][i] = [xc[0] + rng.normal() * sx[0], xc[1] + rng.normal() * sx[1], 1.0 / zp if invdepth else math.log(zp)]
        carried = family == "carried"
        c["ic"][i] = rng.integers(1, 4) if carried else rng.integers(0, 4)
        c["oc"][i] = rng.uniform(0.1, 1.5) if carried or rng.random() < 0.5 else 0.0
        c["Rsbr"][i], c["Tsbr"][i], c["z_true"][i] = Rsbr, Tsbr, z
        for s in range(steps):
            c["Rsb"][s, i], c["Tsb"][s, i], c["xp"][s, i] = Rs[s], Ts[s], xps[s]
        i += 1
    for v in c.values():
        v.setflags(write=False)
    return c


def prior_of(c):
    """the prior of step 0 -> dict(x, P, ic, oc)"""
    return dict(x=c["x"], P=c["P"], ic=c["ic"], oc=c["oc"])


def reference(c, s, prior, family, cam_name, invdepth, T=LD):
    """step s of every case from `prior` (dict(x [n, 3], P [n, 3, 3], ic [n], oc [n])): T = LD the 80-bit restatement, T =
    np.float64 the fp64 oracle (xivo_oracle.subfilter_update / candidate_flags) -> dict of arrays x, P, oc, ic, status, cand
    and, from the restatement only, q, ratio, outlier, z, kappa"""
    o, cam = opts_of(family), CAMS[cam_name]
    n = len(prior["x"])
    out = dict(x=np.zeros((n, 3), dtype=T), P=np.zeros((n, 3, 3), dtype=T), oc=np.zeros(n, dtype=T), ic=np.zeros(n, dtype=np.int32),
               status=np.zeros(n, dtype=np.int32), cand=np.zeros(n, dtype=np.int32))
    if T is LD:
        out.update(q=np.zeros(n, dtype=LD), ratio=np.zeros(n, dtype=LD), outlier=np.zeros(n, dtype=bool), z=np.zeros(n, dtype=LD),
                   kappa=np.zeros(n))
    for i in range(n):
        args = (prior["x"][i], prior["P"][i], c["xp"][s, i], c["Rsb"][s, i], c["Tsb"][s, i], RBC, TBC, c["Rsbr"][i], c["Tsbr"][i], cam,
                o["Rtri"], o["MH_thresh"], o["ready_steps"], int(prior["ic"][i]), float(prior["oc"][i]), invdepth)
        if T is LD:
            r = sr.subfilter_update(*args, T=LD)
            for k in ("x", "P", "status", "q", "ratio", "outlier", "z", "kappa"):
                out[k][i] = r[k]
            out["oc"][i], out["ic"][i] = r["outlier_counter"], r["init_counter"]
            out["cand"][i] = sr.candidate_bits(r["outlier_counter"], r["z"], r["status"], o["min_depth"], o["max_depth"],
                                               o["max_subfilter_outlier"])
        else:
            x, P, st, ic, oc = orc.subfilter_update(*args)
            out["x"][i], out["P"][i], out["status"][i], out["ic"][i], out["oc"][i] = x, P, st, ic, oc
            c1, c2 = orc.candidate_flags(x, st, oc, o["min_depth"], o["max_depth"], o["max_subfilter_outlier"], invdepth)
            out["cand"][i] = (1 if c1 else 0) | (2 if c2 else 0)
    return out


def excluded(ref):
    """cases of A that B covers: the 80-bit ratio within EXCLUDE of 1"""
    return np.abs(ref["ratio"].astype(np.float64) - 1.0) < EXCLUDE


def errors(got, ref, prior):
    """the three metrics of A over the cases kept -> dict(x, P, oc): max |x - x_ref| / d, max |P - P_ref|_ij / (d_i d_j),
    max |oc - oc_ref| / max(1, sqrt(ratio)), d = sqrt(diag P_prior); got: dict(x [n, 3], P [n, 3, 3] row-major, oc [n])"""
    keep = ~excluded(ref)
    d = np.sqrt(np.einsum("nii->ni", np.asarray(prior["P"], dtype=np.float64)))
    ex = np.abs(np.asarray(got["x"]).astype(LD) - ref["x"]) / d
    eP = np.abs(np.asarray(got["P"]).astype(LD) - ref["P"]) / (d[:, :, None] * d[:, None, :])
    eo = np.abs(np.asarray(got["oc"]).astype(LD) - ref["oc"]) / np.maximum(1.0, np.sqrt(np.maximum(ref["ratio"], 0)))
    return dict(x=float(ex[keep].max()), P=float(eP[keep].max()), oc=float(eo[keep].max()))


def bound(worst):
    """four times the oracle's own worst error, floored at 4 * 2^-53; the cap is a condition on the inputs"""
    b = max(4.0 * float(worst), 4.0 * U)
    assert b < CAP, "the oracle itself is too close to the cap: worst %.3e bound %.3e cap %.1e" % (worst, b, CAP)
    return b


def merge(a, b):
    return {k: max(a[k], b[k]) for k in a} if a else dict(b)


@functools.lru_cache(maxsize=None)
def step_reference(family, cam_name, invdepth):
    """step 0 of a family on one camera -> (80-bit reference, the oracle's errors against it)"""
    c = draw(family, cam_name, invdepth)
    ref = reference(c, 0, prior_of(c), family, cam_name, invdepth, LD)
    f64 = reference(c, 0, prior_of(c), family, cam_name, invdepth, np.float64)
    return ref, f64, errors(f64, ref, prior_of(c))


@functools.lru_cache(maxsize=None)
def family_bounds(family, invdepth):
    """-> (worst {metric: value}, bound {metric: value}) of the fp64 oracle over the family's step-0 inputs, every camera. The
    carried family's later steps are fed by the device: their inputs exist only there, and tests/test_pool_edges_gpu.py merges
    the oracle's errors on them into the worst before it takes the bound (carried_oracle_chain here does the same on the
    oracle's own outputs)."""
    worst = {}
    for cam_name in CAMS:
        worst = merge(worst, step_reference(family, cam_name, invdepth)[2])
    return worst, {k: bound(v) for k, v in worst.items()}


def carried_oracle_chain(cam_name, invdepth):
    """the carried family with the oracle feeding itself -> list per step of (prior, 80-bit ref, oracle's errors)"""
    c = draw("carried", cam_name, invdepth)
    prior = prior_of(c)
    out = []
    for s in range(FAMILIES["carried"]["steps"]):
        ref = reference(c, s, prior, "carried", cam_name, invdepth, LD)
        f64 = reference(c, s, prior, "carried", cam_name, invdepth, np.float64)
        out.append((prior, ref, errors(f64, ref, prior)))
        prior = dict(x=f64["x"], P=f64["P"], ic=f64["ic"], oc=f64["oc"])
    return out


def host_arrays(c, s, prior):
    """the host-array problem of step s, one filter per case -> (poses [n], groups [n, NG], feats [n, 1] subfilter_dtype)"""
    n = len(prior["x"])
    poses = np.zeros(n, dtype=L.pose_dtype); groups = np.zeros((n, NG), dtype=L.group_dtype)
    feats = np.zeros((n, 1), dtype=L.subfilter_dtype)
    groups["Rsb"] = cm(np.eye(3))
    for i in range(n):
        poses[i]["Rsb"], poses[i]["Tsb"] = cm(c["Rsb"][s, i]), c["Tsb"][s, i]
        poses[i]["Rbc"], poses[i]["Tbc"], poses[i]["Rsg"] = cm(RBC), TBC, cm(np.eye(3))
        groups[i, 0]["Rsb"], groups[i, 0]["Tsb"] = cm(c["Rsbr"][i]), c["Tsbr"][i]
        feats[i, 0]["x"], feats[i, 0]["P"] = prior["x"][i], cm(prior["P"][i])
    feats["xp"][:, 0] = c["xp"][s]
    feats["init_counter"][:, 0], feats["outlier_counter"][:, 0] = prior["ic"], prior["oc"]
    return poses, groups, feats


def from_feats(feats):
    """device output [n, 1] -> dict(x, P row-major, oc, ic) as reference() returns and takes"""
    f = feats[:, 0]
    return dict(x=f["x"].copy(), P=np.transpose(f["P"].reshape(-1, 3, 3), (0, 2, 1)).copy(), oc=f["outlier_counter"].copy(),
                ic=f["init_counter"].copy())


# ---------------------------------------------------------------- B: exact cases
EXACT_CAM = dict(model=0, rows=512, cols=512, fx=256.0, fy=256.0, cx=256.0, cy=256.0, d=[])
EXACT_RTRI, EXACT_MH = 4.0, 8.0
EXACT_PRED = (320.0, 128.0)              # the predicted pixel of x = (0.25, -0.5, .) at the identity
EXACT_ON = (324.0, 132.0)                # inn = (4, 4): q = 32 / 4 = 8, ratio = 1 exactly
EXACT_OVER = (324.0, 132.0 + 2.0 ** -40)  # ratio = 1 + 2^-42 exactly (the products round the same way contracted or not)
EXACT_RATIO_OVER = 1.0 + 2.0 ** -42


def exact_x(invdepth):
    """x = (0.25, -0.5, x2): z = 2 under inverse depth (x2 = 0.5), z = 1 under log depth (x2 = 0)"""
    return np.array([0.25, -0.5, 0.5 if invdepth else 0.0])


def exact_z(invdepth):
    return 2.0 if invdepth else 1.0


def identity_pose(n):
    poses = np.zeros(n, dtype=L.pose_dtype)
    for k in ("Rsb", "Rbc", "Rsg"):
        poses[k] = cm(np.eye(3))
    groups = np.zeros((n, NG), dtype=L.group_dtype)
    groups["Rsb"] = cm(np.eye(3))
    return poses, groups


def exact_feat(invdepth, pixel, init_counter=0, outlier_counter=0.0):
    f = np.zeros((1, 1), dtype=L.subfilter_dtype)
    f["x"][0, 0] = exact_x(invdepth); f["xp"][0, 0] = pixel
    f["init_counter"], f["outlier_counter"] = init_counter, outlier_counter
    return f


def exact_oracle(invdepth, pixel, ready_steps, init_counter, outlier_counter):
    """the exact case in the fp64 oracle -> (x, P, status, init_counter, outlier_counter)"""
    I3, z3 = np.eye(3), np.zeros(3)
    return orc.subfilter_update(exact_x(invdepth), np.zeros((3, 3)), pixel, I3, z3, I3, z3, I3, z3, EXACT_CAM, EXACT_RTRI, EXACT_MH,
                                ready_steps, init_counter, outlier_counter, invdepth)


# name, pixel, opts that differ from the permissive ones, prior (init_counter, outlier_counter), expected (outlier_counter as a
# function of the prior counter, status, candidate bits). z: exact_z(invdepth). Permissive: ready_steps 0, depth window
# (0.05, 100), max_subfilter_outlier 100.
def exact_cases(invdepth):
    z = exact_z(invdepth)
    grown = 0.5 + math.sqrt(EXACT_RATIO_OVER)          # 1.5 + 2^-43, exact
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    return [
        ("ratio == 1 is no outlier: the counter is reset", EXACT_ON, {}, (0, 0.5), (0.0, READY, 3)),
        ("ratio == 1 + 2^-42 is one: the counter grows by sqrt(ratio)", EXACT_OVER, {}, (0, 0.5), (grown, READY, 3)),
        ("min_depth == z is no candidate", EXACT_ON, dict(min_depth=z), (0, 0.0), (0.0, READY, 0)),
        ("min_depth one ulp below z is one", EXACT_ON, dict(min_depth=dn(z)), (0, 0.0), (0.0, READY, 3)),
        ("max_depth == z is no candidate", EXACT_ON, dict(max_depth=z), (0, 0.0), (0.0, READY, 0)),
        ("max_depth one ulp above z is one", EXACT_ON, dict(max_depth=up(z)), (0, 0.0), (0.0, READY, 3)),
        ("max_subfilter_outlier == counter is no candidate", EXACT_OVER, dict(max_subfilter_outlier=grown), (0, 0.5), (grown, READY, 0)),
        ("max_subfilter_outlier one ulp above the counter is one", EXACT_OVER, dict(max_subfilter_outlier=up(grown)), (0, 0.5),
         (grown, READY, 3)),
        ("max_subfilter_outlier == 0 == the reset counter is no candidate", EXACT_ON, dict(max_subfilter_outlier=0.0), (0, 0.5),
         (0.0, READY, 0)),
        ("init_counter + 1 == ready_steps is INITIALIZING", EXACT_ON, dict(ready_steps=4), (3, 0.0), (0.0, sr.FEAT_INITIALIZING, 1)),
        ("init_counter + 1 == ready_steps + 1 is READY", EXACT_ON, dict(ready_steps=3), (3, 0.0), (0.0, READY, 3)),
    ]


PERMISSIVE = dict(Rtri=EXACT_RTRI, MH_thresh=EXACT_MH, ready_steps=0, min_depth=0.05, max_depth=100.0, max_subfilter_outlier=100.0)

STRADDLE_PER_CAMERA = 6


def straddle_cases(cam_name, invdepth):
    """the first cases of the outlier family (about half take ratio > 1) -> (c, prior, 80-bit ref at the family's own thresholds, idx)"""
    c = draw("outliers", cam_name, invdepth)
    ref = step_reference("outliers", cam_name, invdepth)[0]
    return c, prior_of(c), ref, list(range(STRADDLE_PER_CAMERA))


def straddle_opts(ref, prior, i):
    """per threshold the two option sets at value * (1 -+ OFF) and what the restatement decides there -> list of
    (name, side, opts, expect) with expect = dict(outlier=bool) or dict(cand0=bool). The counter threshold is taken in the
    outlier branch (MH_thresh = q / 4: ratio = 4, the counter is the prior one + 2 > 0); the depth thresholds around the z of
    the family's own MH_thresh, which stays."""
    q, z = float(ref["q"][i]), float(ref["z"][i])
    counter = float(LD(prior["oc"][i]) + np.sqrt(ref["q"][i] / LD(q / 4)))
    base = dict(Rtri=FAMILIES["outliers"]["Rtri"], ready_steps=0, min_depth=1e-3, max_depth=1e3, max_subfilter_outlier=1e3)
    out = []
    for side, f in (("below", 1 - OFF), ("above", 1 + OFF)):
        out.append(("MH_thresh", side, dict(base, MH_thresh=q * f), dict(outlier=f < 1)))
        out.append(("min_depth", side, dict(base, MH_thresh=MH_THRESH, min_depth=z * f), dict(cand0=f < 1)))
        out.append(("max_depth", side, dict(base, MH_thresh=MH_THRESH, max_depth=z * f), dict(cand0=f > 1)))
        out.append(("max_subfilter_outlier", side, dict(base, MH_thresh=q / 4, max_subfilter_outlier=counter * f), dict(cand0=f > 1)))
    return out


# ---------------------------------------------------------------- C: candidate order with ties
ORDER_POOL_MAX = (1, 2, 3, 64, 65, 256, 257, 511, 512)
ORDER_B = 3
ORDER_OPTS = dict(Rtri=3.5 ** 2, MH_thresh=50.0, ready_steps=1, min_depth=0.5, max_depth=8.0, max_subfilter_outlier=0.5)
# filter 0, entry e is kind MIX[e % len(MIX)]: T twin track (two tracks, by (e // len(MIX)) % 2), Z a P = 0 entry, R an ordinary
# random one, W a random one whose second pixel is wild (an outlier: not passing), F free, L* the same added one frame later
# (INITIALIZING at ready_steps = 1 when the early ones are READY)
MIX = ("T", "Z", "R", "F", "T", "LZ", "Z", "W", "LT", "LR", "T", "LZ")


def order_scene(pm, seed=0):
    """-> dict(poses [3 frames][B], early / late pool_new records, xp [2 steps][B, pm, 2], kind [B, pm] of str). Filter 0: the mix;
    filter 1: every entry P = 0 and early - one tie group, all passing; filter 2: P = 0 entries beyond max_depth (never passing)
    and one late ordinary entry at pm // 2 - the single passing entry without `strict`, none with it."""
    rng = np.random.default_rng([seed, pm])
    cam = synth.PINHOLE
    B = ORDER_B
    poses = []
    p0 = np.zeros(B, dtype=L.pose_dtype)
    for b in range(B):
        p0[b]["Rsb"], p0[b]["Tsb"] = cm(orc.so3_exp(rng.normal(size=3) * 0.2)), rng.normal(size=3) * 0.3
        p0[b]["Rbc"], p0[b]["Tbc"], p0[b]["Rsg"] = cm(RBC), TBC, cm(np.eye(3))
    poses.append(p0)
    for _ in range(2):
        p = poses[-1].copy()
        for b in range(B):
            p[b]["Rsb"] = cm(orc.so3_exp(rng.normal(size=3) * 0.001) @ p[b]["Rsb"].reshape(3, 3).T)
            p[b]["Tsb"] = p[b]["Tsb"] + rng.normal(size=3) * 0.004    # (a few pixels at 1 m: far inside MH_thresh = 50 at P = 0)
        poses.append(p)
    kind = np.full((B, pm), "F", dtype=object)
    recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
    recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B)
    recs["xp"] = np.stack([rng.uniform(150, 490, B * pm), rng.uniform(100, 380, B * pm)], 1)
    recs["z0"] = rng.uniform(1.0, 6.0, B * pm); recs["std_xyz"] = [0.002, 0.002, 0.3]
    recs["std_xyz"][:, 2] = rng.uniform(0.2, 0.4, B * pm)
    r2 = recs.reshape(B, pm)
    twin = [dict(xp=[250.0, 180.0], z0=2.0, std=[0.002, 0.002, 0.3]), dict(xp=[400.0, 300.0], z0=3.5, std=[0.002, 0.002, 0.25])]
    noise = rng.normal(size=(2, B, pm, 2))
    twin_noise = rng.normal(size=(2, 2, 2))
    for e in range(pm):
        k = MIX[e % len(MIX)]
        kind[0, e] = k
        if k.endswith("T"):
            t = (e // len(MIX)) % 2
            r2[0, e]["xp"], r2[0, e]["z0"], r2[0, e]["std_xyz"] = twin[t]["xp"], twin[t]["z0"], twin[t]["std"]
            noise[:, 0, e] = twin_noise[:, t]
        if k.endswith("Z"):
            r2[0, e]["std_xyz"] = 0.0
        if k == "W":
            noise[1, 0, e] += 400.0
        kind[1, e] = "Z"; r2[1, e]["std_xyz"] = 0.0
        kind[2, e] = "Z"; r2[2, e]["std_xyz"] = 0.0; r2[2, e]["z0"] = 20.0
    kind[2, pm // 2] = "LR"; r2[2, pm // 2]["std_xyz"] = [0.002, 0.002, 0.3]; r2[2, pm // 2]["z0"] = 2.0
    late = np.array([[str(k).startswith("L") for k in row] for row in kind])
    free = kind == "F"
    xp = np.zeros((2, B, pm, 2))
    for s in range(2):
        xp[s] = r2["xp"] + noise[s] * 0.5
    xp[0][late | free] = np.nan                    # a late entry is not in the pool yet in step 0
    xp[1][free] = np.nan
    return dict(poses=poses, early=r2[~late & ~free].copy(), late=r2[late].copy(), xp=xp, kind=kind, cam=cam)


def simulate_order_scene(sc):
    """the scene through the oracle alone -> entries [B, pm] subfilter_dtype (P column-major) after both steps and live [B, pm].
    Identical inputs are computed once (twins and P = 0 entries of one filter share their pixels only when they are twins)."""
    B, pm = sc["kind"].shape
    cam, o = sc["cam"], ORDER_OPTS
    ent = np.zeros((B, pm), dtype=L.subfilter_dtype)
    ent["ref_sind"] = -1
    live = np.zeros((B, pm), dtype=bool)
    cache = {}
    for recs, first in ((sc["early"], 0), (sc["late"], 1)):
        for r in recs:
            b, e = int(r["b"]), int(r["entry"])
            key = (b, first, r["xp"].tobytes(), float(r["z0"]), r["std_xyz"].tobytes(), sc["xp"][:, b, e].tobytes())
            if key not in cache:
                x = np.array([(r["xp"][0] - cam["cx"]) / cam["fx"], (r["xp"][1] - cam["cy"]) / cam["fy"], math.log(r["z0"])])
                P, ic, oc, st = np.diag(r["std_xyz"] ** 2), 0, 0.0, 0
                pa = sc["poses"][first][b]
                for s in range(first, 2):
                    p = sc["poses"][s + 1][b]
                    x, P, st, ic, oc = orc.subfilter_update(x, P, sc["xp"][s, b, e], p["Rsb"].reshape(3, 3).T, p["Tsb"], RBC, TBC,
                                                            pa["Rsb"].reshape(3, 3).T, pa["Tsb"], cam, o["Rtri"], o["MH_thresh"],
                                                            o["ready_steps"], ic, oc)
                c1, c2 = orc.candidate_flags(x, st, oc, o["min_depth"], o["max_depth"], o["max_subfilter_outlier"])
                cache[key] = (x, P, st, ic, oc, (1 if c1 else 0) | (2 if c2 else 0))
            x, P, st, ic, oc, cand = cache[key]
            f = ent[b, e]
            f["x"], f["P"], f["status"], f["init_counter"], f["outlier_counter"], f["candidate"] = x, cm(P), st, ic, oc, cand
            f["ref_sind"] = 0
            live[b, e] = True
    return ent, live


def python_order(ent, live, strict):
    """the sort on (-rank, P(2,2), entry) over the live entries that pass -> (order [B, pm] padded with -1, n [B], keys)"""
    B, pm = ent.shape
    order = np.full((B, pm), -1, dtype=np.int32); n = np.zeros(B, dtype=np.int32)
    keys = []
    want = 2 if strict else 1
    for b in range(B):
        k = sorted((-(2 if ent[b, e]["status"] == READY else 1), float(ent[b, e]["P"][8]), e) for e in range(pm)
                   if live[b, e] and (int(ent[b, e]["candidate"]) & want))
        n[b] = len(k)
        order[b, :len(k)] = [t[2] for t in k]
        keys.append(k)
    return order, n, keys


def tie_report(keys, pm):
    """of the sorted keys of a batch -> (size of the largest tie group, whether a tie crosses position pm // 2 somewhere)"""
    biggest, crosses = 0, False
    for k in keys:
        run = 0
        for i, t in enumerate(k):
            run = run + 1 if i and t[:2] == k[i - 1][:2] else 1
            biggest = max(biggest, run)
        h = pm // 2
        if 1 <= h < len(k) and k[h][:2] == k[h - 1][:2]:
            crosses = True
    return biggest, crosses


# ---------------------------------------------------------------- D: AdaptInitialDepth
ADAPT_PM, ADAPT_F = 512, 4
ADAPT_Z0, ADAPT_BETA = 2.5, 0.7


def _spread(n, lo=1.0, hi=5.0, seed=0):
    return np.random.default_rng([77, seed, n]).uniform(lo, hi, n)


def adapt_scene():
    """Inverse-depth depth sets, one filter each (P = 0 pool entries whose x never moves, in-state features with x[2] as given):
    -> dict(names [B], feats [B, F] feat_dtype, early / late / fresh pool_new records, drop [B, pm] bool: freed in step 2).
    early entries take steps 1 and 2 (init_counter 2), late ones step 2 only (1), fresh ones none before the first rounds."""
    names, feat_x2, early, late, fresh, drops = [], [], [], [], [], []

    def filt(name, instate=(), e=(), l=(), f=(), d=(), stride=1):
        b = len(names)
        names.append(name); feat_x2.append(list(instate))
        pos = 0
        for lst, vals in ((early, e), (late, l), (fresh, f), (drops, d)):
            for z in vals:
                lst.append((b, pos * stride, float(z)))
                pos += 1
        assert (pos - 1) * stride < ADAPT_PM and len(instate) <= ADAPT_F, name

    inv = lambda z: 1.0 / np.asarray(z, dtype=np.float64)
    filt("n = 0")
    filt("n = 1", instate=inv([3.0]))
    filt("n = 2: the larger of two", instate=inv([3.0, 1.5]))
    filt("n = 3", instate=inv([4.0, 1.25]), e=[2.75])
    filt("n = 255, every other entry", e=_spread(255), stride=2)
    filt("n = 256 = 252 entries + 4 in state", instate=inv(_spread(4, seed=1)), e=_spread(252, seed=1))
    filt("n = 257, entries 0..256", e=_spread(257))
    filt("n = F + 512", instate=inv(_spread(4, seed=2)), e=_spread(512, seed=2))
    filt("all depths equal", instate=inv([2.0, 2.0]), e=[2.0] * 8)
    filt("duplicates of the median on both sides of rank n / 2", e=list(_spread(15, 1.0, 2.9)) + [3.0] * 11 + list(_spread(15, 3.1, 5.0)))
    # a non-finite depth is left out. Each filter's count of finite depths has the parity at which one more value - at the top
    # (+inf), at the bottom (-inf), or uncounted (NaN compares false) - would move the value of rank n / 2
    filt("+inf depth is left out", instate=[0.0, 1.0 / 1.75], e=[1.5, 1.25, 4.0, 4.5, 2.0, 4.75])
    filt("NaN x[2] is left out", instate=[np.nan, 1.0 / 1.75], e=[1.5, 1.25, 4.0, 4.5, 2.0, 4.75])
    filt("-inf depth is left out", instate=[-0.0, 1.0 / 1.75], e=[1.5, 1.25, 4.0, 4.5, 2.0])
    filt("selection", e=[1.0, 2.0, 3.0, 4.0, 4.5], l=[4.6, 4.7, 4.8, 4.9], f=[4.91, 4.92, 4.93, 4.94, 4.95, 4.96], d=[1.1, 1.2, 1.3, 1.4])
    filt("median == min_z", e=[0.75, 0.5, 0.875])
    filt("median == max_z", e=[6.5, 6.25, 7.0])
    B = len(names)
    feats = np.zeros((B, ADAPT_F), dtype=L.feat_dtype)
    feats["sind"] = -1
    for b, xs in enumerate(feat_x2):
        for j, x2 in enumerate(xs):
            feats[b, j]["x"] = [0.01 * j, -0.02, x2]; feats[b, j]["sind"] = j
    rec = lambda lst: _adapt_recs(lst)
    drop = np.zeros((B, ADAPT_PM), dtype=bool)
    for b, e, _ in drops:
        drop[b, e] = True
    return dict(names=names, feats=feats, early=rec(early + drops), late=rec(late), fresh=rec(fresh), drop=drop, B=B)


def _adapt_recs(lst):
    r = np.zeros(len(lst), dtype=L.pool_new_dtype)
    for i, (b, e, z) in enumerate(lst):
        r[i]["b"], r[i]["entry"], r[i]["z0"] = b, e, z
        r[i]["xp"] = [200.0 + (e % 97), 150.0 + 3.0 * b]
    return r                                       # std_xyz = 0: P = 0


def adapt_sim_entries(sc, steps, invdepth=True):
    """the pool of adapt_scene after `steps` pool steps (2: as the first rounds see it, 3: one more), from Python alone: P = 0
    entries keep x, every step adds one to init_counter, ready_steps = 0 makes a stepped entry READY, a NaN pixel in step 2 frees
    -> dict(x2, status, init_counter, live) [B, pm]"""
    B = sc["B"]
    x2 = np.zeros((B, ADAPT_PM)); st = np.zeros((B, ADAPT_PM), dtype=np.int32); ic = np.zeros((B, ADAPT_PM), dtype=np.int32)
    live = np.zeros((B, ADAPT_PM), dtype=bool)
    for recs, first in ((sc["early"], 1), (sc["late"], 2), (sc["fresh"], 3)):
        for r in recs:
            b, e = int(r["b"]), int(r["entry"])
            x2[b, e] = 1.0 / r["z0"] if invdepth else math.log(r["z0"])
            n = max(0, steps - first + 1)
            if sc["drop"][b, e]:
                n = min(n, 1)
            ic[b, e], st[b, e], live[b, e] = n, (READY if n > 0 else 0), not (sc["drop"][b, e] and steps >= 2)
    return dict(x2=x2, status=st, init_counter=ic, live=live)


def adapt_depths(feats_b, sim, b, min_lifetime, invdepth=True):
    """the depth set of filter b as AdaptInitialDepth selects it (manager.cpp:257-261; non-finite depths left out)"""
    x = [f["x"][2] for f in feats_b if f["sind"] >= 0]
    sel = sim["live"][b] & (sim["status"][b] == READY) & (sim["init_counter"][b] > min_lifetime)
    x = np.array(x + list(sim["x2"][b][sel]), dtype=np.float64)
    with np.errstate(all="ignore"):
        d = 1.0 / x if invdepth else np.exp(x)
    return d[np.isfinite(d)]


def adapt_expected(d, z, beta, min_z, max_z):
    """-> (init_z afterwards, 'empty' / 'out of range' / 'update')"""
    if len(d) == 0:
        return z, "empty"
    m = np.sort(d)[len(d) // 2]
    if m < min_z or m > max_z:
        return z, "out of range"
    return (1.0 - beta) * z + beta * m, "update"
