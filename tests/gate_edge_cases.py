"""Inputs, routes and bounds for the in-state gate (Estimator::MHGating, src/update.cpp:60-96) and Estimator::OnePointRANSAC
(src/update.cpp:213-393) at thresholds and ties, against tests/gate_restate.py. tests/test_gate_edges_cpu.py checks that every case
sits where it claims; tests/test_gate_edges_gpu.py runs them on the device.

The gate runs in five kernels, each stating its rules through gate_device.h. What reaches which copy (ROUTES below; asserted from the FLAG_PROFILE stage
labels / last_route() in every GPU test):
  gate_sparse_kernel                 xivo_hip_mh_gate on the resident scene             counts present entries (sind >= 0)
  gate_dense_kernel                  xivo_hip_mh_gate_dense, update_dense_gated on      present = F (a scene's entries are counted only
                                     dense rows / XIVO_HIP_FLAG_DENSE_H                 by the calibration gate, which hands them in)
  gate_ell_kernel                    update_dense_gated on compressed rows, < 512       present = F
                                     filters or the latency route; the 2 x 2 blocks from
                                     the S kernel's compact copy, or off S (ell_blocks_off_S)
  fused_update_f64_kernel's gate     update_dense_gated on the one-kernel route         present = F
  chol_reg_la_f64_kernel's prologue  update_dense_gated, >= 512 filters                 present = F

The feature-level calls exist on two scenes, "feature" (the default build: gate_sparse_kernel) and "calib" (an online-calibration
build, 43-column rows: gate_sparse_kernel's wide form, with XIVO_HIP_FLAG_DENSE_H gate_dense_kernel counting the scene's present
entries, and - through xivo_hip_one_point_ransac - gate_dense_kernel with no_relax, the calibration rescue).
The update-level calls exist on two sets of rows, "update" (21-column rows) and "dense" (the same with every column non-zero),
each with its own bounds: a route runs the set its rows name.

A call is B <= 8 filters of F <= 8 features on ng = 3 groups (N = 65; 90 in the calibration layout) unless it says otherwise. An
update-level call hands over whole rows J (21 columns scattered over the state: the blocks at Wsb, Tsb, Wbc, Tbc, the six group columns, the feature),
a feature-level call a scene whose rows the device's own Jacobian pass makes (an input here: the GPU test reads them back and
the restatement works on what it read).

Families
  A  distance accuracy: one filter per conditioning class (CLASSES), |r| from 1e-6 to 1e3 px over its features, huge threshold.
  B  a chosen feature's innovation scaled so its 80-bit distance is thresh (1 -+ m): filter 2k has feature k just inside,
     filter 2k + 1 just outside; on the `easy` prior and on the k1e8 prior.
  C  exact ties by two calls (built on the device's own distances: see the GPU test); the inputs are family B's easy scene.
  D  the relaxation loop's branches (D_CALLS).
  E  OnePointRANSAC: norm tie, state selection, gauge, FindNewRefGroup ties, mask width (RANSAC section below).

Bounds (family A): per class 4 x the worst relative error of the fp64 oracle (orc.mh_distances) against the 80-bit restatement
over that class's inputs, floored at 4 * 2^-53. They are computed, never typed in: the tests take them from bounds(), and the
table here is bounds_table_lines() as tests/test_gate_edges_cpu.py::test_bounds_table_is_the_one_written_down compares it, line
by line, with this docstring and with DESIGN section 5 (class, bound on the update, dense, feature, calib inputs, x 2^-53; the
priors of the kappa classes are rank one plus eps, so the products J P J^T cancel and fp64 itself pays about kappa u):

  easy         13        17        12        10
  k1e2         1.6e+03   4.3e+03   1.5e+03   9.4e+02
  k1e4         4e+04     9.1e+04   1.1e+05   1.2e+05
  k1e6         2e+07     3.7e+07   4.6e+06   1.4e+07
  k1e8         3.6e+09   2.4e+09   5.2e+08   1.2e+09
  k1e10        1.9e+11   1.5e+11   4.7e+10   1.4e+11
  k1e12        2.6e+13   4.5e+13   1.7e+12   4.2e+12
  r_dominates  10        10        7.3       8.7
  decades      11        22        11        20

Family B's margin is m = max(1e-6, 100 x the class bound)."""
import functools

import numpy as np

import gate_restate as gr
import xivo_oracle as orc
from scene_util import scene_arrays, spd
from xivo_amd import synth
from xivo_amd.lib import (FLAG_DENSE_H, FLAG_MULTI_KERNEL, FLAG_STANDALONE_TAIL, FLAG_SYMMETRIC_FORM, FLAG_THROUGHPUT_ROUTE)

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 4.0 * U
NG, NF, NB = 3, 8, 8
HUGE = 1e300
R_A = 2.0 ** -14                 # family A's measurement variance: small enough that kappa(S) reaches 1e12 with variances <= 1e4
R_B = 1.0
CAM = synth.RADTAN
MT, TP, SYM, TAIL, DH = FLAG_MULTI_KERNEL, FLAG_THROUGHPUT_ROUTE, FLAG_SYMMETRIC_FORM, FLAG_STANDALONE_TAIL, FLAG_DENSE_H
CLASSES = ("k1e2", "k1e4", "k1e6", "k1e8", "k1e10", "k1e12", "r_dominates", "decades")
KAPPA_TARGET = dict(k1e2=1e2, k1e4=1e4, k1e6=1e6, k1e8=1e8, k1e10=1e10, k1e12=1e12)

# name, context flags, rows ("rows": compressed 21-column rows, "dense": every column non-zero, "rows_n320": the compressed rows
# in a state of WIDE_STATE_N columns - zero columns of H, an identity prior on them - where the S kernel walks 32-wide slabs and
# leaves no compact copy of the diagonal blocks: gate_ell_kernel reads them off S), filters, entry point
# ("g" xivo_hip_update_dense_gated, "d" xivo_hip_mh_gate_dense), last_route() ("" = none: no update ran), gate copy
ROUTES = [
    ("fused", 0, "rows", NB, "g", "fused", "fused"),
    ("ell_latency", MT, "rows", NB, "g", "sparse_whitened", "gate_ell"),
    ("ell_in_solve", MT | TP, "rows", NB, "g", "sparse_in_solve", "gate_ell"),
    ("ell_blocks_off_S", MT, "rows_n320", NB, "g", "sparse_whitened", "gate_ell"),
    ("chol_prologue", MT | TP, "rows", 512, "g", "sparse_in_solve", "chol"),
    ("ell_symmetric", SYM, "rows", NB, "g", "sparse_symmetric", "gate_ell"),
    ("ell_tail", TAIL, "rows", NB, "g", "sparse_tail", "gate_ell"),
    ("dense_ascoded", DH, "rows", NB, "g", "dense_ascoded", "gate_dense"),
    ("dense_whitened", 0, "dense", NB, "g", "dense_whitened", "gate_dense"),
    ("dense_whitened_tp", TP, "dense", NB, "g", "dense_whitened", "gate_dense"),
    ("dense_symmetric", SYM, "dense", NB, "g", "dense_symmetric", "gate_dense"),
    ("mh_gate_dense", 0, "rows", NB, "d", "", "gate_dense"),
    ("mh_gate_dense_dh", DH, "rows", NB, "d", "", "gate_dense"),
]
ROUTE_NAMES = [r[0] for r in ROUTES]
WIDE_STATE_N = 320               # 64 values of 320 source columns pass the 160 KB of LDS: the S kernel takes 32-wide slabs
LEVELS = ("update", "dense", "feature", "calib")   # a call's inputs: compressed rows | dense rows | a scene | a scene of an online-calibration build
SCENE_LEVELS = ("feature", "calib")                # the gates of these count the present entries


def level_of(rname):
    return "dense" if route(rname)[2] == "dense" else "update"


def route(name):
    return next(r for r in ROUTES if r[0] == name)


# ---------------------------------------------------------------- rows and priors
def layout(F=NF, ng=NG):
    return orc.Layout(ng, F)


def rows21(B, F, seed, ng=NG, scale=100.0):
    """whole rows of B x F features: 2 x 3 blocks of N(0, scale^2) at Wsb, Tsb, Wbc, Tbc, the group's six columns and the
    feature's three (feature f in slot f, anchored to group f mod ng) - the 21 columns Feature::ComputeJacobian fills"""
    lay = layout(F, ng)
    rng = np.random.default_rng(seed)
    J = np.zeros((B, F, 2, lay.N))
    for f in range(F):
        g = lay.group_begin + 6 * (f % ng)
        s = lay.feature_begin + 3 * f
        for c in (0, 3, 15, 18, g, g + 3, s):
            J[:, f, :, c:c + 3] = rng.normal(0, scale, size=(B, 2, 3))
    return J


def densified(J, seed):
    """the same rows with every column non-zero (no compressed form holds them: the dense pipeline)"""
    rng = np.random.default_rng(seed)
    return J + rng.uniform(-1.0, 1.0, size=J.shape) * 2.0 ** -6


def corr(N, seed):
    C = spd(N, seed)
    s = 1.0 / np.sqrt(np.diag(C))
    C = C * np.outer(s, s)
    return 0.5 * (C + C.T)


def _kappa64(J, P, R):
    out = []
    for f in range(len(J)):
        S = J[f] @ P @ J[f].T + R * np.eye(2)
        out.append(np.linalg.cond(0.5 * (S + S.T)))
    return float(np.median(out))


def prior_parallel(J, seed, target, R, var=1e4):
    """var (eps C + w w^T), |w_i| <= 1: every feature's two rows see nearly the same one-dimensional subspace of P, so S is nearly
    singular; eps by bisection so the median kappa(S) over the filter's features is `target` (variances <= 2 var)."""
    N = J.shape[-1]
    rng = np.random.default_rng(seed)
    w = rng.normal(size=N)
    w /= np.abs(w).max()
    C, W = corr(N, seed + 1), np.outer(w, w)
    lo, hi = -40.0, 4.0                            # log2 eps: kappa falls as eps grows
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if _kappa64(J, var * (2.0 ** mid * C + W), R) > target:
            lo = mid
        else:
            hi = mid
    return var * (2.0 ** (0.5 * (lo + hi)) * C + W)


def prior_decades(J, seed, lo=-6, hi=2):
    """D C D with standard deviations 10^lo .. 10^hi (powers of two: exact) drawn per 3-column block"""
    N = J.shape[-1]
    rng = np.random.default_rng(seed)
    e = np.repeat(rng.integers(int(np.floor(lo * np.log2(10))), int(np.ceil(hi * np.log2(10))) + 1, size=(N + 2) // 3), 3)[:N]
    e[:3] = int(np.floor(lo * np.log2(10)))       # both ends of the range are there: Wsb at the bottom,
    e[3:6] = int(np.ceil(hi * np.log2(10)))       # Tsb at the top - columns every row touches
    D = np.ldexp(1.0, e)
    return corr(N, seed + 1) * np.outer(D, D)


def class_prior(cls, J, seed, R):
    if cls in KAPPA_TARGET:
        return prior_parallel(J, seed, KAPPA_TARGET[cls], R)
    if cls == "r_dominates":
        return prior_decades(J, seed, lo=-6.6, hi=-6.1)    # variances 1e-13 .. 1e-12: J P J^T << R
    if cls == "decades":
        return prior_decades(J, seed)                      # variances 1e-12 .. 1e4: R << J P J^T
    if cls == "easy":
        return corr(J.shape[-1], seed + 1) * 2.0 ** -20    # J P J^T about R_B
    raise KeyError(cls)


def unit_dirs(B, F, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.2, 1.37, size=(B, F)) * rng.choice([-1.0, 1.0], size=(B, F))   # away from the axes
    return np.stack([np.cos(a), np.sin(a)], axis=-1)


# ---------------------------------------------------------------- the feature-level scene
@functools.lru_cache(maxsize=None)
def feature_scene(F=NF, B=NB, ng=NG, seed=11):
    """a synth.g_level scene with the oracle's rows (whole rows over the N columns) and predicted pixels. P and the pixels of
    every feature-level call are built from THESE on the host, so the CPU and the GPU test hold the same inputs; the GPU test's
    restatement then works on the rows and innovations the device's Jacobian pass made of them."""
    sc = synth.g_level(ng, F, F, B, seed=seed, cam=CAM)
    lay = orc.Layout(ng, F, N=sc["N"])
    J = np.zeros((B, F, 2, lay.N)); pred = np.zeros((B, F, 2))
    for b in range(B):
        for i in range(F):
            r, s = int(sc["ref"][b, i]), int(sc["sind"][b, i])
            Jf, inn, _ = orc.compute_jacobian(sc["x"][b, i], np.zeros(2), sc["gR"][b, r], sc["gT"][b, r], sc["Rsb"][b], sc["Tsb"][b],
                                              sc["Rbc"][b], sc["Tbc"][b], CAM, lay, r, s)
            J[b, i] = Jf; pred[b, i] = -inn
    return dict(sc=sc, lay=lay, J=J, pred=pred)


CALIB_CAM_DIM = 9                # Camera::dim() of the radial-tangential model


@functools.lru_cache(maxsize=None)
def calib_scene(F=NF, B=NB, ng=NG, seed=11):
    """feature_scene in the layout of an online-calibration build (td, Cg / Ca, the nine intrinsics are state): the rows have
    43 columns - the 21 of the default build, td, Cg (9), bg (3) and the intrinsics (src/feature.cpp:623-651)"""
    sc = synth.g_level(ng, F, F, B, seed=seed, cam=CAM)
    lay = orc.calib_layout(ng, F, True, True, CALIB_CAM_DIM)
    rng = np.random.default_rng(seed + 1)
    cals = [dict(gyro=rng.normal(size=3) * 0.5, Cg=np.eye(3) + 0.01 * rng.normal(size=(3, 3)), bg=rng.normal(size=3) * 0.01,
                 Vsb=rng.normal(size=3), td=0.01 + 0.005 * b) for b in range(B)]
    J = np.zeros((B, F, 2, lay.N)); pred = np.zeros((B, F, 2))
    for b in range(B):
        for i in range(F):
            r, s_ = int(sc["ref"][b, i]), int(sc["sind"][b, i])
            out = orc.compute_jacobian(sc["x"][b, i], np.zeros(2), sc["gR"][b, r], sc["gT"][b, r], sc["Rsb"][b], sc["Tsb"][b],
                                       sc["Rbc"][b], sc["Tbc"][b], CAM, lay, r, s_, calib=cals[b])
            J[b, i] = out[0]; pred[b, i] = -out[1]
    return dict(sc=sc, lay=lay, J=J, pred=pred, cals=cals)


def calib_arrays(scn, poses):
    """the calibration state of calib_scene as xivo_hip_set_calib_state takes it (and Vsb / bg into the poses)"""
    from xivo_amd.lib import calib_dtype, cam_intr
    calib = np.zeros(len(scn["cals"]), dtype=calib_dtype)
    for b, cal in enumerate(scn["cals"]):
        poses[b]["Vsb"], poses[b]["bg"] = cal["Vsb"], cal["bg"]
        calib[b]["gyro"], calib[b]["Cg"], calib[b]["td"] = cal["gyro"], cal["Cg"].T.reshape(-1), cal["td"]
        calib[b]["Ca"], calib[b]["intr"] = np.eye(3).reshape(-1), cam_intr(CAM)
    return calib


def full_rows_calib(J21, Jc, lay, ref, sind):
    """whole 43-column rows from xivo_hip_get_jacobians and xivo_hip_get_jacobians_calib ([.., F, 2, 22]: td | Cg 9 | bg 3 |
    intrinsics 9, wide_scol of gate_kernels.hip)"""
    out = full_rows(J21, lay, ref, sind)
    cols = np.concatenate([[lay.td], lay.Cg + np.arange(9), BG_COL + np.arange(3), lay.cam_begin + np.arange(lay.cam_dim)])
    here = (np.asarray(sind) >= 0)[..., None, None]
    out[..., cols] = np.where(here, np.asarray(Jc)[..., :13 + lay.cam_dim], 0.0)
    return out


BG_COL = 9                       # Index::bg


def full_rows(J21, lay, ref, sind):
    """compact rows [.., F, 2, 21] as xivo_hip_get_jacobians returns them -> whole rows [.., F, 2, N] (jcol of feature_chi2_device.h);
    an absent entry (sind < 0) is a zero row"""
    J21 = np.asarray(J21)
    out = np.zeros(J21.shape[:-1] + (lay.N,))
    for idx in np.ndindex(J21.shape[:-2]):
        r, s = int(ref[idx]), int(sind[idx])
        if s < 0:
            continue
        cols = np.concatenate([np.arange(0, 6), np.arange(15, 21), lay.group_begin + 6 * r + np.arange(6), lay.feature_begin + 3 * s + np.arange(3)])
        out[idx][:, cols] = J21[idx]
    return out


# ---------------------------------------------------------------- a call
class Call:
    """One launch: B filters x F features. level "update": rows J are handed over as H; "feature": the scene's rows.
    here [B, F]: present entries (update level: an absent entry keeps its row and has a zero innovation - distance 0 - and counts).
    tags / expect: per filter, what the filter is there for and what the restatement must find (checked on the CPU)."""

    def __init__(self, name, family, level, J, P, inn, R, thresh, mult, min_inliers, here=None, tags=None, expect=None, cls=None,
                 scene=None, margin=0.0):
        self.name, self.family, self.level = name, family, level
        self.J, self.P, self.inn, self.R = J, P, inn, R
        self.thresh, self.mult, self.min_inliers = thresh, mult, min_inliers
        self.B, self.F, _, self.N = J.shape
        self.here = np.ones((self.B, self.F), dtype=bool) if here is None else here
        self.tags, self.expect, self.cls, self.scene, self.margin = tags or {}, expect or {}, cls or {}, scene, margin
        if level not in SCENE_LEVELS:       # no measurement at the update level: the row stays, the innovation is zero (distance 0)
            self.inn = inn * self.here[..., None]

    def H(self):
        return self.J.reshape(self.B, 2 * self.F, self.N)

    def pixels(self):
        """feature level: measured pixels = the oracle's prediction + the wanted innovation"""
        return self.scene["pred"] + self.inn

    def feats(self):
        sc = dict(self.scene["sc"])
        sc["sind"] = np.where(self.here, sc["sind"], -1).astype(np.int32)
        return scene_arrays(sc, CAM, xp=self.pixels())


def evaluate(call, J=None, inn=None, counts_present=None):
    """the restatement of a call on rows J / innovations inn (default: the call's own): 80-bit distances, kappa, the oracle's
    fp64 distances, and per filter the gate as coded for the level (or for counts_present given)."""
    J = call.J if J is None else J
    inn = call.inn if inn is None else inn
    cp = (call.level in SCENE_LEVELS) if counts_present is None else counts_present
    d80 = np.zeros((call.B, call.F), dtype=LD); kap = np.zeros((call.B, call.F)); d64 = np.zeros((call.B, call.F))
    masks, dists, recs = [], [], []
    for b in range(call.B):
        d80[b], kap[b] = gr.distances_80(J[b], call.P[b], inn[b], call.R)
        d64[b] = orc.mh_distances(J[b], call.P[b], inn[b], call.R)
        m, d, rec = gr.gate(d80[b].astype(np.float64), call.here[b] if cp else np.ones(call.F, dtype=bool), call.thresh, call.mult,
                            call.min_inliers, cp)
        masks.append(m); dists.append(d); recs.append(rec)
    return dict(d80=d80, kappa=kap, d64=d64, mask=np.array(masks), dist=np.array(dists), rec=recs)


def rel_err(d, d80):
    d80 = np.asarray(d80, dtype=LD)
    return np.abs((np.asarray(d, dtype=LD) - d80) / d80).astype(np.float64)


def scaled_to(J, P, dirs, R, targets):
    """innovations along `dirs` whose 80-bit distance is `targets` (to a few ulp times kappa): d is quadratic in |r|"""
    inn = np.zeros(dirs.shape)
    for b in range(J.shape[0]):
        d, _ = gr.distances_80(J[b], P[b], dirs[b], R)
        inn[b] = dirs[b] * np.sqrt(np.asarray(targets[b], dtype=LD) / d).astype(np.float64)[:, None]
    return inn


def _base(level, F=NF, B=NB, seed=0):
    if level in SCENE_LEVELS:
        scn = feature_scene(F, B) if level == "feature" else calib_scene(F, B)
        return scn["J"], scn
    J = rows21(B, F, 100 + seed, scale=100.0)
    return (densified(J, 7) if level == "dense" else J), None


# ---------------------------------------------------------------- family A
@functools.lru_cache(maxsize=None)
def family_a(level):
    J, scn = _base(level)
    P = np.array([class_prior(c, J[b], 40 + b, R_A) for b, c in enumerate(CLASSES)])
    mag = 10.0 ** (-6.0 + 9.0 * np.arange(NF) / (NF - 1))          # |r| from 1e-6 to 1e3 px
    inn = unit_dirs(NB, NF, 3) * mag[None, :, None]
    return Call("A_" + level, "A", level, J, P, inn, R_A, HUGE, 1.1, 2, cls=dict(enumerate(CLASSES)), scene=scn)


@functools.lru_cache(maxsize=None)
def bounds():
    """{level: {class: 4 x worst oracle error, floored}} over family A's inputs and family B's easy scene"""
    out = {}
    for level in LEVELS:
        ev = evaluate(family_a(level))
        tab = {c: max(4.0 * rel_err(ev["d64"][b], ev["d80"][b]).max(), FLOOR) for b, c in enumerate(CLASSES)}
        eb = evaluate(family_b(level, "easy", _m=1e-6))
        tab["easy"] = max(4.0 * rel_err(eb["d64"], eb["d80"]).max(), FLOOR)
        out[level] = tab
    return out


def margin(level, cls):
    return max(1e-6, 100.0 * bounds()[level][cls])


# ---------------------------------------------------------------- family B
B_THRESH, B_MIN, B_MULT = 5.991, 2, 1.1
B_OTHERS = [0.5, 1.5, 3.0, 4.5, 7.5, 9.0, 12.0, 20.0]             # the other features: none near the threshold


@functools.lru_cache(maxsize=None)
def family_b(level, cls, _m=None):
    """filter 2k: feature k at thresh (1 - m); filter 2k + 1: feature k at thresh (1 + m); k = 0 .. 3"""
    m = margin(level, cls) if _m is None else _m
    J, scn = _base(level, seed=1)
    if cls == "easy":
        P = np.array([class_prior("easy", J[b], 60 + b, R_B) for b in range(NB)])
        R = R_B
    else:
        P = np.array([class_prior(cls, J[b], 70 + b, R_A) for b in range(NB)])
        R = R_A
    targets = np.tile(np.array(B_OTHERS), (NB, 1))
    tags, expect = {}, {}
    for b in range(NB):
        k, inside = b // 2, b % 2 == 0
        targets[b, k] = B_THRESH * (1.0 - m if inside else 1.0 + m)
        tags[b] = (k, "in" if inside else "out")
        expect[b] = dict(feature=k, inlier=inside, relaxations=0)
    inn = scaled_to(J, P, unit_dirs(NB, NF, 5), R, targets)
    return Call("B_%s_%s" % (level, cls), "B", level, J, P, inn, R, B_THRESH, B_MULT, B_MIN, tags=tags, expect=expect,
                cls={b: cls for b in range(NB)}, scene=scn, margin=m)


B_CLASSES = ("easy", "k1e8")


# ---------------------------------------------------------------- family D
INF = float("inf")


def _d_call(name, level, params, filters, F=NF, note=""):
    """filters: list of (tag, targets [F] with None = absent, expected relaxations, expected stop, extra) - distances placed by
    scaling the innovations on the easy prior"""
    thresh, mult, min_inl = params
    B = len(filters)
    J, scn = _base(level, F=F, B=B, seed=2)
    P = np.array([class_prior("easy", J[b], 80 + b, R_B) for b in range(B)])
    here = np.array([[t is not None for t in flt[1]] for flt in filters])
    targets = np.array([[1.0 if t is None else t for t in flt[1]] for flt in filters])
    inn = scaled_to(J, P, unit_dirs(B, F, 9), R_B, targets)
    tags = {b: flt[0] for b, flt in enumerate(filters)}
    expect = {b: dict(relaxations=flt[2], stop=flt[3], **(flt[4] if len(flt) > 4 else {})) for b, flt in enumerate(filters)}
    c = Call(name + "_" + level, "D", level, J, P, inn, R_B, thresh, mult, min_inl, here=here, tags=tags, expect=expect, scene=scn)
    c.note = note
    c.targets = targets
    return c


_X = None      # absent
D_SPECS = {
    # thresh 4, mult 2 (both exact), min_inliers 3
    "branches": ((4.0, 2.0, 3), [
        # present == min_inliers: no gating at the feature level (mask = present entries, dist = 0); the update level takes
        # present = F = 8 > 3 and gates the zero innovations in: the two rules differ here by construction
        ("present_eq_min", [100.0, _X, 1.0, _X, _X, 200.0, _X, _X], 0, None, dict(no_gating_feature=True)),
        # present == min_inliers + 1: gating; absent entries interleaved, in position 0 and last
        ("present_min_plus_1", [_X, 1.0, 2.0, _X, 3.0, 100.0, _X, _X], 0, gr.STOP_MIN_INLIERS),
        # the pass at thresh 8 reaches exactly 3 and stops: 10 lies between 8 and the next threshold 16 and stays out
        ("stop_exact_1_relaxation", [1.0, 2.0, 6.0, 10.0, 100.0, 100.0, 100.0, 100.0], 1, gr.STOP_MIN_INLIERS, dict(out=[3])),
        ("needs_2_relaxations", [1.0, 9.0, 10.0, 20.0, 100.0, 100.0, 100.0, 100.0], 2, gr.STOP_MIN_INLIERS, dict(out=[3])),
        # everything is an outlier until the pass that lets all in
        ("all_out_then_all_in", [9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 15.5], 2, gr.STOP_MIN_INLIERS, dict(all_in=True)),
        # the two rules agree: everything present, the same decisions at both levels
        ("rules_agree", [1.0, 2.0, 3.0, 5.0, 7.0, 17.0, 33.0, 100.0], 0, gr.STOP_MIN_INLIERS),
    ]),
    # 30 relaxations: 1.1^29 = 15.86 < d < 1.1^30 = 17.45 for the three smallest
    "relax30": ((1.0, 1.1, 3), [
        ("needs_30_relaxations", [16.2, 16.6, 17.0, 18.0, 100.0, 100.0, 100.0, 100.0], 30, gr.STOP_MIN_INLIERS, dict(out=[3])),
    ]),
    # min_inliers <= 0, as coded: the loop body never runs and nothing is an inlier (update.cpp:73)
    "min_inliers_0": ((4.0, 2.0, 0), [("no_loop", [1.0, 2.0, 3.0, 5.0, 7.0, 17.0, 33.0, 100.0], 0, gr.NO_LOOP)]),
    "min_inliers_neg": ((4.0, 2.0, -1), [("no_loop", [1.0, 2.0, 3.0, 5.0, 7.0, 17.0, 33.0, 100.0], 0, gr.NO_LOOP)]),
    # mult = 1: the reference never returns from here (one inlier, three wanted, a threshold that does not move). Pinned as coded:
    # 4096 passes, then the unrelaxed threshold decides
    "mult_1": ((4.0, 1.0, 3), [("guard_passes", [1.0, 5.0, 6.0, 7.0, 100.0, 100.0, 100.0, 100.0], gr.MAX_PASSES, gr.GUARD_PASSES)]),
}
# cross-pass: the only inliers sit in the second pass of the 64-lane count (F = 65) or in its last lane (F = 64)
D_WIDE = {
    "f65": (65, (4.0, 2.0, 1), [("inlier_in_lane_64", [100.0] * 64 + [1.0], 0, gr.STOP_MIN_INLIERS),
                                 ("inliers_after_relaxing", [100.0] * 63 + [5.0, 6.0], 1, gr.STOP_MIN_INLIERS)]),
    "f64": (64, (4.0, 2.0, 1), [("inlier_in_lane_63", [100.0] * 63 + [1.0], 0, gr.STOP_MIN_INLIERS)]),
}
WIDE_ROUTES = [("wide_default", 0, "rows", 2, "g", None, "gate_ell"), ("wide_dense", DH, "rows", 2, "g", "dense_ascoded", "gate_dense")]


@functools.lru_cache(maxsize=None)
def d_call(name, level):
    if name in D_SPECS:
        params, filters = D_SPECS[name]
        return _d_call("D_" + name, level, params, filters)
    F, params, filters = D_WIDE[name]
    return _d_call("D_" + name, level, params, filters, F=F)


D_NAMES = list(D_SPECS) + list(D_WIDE)


# ---------------------------------------------------------------- family E: OnePointRANSAC
E_R, E_MH, E_MULT, E_MIN = 1.0, 5.991, 1.1, 2
E_THRESH, E_CHI2 = 2.0, 5.89


def ransac_prior(lay, seed, scale=2.0 ** -14):
    return corr(lay.N, seed) * scale


def find_norm_ties(inn, want=2):
    """features of inn [.., 2] on which the fused and the unfused norm differ: (index, unfused, fused), `want` with
    fused < unfused and `want` with fused > unfused, in index order"""
    lo, hi = [], []
    flat = np.asarray(inn).reshape(-1, 2)
    for i, r in enumerate(flat):
        a, f = gr.norm_unfused(r[0], r[1]), gr.norm_fused(r[0], r[1])
        if f < a and len(lo) < want:
            lo.append((i, a, f))
        elif f > a and len(hi) < want:
            hi.append((i, a, f))
    return lo, hi


def tie_innovations(pred, seed, n=64, scale=1.5):
    """pixel offsets for one feature's prediction: candidates r = fl(fl(pred + o) - pred) the Jacobian pass will form (xp - Predict,
    feature.cpp:654-655) - a single IEEE subtraction of two known doubles, so the host knows the device's innovation exactly"""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, scale, size=(n, 2))
    xp = pred[None, :] + o
    return xp, xp - pred[None, :]


def state_st(sc, b):
    return dict(Rsb=sc["Rsb"][b].copy(), Tsb=sc["Tsb"][b].copy(), Vsb=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3),
                Rbc=sc["Rbc"][b].copy(), Tbc=sc["Tbc"][b].copy(), Rsg=np.eye(3), gR=sc["gR"][b].copy(), gT=sc["gT"][b].copy(),
                x=sc["x"][b].copy(), sind=sc["sind"][b].copy(), ref=sc["ref"][b].copy())


def sub_st(st, idx):
    s = dict(st)
    s["x"], s["sind"], s["ref"] = st["x"][idx], st["sind"][idx], st["ref"][idx]
    return s


def ransac_expect(st, P, xp, lay, mh, inn, thresh, chi2, gauge, ng):
    """OnePointRANSAC of one filter restated: decisions from gate_restate (the low-innovation test on the innovations `inn` the
    device formed), the partial update, AbsorbError and the rescue distances from the oracle with that low set handed in.
    Returns dict(dec, keep [F], chi {feature: d}, nrej)."""
    F = len(xp)
    low_all = np.array([gr.low_unfused(inn[f], thresh) for f in range(F)])
    dec = gr.ransac_decisions(mh, st["sind"], st["ref"], low_all, P, lay.group_begin, ng, gauge)
    idx = np.nonzero(dec["mh"])[0]
    keep = np.zeros(F, dtype=bool); chi = {}
    if len(idx) == 0:
        return dict(dec=dec, keep=keep, chi=chi, chi80={}, nrej=0)
    out = orc.one_point_ransac(sub_st(st, idx), P, xp[idx], CAM, lay, E_R, thresh, chi2, gauge, range(ng), low=dec["low"][idx])
    chi80 = {}
    for i, d in out["chi2"].items():
        chi[int(idx[i])] = d
        assert (i in out["inliers"]) == bool(gr.rescue(d, chi2))
        # the same distance in 80 bits, on the oracle's rows at the (partially updated) state and its P
        chi80[int(idx[i])] = gr.distance_80(out["rows"][i][0], out["P_rescue"], out["rows"][i][1], E_R)[0]
    keep[idx[out["inliers"]]] = True
    return dict(dec=dec, keep=keep, chi=chi, chi80=chi80, nrej=len(out["rejected"]), out=out)


def rescue_margin(expects):
    """family B's rule for the rescue test: m = max(1e-6, 100 x 4 x the oracle's worst relative error against the 80-bit distance
    over every rescue distance of the call)"""
    worst = max(float(abs((LD(e["chi"][f]) - e["chi80"][f]) / e["chi80"][f])) for e in expects for f in e["chi"])
    return max(1e-6, 100.0 * max(4.0 * worst, FLOOR))


RESCUE_PICKS = ((3, 0), (2, 0))      # (filter, feature) of e_states: a state-1 filter (after the partial update), a state-2 one (the prior)


# A route whose distance leaves its class bound, kept as a stated deviation with its measured factor:
# gate_sparse_kernel's 43-column form on the calibration scene at kappa(S) = 1e8 measured 1.75 x the bound (2.0e9 u against
# 4 x the oracle's 2.9e8 u; kappa <= 7.5e8, so 2.7 kappa u). Read from the code: the wide form is the 21-column form's fma chain
# and butterfly sum over 43 terms in the row's order - no slip; the a-priori bound of such a sum is gamma_43 kappa = 43 kappa u,
# sixteen times the measurement, and the same inputs through gate_dense_kernel sit at 0.32 of the class bound. The oracle's worst
# of eight samples is simply small there. Held under 2 x the bound.
STATED_DEVIATIONS = {("mh_gate_calib", "k1e8"): 2.0}


# ---------------------------------------------------------------- the bounds table (docstring above)
def bounds_table_lines():
    """one line per class: `class  update-level bound  feature-level bound`, in units of 2^-53, two significant digits"""
    b = bounds()
    return [(("%-12s" + " %-9.2g" * len(LEVELS)) % ((c,) + tuple(b[lv][c] / U for lv in LEVELS))).rstrip() for c in ("easy",) + CLASSES]


# ---------------------------------------------------------------- family E calls
def embedded_scene(B, F, slots, n_groups, seed=11):
    """feature_scene's filters with their ng = len(slots) groups moved to the given slots of an n_groups layout (identity poses
    in the unused slots); tile: every filter is filter 0"""
    base = feature_scene(F, B, len(slots), seed)["sc"]
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    gR = np.tile(np.eye(3), (B, n_groups, 1, 1)); gT = np.zeros((B, n_groups, 3))
    for k, s in enumerate(slots):
        gR[:, s] = base["gR"][:, k]; gT[:, s] = base["gT"][:, k]
    sc["gR"], sc["gT"] = gR, gT
    sc["ref"] = np.asarray(slots, dtype=np.int32)[base["ref"]]
    sc["n_groups"] = n_groups
    sc["N"] = 23 + 6 * n_groups + 3 * F
    return sc


def tiled(sc, B):
    out = dict(sc)
    for k, v in sc.items():
        if isinstance(v, np.ndarray) and v.shape[:1] == (sc["x"].shape[0],):
            out[k] = np.repeat(v[:1], B, axis=0)
    return out


def oracle_pred(sc, lay):
    B, F = sc["x"].shape[:2]
    pred = np.zeros((B, F, 2))
    for b in range(B):
        for i in range(F):
            r, s = int(sc["ref"][b, i]), int(sc["sind"][b, i])
            pred[b, i] = -orc.compute_jacobian(sc["x"][b, i], np.zeros(2), sc["gR"][b, r], sc["gT"][b, r], sc["Rsb"][b], sc["Tsb"][b],
                                               sc["Rbc"][b], sc["Tbc"][b], CAM, lay, r, s)[1]
    return pred


LOW, HIGH, FAR = 0, 1, 2         # 0.3 px noise | moved 2.5 .. 3.5 px per axis | moved 35 px (no MH inlier)


def noise_for(kinds, seed):
    """kinds [B, F] of LOW / HIGH / FAR -> pixel offsets"""
    kinds = np.asarray(kinds)
    rng = np.random.default_rng(seed)
    n = rng.normal(size=kinds.shape + (2,)) * 0.3
    hi = rng.choice([-1.0, 1.0], size=kinds.shape + (2,)) * rng.uniform(2.5, 3.5, size=kinds.shape + (2,))
    n = np.where((kinds == HIGH)[..., None], n + hi, n)
    return np.where((kinds == FAR)[..., None], n + 35.0, n)


class RansacCall:
    """One xivo_hip_one_point_ransac launch behind jacobians + xivo_hip_mh_gate(E_R, E_MH, E_MULT, E_MIN).
    absent [B, F]: entries with sind < 0 from the start; absent_after_gate: entries made absent between the gate and RANSAC (the
    mask still names them). expect_state / expect_tmpref (a slot, -1: none): per filter, what the restatement must find - on the
    oracle's innovations in the CPU test, on the device's in the GPU test."""

    def __init__(self, name, sc, n_groups, P, kinds, gauge, thresh=E_THRESH, chi2=E_CHI2, absent=None, absent_after_gate=None,
                 tags=None, expect_state=None, expect_tmpref=None, seed=0):
        self.name, self.sc, self.ng = name, sc, n_groups
        self.B, self.F = sc["x"].shape[:2]
        self.lay = orc.Layout(n_groups, self.F)
        self.P, self.kinds, self.gauge = P, np.asarray(kinds), np.asarray(gauge, dtype=np.int32)
        self.thresh, self.chi2 = thresh, chi2
        z = np.zeros((self.B, self.F), dtype=bool)
        self.absent = z if absent is None else np.asarray(absent, dtype=bool)
        self.absent_after = z if absent_after_gate is None else np.asarray(absent_after_gate, dtype=bool)
        self.tags, self.expect_state, self.expect_tmpref = tags or {}, expect_state or {}, expect_tmpref or {}
        self.noise = noise_for(self.kinds, 900 + seed)
        self.pred = oracle_pred(sc, self.lay)

    def arrays(self, xp, absent):
        sc = dict(self.sc)
        sc["sind"] = np.where(absent, -1, self.sc["sind"]).astype(np.int32)
        return scene_arrays(sc, CAM, xp=xp)

    def expect(self, xp, inn, mh):
        """per filter the restated call on measured pixels xp, the device's (or the oracle's) innovations inn and MH mask mh"""
        out = []
        for b in range(self.B):
            st = state_st(self.sc, b)
            st["sind"] = np.where(self.absent[b] | self.absent_after[b], -1, st["sind"])
            out.append(ransac_expect(st, self.P[b], xp[b], self.lay, mh[b], inn[b], self.thresh, self.chi2, int(self.gauge[b]), self.ng))
        return out

    def host_mh(self, inn):
        """the MH mask of the gate in front, restated on the oracle's rows (CPU test; the GPU test takes the device's mask)"""
        scn_J = np.zeros((self.B, self.F, 2, self.lay.N))
        for b in range(self.B):
            for i in range(self.F):
                r, s = int(self.sc["ref"][b, i]), int(self.sc["sind"][b, i])
                scn_J[b, i] = orc.compute_jacobian(self.sc["x"][b, i], np.zeros(2), self.sc["gR"][b, r], self.sc["gT"][b, r], self.sc["Rsb"][b],
                                                   self.sc["Tsb"][b], self.sc["Rbc"][b], self.sc["Tbc"][b], CAM, self.lay, r, s)[0]
        mh = np.zeros((self.B, self.F), dtype=bool)
        for b in range(self.B):
            d = orc.mh_distances(scn_J[b], self.P[b], inn[b], E_R)
            mh[b] = gr.gate(d, ~self.absent[b], E_MH, E_MULT, E_MIN, True)[0]
        return mh


def _spd_priors(N, B, seed):
    return np.array([spd(N, seed + b) * 1e-4 for b in range(B)])


@functools.lru_cache(maxsize=None)
def e_states():
    B, F = NB, NF
    sc = feature_scene(F, B)["sc"]
    L, H, X = LOW, HIGH, FAR
    kinds = [[L] * 8,                         # 0: every entry absent: no MH inlier
             [L] * 8,                         # 1: all low
             [H] * 8,                         # 2: none low
             [H, H, L, H, H, H, H, H],        # 3: exactly one low
             [L, L, L, L, H, L, L, L],        # 4: exactly one not low
             [L, H, L, H, L, H, L, L],        # 5: entry 1 (high) and entry 2 (low) go absent behind the gate: the mask still names them
             [L, H, H, L, L, H, H, L],        # 6: gauge group 1 holds a low inlier (4, 7): no temporary reference
             [H, L, L, H, L, L, H, L]]        # 7: gauge group 0 holds only high inliers (0, 3, 6): temporary reference, group 0 zeroed
    absent = np.zeros((B, F), dtype=bool); absent[0] = True
    after = np.zeros((B, F), dtype=bool); after[5, [1, 2]] = True
    gauge = [0, 0, 1, -1, NG, 2, 1, 0]        # (filter 4: gauge >= n_groups names no group)
    tags = dict(enumerate(["no_mh_inlier", "all_low", "none_low", "one_low", "one_not_low", "masked_but_absent", "gauge_has_low", "gauge_only_high"]))
    return RansacCall("E_states", sc, NG, _spd_priors(sc["N"], B, 300), kinds, gauge, absent=absent, absent_after_gate=after, tags=tags,
                      expect_state={0: 0, 1: 0, 2: 2, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1}, expect_tmpref={3: 2, 4: 2, 5: 0, 6: -1, 7: 2}, seed=1)


TIE_VARIANCES = 2.0 ** -11 * np.array([1.25, 0.125, 0.125, 0.125, 0.125, 0.125])  # their ascending sum, 1.875 * 2^-11, is exact and
                                                                                 # shares the binade of entry 0: one ulp there is one ulp of the sum


def _copy_group_diag(P, lay, groups, bump=2.0 ** -9):
    """the six variances of `groups` set to TIE_VARIANCES - bit copies of each other, larger than what was there, so P only gains
    a non-negative diagonal - and every other group's raised by `bump` so the copies hold the minimum"""
    P = P.copy()
    for g in range(lay.n_groups):
        i = lay.group_begin + 6 * g + np.arange(6)
        assert (P[i, i] < TIE_VARIANCES).all()
        P[i, i] = TIE_VARIANCES if g in groups else P[i, i] + bump
    return P


@functools.lru_cache(maxsize=None)
def e_ref_ties():
    """gauge -1, a low inlier in every group: FindNewRefGroup picks among all three. The same scene in every filter."""
    B, F = 6, NF
    sc = tiled(feature_scene(F, 1)["sc"], B)
    lay = orc.Layout(NG, F)
    P0 = spd(lay.N, 350) * 1e-4
    g = lay.group_begin
    P = []
    P.append(_copy_group_diag(P0, lay, [1, 2]))                         # 0: two-way tie: the lowest slot, 1
    P.append(_copy_group_diag(P0, lay, [0, 1, 2]))                      # 1: three-way tie: 0
    for grp, way in ((2, -np.inf), (1, np.inf), (2, np.inf), (1, -np.inf)):   # 2 .. 5: one variance one ulp down / up
        Pk = _copy_group_diag(P0, lay, [1, 2])
        i = g + 6 * grp
        Pk[i, i] = np.nextafter(Pk[i, i], way)
        P.append(Pk)
    kinds = [[LOW, LOW, LOW, HIGH, HIGH, LOW, LOW, HIGH]] * B           # high inliers to rescue: their chi tells which group went
    return RansacCall("E_ref_ties", sc, NG, np.array(P), kinds, [-1] * B,
                      tags=dict(enumerate(["tie_2", "tie_3", "g2_ulp_down", "g1_ulp_up", "g2_ulp_up", "g1_ulp_down"])),
                      expect_state={b: 1 for b in range(B)}, expect_tmpref={0: 1, 1: 0, 2: 2, 3: 2, 4: 1, 5: 1}, seed=2)


WIDE_SLOTS = (31, 32, 63)


@functools.lru_cache(maxsize=None)
def e_mask_width():
    """64 group slots, the features in slots 31, 32 and 63"""
    B, F, ng = 4, NF, 64
    sc = embedded_scene(B, F, WIDE_SLOTS, ng)
    lay = orc.Layout(ng, F)
    P = _spd_priors(lay.N, B, 370)
    i31 = lay.group_begin + 6 * 31 + np.arange(6)
    for b in range(B):
        P[b][i31, i31] += 1e-4                                          # the temporary reference is never slot 31
    L, H = LOW, HIGH
    # feature f sits in slot WIDE_SLOTS[f mod 3]
    kinds = [[L, L, L, H, L, L, H, L],        # 0: gauge -1: temporary reference in slot 32 or 63
             [L, L, L, H, L, H, L, L],        # 1: gauge 63 holds a low inlier: none
             [L, H, L, L, H, L, L, H],        # 2: slot 32 holds only high inliers (1, 4, 7): zeroed as an active group (bit 32); gauge 32
             [H, L, H, H, L, H, H, L]]        # 3: slots 31 and 63 only high: both zeroed (bits 31, 63), gauge 31: temporary reference 32
    return RansacCall("E_mask_width", sc, ng, P, kinds, [-1, 63, 32, 31],
                      tags=dict(enumerate(["tmpref_high_slot", "gauge_63", "zero_bit_32", "zero_bits_31_63"])),
                      expect_state={b: 1 for b in range(B)}, expect_tmpref={0: 63, 1: -1, 2: 63, 3: 32}, seed=3)


@functools.lru_cache(maxsize=None)
def e_ties_call():
    """the scene of the norm-tie calls: filter 0 carries the tie feature (its pixel is chosen from the predictions, see
    find_tie_pixels); the other filters mix low and high innovations far from every norm tried"""
    B, F = 4, NF
    sc = feature_scene(F, NB)["sc"]
    sc = {k: (v[:B].copy() if isinstance(v, np.ndarray) and v.shape[:1] == (NB,) else v) for k, v in sc.items()}
    L, H = LOW, HIGH
    kinds = [[L, L, L, L, L, L, L, H], [L, H, L, L, H, L, L, L], [H, L, L, L, L, H, L, L], [L, L, L, H, L, L, L, L]]
    return RansacCall("E_norm_ties", sc, NG, _spd_priors(sc["N"], B, 390), kinds, [0, 1, -1, 2], seed=4)


def find_tie_pixels(pred_b, want=2, skip=(7,)):
    """for filter 0 of e_ties_call: (feature, pixel, innovation, unfused norm, direction) with direction -1: fused < unfused,
    +1: fused > unfused - `want` of each, one per feature, in feature order. pred_b [F, 2]: the predictions the innovations
    will be formed against (the device's in the GPU test, the oracle's in the CPU test)."""
    found, count = [], {-1: 0, 1: 0}
    for f in range(len(pred_b)):
        if f in skip:
            continue
        xps, rs = tie_innovations(pred_b[f], 700 + f, n=1500, scale=0.9)
        for xp, r in zip(xps, rs):
            u, a = gr.norm_unfused(r[0], r[1]), gr.norm_fused(r[0], r[1])
            d = -1 if a < u else (1 if a > u else 0)
            if d and count[d] < want and 1.0 < u < 1.5:      # above the 0.3 px noise of the low features, below every high one
                found.append((f, xp, r, u, d)); count[d] += 1
                break
    return found, count
