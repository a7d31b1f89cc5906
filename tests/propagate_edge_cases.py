"""Inputs, metrics and bounds for Estimator::Propagate on the device (propagate_state_wave_kernel<4|7>,
propagate_state_calib_kernel and the covariance tail) against tests/propagate_restate.py, the reference's propagation in 80 bits.

Metrics, per filter, against the restatement (P' the propagated covariance, d = sqrt(diag P) of the PRIOR):
  rel   ||E||_F / ||P'_ref||_F, E = P' - P'_ref
  corr  max |E_ij| / (d_i d_j)            the `corr` of tests/precise_ref.py: blind to how many decades the variances span
  sym   max |A - A_ref|_ij / (d_i d_j), A = P' - P'^T: with a symmetric prior A_ref is zero to 80-bit rounding and this is the
        symmetry defect of the result itself; with the asymmetric priors it is the defect beyond what exact arithmetic keeps
  Rsb   max entry error of Rsb
  Tsb, Vsb  max entry error / max(1, |value|)
  orth  max |Rsb^T Rsb - I|               (of the result itself: the reference normalises, estimator.cpp:612; the device and the
                                           fp64 oracle, which carry a matrix, do not)
A bound is never typed in: it is 4 x the fp64 oracle's worst value of the metric over the batch's filters (the oracle is the same
algorithm in plain fp64, so this is what fp64 itself costs on these inputs), floored at 4 * 2^-53, and has to come out under
the cap - the suite's typed-in tolerances, 1e-11 for the P metrics and 1e-12 for the state metrics. The cap is a condition on the
inputs: `spread`, the sub-step count and the long chain's length below are what keeps the oracle alone within it
(tests/test_propagate_accuracy_cpu.py asserts that for every batch).

Prior covariances: a correlation-like SPD matrix in other units, P -> D P D with D powers of two (precise_ref.scale: exact).
precise_ref.pow2_scales draws the structure columns (exponents -20 .. 2). Its block of smallest exponents sits at columns 16..31,
which in the motion block is Wbc / Tbc / Wsg, so the motion exponents are drawn here by the same rule with the low block where a
real filter has it: Wsb, Tsb, Vsb, Wbc, Tbc in [-spread, 0], and bg, ba, Wsg another 7 .. 13 below (standard deviations; variances
twice that: 4 .. 8 decades under pose and velocity). What limits `spread` is what propagation multiplies together - |accel| dt
d_W / d_V, dt d_V / d_T, ... - errors of a large-variance state carried into a row of a small-variance one."""
import functools
import operator

import numpy as np

import xivo_oracle as orc
import precise_ref as prf
import propagate_restate as pr
from scene_util import spd

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 4.0 * U
CAP_P, CAP_X = 1e-11, 1e-12
P_METRICS, X_METRICS = ("rel", "corr", "sym"), ("Rsb", "Tsb", "Vsb", "orth")
CAPS = dict(rel=CAP_P, corr=CAP_P, sym=CAP_P, Rsb=CAP_X, Tsb=CAP_X, Vsb=CAP_X, orth=CAP_X)
NG, NF = 1, 3                               # one group + three features behind the motion block
G_NOMINAL = np.array([0.0, 0.0, -9.796])
G_DYADIC = np.array([0.0, 0.0, -9.75])
H9 = 2.0 ** -9                              # the exact cases' stepsize
METHODS = ("RK4", "PrinceDormand")
LONG_CHAIN_SAMPLES = 256                    # the largest count tried; the bounds stay under the caps at it
SPREAD = dict(nominal=12, fast=12, norot=12, rest=12, chain=4, ctl=12, calib=12, exact=12, thr=12, mixed=12)


# ---------------------------------------------------------------- inputs
def motion_scales(seed, spread, nm=23):
    """one set of motion-block standard deviations per batch: Qimu and Qmodel are options of the call, one for all its filters,
    and have to sit in the same units"""
    rng = np.random.default_rng(seed)
    e = np.zeros(nm, dtype=np.int64)
    for blk in (0, 3, 6, 15, 18):
        e[blk:blk + 3] = rng.integers(-spread, 1)
    for blk, n in ((9, 3), (12, 3), (21, 2)):
        e[blk:blk + n] = rng.integers(-spread - 13, -spread - 6)
    if nm > 23:                             # td, Cg, Ca: calibration states, at the bottom as well
        e[23:] = rng.integers(-spread - 13, -spread - 6, size=nm - 23)
    return np.ldexp(1.0, e)


def prior(N, seed, Dm):
    C = spd(N, seed)
    s = 1.0 / np.sqrt(np.diag(C))
    C = C * np.outer(s, s)
    C = 0.5 * (C + C.T)
    D = prf.pow2_scales(N, seed)
    D[:len(Dm)] = Dm
    return prf.scale(D, C, np.ones((1, N)))[0]


def random_state(rng):
    return orc.MotionState(orc.so3_exp(rng.normal(size=3)), rng.normal(size=3), rng.normal(size=3) * 0.5,
                           rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05, orc.so3_exp(np.array([0.02, -0.03, 0.0])))


ROT90Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def dyadic_state(v=(0.5, -0.25, 0.125)):
    return orc.MotionState(ROT90Z, [1.0, -2.0, 0.5], v, [2.0 ** -6, -2.0 ** -7, 2.0 ** -6], [2.0 ** -4, 2.0 ** -5, -2.0 ** -4], np.eye(3))


class Batch:
    """One launch (or two: `split`) of B filters. imu: gyro / accel / sg / sa [B, n, 3], dt [B, n]."""

    def __init__(self, name, method, stepsize, X0, Dm, P0, imu, g, seed, ctl=None, split=None, layout=None, Cg=None, Ca=None, td=None,
                 distinct=None, expect=None, tags=None):
        self.name, self.method, self.stepsize, self.X0, self.P0, self.imu, self.g = name, method, stepsize, X0, P0, imu, g
        self.ctl, self.split, self.layout, self.Cg, self.Ca, self.td = ctl, split, layout, Cg, Ca, td
        self.B, self.n = imu["dt"].shape
        self.N = P0.shape[1]
        self.nm = 23 if layout is None else layout.motion_size
        # the noise in the batch's units: gyro / accel / bias noise densities of the order of the prior variance of the state
        # each drives per second, Qmodel a thousandth of the prior
        rng = np.random.default_rng(seed)
        self.Dm = Dm
        self.Qi = np.diag(rng.uniform(0.5, 2.0, 12) * np.concatenate([Dm[0:3], Dm[6:9], Dm[9:12], Dm[12:15]]) ** 2)
        A = rng.normal(size=(self.nm, self.nm)) / np.sqrt(self.nm) * Dm[:, None]
        self.Qm = A @ A.T * 1e-3
        self.distinct = list(range(self.B)) if distinct is None else distinct
        self.expect = expect or {}          # filter -> per sample a string of F (== stepsize), H (== stepsize / 2), R (another length)
        self.tags = tags or {}              # filter -> what the input is there for


def _imu(B, n):
    return dict(gyro=np.zeros((B, n, 3)), accel=np.zeros((B, n, 3)), sg=np.zeros((B, n, 3)), sa=np.zeros((B, n, 3)), dt=np.zeros((B, n)))


def _random_imu(rng, B, n, gyro=0.3):
    im = _imu(B, n)
    im["gyro"] = rng.normal(size=(B, n, 3)) * gyro
    im["accel"] = rng.normal(size=(B, n, 3)) + np.array([0, 0, 9.8])
    im["sg"] = rng.normal(size=(B, n, 3)) * 5.0
    im["sa"] = rng.normal(size=(B, n, 3)) * 20.0
    return im


def _N(layout=None):
    return (23 if layout is None else layout.group_begin) + 6 * NG + 3 * NF


def nominal(method, stepsize, B=64, seed=100):
    """gyro 0.3 rad/s, slopes 5 / 20, dt log-uniform in 2 .. 12 ms"""
    rng = np.random.default_rng(seed)
    im = _random_imu(rng, B, 1)
    im["dt"] = np.exp(rng.uniform(np.log(0.002), np.log(0.012), size=(B, 1)))
    X0 = [random_state(rng) for _ in range(B)]
    Dm = motion_scales(seed, SPREAD["nominal"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("nominal", method, stepsize, X0, Dm, P0, im, G_NOMINAL, seed)


def fast_spin(method, B=64, seed=200):
    """|gyro - bg| dt in (0.25, 1.5] rad in ONE step (stepsize -1, dt 0.1 s): one to three halvings of so3_exp_small"""
    rng = np.random.default_rng(seed)
    im = _random_imu(rng, B, 1)
    X0 = [random_state(rng) for _ in range(B)]
    for b in range(B):
        ax = rng.normal(size=3)
        im["gyro"][b, 0] = X0[b].bg + ax / np.linalg.norm(ax) * rng.uniform(2.6, 15.0)
        im["sg"][b, 0] = 0.0
    im["dt"][:] = 0.1
    Dm = motion_scales(seed, SPREAD["fast"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("fast_spin", method, -1.0, X0, Dm, P0, im, G_NOMINAL, seed)


def t2_threshold(method, seed=300):
    """the `t2 > 0.0625` switch of so3_exp_small on its threshold: bias-corrected gyro along one axis, |w| h = 0.25 (1 -+ 1e-6) and
    the dyadic |w| h = 0.25 itself (t2 == 0.0625: no halving); h = dt = 2^-3 in one step, no slope. tags: (axis, side) with side
    -1 / 0 / +1 = below / on / above"""
    rng = np.random.default_rng(seed)
    cases = [(ax, sd) for ax in range(3) for sd in (-1, 0, 1)]
    B = len(cases)
    im = _random_imu(rng, B, 1)
    im["sg"][:] = 0.0
    X0 = []
    for b, (ax, sd) in enumerate(cases):
        X = dyadic_state()
        X.Rsb = orc.so3_exp(rng.normal(size=3))
        w = np.zeros(3)
        w[ax] = 2.0 * (1.0 + sd * 1e-6)
        im["gyro"][b, 0] = X.bg + w          # exact for sd = 0: bg dyadic, small
        X0.append(X)
    im["dt"][:] = 0.125
    Dm = motion_scales(seed, SPREAD["thr"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("t2_threshold", method, -1.0, X0, Dm, P0, im, G_NOMINAL, seed, tags=dict(enumerate(cases)))


def t2_side(bt, b, T):
    """which side of 0.0625 the full step's t2 = |(gyro - bg) dt|^2 falls on, evaluated in dtype T as so3_exp_small forms it"""
    w = (np.asarray(bt.imu["gyro"][b, 0], dtype=T) - np.asarray(bt.X0[b].bg, dtype=T)) * T(bt.imu["dt"][b, 0])
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    return int(t2 > T(0.0625)) - int(t2 < T(0.0625))


def no_rotation(method, B=64, seed=400):
    """gyro == bg exactly and zero slope (w = 0 in every stage: Sophus's small-angle branch, the device's a = 1, b = 1/2), then
    |w| h around 1e-11 (still that branch: theta^2 < 1e-20), 1e-8 and 1e-5; one step of 5 ms"""
    rng = np.random.default_rng(seed)
    im = _random_imu(rng, B, 1)
    im["sg"][:] = 0.0
    X0 = [random_state(rng) for _ in range(B)]
    tags = {}
    for b in range(B):
        mag = (0.0, 1e-11, 1e-8, 1e-5)[b % 4]
        ax = rng.normal(size=3)
        im["gyro"][b, 0] = X0[b].bg + ax / np.linalg.norm(ax) * (mag / 0.005) if mag else X0[b].bg
        tags[b] = mag
    im["dt"][:] = 0.005
    Dm = motion_scales(seed, SPREAD["norot"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("no_rotation", method, -1.0, X0, Dm, P0, im, G_NOMINAL, seed, tags=tags)


def at_rest(method, B=64, seed=500):
    """Rsb accel_calib + Rsg g == 0 in dyadic values, zero velocity: Vsb and Tsb must not move at all. Even filters do not rotate
    either (gyro == bg); odd ones spin about z, which leaves the third column of Rsb - the one accel_calib meets - alone"""
    rng = np.random.default_rng(seed)
    im = _imu(B, 1)
    X0 = []
    for b in range(B):
        X = dyadic_state(v=(0.0, 0.0, 0.0))
        X0.append(X)
        im["accel"][b, 0] = X.ba + np.array([0.0, 0.0, 9.75])
        im["gyro"][b, 0] = X.bg + (np.array([0.0, 0.0, 0.25 * (1 + b // 2)]) if b % 2 else 0.0)
    im["dt"][:] = np.ldexp(1.0, -8) * (1 + np.arange(B) % 5)[:, None]
    Dm = motion_scales(seed, SPREAD["rest"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("at_rest", method, 2.0 ** -9, X0, Dm, P0, im, G_DYADIC, seed)


def long_chain(method, n=LONG_CHAIN_SAMPLES, B=64, seed=600):
    """ONE call with n samples of 5 ms at stepsize 0.002 (three sub-steps a sample), gyro 1 rad/s with a slope that changes
    sign from sample to sample; the 64 filters are copies of one (the restatement of 3 n steps is what costs)"""
    rng = np.random.default_rng(seed)
    im = _imu(1, n)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    sg = rng.normal(size=3) * 5.0
    gy = ax.copy()
    for k in range(n):
        s = sg if k % 2 == 0 else -sg
        im["gyro"][0, k] = gy
        im["sg"][0, k] = s
        gy = gy + s * 0.005
    im["accel"][0] = rng.normal(size=(n, 3)) * 0.2 + np.array([0, 0, 9.8])
    im["sa"][0] = rng.normal(size=(n, 3)) * 20.0
    im["dt"][:] = 0.005
    im = {k: np.repeat(v, B, axis=0) for k, v in im.items()}
    X = random_state(rng)
    Dm = motion_scales(seed, SPREAD["chain"])
    P = prior(_N(), seed, Dm)
    return Batch("long_chain", method, 0.002, [X] * B, Dm, np.repeat(P[None], B, axis=0), im, G_NOMINAL, seed, distinct=[0] * B)


_Q = 1e-6 / 4        # 4 * _Q == 1e-6 exactly (a power-of-two scaling)
CTL_CHAINS = {
    # per max_scale_factor: chains of sample lengths (s); the first call takes the first CTL_SPLIT samples
    1.0: [(0.0041, 0.0025, 0.009, 0.0006, 0.003), (0.0031, 0.0047, 0.0021, 0.0055, 0.0012)],
    1.5: [(0.004, 0.0025, 0.009, 0.0006, 0.003), (0.002 + 2e-7, 0.005, 0.0031, 0.0042, 0.0017), (0.0031, 0.0047, 0.0021, 0.0055, 0.0012)],
    4.0: [(0.004, 0.0025, 0.009, 0.0006, 0.003),
          (_Q, 0.003, 0.0042, 0.0017, 0.005),                        # carried h == 1e-6 exactly at sample 2: no reset (:32-34)
          (np.nextafter(_Q, 0.0), 0.003, 0.0042, 0.0017, 0.005),     # one ulp under: reset to stepsize
          (0.003, 0.0042, _Q, 0.0017, 0.005),                        # the same across the two calls
          (0.009, 0.001, 0.012, 0.0005, 0.004)],                     # carried h exceeds the next dt
}
CTL_SPLIT = 3


def controlled(max_scale, seed=700):
    """step-size-controlled Dormand-Prince as coded: chains of samples of different lengths, split over two calls, per filter a
    different chain (the listed ones, then random ones to fill 8 filters)"""
    rng = np.random.default_rng(seed + int(max_scale * 10))
    chains = list(CTL_CHAINS[max_scale])
    B, n = 8, 5
    while len(chains) < B:
        chains.append(tuple(np.exp(rng.uniform(np.log(0.0005), np.log(0.012), size=n))))
    im = _random_imu(rng, B, n)
    im["dt"] = np.array(chains)
    X0 = [random_state(rng) for _ in range(B)]
    Dm = motion_scales(seed, SPREAD["ctl"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("controlled_%g" % max_scale, "PrinceDormand", 0.002, X0, Dm, P0, im, G_NOMINAL, seed, ctl=max_scale, split=CTL_SPLIT)


CALIB_BUILDS = {24: (True, False), 38: (False, True), 39: (True, True)}


def calibration(method, nm, seed=800):
    """propagate_state_calib_kernel: kMotionSize 24 / 38 / 39, four filters, two samples, Cg / Ca away from identity, td non-zero"""
    temporal, imu_cal = CALIB_BUILDS[nm]
    lay = orc.calib_layout(NG, NF, temporal, imu_cal, 0)
    assert lay.motion_size == nm
    rng = np.random.default_rng(seed + nm)
    B = 4
    im = _random_imu(rng, B, 2)
    im["dt"] = np.exp(rng.uniform(np.log(0.002), np.log(0.012), size=(B, 2)))
    X0 = [random_state(rng) for _ in range(B)]
    Cg = [np.eye(3) + 0.05 * rng.normal(size=(3, 3)) if imu_cal else np.eye(3) for _ in range(B)]
    Ca = [np.triu(np.eye(3) + 0.05 * rng.normal(size=(3, 3))) if imu_cal else np.eye(3) for _ in range(B)]
    td = [0.004 * (b + 1) for b in range(B)]
    Dm = motion_scales(seed, SPREAD["calib"], nm)
    P0 = np.array([prior(lay.N, seed + b, Dm) for b in range(B)])
    return Batch("calib_%d" % nm, method, 0.002, X0, Dm, P0, im, G_NOMINAL, seed, layout=lay, Cg=Cg, Ca=Ca, td=td)


def asymmetric(method, rel, seed=100):
    """the nominal inputs (stepsize 0.002) with the upper triangle of the motion block perturbed: rel = 0 by a few ulps, else
    by that relative amount. The routes do emit it: every measurement update writes lower + mirror, but propagation's own P_mm
    carries the rounding-level asymmetry of G Q G^T into the next sample or call, and xivo_hip_propagate_cov stores the P_mm it
    is handed as it is (xivo_hip_upload_P does not: it keeps the lower triangle and mirrors it, so the device test plants these
    priors through xivo_hip_propagate_cov)."""
    bt = nominal(method, 0.002, B=16, seed=seed)
    rng = np.random.default_rng(seed + 7)
    for b in range(bt.B):
        Pm = bt.P0[b][:23, :23]
        iu = np.triu_indices(23, 1)
        if rel == 0:
            k = rng.integers(-3, 4, size=len(iu[0]))
            Pm[iu] = Pm[iu] + k * np.spacing(Pm[iu])
        else:
            Pm[iu] = Pm[iu] * (1.0 + rel * rng.uniform(-1, 1, size=len(iu[0])))
    bt.name = "asym_%s" % ("ulps" if rel == 0 else "%g" % rel)
    return bt


# ---- exact step cases: stepsize 2^-9, every input dyadic
def _tok(h, step):
    return "F" if h == step else ("H" if h == 0.5 * step else "R")


# name -> (per sample dt / 2^-9, per sample the steps as F / H / R (fixed branch), same for the controlled branch at
#          max_scale_factor 1, which comparison of rk4.cpp:21 / :23 the case sits on: 1, 2 or 0 = none, and which of
#          princedormand.cpp:53 / :55 in the controlled branch)
EXACT_CASES = {
    "k1": ((1.0,), ("HH",), ("F",), 1, 0),
    "k2": ((2.0,), ("FHH",), None, 1, 1),
    "k3": ((3.0,), ("FFHH",), None, 1, 1),
    "k2.5": ((2.5,), ("FFH",), ("FFH",), 2, 2),
    "k1.5": ((1.5,), ("FH",), ("FH",), 2, 0),
    "k0.5": ((0.5,), ("H",), ("H",), 0, 0),
    "k1+ulp": ((1.0 + 2.0 ** -52,), ("HR",), ("FR",), 0, 0),       # dt = 2^-9 + 2^-61: the smallest remainder fp64 has there (2^-9 + 2^-62 IS 2^-9)
    "n2_k1.5_k2": ((1.5, 2.0), ("FH", "FHH"), None, 1, 0),          # the second sample on the threshold; Qmodel once per sample
    "n2_k0.5_k2.5": ((0.5, 2.5), ("H", "FFH"), None, 2, 0),         # ... also when a sample takes one step
}
STRADDLE = {
    # dt = k 2^-9 (1 -+ 1e-6): name -> (k, sign, steps)
    "k1-": (1.0, -1, "R"), "k1+": (1.0, 1, "HR"), "k2-": (2.0, -1, "FR"), "k2+": (2.0, 1, "FHR"),
    "k3-": (3.0, -1, "FFR"), "k3+": (3.0, 1, "FFHR"), "k2.5-": (2.5, -1, "FHR"), "k2.5+": (2.5, 1, "FFR"),
    "k1.5-": (1.5, -1, "HR"), "k1.5+": (1.5, 1, "FR"), "k0.5-": (0.5, -1, "R"), "k0.5+": (0.5, 1, "R"),
}


def _exact_imu(B, n):
    im = _imu(B, n)
    X = dyadic_state()
    im["gyro"][:] = X.bg + np.array([0.25, -0.3125, 0.375])
    im["accel"][:] = np.array([0.5, -0.25, 9.75])
    im["sg"][:] = np.array([4.0, -8.0, 16.0])
    im["sa"][:] = np.array([16.0, -32.0, 8.0])
    return im


def exact_steps(method, ctl=None, nm=None, seed=900):
    """the exact cases (one filter each; two-sample cases fill the second sample of the others with a plain 2^-9 * 1.25).
    nm: through propagate_state_calib_kernel, which has the step rule a second time (dyadic Cg / Ca / td)"""
    names = [k for k, v in EXACT_CASES.items() if ctl is None or len(v[0]) == 1]
    B = len(names)
    im = _exact_imu(B, 2)
    im["dt"][:] = 1.25 * H9
    expect = {}
    for b, k in enumerate(names):
        dts, fixed, ctld = EXACT_CASES[k][:3]
        for s, d in enumerate(dts):
            im["dt"][b, s] = d * H9
        if ctl is None:
            expect[b] = list(fixed) + (["HR"] if len(dts) == 1 else [])
        elif ctld is not None:
            expect[b] = list(ctld)
    if ctl is not None:
        im = {k: v[:, :1] for k, v in im.items()}
    X0 = [dyadic_state() for _ in range(B)]
    lay, kw = None, {}
    if nm is not None:
        lay = orc.calib_layout(NG, NF, *CALIB_BUILDS[nm], 0)
        imu_cal = CALIB_BUILDS[nm][1]
        Cg = np.eye(3) + (np.array([[2.0 ** -5, -2.0 ** -6, 0.0], [2.0 ** -7, -2.0 ** -5, 2.0 ** -6], [0.0, 2.0 ** -6, 2.0 ** -5]]) if imu_cal else 0.0)
        Ca = np.eye(3) + (np.array([[-2.0 ** -5, 2.0 ** -6, 2.0 ** -7], [0.0, 2.0 ** -5, -2.0 ** -6], [0.0, 0.0, 2.0 ** -6]]) if imu_cal else 0.0)
        kw = dict(layout=lay, Cg=[Cg] * B, Ca=[Ca] * B, td=[2.0 ** -8] * B)
    Dm = motion_scales(seed, SPREAD["exact"], 23 if nm is None else nm)
    P0 = np.array([prior(_N(lay), seed + b, Dm) for b in range(B)])
    name = ("exact_ctl" if ctl else "exact") + ("" if nm is None else "_calib_%d" % nm)
    return Batch(name, method, H9, X0, Dm, P0, im, G_DYADIC, seed, ctl=ctl, expect=expect, tags=dict(enumerate(names)), **kw)


def straddle(method, seed=950):
    names = list(STRADDLE)
    B = len(names)
    im = _exact_imu(B, 1)
    expect = {}
    for b, k in enumerate(names):
        kk, sgn, toks = STRADDLE[k]
        im["dt"][b, 0] = kk * H9 * (1.0 + sgn * 1e-6)
        expect[b] = [toks]
    X0 = [dyadic_state() for _ in range(B)]
    Dm = motion_scales(seed, SPREAD["exact"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("straddle", method, H9, X0, Dm, P0, im, G_DYADIC, seed, expect=expect, tags=dict(enumerate(names)))


def mixed(method, seed=1000):
    """fast-spin, no-rotation and nominal filters in one launch (one step of 0.1 s): the halving loop's trip count differs from
    lane to lane of the pre-pass and from filter to filter"""
    rng = np.random.default_rng(seed)
    B = 12
    im = _random_imu(rng, B, 1)
    X0 = [random_state(rng) for _ in range(B)]
    tags = {}
    for b in range(B):
        kind = ("fast", "norot", "nominal")[b % 3]
        tags[b] = kind
        if kind == "fast":
            ax = rng.normal(size=3)
            im["gyro"][b, 0] = X0[b].bg + ax / np.linalg.norm(ax) * rng.uniform(3.0, 15.0)
            im["sg"][b, 0] = 0.0
        elif kind == "norot":
            im["gyro"][b, 0] = X0[b].bg
            im["sg"][b, 0] = 0.0
    im["dt"][:] = 0.1
    Dm = motion_scales(seed, SPREAD["mixed"])
    P0 = np.array([prior(_N(), seed + b, Dm) for b in range(B)])
    return Batch("mixed", method, -1.0, X0, Dm, P0, im, G_NOMINAL, seed, tags=tags)


# every batch the two test files run: key -> builder
BATCHES = {}
for _m in METHODS:
    BATCHES[("nominal", _m, 0.002)] = functools.partial(nominal, _m, 0.002)
    BATCHES[("nominal", _m, -1.0)] = functools.partial(nominal, _m, -1.0)
    BATCHES[("fast_spin", _m)] = functools.partial(fast_spin, _m)
    BATCHES[("t2_threshold", _m)] = functools.partial(t2_threshold, _m)
    BATCHES[("no_rotation", _m)] = functools.partial(no_rotation, _m)
    BATCHES[("at_rest", _m)] = functools.partial(at_rest, _m)
    BATCHES[("long_chain", _m)] = functools.partial(long_chain, _m)
    BATCHES[("exact", _m)] = functools.partial(exact_steps, _m)
    BATCHES[("straddle", _m)] = functools.partial(straddle, _m)
    BATCHES[("mixed", _m)] = functools.partial(mixed, _m)
    BATCHES[("asym", _m, 0)] = functools.partial(asymmetric, _m, 0)
    BATCHES[("asym", _m, 1e-9)] = functools.partial(asymmetric, _m, 1e-9)
    for _nm in CALIB_BUILDS:
        BATCHES[("calib", _m, _nm)] = functools.partial(calibration, _m, _nm)
    BATCHES[("exact_calib", _m)] = functools.partial(exact_steps, _m, None, 39)
for _s in CTL_CHAINS:
    BATCHES[("controlled", _s)] = functools.partial(controlled, _s)
BATCHES[("exact_ctl",)] = functools.partial(exact_steps, "PrinceDormand", 1.0)
BATCHES[("exact_ctl_calib",)] = functools.partial(exact_steps, "PrinceDormand", 1.0, 24)


# ---------------------------------------------------------------- step patterns
def step_pattern(dt, stepsize, T=float, cmp1=operator.gt, cmp2=operator.gt, ctl_h=None, max_scale=None, h0=None):
    """The steps rk4.cpp:19-31 / princedormand.cpp:62-81 (ctl_h None) or princedormand.cpp:28-59 (ctl_h: the carried step) cut
    a sample into, every quantity and comparison in dtype T; cmp1 / cmp2: the two step comparisons (`>` in the reference -
    operator.ge is the flipped one). -> (steps, carried h)"""
    dt, total, steps = T(dt), T(0), []
    if ctl_h is None:
        if stepsize < 0:
            return [dt], None
        while total < dt:
            h = T(stepsize)
            if cmp1(total + h, dt):
                h = dt - total
            elif cmp2(total + h + T(0.5) * h, dt):
                h = T(0.5) * h
            steps.append(h)
            total = total + h
            assert len(steps) < 4096
        return steps, None
    h = T(ctl_h)
    if h < T(1e-6):
        h = T(h0)
    h = min(h, dt)
    while total < dt:
        steps.append(h)
        total = total + h
        h = h * T(max_scale)
        if total < dt:
            if cmp1(total + h, dt):
                h = dt - total
            elif cmp2(total + h + T(0.5) * h, dt):
                h = T(0.5) * h
        assert len(steps) < 4096
    return steps, h


def tokens(steps, stepsize):
    return "".join(_tok(float(h), stepsize) for h in steps)


# ---------------------------------------------------------------- the two references and the metrics
def _restate_state(X):
    return pr.State.from_matrices(X.Rsb, X.Tsb, X.Vsb, X.bg, X.ba, X.Rsg)


def restate(bt, b, patterns=None, P0=None, mirror=False):
    """the 80-bit restatement of filter b over its samples -> (State, P, [steps per sample]); patterns: per sample a list of
    steps to take in place of the decided ones (None: decide); mirror: the device's as-coded P0 F^T = (F P0)^T"""
    X, P = _restate_state(bt.X0[b]), (bt.P0[b] if P0 is None else P0)
    ctl = pr.PDControl(bt.stepsize, bt.ctl) if bt.ctl is not None else None
    steps = []
    for s in range(bt.n):
        X, P, st = pr.propagate(X, P, bt.imu["gyro"][b, s], bt.imu["accel"][b, s], bt.imu["sg"][b, s], bt.imu["sa"][b, s],
                                float(bt.imu["dt"][b, s]), bt.Qi, bt.Qm, bt.g, bt.method, bt.stepsize,
                                None if bt.Cg is None else bt.Cg[b], None if bt.Ca is None else bt.Ca[b], bt.layout, ctl,
                                None if patterns is None else patterns[s], mirror)
        steps.append(st)
    return X, P, steps


def oracle(bt, b):
    """the fp64 oracle on the same inputs -> (MotionState, P, [steps per sample]); the steps are read off the lengths it hands
    its integrator_step"""
    X, P = bt.X0[b].copy(), bt.P0[b]
    ctl = orc.PDControl(stepsize=bt.stepsize, max_scale_factor=bt.ctl) if bt.ctl is not None else None
    steps, seen = [], []
    inner = orc.integrator_step

    def spy(X_, P_, g0, a0, sg, sa, dt, *a, **k):
        seen.append(dt)
        return inner(X_, P_, g0, a0, sg, sa, dt, *a, **k)
    orc.integrator_step = spy
    try:
        for s in range(bt.n):
            del seen[:]
            X, P = orc.propagate(X, P, bt.imu["gyro"][b, s], bt.imu["accel"][b, s], bt.imu["sg"][b, s], bt.imu["sa"][b, s],
                                 float(bt.imu["dt"][b, s]), bt.Qi, bt.Qm, bt.g, method=bt.method, stepsize=bt.stepsize,
                                 Cg=None if bt.Cg is None else bt.Cg[b], Ca=None if bt.Ca is None else bt.Ca[b], layout=bt.layout,
                                 pd_control=ctl)
            steps.append(list(seen))
    finally:
        orc.integrator_step = inner
    return X, P, steps


def metrics(P, Rsb, Tsb, Vsb, ref_X, ref_P, d):
    """the seven metrics of one filter's result (fp64 arrays) against the restatement (ref_X, ref_P); d: the prior's sqrt(diag)"""
    Pl = np.asarray(P).astype(LD)
    E = Pl - ref_P
    dd = np.outer(d, d).astype(LD)
    R = np.asarray(Rsb).astype(LD)

    def relv(v, r):
        return float(np.max(np.abs(np.asarray(v).astype(LD) - r) / np.maximum(LD(1), np.abs(r))))
    return dict(rel=float(np.sqrt(np.sum(E * E)) / np.sqrt(np.sum(ref_P * ref_P))),
                corr=float(np.max(np.abs(E) / dd)),
                sym=float(np.max(np.abs((Pl - Pl.T) - (ref_P - ref_P.T)) / dd)),
                Rsb=float(np.max(np.abs(R - ref_X.Rsb))),
                Tsb=relv(Tsb, ref_X.Tsb), Vsb=relv(Vsb, ref_X.Vsb),
                orth=float(np.max(np.abs(R.T @ R - np.eye(3, dtype=LD)))))


def distance(Xa, Pa, Xb, Pb, d):
    """the metrics between two restatement results (what separates two step patterns)"""
    return metrics(Pa, Xa.Rsb, Xa.Tsb, Xa.Vsb, Xb, Pb, d)


class Evaluated:
    """A batch with, per distinct filter, the restatement (ref), the oracle's metrics against it and the batch's bounds"""

    def __init__(self, bt):
        self.bt = bt
        self.ref, self.orc_steps, self.orc_metrics, self.d, self.coded = {}, {}, {}, {}, {}
        for b in sorted(set(bt.distinct)):
            Xr, Pr, steps = restate(bt, b)
            Xo, Po, osteps = oracle(bt, b)
            d = np.sqrt(np.diag(bt.P0[b]))
            self.ref[b], self.orc_steps[b], self.d[b] = (Xr, Pr, steps), osteps, d
            self.orc_metrics[b] = metrics(Po, Xo.Rsb, Xo.Tsb, Xo.Vsb, Xr, Pr, d)
            if bt.name.startswith("asym"):                                   # the as-coded variant, where it differs
                self.coded[b] = restate(bt, b, mirror=True)[:2]
        self.worst = {m: max(v[m] for v in self.orc_metrics.values()) for m in P_METRICS + X_METRICS}
        self.bounds = {m: max(4.0 * self.worst[m], FLOOR) for m in self.worst}

    def check(self, b, P, Rsb, Tsb, Vsb, extra=None, coded=False):
        """assert filter b's result within the bounds (extra: metric -> an additive term) of the restatement, or with `coded` of
        its as-coded variant; returns its metrics"""
        r = self.bt.distinct[b]
        Xr, Pr = self.coded[r] if coded else self.ref[r][:2]
        got = metrics(P, Rsb, Tsb, Vsb, Xr, Pr, self.d[r])
        for m, v in got.items():
            lim = self.bounds[m] + (extra or {}).get(m, 0.0)
            assert v <= lim, (self.bt.name, self.bt.method, b, m, v, lim)
        return got


@functools.lru_cache(maxsize=None)
def evaluated(key):
    return Evaluated(BATCHES[key]())


def asym_extra(ev, b):
    """the one additive term of the asymmetric family: the restatement's own distance between filter b's result on P as given
    and on its symmetrised copy (the reference multiplies the P it was given; the device mirrors F P0)"""
    bt = ev.bt
    P = bt.P0[b]
    Xs, Ps, _ = restate(bt, b, P0=0.5 * (P + P.T))
    Xr, Pr, _ = ev.ref[b]
    return distance(Xs, Ps, Xr, Pr, ev.d[b])

