"""Estimator::Propagate of the reference, from the integrator call on (src/estimator.cpp:580-590), in np.longdouble: on x86-64
an 80-bit float with eleven more mantissa bits, which next to an fp64 result stands for the exact answer (as in
tests/precise_ref.py and tests/subfilter_restate.py).

Restated line by line, dense, as the reference codes it:
  RK4 / RK4Step                    src/rk4.cpp:5-33, :35-103
  PrinceDormand / PrinceDormandStep src/princedormand.cpp:7-83 (fixed and step-size-controlled, as coded), :85-221
  ComposeMotion                    src/estimator.cpp:598-613 with imu_.Cg() / imu_.Ca(), SO3::exp as Sophus codes it
                                   (thirdparty/sophus/sophus/so3.hpp:669-705: a quaternion, its small-angle branch under
                                   theta^2 < 1e-20, sinl / cosl above), the quaternion product of SO3::operator* (:326-351)
                                   and normalize() (:301-307)
  ComputeMotionJacobianAt          src/estimator.cpp:615-704 with the dWsb/dCg and dVsb/dCa columns (:626-638, :674-685);
                                   the td row and column of an online-calibration build are zero (no line writes them)
  the motion-structure tail        src/rk4.cpp:92-102, src/princedormand.cpp:206-215
P0 * F_.transpose() is formed from P0 as given - nothing is mirrored, no structural zero is skipped. The fixed branch carries
the running sums gyro += slope * h (rk4.cpp:28-29), the controlled branch starts each step from gyro0 + slope * total_step
(princedormand.cpp:39-40).

The step pattern - every comparison of rk4.cpp:19-26 and princedormand.cpp:32-58 - is decided in fp64, as the reference
decides it, and the steps taken are returned; only the arithmetic inside a step is in 80 bits. `pattern` overrides the
decisions with a given list of steps (what a flipped comparison would have taken).

One switch leaves the reference: mirror=True forms P0 F^T as (F P0)^T, which is what the device does on the assumption that P_mm
is symmetric (propagate_kernels.hip). On a symmetric P_mm the two agree to 80-bit rounding; on an asymmetric one they do not, and
the asymmetric family of tests/propagate_edge_cases.py pins the device to this variant."""
import numpy as np

LD = np.longdouble
WSB, TSB, VSB, BG, BA, WBC, TBC, WSG = 0, 3, 6, 9, 12, 15, 18, 21
K_MOTION = 23


def _ld(a):
    return np.array(a, dtype=LD)


class State:
    """The part of `State` (src/core.h:117-180) that Propagate touches. Rsb is a Sophus SO3: a unit quaternion (w, x, y, z)."""

    def __init__(self, q, Tsb, Vsb, bg, ba, Rsg):
        self.q, self.Tsb, self.Vsb, self.bg, self.ba, self.Rsg = _ld(q), _ld(Tsb), _ld(Vsb), _ld(bg), _ld(ba), _ld(Rsg)

    @classmethod
    def from_matrices(cls, Rsb, Tsb, Vsb, bg, ba, Rsg):
        return cls(quat_of(_ld(Rsb)), Tsb, Vsb, bg, ba, Rsg)

    def copy(self):
        return State(self.q, self.Tsb, self.Vsb, self.bg, self.ba, self.Rsg)

    @property
    def Rsb(self):
        return rot_of(self.q)


def quat_of(R):
    """unit quaternion of a rotation matrix (Shepperd's branches), normalised"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    two, q4 = LD(2), LD(0.25)
    if t > 0:
        s = np.sqrt(t + LD(1)) * two
        q = [q4 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(LD(1) + R[0, 0] - R[1, 1] - R[2, 2]) * two
        q = [(R[2, 1] - R[1, 2]) / s, q4 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(LD(1) + R[1, 1] - R[0, 0] - R[2, 2]) * two
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, q4 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(LD(1) + R[2, 2] - R[0, 0] - R[1, 1]) * two
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, q4 * s]
    q = _ld(q)
    return q / np.sqrt(q @ q)


def rot_of(q):
    """Eigen's Quaternion::toRotationMatrix (what SO3::matrix() returns, so3.hpp:314-316)"""
    w, x, y, z = q
    two = LD(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = LD(1)
    return _ld([[one - (tyy + tzz), txy - twz, txz + twy],
                [txy + twz, one - (txx + tzz), tyz - twx],
                [txz - twy, tyz + twx, one - (txx + tyy)]])


def hat(w):
    z = LD(0)
    return _ld([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]])


def so3_exp_quat(omega):
    """SO3::expAndTheta (so3.hpp:669-705) -> (quaternion, small-angle branch taken)"""
    theta_sq = omega @ omega
    small = bool(theta_sq < LD(1e-10) * LD(1e-10))
    if small:
        theta_po4 = theta_sq * theta_sq
        imag = LD(0.5) - LD(1.0 / 48.0) * theta_sq + LD(1.0 / 3840.0) * theta_po4
        real = LD(1) - LD(1.0 / 8.0) * theta_sq + LD(1.0 / 384.0) * theta_po4
    else:
        theta = np.sqrt(theta_sq)
        half = LD(0.5) * theta
        imag = np.sin(half) / theta
        real = np.cos(half)
    return _ld([real, imag * omega[0], imag * omega[1], imag * omega[2]]), small


def quat_mul(a, b):
    """SO3Base::QuaternionProduct (so3.hpp:326-335)"""
    return _ld([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


class Model:
    """What a step reads besides the state: slopes, noise, gravity, imu_.Cg() / imu_.Ca() and the build's layout"""

    def __init__(self, slope_gyro, slope_accel, Qimu, g_vec, Cg=None, Ca=None, layout=None, mirror=False):
        self.slope = np.concatenate([_ld(slope_gyro), _ld(slope_accel)])
        self.Qimu, self.g = _ld(Qimu), _ld(g_vec)
        self.Cg = np.eye(3, dtype=LD) if Cg is None else _ld(Cg)
        self.Ca = np.eye(3, dtype=LD) if Ca is None else _ld(Ca)
        self.layout = layout
        self.mirror = mirror
        self.nm = K_MOTION if layout is None else layout.motion_size


def compose_motion(X, V, gyro_accel, dt, md):
    """Estimator::ComposeMotion (estimator.cpp:598-613), in place"""
    gyro, accel = gyro_accel[:3], gyro_accel[3:]
    gyro_calib = md.Cg @ gyro - X.bg                                         # :604
    accel_calib = md.Ca @ accel - X.ba                                       # :605
    X.Tsb = X.Tsb + V * dt                                                   # :608
    X.Vsb = X.Vsb + (X.Rsb @ accel_calib + X.Rsg @ md.g) * dt                # :609
    e, _ = so3_exp_quat(gyro_calib * dt)
    X.q = quat_mul(X.q, e)                                                   # :610
    X.q = X.q / np.sqrt(X.q @ X.q)                                           # :612 normalize()


def motion_jacobian(X, gyro_accel, md):
    """Estimator::ComputeMotionJacobianAt (estimator.cpp:615-704) -> (F_, G_), dense"""
    nm, lay = md.nm, md.layout
    gyro, accel = gyro_accel[:3], gyro_accel[3:]
    gyro_calib = md.Cg @ gyro - X.bg                                         # :621
    accel_calib = md.Ca @ accel - X.ba                                       # :622
    Rsb = X.Rsb                                                              # :625
    dWsb_dWsb = -hat(gyro_calib)                                             # :639
    dV_dWsb = -Rsb @ hat(accel_calib)                                        # :644
    dV_dba = -Rsb                                                            # :645
    dV_dWsg = -Rsb @ hat(md.g)                                               # :647
    F = np.zeros((nm, nm), dtype=LD)                                         # :650
    G = np.zeros((nm, 12), dtype=LD)                                         # :693
    for j in range(3):                                                       # :652-672
        F[WSB + j, BG + j] = -1
        F[TSB + j, VSB + j] = 1
        for i in range(3):
            F[WSB + i, WSB + j] = dWsb_dWsb[i, j]
            F[VSB + i, WSB + j] = dV_dWsb[i, j]
            F[VSB + i, BA + j] = dV_dba[i, j]
            if j < 2:
                F[VSB + i, WSG + j] = dV_dWsg[i, j]
    if lay is not None and lay.Cg >= 0:                                      # USE_ONLINE_IMU_CALIB
        dWsb_dCg = np.zeros((3, 9), dtype=LD)                                # :627-632: the RAW gyro sample
        for i in range(3):
            dWsb_dCg[i, 3 * i:3 * i + 3] = gyro
        # :634-637 dV_dCa = dAB_dA<3,3>(accel) * dAB_dB<3,3>(Rsb) * dA_dAu<3>() (common/rodrigues.h:143-165, :208-227, :26-37)
        dV_dRCa = np.zeros((3, 9), dtype=LD)
        for n in range(3):
            for m in range(3):
                dV_dRCa[n, n * 3 + m] += accel[m]
        dRCa_dCafm = np.zeros((9, 9), dtype=LD)
        for n in range(3):
            for p in range(3):
                for m in range(3):
                    dRCa_dCafm[p * 3 + n, m * 3 + p] = Rsb[n, m]
        dCafm_dCa = np.zeros((9, 6), dtype=LD)
        idx = 0
        for i in range(3):
            for j in range(i, 3):
                dCafm_dCa[i * 3 + j, idx] = 1
                idx += 1
        dV_dCa = dV_dRCa @ dRCa_dCafm @ dCafm_dCa
        F[WSB:WSB + 3, lay.Cg:lay.Cg + 9] = dWsb_dCg                         # :675-679
        F[VSB:VSB + 3, lay.Ca:lay.Ca + 6] = dV_dCa                           # :680-684
    for j in range(3):                                                       # :694-703
        G[WSB + j, j] = -1
        G[BG + j, 6 + j] = 1
        G[BA + j, 9 + j] = 1
        for i in range(3):
            G[VSB + i, 3 + j] = -Rsb[i, j]
    return F, G


def _pk(F, G, P0, md):
    if md.mirror:                                                            # the device, as coded: P0 F^T taken as (F P0)^T
        FP = F @ P0
        return FP + FP.T + G @ md.Qimu @ G.T
    return F @ P0 + P0 @ F.T + G @ md.Qimu @ G.T                             # rk4.cpp:55, princedormand.cpp:111


def _finish(X, P, K, FK, PK, ga0, dt, md):
    """the end of both steps (rk4.cpp:88-102, princedormand.cpp:202-215): the state, then P"""
    nm = md.nm
    compose_motion(X, K, ga0 + md.slope * dt, dt, md)
    F = np.eye(nm, dtype=LD) + FK * dt
    P = P.copy()
    P[:nm, :nm] = P[:nm, :nm] + PK * dt
    P[:nm, nm:] = F @ P[:nm, nm:]
    P[nm:, :nm] = P[nm:, :nm] @ F.T
    return X, P


def rk4_step(X, P, ga0, dt, md):
    """Estimator::RK4Step (rk4.cpp:35-103); X is replaced, P returned"""
    nm = md.nm
    dt = LD(dt)
    half = LD(0.5) * dt
    Pmm = P[:nm, :nm]
    X0 = X.copy()
    K1 = X0.Vsb
    F, G = motion_jacobian(X0, ga0, md)
    FK1 = F
    PK1 = _pk(F, G, Pmm.copy(), md)

    X0 = X.copy()
    ga = ga0 + half * md.slope
    compose_motion(X0, LD(0.5) * K1, ga, half, md)
    K2 = X0.Vsb
    F, G = motion_jacobian(X0, ga, md)
    FK2 = F + F @ FK1 * half
    PK2 = _pk(F, G, Pmm + half * PK1, md)

    X0 = X.copy()
    compose_motion(X0, LD(0.5) * K2, ga, half, md)
    K3 = X0.Vsb
    F, G = motion_jacobian(X0, ga, md)
    FK3 = F + F @ FK2 * half
    PK3 = _pk(F, G, Pmm + half * PK2, md)

    X0 = X.copy()
    compose_motion(X0, K3, ga, dt, md)                                       # :76-77: the half-step sample again
    K4 = X0.Vsb
    F, G = motion_jacobian(X0, ga, md)
    FK4 = F + F @ FK3 * dt
    PK4 = _pk(F, G, Pmm + dt * PK3, md)

    six, two = LD(6), LD(2)
    K = (K1 + two * (K2 + K3) + K4) / six
    FK = (FK1 + two * (FK2 + FK3) + FK4) / six
    PK = (PK1 + two * (PK2 + PK3) + PK4) / six
    return _finish(X, P, K, FK, PK, ga0, dt, md)


# princedormand.cpp:87-93 (the reference's constants are doubles) and the stages :113-192: (step / dt, r, [(weight, stage)])
_R9, _R29, _R12, _R324, _R330, _R28, _R400 = 1.0 / 9.0, 2.0 / 9.0, 1.0 / 12.0, 1.0 / 324.0, 1.0 / 330.0, 1.0 / 28.0, 1.0 / 400.0
_PD_STAGES = (
    (_R29, _R29, ((1.0, 0),)),
    (3.0 * _R9, _R12, ((1.0, 0), (3.0, 1))),
    (5.0 * _R9, _R324, ((55.0, 0), (-75.0, 1), (200.0, 2))),
    (6.0 * _R9, _R330, ((83.0, 0), (-195.0, 1), (305.0, 2), (27.0, 3))),
    (1.0, _R28, ((-19.0, 0), (63.0, 1), (4.0, 2), (-108.0, 3), (88.0, 4))),
    (1.0, _R400, ((38.0, 0), (240.0, 2), (-243.0, 3), (330.0, 4), (35.0, 5))),
)
_PD_B = ((0.0862, 0), (0.6660, 2), (-0.7857, 3), (0.9570, 4), (0.0965, 5), (-0.0200, 6))   # :195-200


def _comb(ws, Ms):
    out = LD(ws[0][0]) * Ms[ws[0][1]]
    for w, q in ws[1:]:
        out = out + LD(w) * Ms[q]
    return out


def prince_dormand_step(X, P, ga0, dt, md):
    """Estimator::PrinceDormandStep (princedormand.cpp:85-221); returns 0 in the reference (:216-220)"""
    nm = md.nm
    dt = LD(dt)
    Pmm = P[:nm, :nm]
    X0 = X.copy()
    Ks = [X0.Vsb]
    F, G = motion_jacobian(X0, ga0, md)
    FKs = [F]
    PKs = [_pk(F, G, Pmm.copy(), md)]
    for c, r, ws in _PD_STAGES:
        X0 = X.copy()
        step = LD(c) * dt
        ga = ga0 + md.slope * step
        compose_motion(X0, LD(r) * _comb(ws, Ks), ga, step, md)
        F, G = motion_jacobian(X0, ga, md)
        Ks.append(X0.Vsb)
        FKs.append(F + F @ (LD(r) * _comb(ws, FKs)) * dt)
        PKs.append(_pk(F, G, Pmm + LD(r) * _comb(ws, PKs) * dt, md))
    return _finish(X, P, _comb(_PD_B, Ks), _comb(_PD_B, FKs), _comb(_PD_B, PKs), ga0, dt, md)


class PDControl:
    """cfg_["PrinceDormand"] of the controlled branch and the function-local static h it carries (princedormand.cpp:12-26)"""

    def __init__(self, stepsize=0.002, max_scale_factor=4.0):
        self.h0 = float(stepsize)
        self.h = float(stepsize)
        self.max_scale_factor = float(max_scale_factor)


def integrate(X, P, gyro0, accel0, dt, md, method="RK4", stepsize=0.002, ctl=None, pattern=None):
    """Estimator::RK4 (rk4.cpp:5-33) / Estimator::PrinceDormand (princedormand.cpp:28-82) -> (X, P, steps taken).
    dt, stepsize, the carried h and every comparison are fp64."""
    step = rk4_step if method == "RK4" else prince_dormand_step
    dt = float(dt)
    ga0 = np.concatenate([_ld(gyro0), _ld(accel0)])
    steps = []
    if pattern is not None:
        # a given list of steps in place of the decisions; the sample of each step as the branch in force forms it
        ga, total = ga0.copy(), 0.0
        for h in pattern:
            X, P = step(X, P, ga0 + md.slope * LD(total) if ctl is not None else ga, h, md)
            ga = ga + md.slope * LD(h)
            total += h
            steps.append(h)
        return X, P, steps
    if ctl is not None:                                                      # princedormand.cpp:28-59
        assert method != "RK4"
        total = 0.0
        h = ctl.h
        if h < 1e-6:                                                         # :32-34
            h = ctl.h0
        h = min(h, dt)                                                       # :36
        while total < dt:                                                    # :38
            X, P = step(X, P, ga0 + md.slope * LD(total), h, md)             # :39-40
            steps.append(h)
            total += h                                                       # :41
            h *= ctl.max_scale_factor                                        # :42-43, :51 (err == 0, :220)
            if total < dt:                                                   # :52-58
                if total + h > dt:
                    h = dt - total
                elif total + h + 0.5 * h > dt:
                    h = 0.5 * h
        ctl.h = h
        return X, P, steps
    if stepsize < 0:                                                         # rk4.cpp:13-14, princedormand.cpp:62-63
        X, P = step(X, P, ga0, dt, md)
        return X, P, [dt]
    total = 0.0
    ga = ga0.copy()
    while total < dt:                                                        # rk4.cpp:19-31, princedormand.cpp:68-80
        h = float(stepsize)
        if total + h > dt:
            h = dt - total
        elif total + h + 0.5 * h > dt:
            h = 0.5 * h
        X, P = step(X, P, ga, h, md)
        ga = ga + md.slope * LD(h)
        total += h
        steps.append(h)
    return X, P, steps


def propagate(X, P, gyro0, accel0, slope_gyro, slope_accel, dt, Qimu, Qmodel, g_vec, method="RK4", stepsize=0.002,
              Cg=None, Ca=None, layout=None, ctl=None, pattern=None, mirror=False):
    """Estimator::Propagate from the integrator call on (estimator.cpp:580-590): one IMU sample. X: State (replaced), P: the
    full covariance. -> (X, P, steps)"""
    md = Model(slope_gyro, slope_accel, Qimu, g_vec, Cg, Ca, layout, mirror)
    X, P, steps = integrate(X.copy(), _ld(P), gyro0, accel0, dt, md, method, stepsize, ctl, pattern)
    P[:md.nm, :md.nm] = P[:md.nm, :md.nm] + _ld(Qmodel)                      # :590
    return X, P, steps
