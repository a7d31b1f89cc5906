"""numpy restatement of xivo_amd/csrc/trajsim_device.h in the header's evaluation order: one IMU sample of one filter, vectorised
over filters (axis 0) and samples (axis 1). Elementwise only - no einsum / @, whose summation order is not fixed. What the
CPU tests hold the header under g++ against and the GPU tests hold the kernel against; sin / cos / log are numpy's (glibc's).

The bounds (both test files use them): the restatement and the code under test run the same operations in the same order on
the same inputs, so they differ only where sin / cos / log / (sqrt, /: correctly rounded on both sides) differ. OpenCL's
bound for the device library is 4 ulp for sin and cos and 3 for log, glibc's own error is below 1: two evaluations of one
transcendental differ by at most 5 ulp of its value. An output is a sum of products of at most three such values (curve:
c2 c3; rotation: the profile's sines, then sin th / th, (1 - cos th) / th^2 whose cancellation is paid for in units of the
identity's 1, times W2 <= th^2), so with the roundings that follow it stays within ULPS = 64 ulp of the LARGEST INTERMEDIATE of
that output - `scale` below, the sum of the absolute values of the terms the output is added up from. A slope divides the
difference of two such values by dt: its bound is the two measurements' bounds over dt. Times, dt, and the generator's words
and uniforms involve no transcendental and are exact."""
import numpy as np

from xivo_amd import lib as L
from xivo_amd import pcw

ULPS = 64
EPS = 2.0 ** -52
NORMAL_MAX = 8.6     # |normal| <= sqrt(106 ln 2) (philox_device.h)
MOTIONS = {"lissajous": 0, "trefoil": 1}


class Model:
    def __init__(self, imu_dt=0.0025, rot_amp=0.2, rot_w=(0.3 * 3.0, 0.4 * 3.0, 0.1 * 3.0), noise_accel=1e-4, noise_gyro=1e-5,
                 grav_s=(0, 0, -9.8), Rbc=None, Tbc=(0, 0, 0), seed=1):
        self.imu_dt, self.rot_amp = float(imu_dt), float(rot_amp)
        self.rot_w = np.array([0.3, 0.4, 0.1]) * 3.0 if rot_w is None else np.asarray(rot_w, dtype=float)
        self.noise_accel, self.noise_gyro = float(noise_accel), float(noise_gyro)
        self.grav_s = np.asarray(grav_s, dtype=float)
        self.Rbc = np.eye(3) if Rbc is None else np.asarray(Rbc, dtype=float)
        self.Tbc = np.asarray(Tbc, dtype=float)
        self.seed = int(seed)

    def config_kw(self):
        """the keyword arguments of Context.trajsim_config"""
        return dict(imu_dt=self.imu_dt, rot_amp=self.rot_amp, rot_w=self.rot_w, noise_accel=self.noise_accel,
                    noise_gyro=self.noise_gyro, grav_s=self.grav_s, Rbc=self.Rbc, Tbc=self.Tbc, seed=self.seed)

    def packed(self):
        """the doubles of TrajsimModel in order, then the seed (tests/trajsim_driver.cpp reads this)"""
        return (np.concatenate([[self.imu_dt, self.rot_amp], self.rot_w, [self.noise_accel, self.noise_gyro], self.grav_s,
                                self.Rbc.reshape(-1), self.Tbc]).astype(np.float64), np.uint64(self.seed))


def times(k, imu_dt):
    return np.asarray(k, dtype=np.uint64).astype(np.float64) * imu_dt


def dt_of(k, imu_dt):
    k = np.asarray(k, dtype=np.uint64)
    return times(k, imu_dt) - times(k - np.uint64(1), imu_dt)


def profile(m, t):
    """t [...] -> R [..., 3, 3], Jr [..., 3, 3], wd [..., 3], th"""
    t = np.asarray(t, dtype=float)
    a = [m.rot_w[i] * t for i in range(3)]
    w = [m.rot_amp * np.sin(a[i]) for i in range(3)]
    wd = [m.rot_amp * m.rot_w[i] * np.cos(a[i]) for i in range(3)]
    xx, yy, zz, xy, xz, yz = w[0] * w[0], w[1] * w[1], w[2] * w[2], w[0] * w[1], w[0] * w[2], w[1] * w[2]
    th = np.sqrt(xx + yy + zz)
    z = np.zeros_like(t)
    W = [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]
    W2 = [-(yy + zz), xy, xz, xy, -(xx + zz), yz, xz, yz, -(xx + yy)]
    tiny, small = th < 1e-9, th < 1e-6
    with np.errstate(invalid="ignore", divide="ignore"):
        ths = np.where(tiny, 1.0, th)
        a_ = np.where(tiny, 1.0, np.sin(ths) / ths)
        b_ = np.where(tiny, 0.5, (1.0 - np.cos(ths)) / (ths * ths))
        thj = np.where(small, 1.0, th)
        c_ = np.where(small, 0.5, (1.0 - np.cos(thj)) / (thj * thj))
        e_ = (thj - np.sin(thj)) / (thj * thj * thj)
    R, Jr = [], []
    for i in range(9):
        eye = 1.0 if i in (0, 4, 8) else 0.0
        R.append(eye + a_ * W[i] + b_ * W2[i])
        Jr.append(eye - c_ * W[i] + np.where(small, W2[i] / 6.0, e_ * W2[i]))
    sh = t.shape
    return (np.stack(R, -1).reshape(sh + (3, 3)), np.stack(Jr, -1).reshape(sh + (3, 3)), np.stack(wd, -1), th)


def curve(motion, s):
    """motion, s broadcast -> p [..., 3], acc [..., 3]"""
    motion, s = np.broadcast_arrays(np.asarray(motion), np.asarray(s, dtype=float))
    c2, s2, c3, s3, s7 = np.cos(2 * s), np.sin(2 * s), np.cos(3 * s), np.sin(3 * s), np.sin(7 * s)
    pl = [4 * c3, 0.1 * s7, 4 * s2]
    al = [-36 * c3, -4.9 * s7, -16 * s2]
    pt = [(4 + c3) * c2, (4 + c3) * s2, s3]
    at = [12 * s2 * s3 - 9 * c2 * c3 - 4 * c2 * (c3 + 4), -4 * s2 * (c3 + 4) - 12 * c2 * s3 - 9 * c3 * s2, -9 * s3]
    tre = motion == 1
    return (np.stack([np.where(tre, pt[i], pl[i]) for i in range(3)], -1), np.stack([np.where(tre, at[i], al[i]) for i in range(3)], -1))


def normals(m, k, B):
    """k [n] -> n_a [B, n, 3], n_g [B, n, 3] (zeros for a sensor whose std is 0: nothing is drawn)"""
    k = np.asarray(k, dtype=np.uint64)
    out = np.zeros((B, k.shape[0], 6))
    if m.noise_accel != 0.0 or m.noise_gyro != 0.0:
        for i, kk in enumerate(k):
            out[:, i] = pcw.trajsim_normals(m.seed, int(kk), np.arange(B))
    n_a, n_g = out[..., :3].copy(), out[..., 3:].copy()
    if m.noise_accel == 0.0:
        n_a[:] = 0.0
    if m.noise_gyro == 0.0:
        n_g[:] = 0.0
    return n_a, n_g


def meas(m, motion, rate, k):
    """motion [B], rate [B], k [n] -> accel [B, n, 3], gyro [B, n, 3] and the bounds' scales of both (same shapes)"""
    motion, rate = np.asarray(motion), np.asarray(rate, dtype=float)
    B = rate.shape[0]
    t = times(k, m.imu_dt)[None, :]                                    # [1, n]
    R, Jr, wd, _ = profile(m, t)                                       # [1, n, ...]
    _, acc = curve(motion[:, None], rate[:, None] * t)                 # [B, n, 3]
    r2 = (rate * rate)[:, None]
    d = [r2 * acc[..., j] - m.grav_s[j] for j in range(3)]
    accel = np.stack([R[..., 0, i] * d[0] + R[..., 1, i] * d[1] + R[..., 2, i] * d[2] for i in range(3)], -1)
    gyro = np.stack([Jr[..., i, 0] * wd[..., 0] + Jr[..., i, 1] * wd[..., 1] + Jr[..., i, 2] * wd[..., 2] for i in range(3)], -1)
    gyro = np.broadcast_to(gyro, accel.shape).copy()
    # the largest intermediates: every |term| of d (36 rate^2 bounds the curves' second derivatives term by term: 12 + 9 + 20)
    # through a rotation whose entries are at most 1, and |wd| through Jr, whose entries are at most 1 + th / 2 + th^2 / 6 < 2
    sa = (41.0 * r2 + np.abs(m.grav_s).sum())[..., None] * np.ones(3) + m.noise_accel * NORMAL_MAX
    sg = 2.0 * np.abs(m.rot_amp * m.rot_w).sum() * np.ones(accel.shape) + m.noise_gyro * NORMAL_MAX
    sa = np.broadcast_to(sa, accel.shape).copy()
    n_a, n_g = normals(m, k, B)
    if m.noise_accel != 0.0:
        accel = accel + m.noise_accel * n_a
    if m.noise_gyro != 0.0:
        gyro = gyro + m.noise_gyro * n_g
    return accel, gyro, sa, sg


def records(m, motion, rate, k0, n):
    """records k0 + 1 .. k0 + n -> (recs [B, n] imu_dtype, bound [B, n] imu_dtype: the absolute bound of every field; dt's is 0)"""
    k = np.uint64(k0) + np.arange(n + 1, dtype=np.uint64)
    accel, gyro, sa, sg = meas(m, motion, rate, k)
    dt = dt_of(k[1:], m.imu_dt)[None, :, None]
    B = accel.shape[0]
    recs, bound = np.zeros((B, n), dtype=L.imu_dtype), np.zeros((B, n), dtype=L.imu_dtype)
    recs["gyro"], recs["accel"] = gyro[:, :-1], accel[:, :-1]
    recs["slope_gyro"], recs["slope_accel"] = (gyro[:, 1:] - gyro[:, :-1]) / dt, (accel[:, 1:] - accel[:, :-1]) / dt
    recs["dt"] = dt[..., 0]
    bound["gyro"], bound["accel"] = ULPS * EPS * sg[:, :-1], ULPS * EPS * sa[:, :-1]
    bound["slope_gyro"], bound["slope_accel"] = ULPS * EPS * (sg[:, 1:] + sg[:, :-1]) / dt, ULPS * EPS * (sa[:, 1:] + sa[:, :-1]) / dt
    return recs, bound


def truth(m, motion, rate, k):
    """the poses at sample k (scalar) -> gt [B, 12] (Rsb column-major, Tsb), gsc [B, 12] (Rsc row-major, Tsc) and their bounds"""
    motion, rate = np.asarray(motion), np.asarray(rate, dtype=float)
    B = rate.shape[0]
    t = times(k, m.imu_dt)
    R, _, _, _ = profile(m, t)                                          # [3, 3]
    p, _ = curve(motion, rate * t)
    p0, _ = curve(motion, rate * 0.0)
    T = p - p0
    gt, gsc = np.zeros((B, 12)), np.zeros((B, 12))
    for i in range(3):
        for j in range(3):
            gt[:, 3 * j + i] = R[i, j]
            gsc[:, 3 * i + j] = R[i, 0] * m.Rbc[0, j] + R[i, 1] * m.Rbc[1, j] + R[i, 2] * m.Rbc[2, j]
        gt[:, 9 + i] = T[:, i]
        gsc[:, 9 + i] = R[i, 0] * m.Tbc[0] + R[i, 1] * m.Tbc[1] + R[i, 2] * m.Tbc[2] + T[:, i]
    # largest intermediates: 1 for a rotation entry, |p| + |p0| <= 5 + 5 for Tsb, the column sums of |Rbc| and |Tbc| on top
    bgt = ULPS * EPS * np.concatenate([np.ones(9), np.full(3, 10.0)])
    bgsc = ULPS * EPS * np.concatenate([np.tile(np.abs(m.Rbc).sum(axis=0), 3), np.full(3, 10.0 + np.abs(m.Tbc).sum())])
    return gt, gsc, np.broadcast_to(bgt, gt.shape), np.broadcast_to(bgsc, gsc.shape)


def worst(got, want, bound, fields=("gyro", "accel", "slope_gyro", "slope_accel")):
    """largest |got - want| / bound over the fields that have a bound (1.0 = at the bound)"""
    r = 0.0
    for f in fields:
        d = np.abs(got[f] - want[f]) / bound[f]
        r = max(r, float(d.max())) if d.size else r
    return r
