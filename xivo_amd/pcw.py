"""Image-free sequence source: a point-cloud world seen by a moving camera + a simulated IMU.

Restates what the reference's simulation scripts feed `Estimator::InertialMeas` / `VisualMeasPointCloud`:
  * `RandomPCW` follows scripts/point_cloud_world.py:44-131 (uniform points in a box, pinhole visibility test, pixel
    noise, track ids that start at 10000 - `counter0` of src/feature.h - are handed out when a point becomes visible
    and dropped when it leaves the image, so a point that comes back is a NEW track, as for `Tracker::UpdatePointCloud`,
    src/tracker.cpp:632-702);
  * `TrajectorySim` plays the role of scripts/imu_sim.py:IMUSimBase with the curves of scripts/imu_trajectories.py
    (LissajousSim :289-313, TrefoilSim :316-341), but in closed form: position, velocity and acceleration are the
    analytic curve and its derivatives, orientation is exp(hat(w(t))) with the body rate from the right Jacobian, so no
    ODE solve / interpolation table is needed and ground truth is exact at any t.
The accelerometer model is the one the filter integrates (src/estimator.cpp:598-613: Vsb' = Rsb (accel - ba) + Rsg g):
accel = Rsb^T (a_s - g_s) + ba + noise, gyro = w_b + bg + noise.

Host-side numpy only; nothing here touches the GPU or the oracle.
"""
import numpy as np


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_exp(w):
    th = float(np.linalg.norm(w))
    W = _hat(w)
    if th < 1e-9:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / (th * th) * W @ W


def so3_log(R):
    c = max(-1.0, min(1.0, (np.trace(R) - 1.0) * 0.5))
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-9:
        return 0.5 * v
    return th / (2.0 * np.sin(th)) * v


def _right_jacobian(w):
    th = float(np.linalg.norm(w))
    W = _hat(w)
    if th < 1e-6:
        return np.eye(3) - 0.5 * W + W @ W / 6.0
    return np.eye(3) - (1.0 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W


class RandomPCW:
    """scripts/point_cloud_world.py RandomPCW: `npts` points uniform in xlim x ylim x zlim."""

    def __init__(self, npts=1000, xlim=(-10, 10), ylim=(-10, 10), zlim=(-5, 5), seed=0):
        self.rng = np.random.default_rng(seed)
        lo = np.array([xlim[0], ylim[0], zlim[0]], dtype=float)
        hi = np.array([xlim[1], ylim[1], zlim[1]], dtype=float)
        self.Xs = self.rng.uniform(lo, hi, size=(npts, 3))
        self.ids = np.full(npts, -1, dtype=np.int64)
        self.next_pt_id = 10000
        self.last_point_index = np.zeros(0, dtype=np.int64)   # world-point index of every track the last call returned

    def generate_measurements(self, Rsc, Tsc, K, imw, imh, noise_px_std):
        """-> (feature_ids [n], xp_and_depths [n x 3]) of the points inside the image, ascending point order
        (point_cloud_world.py:64-99). Noise is drawn for every point in front of the camera, visible or not, as the
        reference does, so that the stream does not depend on who is visible. last_point_index keeps the world-point index of
        every returned track, parallel to the ids: a point that leaves and returns gets a new id and keeps its index (a loop
        closure key, xivo_hip_lcmap_*)."""
        Xc = (self.Xs - Tsc) @ Rsc          # rows: Rsc^T (Xs - Tsc)
        front = Xc[:, 2] > 0
        z = np.where(front, Xc[:, 2], 1.0)
        u = K[0, 0] * Xc[:, 0] / z + K[0, 2]
        v = K[1, 1] * Xc[:, 1] / z + K[1, 2]
        vis = front & (u >= 0) & (v >= 0) & (u <= imw) & (v <= imh)
        noise = noise_px_std * self.rng.standard_normal((self.Xs.shape[0], 2))
        new = vis & (self.ids < 0)
        n_new = int(new.sum())
        self.ids[new] = self.next_pt_id + np.arange(n_new)
        self.next_pt_id += n_new
        self.ids[~vis] = -1
        sel = np.nonzero(vis)[0]
        out = np.stack([u[sel] + noise[sel, 0], v[sel] + noise[sel, 1], Xc[sel, 2]], axis=1)
        self.last_point_index = sel.astype(np.int64)
        return self.ids[sel].copy(), out


_CURVES = {
    # p(s), p'(s), p''(s); s = rate * t
    "lissajous": (lambda s: np.array([4 * np.cos(3 * s), 0.1 * np.sin(7 * s), 4 * np.sin(2 * s)]),
                  lambda s: np.array([-12 * np.sin(3 * s), 0.7 * np.cos(7 * s), 8 * np.cos(2 * s)]),
                  lambda s: np.array([-36 * np.cos(3 * s), -4.9 * np.sin(7 * s), -16 * np.sin(2 * s)])),
    "trefoil": (lambda s: np.array([(4 + np.cos(3 * s)) * np.cos(2 * s), (4 + np.cos(3 * s)) * np.sin(2 * s), np.sin(3 * s)]),
                lambda s: np.array([-3 * np.sin(3 * s) * np.cos(2 * s) - 2 * (4 + np.cos(3 * s)) * np.sin(2 * s),
                                    -3 * np.sin(3 * s) * np.sin(2 * s) + 2 * (4 + np.cos(3 * s)) * np.cos(2 * s),
                                    3 * np.cos(3 * s)]),
                lambda s: np.array([12 * np.sin(2 * s) * np.sin(3 * s) - 9 * np.cos(2 * s) * np.cos(3 * s)
                                    - 4 * np.cos(2 * s) * (np.cos(3 * s) + 4),
                                    -4 * np.sin(2 * s) * (np.cos(3 * s) + 4) - 12 * np.cos(2 * s) * np.sin(3 * s)
                                    - 9 * np.cos(3 * s) * np.sin(2 * s),
                                    -9 * np.sin(3 * s)])),
}


class TrajectorySim:
    """Ground truth + IMU samples along an analytic curve (see the module docstring).

    `rate` slows the reference curves down (their accelerations reach 36 m/s^2 at rate 1); the position is shifted
    so that Tsb(0) = 0, and Rsb(0) = I, like the reference sims (imu_sim.py:226-228)."""

    def __init__(self, motion_type="lissajous", rate=0.1, rot_amp=0.2, noise_accel=1e-4, noise_gyro=1e-5,
                 bias_accel=(0, 0, 0), bias_gyro=(0, 0, 0), grav_s=(0, 0, -9.8), seed=1):
        self.p, self.dp, self.ddp = _CURVES[motion_type]
        self.rate = float(rate)
        self.p0 = self.p(0.0)
        self.rot_amp = float(rot_amp)
        self.rot_w = np.array([0.3, 0.4, 0.1]) * 3.0   # rad/s of the three rotation-vector components
        self.noise_accel, self.noise_gyro = noise_accel, noise_gyro
        self.bias_accel = np.asarray(bias_accel, dtype=float)
        self.bias_gyro = np.asarray(bias_gyro, dtype=float)
        self.grav_s = np.asarray(grav_s, dtype=float)
        self.rng = np.random.default_rng(seed)

    def _w(self, t):
        return self.rot_amp * np.sin(self.rot_w * t), self.rot_amp * self.rot_w * np.cos(self.rot_w * t)

    def gsb(self, t):
        w, _ = self._w(t)
        return so3_exp(w), self.p(self.rate * t) - self.p0

    def vel(self, t):
        return self.rate * self.dp(self.rate * t)

    def real_accel_gyro(self, t):
        w, wd = self._w(t)
        Rsb = so3_exp(w)
        a_s = self.rate ** 2 * self.ddp(self.rate * t)
        return Rsb.T @ a_s, _right_jacobian(w) @ wd

    def meas(self, t):
        """-> (accel, gyro) as an IMU at time t would report them."""
        Rsb, _ = self.gsb(t)
        a_b, w_b = self.real_accel_gyro(t)
        accel = a_b - Rsb.T @ self.grav_s + self.bias_accel + self.noise_accel * self.rng.standard_normal(3)
        gyro = w_b + self.bias_gyro + self.noise_gyro * self.rng.standard_normal(3)
        return accel, gyro


# ---- the same two simulators for B sequences at once (numpy over the sequence axis): what feeds thousands of
# ---- filters per frame; formulas identical to RandomPCW / TrajectorySim above (tests compare them)
def so3_exp_batch(w):
    """w: [B, 3] -> [B, 3, 3]"""
    th = np.linalg.norm(w, axis=1)
    W = np.zeros((w.shape[0], 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    small = th < 1e-9
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(ths) / ths)
    b = np.where(small, 0.5, (1.0 - np.cos(ths)) / (ths * ths))
    return np.eye(3)[None] + a[:, None, None] * W + b[:, None, None] * (W @ W), W, th


class BatchTrajectorySim:
    """B trajectories: motion[b] in {"lissajous", "trefoil"}, rate[b]; one noise stream for all.
    noise: "numpy" (default) draws the IMU noise from the simulator's numpy generator; "philox" draws the stream of the device
    producer (trajsim_normals, keyed by noise_seed, the sample index k handed to meas() and the sequence), so that a host arm
    can be held against a device arm. The arithmetic is the same either way."""

    def __init__(self, motion, rate, rot_amp=0.2, noise_accel=1e-4, noise_gyro=1e-5, grav_s=(0, 0, -9.8), seed=1, noise="numpy",
                 noise_seed=0):
        if noise not in ("numpy", "philox"):
            raise ValueError("noise must be 'numpy' or 'philox'")
        self.noise, self.noise_seed = noise, int(noise_seed)
        self.is_tre = np.array([m == "trefoil" for m in motion])
        self.rate = np.asarray(rate, dtype=float)
        self.B = len(self.rate)
        self.rot_amp = float(rot_amp)
        self.rot_w = np.array([0.3, 0.4, 0.1]) * 3.0
        self.noise_accel, self.noise_gyro = noise_accel, noise_gyro
        self.grav_s = np.asarray(grav_s, dtype=float)
        self.rng = np.random.default_rng(seed)
        self.p0 = self._curve(np.zeros(self.B))[0]

    def _curve(self, s):
        c2, s2, c3, s3, c7, s7 = np.cos(2 * s), np.sin(2 * s), np.cos(3 * s), np.sin(3 * s), np.cos(7 * s), np.sin(7 * s)
        pl = np.stack([4 * c3, 0.1 * s7, 4 * s2], 1)
        dl = np.stack([-12 * s3, 0.7 * c7, 8 * c2], 1)
        al = np.stack([-36 * c3, -4.9 * s7, -16 * s2], 1)
        pt = np.stack([(4 + c3) * c2, (4 + c3) * s2, s3], 1)
        dt = np.stack([-3 * s3 * c2 - 2 * (4 + c3) * s2, -3 * s3 * s2 + 2 * (4 + c3) * c2, 3 * c3], 1)
        at = np.stack([12 * s2 * s3 - 9 * c2 * c3 - 4 * c2 * (c3 + 4), -4 * s2 * (c3 + 4) - 12 * c2 * s3 - 9 * c3 * s2, -9 * s3], 1)
        m = self.is_tre[:, None]
        return np.where(m, pt, pl), np.where(m, dt, dl), np.where(m, at, al)

    def gsb(self, t):
        w = np.tile(self.rot_amp * np.sin(self.rot_w * t), (self.B, 1))
        R, _, _ = so3_exp_batch(w)
        return R, self._curve(self.rate * t)[0] - self.p0

    def vel(self, t):
        return self.rate[:, None] * self._curve(self.rate * t)[1]

    def meas(self, t, k=None):
        """-> (accel [B, 3], gyro [B, 3]); k: the sample's index (noise="philox" needs it: the generator's counter)"""
        w = np.tile(self.rot_amp * np.sin(self.rot_w * t), (self.B, 1))
        wd = self.rot_amp * self.rot_w * np.cos(self.rot_w * t)
        R, W, th = so3_exp_batch(w)
        a_s = (self.rate ** 2)[:, None] * self._curve(self.rate * t)[2]
        Jr = _right_jacobian(w[0])                       # the orientation profile is shared by all sequences
        if self.noise == "philox":
            if k is None:
                raise ValueError("noise='philox' needs the sample index k")
            n6 = trajsim_normals(self.noise_seed, k, np.arange(self.B))
            n_a, n_g = n6[:, :3], n6[:, 3:]
        else:
            n_a, n_g = self.rng.standard_normal((self.B, 3)), self.rng.standard_normal((self.B, 3))
        accel = np.einsum("bji,bj->bi", R, a_s - self.grav_s) + self.noise_accel * n_a
        gyro = (Jr @ wd)[None] + self.noise_gyro * n_g
        return accel, gyro


# ---- the device producer's noise stream on the host (xivo_amd/csrc/pcw_device.h is the specification)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr [..., 4], key [..., 2] (uint32, broadcast against each other) -> words [..., 4] uint32"""
    ctr, key = np.asarray(ctr, dtype=np.uint32), np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).copy() for i in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape).copy(), np.broadcast_to(key[..., 1], shape).copy()
    for r in range(10):
        if r > 0:
            with np.errstate(over="ignore"):               # uint32: meant to wrap
                k0, k1 = k0 + _PHILOX_W0, k1 + _PHILOX_W1
        p0, p1 = _PHILOX_M0 * c[0].astype(np.uint64), _PHILOX_M1 * c[2].astype(np.uint64)
        c = [(p1 >> np.uint64(32)).astype(np.uint32) ^ c[1] ^ k0, (p1 & _LO32).astype(np.uint32),
             (p0 >> np.uint64(32)).astype(np.uint32) ^ c[3] ^ k1, (p0 & _LO32).astype(np.uint32)]
    return np.stack(c, axis=-1)


def philox_words(seed, frame, b, p):
    """the generator's four words of point p of filter b in that frame: key = the halves of seed, counter = (point, filter,
    frame low, frame high); b and p broadcast -> [..., 4] uint32"""
    b, p = np.broadcast_arrays(np.asarray(b, dtype=np.uint32), np.asarray(p, dtype=np.uint32))
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    ctr = np.stack([p, b, np.full(p.shape, frame & 0xFFFFFFFF, dtype=np.uint32), np.full(p.shape, frame >> 32, dtype=np.uint32)], axis=-1)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


def philox_normal(seed, frame, b, p):
    """the pair of unit normals (noise_u, noise_v) the device producer draws for point p of filter b in that frame -> [..., 2].
    Words to uniforms: u1 = ((w0 << 20 | w1 >> 12) + 0.5) 2^-52, u2 the same of (w2, w3); one Box-Muller pair. The words are
    the device's exactly; log / sin / cos are numpy's, so a value may differ from the device's in the last places."""
    w = philox_words(seed, frame, b, p).astype(np.uint64)
    u1 = (((w[..., 0] << np.uint64(20)) | (w[..., 1] >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (((w[..., 2] << np.uint64(20)) | (w[..., 3] >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
    r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1)


def trajsim_normals(seed, k, b):
    """the six unit normals (accel x y z, gyro x y z) the device trajectory producer draws for IMU sample k of filter b
    (xivo_amd/csrc/trajsim_device.h): the same generator with counter = (pair j, filter, k low, k high), pair 0 = accel x y,
    pair 1 = accel z, gyro x, pair 2 = gyro y z -> [..., 6]. With the same seed these are the words of philox_normal for
    point j, filter b, frame k: give the IMU and the pixel noise different seeds."""
    b = np.asarray(b)
    return philox_normal(seed, k, b[..., None], np.arange(3)).reshape(b.shape + (6,))


# ---- the device producer's track faults on the host (xivo_amd/csrc/pcw_device.h "Track faults" is the specification)
FAULT_NOMINAL, FAULT_DROP, FAULT_OUTLIER, FAULT_TAIL = 0, 1, 2, 3        # the event of draw A
FLAG_OUTLIER, FLAG_TAIL, FLAG_BIASED = 1, 2, 4                            # a track's flag byte; faulty: flag & 5
FAULT_COUNTERS = ("tracks", "dropped", "outlier_events", "tail_events", "biased")
_FAULT_DEFAULTS = dict(sticky=0, p_drop=0.0, p_outlier=0.0, p_tail=0.0, outlier_min_px=0.0, outlier_max_px=0.0, tail_scale=1.0)


def fault_opts(faults=None, **kw):
    """the fields of xivo_pcw_fault_opts as a dict, defaults filled in (no event, scale 1); refuses what
    xivo_hip_pcw_fault_config refuses"""
    o = dict(_FAULT_DEFAULTS)
    o.update(faults or {})
    o.update(kw)
    if set(o) != set(_FAULT_DEFAULTS):
        raise ValueError("unknown fault option(s) %s" % sorted(set(o) - set(_FAULT_DEFAULTS)))
    if o["sticky"] not in (0, 1, False, True):
        raise ValueError("sticky must be 0 or 1")
    o["sticky"] = int(o["sticky"])
    for k in _FAULT_DEFAULTS:
        if k != "sticky":
            o[k] = float(o[k])
            if not np.isfinite(o[k]):
                raise ValueError("%s is not finite" % k)
    if any(not 0.0 <= o[k] <= 1.0 for k in ("p_drop", "p_outlier", "p_tail")) or (o["p_drop"] + o["p_outlier"]) + o["p_tail"] > 1.0:
        raise ValueError("p_drop, p_outlier, p_tail must lie in [0, 1] and sum to at most 1")
    if o["outlier_min_px"] < 0.0 or o["outlier_min_px"] > o["outlier_max_px"]:
        raise ValueError("0 <= outlier_min_px <= outlier_max_px")
    if o["tail_scale"] < 1.0:
        raise ValueError("tail_scale >= 1")
    return o


def _philox_uniform(hi, lo):
    hi, lo = hi.astype(np.uint64), lo.astype(np.uint64)
    return (((hi << np.uint64(20)) | (lo >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52


def fault_words(seed, frame, b, p, draw):
    """the four words of draw "A" (word 0 of the counter: p | 0x80000000) or "B" (p | 0x40000000) of point p, filter word b"""
    tag = {"A": 0x80000000, "B": 0x40000000}[draw]
    return philox_words(seed, frame, b, np.asarray(p, dtype=np.uint32) | np.uint32(tag))


def fault_draw(seed, frame, b, p, opts):
    """what the device producer draws for point p of filter (word) b in that frame, b and p broadcast ->
    dict(event [...] (FAULT_*), off [..., 2] the outlier offset (meaningful on an outlier event), tail [...] bool).
    Integer words, 52-bit uniforms and one multiply-add without contraction: the device's values bit for bit."""
    o = fault_opts(opts)
    t1 = o["p_drop"]; t2 = t1 + o["p_outlier"]; t3 = t2 + o["p_tail"]
    wa, wb = fault_words(seed, frame, b, p, "A"), fault_words(seed, frame, b, p, "B")
    e = _philox_uniform(wa[..., 0], wa[..., 1])
    event = np.where(e < t1, FAULT_DROP, np.where(e < t2, FAULT_OUTLIER, np.where(e < t3, FAULT_TAIL, FAULT_NOMINAL)))
    span = o["outlier_max_px"] - o["outlier_min_px"]
    a_u = o["outlier_min_px"] + span * _philox_uniform(wb[..., 0], wb[..., 1])
    a_v = o["outlier_min_px"] + span * _philox_uniform(wb[..., 2], wb[..., 3])
    off = np.stack([np.where(wa[..., 2] & np.uint32(1), -a_u, a_u), np.where(wa[..., 2] & np.uint32(2), -a_v, a_v)], axis=-1)
    return dict(event=event, off=off, tail=event == FAULT_TAIL)


def fault_cell(mask, flag):
    """the score's rule (pcw_fault_cell): 0 outlier_rejected, 1 outlier_kept, 2 nominal_rejected, 3 nominal_kept"""
    return (0 if flag & (FLAG_OUTLIER | FLAG_BIASED) else 2) + (0 if not mask else 1)


def project_points(Xs, Rsc, Tsc, K, imw, imh):
    """the projection and the visibility test in the evaluation order of pcw_device.h, elementwise (no einsum: its summation
    order is not fixed): Xs [B, npts, 3], Rsc [B, 3, 3], Tsc [B, 3] -> (vis [B, npts] bool, u, v, Xc_2 [B, npts])"""
    d = [Xs[..., i] - Tsc[:, None, i] for i in range(3)]
    Xc = [(Rsc[:, None, 0, i] * d[0] + Rsc[:, None, 1, i] * d[1]) + Rsc[:, None, 2, i] * d[2] for i in range(3)]
    front = Xc[2] > 0
    z = np.where(front, Xc[2], 1.0)
    u = K[0, 0] * Xc[0] / z + K[0, 2]
    v = K[1, 1] * Xc[1] / z + K[1, 2]
    return front & (u >= 0) & (v >= 0) & (u <= imw) & (v <= imh), u, v, Xc[2]


CAM_PINHOLE, CAM_ATAN, CAM_RADTAN, CAM_EQUI = 0, 1, 2, 3      # XIVO_CAM_* of include/xivo_hip.h
# one simulated 640 x 480 camera per model around the default pinhole (d: atan w; radtan p1, p2, k1, k2, k3; equidistant
# k0 .. k3). None of the three folds back inside the image; scripts/run_pcw.py -cam-model and the tests take them from here
SIM_CAMERAS = {
    "pinhole": dict(model=CAM_PINHOLE, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[]),
    "atan": dict(model=CAM_ATAN, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[0.95]),
    "radtan": dict(model=CAM_RADTAN, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[1e-3, -5e-4, -0.28, 0.07, 0.0]),
    "equi": dict(model=CAM_EQUI, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[0.01, -0.005, 0.002, -0.001]),
}


def camera_project(cam, x, y):
    """normalised camera coordinates -> pixel (u, v) through the camera dict `cam` (model, fx, fy, cx, cy, d), elementwise in
    the statement order of camera_project of xivo_amd/csrc/camera_device.h; works in the dtype of x / y (float64, or
    np.longdouble for a more precise restatement)"""
    x, y = np.asarray(x), np.asarray(y)
    T = np.result_type(x.dtype, y.dtype).type
    fx, fy, cx, cy = (T(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    d = [T(v) for v in cam.get("d", [])] + [T(0)] * 5
    model = cam["model"]
    if model == CAM_PINHOLE:
        return fx * x + cx, fy * y + cy
    if model == CAM_EQUI:
        k0, k1, k2, k3 = d[:4]
        th = np.arctan2(np.sqrt(x * x + y * y), T(1))
        phi = np.arctan2(y, x)
        th2 = th * th; th3 = th2 * th; th5 = th3 * th2; th7 = th5 * th2; th9 = th7 * th2
        r = th + k0 * th3 + k1 * th5 + k2 * th7 + k3 * th9
        return fx * r * np.cos(phi) + cx, fy * r * np.sin(phi) + cy
    if model == CAM_RADTAN:
        p1, p2, k1, k2, k3 = d[:5]
        t2, t3 = x * x, y * y
        t6, t7 = p1 * x * T(2), p2 * y * T(2)
        t8, t9 = t2 * T(3), t3 * T(3)
        t10, t11, t12, t13, t14 = t6 * y, t7 * x, t2 + t3, t3 + t8, t2 + t9
        t15, t16, t17 = t12 * t12, t12 * t12 * t12, k1 * t12
        t18, t19, t20, t21 = k2 * t15, k3 * t16, p1 * t14, p2 * t13
        t28 = t17 + t18 + t19 + T(1)
        t29, t30 = t28 * x, t28 * y
        return cx + fx * (t10 + t21 + t29), cy + fy * (t11 + t20 + t30)
    if model != CAM_ATAN:
        raise ValueError("camera model %r" % (model,))
    w = d[0]
    invw, w2 = T(1) / w if w != 0 else T(np.inf), T(2) * np.tan(w * T(0.5))
    R = np.sqrt(x * x + y * y)
    singular = (R < T(0.0001)) | (w == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(singular, T(1), invw * np.arctan(w2 * R) / np.where(singular, T(1), R))
    return fx * f * x + cx, fy * f * y + cy


def project_points_cam(Xs, Rsc, Tsc, cam, max_radius=np.inf):
    """project_points through one of the estimator's camera models, in the evaluation order pcw_device.h states for
    xivo_hip_pcw_camera: cam a camera dict (the image is cols x rows), a point whose normalised radius hypot(x, y) exceeds
    max_radius is not visible -> (vis [B, npts] bool, u, v, Xc_2 [B, npts])"""
    d = [Xs[..., i] - Tsc[:, None, i] for i in range(3)]
    Xc = [(Rsc[:, None, 0, i] * d[0] + Rsc[:, None, 1, i] * d[1]) + Rsc[:, None, 2, i] * d[2] for i in range(3)]
    front = Xc[2] > 0
    z = np.where(front, Xc[2], Xc[2].dtype.type(1))
    x, y = Xc[0] / z, Xc[1] / z
    radius = np.hypot(x, y)
    if cam["model"] == CAM_PINHOLE:
        T = Xc[2].dtype.type
        u = T(cam["fx"]) * Xc[0] / z + T(cam["cx"])
        v = T(cam["fy"]) * Xc[1] / z + T(cam["cy"])
    else:
        u, v = camera_project(cam, x, y)
    vis = front & (radius <= max_radius) & (u >= 0) & (v >= 0) & (u <= cam.get("cols", 640)) & (v <= cam.get("rows", 480))
    return vis, u, v, Xc[2]


class BatchPCW:
    """B point-cloud worlds with RandomPCW's track-id semantics; generate() returns the concatenated track lists in the
    layout xivo::hip::BatchEstimator::VisualMeasPointCloud takes (offsets, ids, (x, y, depth) rows).
    noise: "numpy" (default) draws the pixel noise from the world's numpy generator; "philox" draws the stream of the device
    producer (philox_normal, keyed by noise_seed and the number of generate() calls so far as the frame) and projects in its
    evaluation order (project_points), so that a host arm can be held against a device arm.
    faults (a dict of xivo_pcw_fault_opts' fields; needs noise="philox"): the device producer's track faults, restated - loss,
    outliers (with the sticky bias state in self.bias), heavy tails; generate() then leaves the tracks' flag bytes in
    last_fault_flags and adds to fault_stats, the producer's five counters per world. stream_mod (philox too): world b draws the
    words of filter b % stream_mod (xivo_hip_pcw_stream_share)."""

    def __init__(self, B, npts=1000, xlim=(-10, 10), ylim=(-10, 10), zlim=(-5, 5), seed=0, Xs=None, noise="numpy", noise_seed=0,
                 faults=None, stream_mod=0):
        if noise not in ("numpy", "philox"):
            raise ValueError("noise must be 'numpy' or 'philox'")
        if noise != "philox" and (faults is not None or stream_mod):
            raise ValueError("faults and stream_mod need noise='philox': they are draws of the device producer's generator")
        if int(stream_mod) < 0:
            raise ValueError("stream_mod >= 0")
        self.faults, self.stream_mod = (None if faults is None else fault_opts(faults)), int(stream_mod)
        self.noise, self.noise_seed, self.frame = noise, int(noise_seed), 0
        self.rng = np.random.default_rng(seed)
        lo = np.array([xlim[0], ylim[0], zlim[0]], dtype=float); hi = np.array([xlim[1], ylim[1], zlim[1]], dtype=float)
        self.Xs = self.rng.uniform(lo, hi, size=(B, npts, 3)) if Xs is None else np.asarray(Xs, dtype=float)
        self.ids = np.full(self.Xs.shape[:2], -1, dtype=np.int64)
        self.next_pt_id = np.full(self.Xs.shape[0], 10000, dtype=np.int64)
        self.last_point_index = np.zeros(0, dtype=np.int64)   # world-point index of every track the last generate() returned
        self.last_fault_flags = np.zeros(0, dtype=np.uint8)   # and its flag byte (faults)
        self.bias = np.zeros(self.Xs.shape[:2] + (2,))        # the sticky outliers' offsets (faults with sticky = 1)
        self.fault_stats = {k: np.zeros(self.Xs.shape[0], dtype=np.int64) for k in FAULT_COUNTERS}

    def generate(self, Rsc, Tsc, K, imw, imh, noise_px_std, cam=None, max_radius=np.inf):
        """cam (a camera dict, any model) and max_radius: project through it as the device producer does after
        xivo_hip_pcw_camera (project_points_cam; K, imw, imh are then not read); None: the pinhole K. last_point_index keeps the
        index of every returned track's point inside its world, parallel to the ids (the same for a point that returns under a
        new id: a loop closure key)"""
        if self.noise == "philox" or cam is not None:
            if cam is not None:
                vis, u, v, zc = project_points_cam(self.Xs, Rsc, Tsc, cam, max_radius)
            else:
                vis, u, v, zc = project_points(self.Xs, Rsc, Tsc, K, imw, imh)
            Xc = np.stack([u, v, zc], axis=-1)                                # (only [..., 2] is read below)
            B, npts = u.shape
            if self.noise == "philox":
                bw = np.arange(B) % self.stream_mod if self.stream_mod else np.arange(B)
                std = noise_px_std
                if self.faults is not None:
                    vis, off, std = self._faults(vis, bw, npts, noise_px_std)   # from here on vis is vis_eff
                    u, v = u + off[..., 0], v + off[..., 1]                      # the sum with the offset first
                    std = std[..., None]
                noise = std * philox_normal(self.noise_seed, self.frame, bw[:, None], np.arange(npts)[None, :])
                self.frame += 1
            else:
                noise = noise_px_std * self.rng.standard_normal(u.shape + (2,))
        else:
            Xc = np.einsum("bpj,bji->bpi", self.Xs - Tsc[:, None, :], Rsc)   # Rsc^T (Xs - Tsc)
            front = Xc[..., 2] > 0
            z = np.where(front, Xc[..., 2], 1.0)
            u = K[0, 0] * Xc[..., 0] / z + K[0, 2]
            v = K[1, 1] * Xc[..., 1] / z + K[1, 2]
            vis = front & (u >= 0) & (v >= 0) & (u <= imw) & (v <= imh)
            noise = noise_px_std * self.rng.standard_normal(u.shape + (2,))
        new = vis & (self.ids < 0)
        rank = np.cumsum(new, axis=1) - 1                                     # order of appearance inside a world
        self.ids = np.where(new, self.next_pt_id[:, None] + rank, self.ids)
        self.next_pt_id = self.next_pt_id + new.sum(axis=1)
        self.ids = np.where(vis, self.ids, -1)
        off = np.zeros(self.Xs.shape[0] + 1, dtype=np.int32)
        off[1:] = np.cumsum(vis.sum(axis=1))
        sel = np.nonzero(vis)                                                 # row-major: sequences in order, points ascending
        meas = np.stack([u[sel] + noise[sel][:, 0], v[sel] + noise[sel][:, 1], Xc[..., 2][sel]], axis=1)
        self.last_point_index = sel[1].astype(np.int64)
        self.last_fault_flags = self._flags[sel] if self.faults is not None else np.zeros(len(sel[0]), dtype=np.uint8)
        return off, self.ids[sel].copy(), np.ascontiguousarray(meas)

    def _faults(self, vis, bw, npts, noise_px_std):
        """steps 2 - 4 and 6 of pcw_device.h "Track faults" for every point: geometric vis -> (vis_eff, offset [B, npts, 2],
        noise std [B, npts]); leaves the flag bytes in self._flags, updates self.bias and self.fault_stats"""
        o = self.faults
        d = fault_draw(self.noise_seed, self.frame, bw[:, None], np.arange(npts)[None, :], o)
        ev = np.where(vis, d["event"], FAULT_NOMINAL)
        dropped = ev == FAULT_DROP
        vis_eff = vis & ~dropped
        outl, tail = ev == FAULT_OUTLIER, ev == FAULT_TAIL
        if o["sticky"]:
            carried = vis_eff & ~outl & (self.bias != 0.0).any(axis=-1)
            self.bias = np.where(outl[..., None], d["off"], self.bias)
            self.bias = np.where(vis_eff[..., None], self.bias, 0.0)
            off = self.bias
        else:
            carried = np.zeros_like(vis)
            off = np.where(outl[..., None], d["off"], 0.0)
        self._flags = (outl * FLAG_OUTLIER + tail * FLAG_TAIL + carried * FLAG_BIASED).astype(np.uint8)
        for k, m in zip(FAULT_COUNTERS, (vis_eff, dropped, outl, tail, carried)):
            self.fault_stats[k] += m.sum(axis=1)
        return vis_eff, off, noise_px_std * np.where(tail, o["tail_scale"], 1.0)
