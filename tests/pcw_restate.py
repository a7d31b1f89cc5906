"""Shared by tests/test_pcw_tracks_cpu.py and tests/test_pcw_tracks_gpu.py (not a test module): the numpy restatement of the
device track producer (xivo_amd/csrc/pcw_device.h) frame by frame, and the worlds and camera motions the tests run it on.

The restatement projects with pcw.project_points - explicit elementwise operations in the header's evaluation order - and
hands out ids as BatchPCW.generate does. Every step asserts the border condition the comparisons rest on: no point within 1e-9
of the camera plane and no pixel within 1e-9 px of an image border, so that a last-place difference cannot flip a decision."""
import numpy as np

from xivo_amd import pcw

CAM = dict(fx=275.0, fy=275.0, cx=320.0, cy=240.0, imw=640.0, imh=480.0)
K = np.array([[CAM["fx"], 0, CAM["cx"]], [0, CAM["fy"], CAM["cy"]], [0, 0, 1.0]])
BIG = (1 << 33) + 5


def gsc_of(Rsc, Tsc):
    return np.concatenate([np.asarray(Rsc).reshape(-1, 9), np.asarray(Tsc).reshape(-1, 3)], axis=1)


class Restate:
    def __init__(self, Xs, ids=None, next_id=None):
        self.Xs = np.asarray(Xs, dtype=float)
        B, npts, _ = self.Xs.shape
        self.ids = np.full((B, npts), -1, dtype=np.int64) if ids is None else np.array(ids, dtype=np.int64)
        self.next_id = np.full(B, 10000, dtype=np.int64) if next_id is None else np.array(next_id, dtype=np.int64)

    def step(self, gsc, noise_px_std=0.0, seed=0, frame=0):
        """-> dict(vis, u, v, z [B, npts] noise-free, ids, next_id after the frame, cnt [B], off [B + 1], track_ids [n],
        meas [n, 3] with noise, front)"""
        gsc = np.asarray(gsc, dtype=float)
        B, npts = self.ids.shape
        Rsc, Tsc = gsc[:, :9].reshape(B, 3, 3), gsc[:, 9:]
        vis, u, v, z = pcw.project_points(self.Xs, Rsc, Tsc, K, CAM["imw"], CAM["imh"])
        # the border condition (a precondition of every comparison, not a measurement)
        assert np.abs(z).min() >= 1e-9, "a point within 1e-9 of the camera plane"
        for x, hi in ((u, CAM["imw"]), (v, CAM["imh"])):
            assert min(np.abs(x).min(), np.abs(x - hi).min()) >= 1e-9, "a pixel within 1e-9 px of an image border"
        new = vis & (self.ids < 0)
        rank = np.cumsum(new, axis=1) - 1
        self.ids = np.where(new, self.next_id[:, None] + rank, self.ids)
        self.next_id = self.next_id + new.sum(axis=1)
        self.ids = np.where(vis, self.ids, -1)
        noise = np.zeros(u.shape + (2,))
        if noise_px_std != 0.0:
            noise = noise_px_std * pcw.philox_normal(seed, frame, np.arange(B)[:, None], np.arange(npts)[None, :])
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum(vis.sum(axis=1))
        sel = np.nonzero(vis)
        meas = np.stack([u[sel] + noise[sel][:, 0], v[sel] + noise[sel][:, 1], z[sel]], axis=1)
        return dict(vis=vis, front=z > 0, u=u, v=v, z=z, ids=self.ids.copy(), next_id=self.next_id.copy(),
                    cnt=vis.sum(axis=1).astype(np.int32), off=off, track_ids=self.ids[sel].copy(), meas=np.ascontiguousarray(meas))


def strided(r, tracks_max):
    """a step's tracks in the layout of xivo_hip_pcw_get_tracks: (cnt [B], ids [B, tracks_max], meas [B, tracks_max, 3])"""
    B = len(r["cnt"])
    ids, meas = np.full((B, tracks_max), -1, dtype=np.int64), np.zeros((B, tracks_max, 3))
    for b in range(B):
        n = r["cnt"][b]
        ids[b, :n] = r["track_ids"][r["off"][b]:r["off"][b + 1]]
        meas[b, :n] = r["meas"][r["off"][b]:r["off"][b + 1]]
    return r["cnt"], ids, meas


def moving_poses(B, T, seed):
    """T frames of B cameras that look along +z of the world, pan and drift a little -> gsc [T, B, 12]"""
    rng = np.random.default_rng(seed)
    w0, dw = rng.normal(size=(B, 3)) * 0.05, rng.normal(size=(B, 3)) * 0.04
    p0, dp = rng.normal(size=(B, 3)) * 0.3, rng.normal(size=(B, 3)) * 0.15
    out = np.zeros((T, B, 12))
    for t in range(T):
        for b in range(B):
            out[t, b] = gsc_of(pcw.so3_exp(w0[b] + t * dw[b]), p0[b] + t * dp[b])[0]
    return out


def box_world(B, npts, seed):
    return np.random.default_rng(seed).uniform([-10, -10, -5], [10, 10, 5], size=(B, npts, 3))


def edge_case_worlds(npts, seed):
    """Three worlds and four frames that hold the cases of the scan: -> (Xs [3, npts, 3], next_id [3], gsc [4, 3, 12])
      filter 0  a box world whose point 0 sits near the left image border of a camera that pans away and back: visible, gone,
                visible again - with a new id; its ids start at 2^33 + 5
      filter 1  a cone in front of a camera that barely moves: every point visible in every frame
      filter 2  the same cone: frame 0 behind the camera, frame 1 in front but far outside the image, frame 2 all visible, frame 3
                behind again"""
    rng = np.random.default_rng(seed)
    Xs = np.zeros((3, npts, 3))
    Xs[0] = rng.uniform([-10, -10, 1], [10, 10, 9], size=(npts, 3))
    Xs[0, 0] = [-1.1 * 4.0, 0.1, 4.0]                         # u = 320 - 302.5 at the identity pose
    z = rng.uniform(3.0, 6.0, size=(2, npts))
    for b in (1, 2):
        Xs[b] = np.stack([rng.uniform(-0.5, 0.5, npts) * z[b - 1], rng.uniform(-0.4, 0.4, npts) * z[b - 1], z[b - 1]], axis=1)
    gsc = np.zeros((4, 3, 12))
    turn = pcw.so3_exp(np.array([0.0, np.pi, 0.0]))
    for t in range(4):
        gsc[t, 0] = gsc_of(pcw.so3_exp(np.array([0.0, 0.3 * (t % 2), 0.0])), [0.001 * t, 0.0, 0.0])[0]
        gsc[t, 1] = gsc_of(pcw.so3_exp(np.array([0.01 * t, -0.02 * t, 0.005])), [0.02 * t, -0.01 * t, 0.03 * t])[0]
    gsc[0, 2] = gsc_of(turn, [0.0, 0.0, 0.0])[0]
    gsc[1, 2] = gsc_of(np.eye(3), [100.0, 0.0, 0.0])[0]
    gsc[2, 2] = gsc_of(np.eye(3), [0.01, 0.02, 0.0])[0]
    gsc[3, 2] = gsc_of(turn, [0.0, 0.0, -20.0])[0]
    return Xs, np.array([BIG, 10000, 10000], dtype=np.int64), gsc


def assert_edge_cases(steps):
    """the four frames of edge_case_worlds, restated, hold what they were built for"""
    v0 = [s["vis"][0, 0] for s in steps]
    assert v0 == [True, False, True, False], v0                                   # leaves and returns ...
    assert steps[2]["ids"][0, 0] > steps[0]["ids"][0, 0] >= BIG                   # ... with a new id, above 2^33
    assert all(s["vis"][1].all() for s in steps)                                  # every point visible
    assert not steps[0]["front"][2].any() and not steps[3]["front"][2].any()      # every point behind the camera
    assert steps[1]["front"][2].all() and not steps[1]["vis"][2].any()            # in front, none visible
    assert steps[2]["vis"][2].all()
