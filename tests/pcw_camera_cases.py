"""Inputs, restatements and the host build shared by tests/test_pcw_camera_cpu.py and tests/test_pcw_camera_gpu.py: the worlds and
poses of the camera-model tests, pcw.project_points_cam in fp64 (the restatement of the evaluation order) and in np.longdouble
(on x86-64 an 80-bit float with eleven more mantissa bits: next to an fp64 result the exact answer, as in tests/precise_ref.py),
the walk of the ids, and tests/pcw_camera_driver.cpp built with g++ against xivo_amd/csrc/pcw_device.h.

The pixel bound is not a constant. host_error measures, on the inputs of the test at hand, the largest |du|, |dv| of the g++
build against the 80-bit restatement; the bound of a test is four times that (a device's atan2 / sin / cos / tan may be a few
ulp worse than libm's) and must itself stay below CAP = 1e-9 px."""
import os
import shutil
import subprocess

import numpy as np

import pcw_restate as R
from xivo_amd import pcw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
LD = np.longdouble
B, NPTS, T = 3, 257, 3
MODELS = ("atan", "radtan", "equi")
# the guard: inside the image's corners (normalised radius about 1.45 for the pinhole of the same intrinsics), so it removes points
MAX_RADIUS = {"pinhole": 1.3, "atan": 1.3, "radtan": 1.2, "equi": 1.3}
CAP = 1e-9
# a radial distortion that folds back: r (1 - 0.3 r^2) falls from r = 1.054 on and is 0 at r = 1.826
FOLD_CAM = dict(model=pcw.CAM_RADTAN, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0, d=[0.0, 0.0, -0.3, 0.0, 0.0])


def case(model, seed=None):
    """-> dict(cam, max_radius, Xs [B, NPTS, 3], gsc [T, B, 12]): box worlds seen by cameras that pan and drift"""
    seed = {"pinhole": 10, "atan": 11, "radtan": 12, "equi": 13}[model] if seed is None else seed
    return dict(cam=pcw.SIM_CAMERAS[model], max_radius=MAX_RADIUS[model], Xs=R.box_world(B, NPTS, seed),
                gsc=R.moving_poses(B, T, seed))


def project(c, t, dtype=float, max_radius=None):
    """frame t of a case through pcw.project_points_cam in dtype -> (vis, u, v, z) [B, NPTS]"""
    g = c["gsc"][t].astype(dtype)
    return pcw.project_points_cam(c["Xs"].astype(dtype), g[:, :9].reshape(-1, 3, 3), g[:, 9:], c["cam"],
                                  c["max_radius"] if max_radius is None else max_radius)


def assert_margins(c):
    """the precondition of every comparison of decisions: in the 80-bit restatement no point lies within 1e-9 of the camera
    plane, no noise-free pixel within 1e-6 px of an image border and no normalised radius within 1e-9 of max_radius"""
    cam = c["cam"]
    for t in range(c["gsc"].shape[0]):
        g = c["gsc"][t].astype(LD)
        Xs, Rsc, Tsc = c["Xs"].astype(LD), g[:, :9].reshape(-1, 3, 3), g[:, 9:]
        _, u, v, z = pcw.project_points_cam(Xs, Rsc, Tsc, cam, c["max_radius"])
        assert np.abs(z).min() > 1e-9, "a point within 1e-9 of the camera plane"
        front = z > 0
        for x, hi in ((u, cam["cols"]), (v, cam["rows"])):
            assert min(np.abs(x[front]).min(), np.abs(x[front] - hi).min()) > 1e-6, "a pixel within 1e-6 px of an image border"
        d = [Xs[..., i] - Tsc[:, None, i] for i in range(3)]
        Xc = [(Rsc[:, None, 0, i] * d[0] + Rsc[:, None, 1, i] * d[1]) + Rsc[:, None, 2, i] * d[2] for i in range(2)]
        radius = np.hypot(Xc[0][front] / z[front], Xc[1][front] / z[front])
        assert np.abs(radius - c["max_radius"]).min() > 1e-9, "a radius within 1e-9 of max_radius"


class Walk:
    """the ids of a case's worlds frame after frame (the rules of pcw_device.h, as tests/pcw_restate.py walks them), on the
    fp64 restatement of the projection"""

    def __init__(self, c):
        self.c = c
        self.ids = np.full((B, NPTS), -1, dtype=np.int64)
        self.next_id = np.full(B, 10000, dtype=np.int64)

    def step(self, t, tracks_max, max_radius=None):
        """-> dict(vis, u, v, z, ids, next_id, cnt, track_ids [B, tracks_max] (-1 behind cnt), meas [B, tracks_max, 3])"""
        vis, u, v, z = project(self.c, t, float, max_radius)
        new = vis & (self.ids < 0)
        self.ids = np.where(new, self.next_id[:, None] + np.cumsum(new, axis=1) - 1, self.ids)
        self.next_id = self.next_id + new.sum(axis=1)
        self.ids = np.where(vis, self.ids, -1)
        tid, meas = np.full((B, tracks_max), -1, dtype=np.int64), np.zeros((B, tracks_max, 3))
        for b in range(B):
            k = np.nonzero(vis[b])[0]
            tid[b, :len(k)] = self.ids[b, k]
            meas[b, :len(k)] = np.stack([u[b, k], v[b, k], z[b, k]], axis=1)
        return dict(vis=vis, u=u, v=v, z=z, ids=self.ids.copy(), next_id=self.next_id.copy(), cnt=vis.sum(axis=1).astype(np.int32),
                    track_ids=tid, meas=meas)


def build_driver(tmp, flags=(), name="pcw_camera_driver"):
    """tests/pcw_camera_driver.cpp under g++ without contraction (x86-64 without -mfma has none to begin with)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pcw_camera_driver.cpp"
    exe = os.path.join(str(tmp), name)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "pcw_camera_driver.cpp"), "-o", exe] + list(flags), check=True)
    return exe


def run_driver(exe, tmp, cam, max_radius, X, g):
    """pcw_project of the host build over n (point X [n, 3], pose g [n, 12]) pairs -> (vis [n] bool, uvz [n, 3])"""
    X, g = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(g, dtype=np.float64).reshape(-1, 12)
    n = X.shape[0]
    assert g.shape[0] == n
    fin, fout = os.path.join(str(tmp), "cam_in.bin"), os.path.join(str(tmp), "cam_out.bin")
    d = list(cam.get("d", [])) + [0.0] * 5
    with open(fin, "wb") as f:
        f.write(np.array([n, cam["model"], cam["rows"], cam["cols"]], dtype=np.int64).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]] + d[:5] + [max_radius], dtype=np.float64).tobytes())
        f.write(X.tobytes()); f.write(g.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    with open(fout, "rb") as f:
        raw = f.read()
    assert len(raw) == n + 24 * n
    return np.frombuffer(raw[:n], dtype=np.uint8).astype(bool), np.frombuffer(raw[n:], dtype=np.float64).reshape(n, 3)


def driver_frame(exe, tmp, c, t, max_radius=None):
    """frame t of a case through the host build -> (vis, u, v, z) [B, NPTS]"""
    g = np.repeat(c["gsc"][t][:, None, :], NPTS, axis=1)
    vis, uvz = run_driver(exe, tmp, c["cam"], c["max_radius"] if max_radius is None else max_radius, c["Xs"], g)
    uvz = uvz.reshape(B, NPTS, 3)
    return vis.reshape(B, NPTS), uvz[..., 0], uvz[..., 1], uvz[..., 2]


def host_error(exe, tmp, c):
    """the largest |du|, |dv| in px of the host build against the 80-bit restatement over the points visible in it, all frames"""
    worst = 0.0
    for t in range(c["gsc"].shape[0]):
        vis, u, v, _ = project(c, t, LD)
        _, hu, hv, _ = driver_frame(exe, tmp, c, t)
        assert vis.sum() > 0
        worst = max(worst, float(np.abs(hu.astype(LD) - u)[vis].max()), float(np.abs(hv.astype(LD) - v)[vis].max()))
    return worst
