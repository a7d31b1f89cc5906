"""GPU: the trajectory producer on the device (xivo_hip_trajsim_*, trajsim_kernels.hip) against the numpy restatement of
tests/trajsim_restate.py (which tests/test_trajsim_cpu.py holds against the header under a host compiler, BatchTrajectorySim
and ImuFeeder, and where the bounds are derived), the resident propagate and track entries against the host-pointer ones they
restate, and the upper layers.

Largest differences seen on an MI355X are printed by the tests and recorded in DESIGN.md, "Trajectory producer"."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcw_restate as PR
import trajsim_restate as R
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_groups=2, n_features=4, min_new_features=2)
IMU_DT = 0.0025


def _curves(B):
    motion = np.array([b % 2 for b in range(B)], dtype=np.int32)
    rate = np.array([(0.0, 0.08, 0.1, 0.12, 0.09)[b % 5] for b in range(B)])
    return motion, rate


def _model(noise, **kw):
    return R.Model(noise_accel=1e-4 if noise else 0.0, noise_gyro=1e-5 if noise else 0.0,
                   Rbc=pcw.so3_exp(np.array([-1.57079633, 0.0, 0.0])), Tbc=(0.05, -0.02, 0.1), seed=77, **kw)


def _check_frame(ctx, m, motion, rate, k0, n, B, frame):
    """one trajsim_frame against the restatement -> largest difference as a fraction of the bound"""
    ctx.trajsim_frame(k0, n, B=B)
    recs, gsc = ctx.trajsim_get(0, B)
    want, bound = R.records(m, motion, rate, k0, n)
    assert recs.shape == (B, n) and recs["dt"].tobytes() == want["dt"].tobytes()
    w = R.worst(recs, want, bound)
    wgt, wgsc, bgt, bgsc = R.truth(m, motion, rate, k0 + n)
    gt = ctx.trajsim_get_gt(0, B, frame, 1)[0]
    w = max(w, float((np.abs(gt - wgt) / bgt).max()), float((np.abs(gsc - wgsc) / bgsc).max()))
    return w


@pytest.mark.parametrize("k0", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_records_poses_and_log_against_the_restatement(built, B, k0):
    """n in {0, 1, 2, 63, 64, 65} (a filter's items straddle a workgroup of 256 from n = 63 on with B = 65), both curves, rates
    including 0, noise off and on, k0 across 2^32: dt exact, every other value of the records, the camera poses and the log's
    body poses within the bound of tests/trajsim_restate.py (64 ulp of the largest intermediate; slopes: over dt)"""
    motion, rate = _curves(B)
    worst = 0.0
    with L.Context(47, 8, B) as ctx:
        for noise in (False, True):
            m = _model(noise)
            ctx.trajsim_config(65, 6, **m.config_kw())
            ctx.trajsim_set(motion, rate)
            for f, n in enumerate((0, 1, 2, 63, 64, 65)):
                worst = max(worst, _check_frame(ctx, m, motion, rate, k0, n, B, f))
            assert ctx.trajsim_count() == 6
    print("B %d k0 %d: largest difference %.3f of the bound" % (B, k0, worst))
    assert worst <= 1.0


def test_same_bits_whatever_the_batch(built):
    """a value depends on (seed, k, filter) and the filter's curve alone: filter 2's records, camera pose and log entry with
    B = 3 and with B = 65 are byte-equal"""
    got = {}
    m = _model(True)
    for B in (3, 65):
        motion, rate = _curves(B)
        with L.Context(47, 8, B) as ctx:
            ctx.trajsim_config(65, 2, **m.config_kw())
            ctx.trajsim_set(motion, rate)
            ctx.trajsim_frame(2 ** 32 - 3, 65, B=B)
            recs, gsc = ctx.trajsim_get(2, 1)
            got[B] = (recs.tobytes(), gsc.tobytes(), ctx.trajsim_get_gt(2, 1).tobytes())
    assert got[3] == got[65] and len(got[3][0]) == 65 * 104


def _backend(B, npts=300, track_source="device", imu=True, model=None, k0=0, T_max=8, n_max=16, **kw):
    cfg = sequence.SequenceConfig(lifecycle="device", track_source=track_source, npts=npts, tracks_max=320,
                                  imu_source="device" if (imu and track_source == "device") else "host", **{**SMALL, **kw})
    motion, rate = _curves(B + 1)
    motion, rate = motion[1:], rate[1:]                    # (no stationary filter: its features never triangulate well)
    sims = [pcw.TrajectorySim("trefoil" if motion[b] else "lissajous", rate=rate[b]) for b in range(B)]
    poses = sequence.initial_poses(cfg, sims, t0=k0 * IMU_DT)
    be = sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0))
    if imu:
        m = model or R.Model(seed=77)
        sim = m.config_kw()
        del sim["Rbc"], sim["Tbc"]
        be.enable_device_imu(motion, rate, n_max, T_max, sim.pop("imu_dt"), **sim)
    return be, cfg


def _state(be):
    P, scene = be.covariance(), be.scene()
    return [P.tobytes()] + [x.tobytes() for x in scene]


@pytest.mark.parametrize("method", ["RK4", "PD"])
@pytest.mark.parametrize("n", [1, 16])
def test_propagate_resident_against_propagate(built, method, n):
    """context 1 propagates over the records where the kernel left them; context 2 is handed the records read back through
    xivo_hip_propagate: poses and P byte-equal"""
    B = 2
    one, cfg = _backend(B, integration_method="RK4" if method == "RK4" else "PrinceDormand")
    two, _ = _backend(B, imu=False, integration_method=cfg.integration_method)
    try:
        assert _state(one) == _state(two)
        for f in range(2):
            one.make_imu(f * n, n)
            one.propagate_resident()
            recs, _ = one.ctx.trajsim_get(0, B)
            two.propagate(recs)
            assert _state(one) == _state(two), f
        assert not np.array_equal(one.scene()[0]["Tsb"], np.zeros((B, 3)))
    finally:
        one.close(); two.close()


def test_propagate_resident_with_stepsize_control(built):
    """two consecutive frames under control_stepsize: the step each filter carries goes from one call to the next on both
    contexts alike"""
    B, n = 2, 16
    one, cfg = _backend(B)
    two, _ = _backend(B, imu=False)
    pd = dict(tolerance=1e-3, attempts=12, min_scale_factor=0.125, max_scale_factor=4.0)
    try:
        for f in range(2):
            one.make_imu(f * n, n)
            one.ctx.propagate_resident(one.Qimu, one.Qmodel, cfg.gravity, "PD", cfg.stepsize, pd, B=B)
            recs, _ = one.ctx.trajsim_get(0, B)
            two.ctx.propagate(recs, two.Qimu, two.Qmodel, cfg.gravity, "PD", cfg.stepsize, pd_control=pd)
            assert _state(one) == _state(two), f
    finally:
        one.close(); two.close()


def _tracks_same(a, b):
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_pcw_tracks_resident_against_pcw_tracks(built):
    """the producer on the poses the kernel left against the producer handed the poses read back, on a second context: counts,
    ids and measurements byte-equal over three frames (ids carry over from frame to frame)"""
    B, npts = 2, 300
    Xs = PR.box_world(B, npts, 8)
    one, cfg = _backend(B, npts)
    two, _ = _backend(B, npts, imu=False)
    try:
        one.set_world(Xs); two.set_world(Xs)
        seen = 0
        for f in range(3):
            one.make_imu(16 * f, 16)
            one.make_tracks_resident(1.0, 21, f)
            _, gsc = one.ctx.trajsim_get(0, B)
            two.make_tracks(gsc, 1.0, 21, f)
            a, b = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B), two.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)
            _tracks_same(a, b)
            seen += int(a[0].sum())
        assert seen > 30
    finally:
        one.close(); two.close()


def _snapshot(be):
    return _state(be) + [x.tobytes() for x in be.life_book()] + [be.life_stats().tobytes()]


@pytest.mark.parametrize("alternate", [False, True])
def test_whole_frames_resident_against_host_pointer_entries(built, alternate):
    """6 frames, 2 filters, IMU and pixel noise on. Context 1 runs resident frames (SequenceRunner.frame_resident); context 2 is
    fed the same records and poses through xivo_hip_propagate / xivo_hip_pcw_tracks. P, scene, book and xivo_life_stats are
    byte-equal after every frame. alternate: context 1 takes every other frame through the host-pointer entries too (on what
    its own kernel produced and it read back), so that the two kinds of frames follow each other on one context."""
    B, npts, n = 2, 300, 16
    Xs = PR.box_world(B, npts, 8)
    one, cfg = _backend(B, npts)
    two, _ = _backend(B, npts, imu=False)
    try:
        one.set_world(Xs); two.set_world(Xs)
        r1 = sequence.SequenceRunner(one, cfg, B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        for f in range(6):
            k0, nn = (0, 0) if f == 0 else ((f - 1) * n, n)
            if alternate and f % 2 == 1:
                one.make_imu(k0, nn)
                recs, gsc = one.ctx.trajsim_get(0, B)
                one.propagate(recs)
                one.make_tracks(gsc, 1.0, 21, f)
                one.life_begin_tracks(); one.update(download=False); one.life_end()
            else:
                r1.frame_resident(k0, nn, f)
                recs, gsc = one.ctx.trajsim_get(0, B)
            if nn:
                two.propagate(recs)
            two.make_tracks(gsc, 1.0, 21, f)
            two.life_begin_tracks(); two.update(download=False); two.life_end()
            assert _snapshot(one) == _snapshot(two), f
        st = one.life_stats()
        assert int(st["admitted"].sum()) > 0 and int(st["updates"].sum()) > 0
        assert one.ground_truth().shape == (6, B, 12)
    finally:
        one.close(); two.close()


def test_refusals_change_nothing(built):
    """refused with nothing changed: n > n_max; a full log; propagate_resident without fresh records, for another B, and a
    second time; pcw_tracks_resident without a pose; trajsim_frame inside an open frame; a calibration-build context"""
    def refused(f, *a, status=-1, **k):
        with pytest.raises(L.XivoHipError) as e:
            f(*a, **k)
        assert e.value.status == status

    B, npts = 2, 64
    be, cfg = _backend(B, npts, T_max=3, n_max=4)
    try:
        be.set_world(PR.box_world(B, npts, 2))
        refused(be.propagate_resident)                         # nothing produced yet
        refused(be.make_tracks_resident, 0.0, 0, 0)            # no pose yet
        be.make_imu(0, 4)
        keep = (be.ctx.trajsim_get(0, B), be.ctx.trajsim_get_gt(0, B), _snapshot(be))

        def unchanged():
            now = (be.ctx.trajsim_get(0, B), be.ctx.trajsim_get_gt(0, B), _snapshot(be))
            assert now[0][0].tobytes() == keep[0][0].tobytes() and now[0][1].tobytes() == keep[0][1].tobytes()
            assert now[1].tobytes() == keep[1].tobytes() and now[2] == keep[2] and be.ctx.trajsim_count() == 1
        refused(be.make_imu, 4, 5)                             # n > n_max
        refused(be.ctx.trajsim_frame, 4, 1, B=3)               # B out of range
        refused(be.ctx.propagate_resident, opts=be._prop_opts, B=1)
        refused(be.ctx.pcw_tracks_resident, 0.0, 0, 0, B=1)
        unchanged()
        be.propagate_resident()
        after = _snapshot(be)
        refused(be.propagate_resident)                         # consumed
        assert _snapshot(be) == after
        be.make_tracks_resident(0.0, 0, 0)
        be.life_begin_tracks()
        refused(be.make_imu, 4, 4)                             # inside the open frame
        be.update(download=False); be.life_end()
        be.make_imu(4, 0)                                      # poses only: no records to propagate over
        refused(be.propagate_resident)
        be.make_imu(4, 4)
        assert be.ctx.trajsim_count() == 3
        last = be.ctx.trajsim_get(0, B)
        refused(be.make_imu, 8, 4, status=-6)                  # the log is full
        assert be.ctx.trajsim_get(0, B)[0].tobytes() == last[0].tobytes() and be.ctx.trajsim_count() == 3
        be.propagate_resident()                                # (the refused frame did not take the records away)
        be.ctx.trajsim_reset()
        assert be.ctx.trajsim_count() == 0
        be.make_imu(8, 4)
        # a configuration that is refused leaves the one in place
        last = be.ctx.trajsim_get(0, B)
        for bad in (dict(imu_dt=0.0), dict(imu_dt=float("nan")), dict(noise_accel=-1.0), dict(rot_amp=float("inf")),
                    dict(T_max=0), dict(n_max=-1)):
            refused(be.ctx.trajsim_config, **{**dict(n_max=4, T_max=3), **bad})
        o = np.zeros(1, dtype=L.trajsim_opts_dtype)
        o["struct_size"], o["n_max"], o["T_max"], o["imu_dt"] = 199, 4, 3, IMU_DT
        assert be.ctx.lib.xivo_hip_trajsim_config(be.ctx.h, o.ctypes.data) == -1
        assert be.ctx.trajsim_count() == 1 and be.ctx.trajsim_get(0, B)[0].tobytes() == last[0].tobytes()
        be.ctx.trajsim_config(0)                               # releases
        refused(be.make_imu, 8, 4)
    finally:
        be.close()
    # an online-calibration build: its motion block is not the default build's 23
    with L.Context(24 + 12 + 12, 8, 2) as ctx:
        ctx.set_layout(48, 24, 2, 36, 4, sequence.SequenceConfig().cam)
        ctx.set_calib(td=23, Cg=-1, cam_begin=0, cam_dim=0)
        refused(ctx.trajsim_config, 4, 4, status=-5)


def _ate(out):
    return np.sqrt(np.mean(np.sum((out["Tsb"] - out["gt_Tsb"]) ** 2, axis=2), axis=0))


def _books(out, B):
    return [tuple(x.tobytes() for x in out["estimator"].book(b)) for b in range(B)]


def test_run_pcw_batch_device_imu_against_host_imu(built):
    """run_pcw_batch (the C++ estimator), 4 sequences, 10 frames, device tracks on both arms: the device IMU arm
    (BatchEstimator::FrameResident) against the host arm with imu_noise="philox" (InertialMeas per sample). Books and counters
    equal; gt_Tsb within the restatement's bounds (the host simulator against the restatement, 16 ulp, plus the restatement
    against the device, 64 ulp, of |p| + |p0| <= 10); the ATE agrees to 1e-6 m - input differences in the last places cannot
    move it by a micrometre unless a decision flipped, which the equal books exclude"""
    B = 4
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device")
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, B, total_time=0.4, noise_vision_std=1.0, noise_seed=5, imu_source=src,
                                               imu_noise="philox")
        st = {k: o["estimator"].stats() for k, o in outs.items()}
        assert len(outs["device"]["ts"]) == 10 and np.array_equal(outs["device"]["ts"], outs["host"]["ts"])
        assert _books(outs["device"], B) == _books(outs["host"], B)
        assert st["device"]["updates"] == st["host"]["updates"] > 0 and st["device"]["mh_rejected"] == st["host"]["mh_rejected"]
        dg = np.abs(outs["device"]["gt_Tsb"] - outs["host"]["gt_Tsb"]).max()
        d = np.abs(_ate(outs["device"]) - _ate(outs["host"])).max()
        print("max |gt_Tsb device - host| = %.3e m, max |ATE device IMU - ATE host IMU| = %.3e m" % (dg, d))
        assert dg <= (16 + R.ULPS) * R.EPS * 10.0
        assert d <= 1e-6
    finally:
        for o in outs.values():
            o["estimator"].close()


def test_python_runner_against_the_cpp_estimator_on_resident_frames(built):
    """SequenceRunner.frame_resident against BatchEstimator::FrameResident on the same worlds, curves and seeds: updates and
    rejections equal, Tsb within 1e-10 as between the two host sides on device tracks"""
    from xivo_amd.batch import BatchEstimator
    B, npts, n, T = 3, 500, 16, 10
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", imu_source="device", npts=npts)
    motion = ["trefoil" if b % 2 else "lissajous" for b in range(B)]
    rate = [0.08, 0.1, 0.12]
    sims = [pcw.TrajectorySim(motion[b], rate=rate[b]) for b in range(B)]
    Xs = PR.box_world(B, npts, 20)
    poses = sequence.initial_poses(cfg, sims)
    be = sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0))
    est = BatchEstimator(cfg, B, poses, cfg.P_init())
    try:
        be.set_world(Xs)
        be.enable_device_imu(motion, rate, n, T, IMU_DT, seed=9)
        est.enable_device_world(Xs)
        est.enable_device_imu(motion, rate, n, T, IMU_DT, seed=9)
        run = sequence.SequenceRunner(be, cfg, B)
        run.noise_px_std, run.noise_seed = 1.0, 3
        worst = 0.0
        for f in range(T):
            k0, nn = (0, 0) if f == 0 else ((f - 1) * n, n)
            run.frame_resident(k0, nn, f)
            est.FrameResident(k0, nn, 1.0, 3)
            worst = max(worst, float(np.abs(est.gsb()[1] - be.poses()[1]).max()))
        st = est.stats()
        assert st["updates"] == run.n_updates > 0 and st["mh_rejected"] == run.n_rejected
        assert worst < 1e-10
    finally:
        be.close(); est.close()


def test_run_pcw_cli_with_the_device_imu(built):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-vectorized", "-sequences", "4", "-total_time", "0.4",
           "-lifecycle", "device", "-tracks", "device", "-imu", "device"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["imu"] == "device" and rep["tracks"] == "device" and rep["updates"] > 0
    assert rep["ate_m"]["max"] < 0.2
