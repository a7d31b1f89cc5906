"""GPU: the device life cycle of the "subfilter" mode on tracks the device produces (xivo_hip_pool_life_begin_tracks): the strided
form of the track block under pool_life_begin_kernel / pool_life_admit_kernel / pool_life_end_kernel against their packed form on
the same tracks uploaded, resident frames against frames fed the poses read back, the refusals, and the upper layers
(run_pcw_batch, the C++ BatchEstimator, the command line). Both forms run the same kernels on the same values, so the
comparisons of the first two are for equal bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sub-filter set-up of tests/test_pool_lifecycle_gpu.py (tracks pass the candidate test within a few frames) on the smallest
# tables, which all fill; triangulation and the adaptive initial depth on, so that the begin call enqueues every kernel it can
QUICK = dict(feature_init="subfilter", initial_z=5.0, initial_std_z=0.5, max_group_lifetime=3,
             subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2))
TABLES = dict(QUICK, n_groups=3, n_features=6, pool_max=8, anchor_max=3, triangulate_pre_subfilter=True, adaptive_initial_depth=True)
B, NPTS, T, EVERY, IMU_DT = 3, 300, 6, 16, 0.0025
MOTION, RATE = ["lissajous", "trefoil", "lissajous"], [0.08, 0.1, 0.12]


def _sims():
    return [pcw.TrajectorySim(MOTION[b], rate=RATE[b]) for b in range(B)]


def frustum_world(cfg, sims, npts, seed):
    """one world per filter whose points fill and overlap the first frame's image (depths 3 .. 8 m): about nine in ten are
    visible, and the camera's motion moves some across the borders in every frame"""
    rng = np.random.default_rng(seed)
    Rbc = pcw.so3_exp(cfg.Wbc)
    cam = cfg.cam
    Xs = np.zeros((len(sims), npts, 3))
    for b, s in enumerate(sims):
        Rsb, Tsb = s.gsb(0.0)
        Rsc, Tsc = Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb
        z = rng.uniform(3.0, 8.0, npts)
        u, v = rng.uniform(-20.0, cam["cols"] + 20.0, npts), rng.uniform(-15.0, cam["rows"] + 15.0, npts)
        Xc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], axis=1)
        Xs[b] = Xc @ Rsc.T + Tsc
    return Xs


def _backend(track_source="device", imu_source="host", pool_lifecycle="device", sims=None, **kw):
    cfg = sequence.SequenceConfig(pool_lifecycle=pool_lifecycle, track_source=track_source, imu_source=imu_source, npts=NPTS,
                                  tracks_max=NPTS, **{**TABLES, **kw})
    sims = sims or _sims()
    poses = sequence.initial_poses(cfg, sims)
    be = sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0))
    if track_source == "device":
        be.set_world(frustum_world(cfg, sims, NPTS, 3))
    if imu_source == "device":
        be.enable_device_imu(MOTION, RATE, EVERY, T + 2, IMU_DT, seed=9)
    return be, cfg, sims


NAMES = ("P", "poses", "groups", "feats", "pool entries", "anchor poses", "anchor slots", "init_z", "feat_id", "feat_ref",
         "group_refs", "ent_id", "ent_born", "anc_used", "anc_life", "counters")


def _snapshot(be):
    """P, the scene, the pool, the anchors, init_z, both books and the twelve counters as bytes"""
    ent, ap, sl = be.ctx.pool_get(0, be.B)
    bk = be.pool_life_book()
    parts = [be.covariance()] + list(be.scene()) + [ent, ap, sl, be.ctx.pool_get_init_z(0, be.B)]
    parts += [bk[k] for k in ("feat_id", "feat_ref", "group_refs", "ent_id", "ent_born", "anc_used", "anc_life")]
    st = be.pool_life_stats()
    assert len(st.dtype.names) == 12
    return [np.ascontiguousarray(x).tobytes() for x in parts] + [st.tobytes()]


def _same(a, b, tag):
    assert len(a) == len(b) == len(NAMES)
    for x, y, name in zip(a, b, NAMES):
        assert x == y, (tag, name)


def _packed(cnt, ids, meas):
    off = np.zeros(len(cnt) + 1, dtype=np.int32)
    off[1:] = np.cumsum(cnt)
    return (off, np.concatenate([ids[b, :cnt[b]] for b in range(len(cnt))]),
            np.concatenate([meas[b, :cnt[b]] for b in range(len(cnt))]))


def _host_frames(cfg, sims):
    """per camera frame (every 16 IMU samples): the feeder's records since the last frame (None at t = 0) and the ground-truth
    camera poses gsc [B, 12]"""
    Rbc = pcw.so3_exp(cfg.Wbc)
    m0 = [s.meas(0.0) for s in sims]
    feeder = sequence.ImuFeeder(B, 0.0, [m[1] for m in m0], [m[0] for m in m0])
    for t in range(T):
        for k in range(EVERY * t - EVERY + 1 if t else 0, EVERY * t + 1):
            if k > 0:
                m = [s.meas(k * IMU_DT) for s in sims]
                feeder.imu(k * IMU_DT, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
        tt = EVERY * t * IMU_DT
        feeder.visual(tt)
        g = [s.gsb(tt) for s in sims]
        yield feeder.take(), np.array([np.concatenate([(R @ Rbc).reshape(-1), R @ cfg.Tbc + p]) for R, p in g])


def _check_run(st, most_tracks):
    """the run reached what it is for: more tracks in a filter than one pass of the workgroup, full tables, admissions"""
    print("most tracks in a filter %d; admitted %d, pool added / dropped %d / %d, dropped %d, rejected %d, updates %d" % (
        most_tracks, st["admitted"].sum(), st["pool_added"].sum(), st["pool_dropped"].sum(), st["dropped"].sum(),
        st["rejected"].sum(), st["updates"].sum()))
    assert most_tracks > 256
    assert st["pool_added"].sum() > 0 and st["pool_dropped"].sum() > 0 and st["admitted"].sum() > 0 and st["updates"].sum() > 0


@pytest.mark.parametrize("alternate", [False, True])
def test_frames_on_produced_tracks_equal_frames_on_the_same_tracks_uploaded(built, alternate):
    """6 frames, 3 filters, pixel noise on. Context 1 runs propagate -> pcw_tracks -> pool_life_begin_tracks -> update ->
    pool_life_end (SequenceRunner.frame_world); context 2 is fed context 1's tracks, read back, through the host-track
    xivo_hip_pool_life_begin. After every frame P, the scene, the pool, the anchors, init_z, both books and the twelve counters
    are byte-equal. alternate: context 1 takes every other frame through xivo_hip_pool_life_begin too (on the tracks it just
    produced and read back), so that the packed and the strided form of the block follow each other on one context."""
    one, cfg, sims = _backend()
    two, _, _ = _backend(track_source="host")
    try:
        r1 = sequence.SequenceRunner(one, cfg, B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        most = 0
        for k, (rec, gsc) in enumerate(_host_frames(cfg, sims)):
            strict = k + 1 >= cfg.strict_criteria_timesteps
            if alternate and k % 2 == 1:
                one.propagate(rec)
                one.make_tracks(gsc, 1.0, 21, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)
                r1.vision_counter += 1
                one.pool_life_begin(*_packed(*tr), strict)
                one.update(download=False)
                one.pool_life_end()
            else:
                r1.frame_world(rec, gsc, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)      # (the frame only read them: still in the block)
            assert r1.vision_counter == k + 1
            most = max(most, int(tr[0].max()))
            if rec is not None:
                two.propagate(rec)
            two.pool_life_begin(*_packed(*tr), strict)
            two.update(download=False)
            two.pool_life_end()
            _same(_snapshot(one), _snapshot(two), "frame %d" % k)
        _check_run(one.pool_life_stats(), most)
    finally:
        one.close(); two.close()


def test_resident_frames_equal_frames_fed_the_poses_read_back(built):
    """6 frames, IMU and pixel noise on. Context 1 runs SequenceRunner.frame_resident (trajsim_frame -> propagate_resident ->
    pcw_tracks_resident -> pool life cycle); context 2 runs frame_world on the records and camera poses read back with
    xivo_hip_trajsim_get. The same byte equality after every frame."""
    one, cfg1, _ = _backend(imu_source="device")
    two, cfg2, _ = _backend()
    try:
        r1, r2 = sequence.SequenceRunner(one, cfg1, B), sequence.SequenceRunner(two, cfg2, B)
        for r in (r1, r2):
            r.noise_px_std, r.noise_seed = 1.0, 21
        most = 0
        for f in range(T):
            k0, n = (0, 0) if f == 0 else ((f - 1) * EVERY, EVERY)
            r1.frame_resident(k0, n, f)
            recs, gsc = one.ctx.trajsim_get(0, B)
            most = max(most, int(one.ctx.pcw_get_tracks(cfg1.tracks_max, 0, B)[0].max()))
            r2.frame_world(recs if n else None, gsc, f)
            _same(_snapshot(one), _snapshot(two), "frame %d" % f)
        assert r1.vision_counter == r2.vision_counter == T
        _check_run(one.pool_life_stats(), most)
        assert one.ground_truth().shape == (T, B, 12)
    finally:
        one.close(); two.close()


def _refused(f, *a, **k):
    with pytest.raises(L.XivoHipError) as e:
        f(*a, **k)
    assert e.value.status == -1


def test_refusals_change_nothing(built):
    """XIVO_HIP_ERR_INVALID with nothing changed: pool_life_begin_tracks with nothing produced, with another B, inside an open
    frame and a second time on the same tracks; the producer inside an open pool frame; each life cycle's begin_tracks on the
    other's context; pcw_config with neither life cycle; and pool_life_config releases the worlds with the track block"""
    be, cfg, sims = _backend()
    F = cfg.n_features
    gsc = next(_host_frames(cfg, sims))[1]
    try:
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=B)          # nothing produced yet
        be.make_tracks(gsc, 0.0, 0, 0)
        keep = (be.ctx.pcw_get_tracks(NPTS), be.world_ids(), _snapshot(be))

        def unchanged():
            now = (be.ctx.pcw_get_tracks(NPTS), be.world_ids(), _snapshot(be))
            for x, y in zip(now[0] + now[1], keep[0] + keep[1]):
                assert x.tobytes() == y.tobytes()
            _same(now[2], keep[2], "refused")
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=2)          # produced for another B
        _refused(be.ctx.pool_life_begin_tracks, 0, False, B=B)          # (and what pool_life_begin refuses: F out of range)
        _refused(be.ctx.life_begin_tracks, F, B=B)                      # the immediate life cycle's call on a pool context
        unchanged()
        be.pool_life_begin_tracks(False)
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=B)          # inside the open frame
        _refused(be.make_tracks, gsc, 0.0, 0, 1)
        _refused(be.ctx.pcw_config, NPTS, 275.0, 275.0, 320.0, 240.0, 640.0, 480.0)
        be.update(download=False)
        be.pool_life_end()
        after = _snapshot(be)
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=B)          # consumed: nothing produced since
        _same(_snapshot(be), after, "consumed")
        assert int(be.pool_life_stats()["pool_added"].sum()) > 0
        # a host-track frame overwrites the block: no device tracks to read or to begin on
        be.pool_life_begin(np.zeros(B + 1, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros((0, 3)), False)
        be.update(download=False)
        be.pool_life_end()
        _refused(be.ctx.pcw_get_tracks, NPTS)
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=B)
        be.make_tracks(gsc, 0.0, 0, 2)                                  # (the worlds are still there)
        # pool_life_config releases the worlds with the block; with neither life cycle left they cannot come back
        be.ctx.pool_life_config(0)
        _refused(be.make_tracks, gsc, 0.0, 0, 3)
        _refused(be.ctx.pool_life_begin_tracks, F, False, B=B)
        _refused(be.ctx.pcw_config, NPTS, 275.0, 275.0, 320.0, 240.0, 640.0, 480.0)
    finally:
        be.close()
    # the host sub-filter life cycle: no device life cycle at all
    be, cfg, _ = _backend(track_source="host", pool_lifecycle="host")
    try:
        _refused(be.ctx.pcw_config, NPTS, 275.0, 275.0, 320.0, 240.0, 640.0, 480.0)
    finally:
        be.close()
    # the immediate device life cycle: its context refuses the pool's call, fresh tracks or not
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", npts=NPTS, tracks_max=NPTS, n_groups=3, n_features=6)
    sims = _sims()
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        be.set_world(frustum_world(cfg, sims, NPTS, 3))
        be.make_tracks(gsc, 0.0, 0, 0)
        state = [be.covariance().tobytes()] + [x.tobytes() for x in be.scene()] + [x.tobytes() for x in be.life_book()]
        _refused(be.ctx.pool_life_begin_tracks, cfg.n_features, False, B=B)
        assert state == [be.covariance().tobytes()] + [x.tobytes() for x in be.scene()] + [x.tobytes() for x in be.life_book()]
        be.life_begin_tracks()                                          # (the refusal did not consume them)
        be.update(download=False)
        be.life_end()
    finally:
        be.close()


SEQ = dict(QUICK, pool_max=64, anchor_max=16)


def _ate(out):
    return np.sqrt(np.mean(np.sum((out["Tsb"] - out["gt_Tsb"]) ** 2, axis=2), axis=0))


def _books(out, n):
    return [tuple(x.tobytes() for x in out["estimator"].book(b)) for b in range(n)]


def _counters(out):
    st = out["estimator"].stats()
    return {k: st[k] for k in ("updates", "mh_rejected", "admitted", "pool_dropped")}


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_run_pcw_batch_device_tracks_against_host_tracks(built, sigma):
    """run_pcw_batch (the C++ estimator: VisualMeasDeviceWorld with the device pool life cycle), 4 sequences, 10 frames: tracks
    from the device against BatchPCW(noise="philox") uploaded. Without noise Tsb and the books are byte-equal; with noise the
    books and the counters are equal and the ATE agrees to 1e-6 m (pixel differences of 1e-13 px cannot move it by a micrometre
    unless a decision flipped, which the equal books exclude: the bound and the argument of tests/test_pcw_tracks_gpu.py)"""
    n = 4
    cfg = sequence.SequenceConfig(pool_lifecycle="device", **SEQ)
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, n, total_time=0.4, noise_vision_std=sigma, track_source=src, noise="philox",
                                               noise_seed=5)
        c = {k: _counters(o) for k, o in outs.items()}
        print("sigma %.1f: counters %s" % (sigma, c["device"]))
        assert len(outs["device"]["ts"]) == 10
        assert _books(outs["device"], n) == _books(outs["host"], n)
        assert c["device"] == c["host"] and c["device"]["updates"] > 0
        d = np.abs(_ate(outs["device"]) - _ate(outs["host"])).max()
        print("sigma %.1f: max |ATE device tracks - ATE host tracks| = %.3e m" % (sigma, d))
        if sigma == 0.0:
            assert outs["device"]["Tsb"].tobytes() == outs["host"]["Tsb"].tobytes()
        else:
            assert d <= 1e-6
    finally:
        for o in outs.values():
            o["estimator"].close()


def test_run_pcw_batch_device_imu_against_host_imu(built):
    """the same with the IMU from the device too (BatchEstimator::FrameResident on the pool life cycle) against the host arm with
    imu_noise="philox", device tracks on both arms, sigma = 1 px: books and counters equal, the ATE within 1e-6 m (the argument
    of tests/test_trajsim_gpu.py: input differences in the last places cannot move it by a micrometre unless a decision
    flipped)"""
    n = 4
    cfg = sequence.SequenceConfig(pool_lifecycle="device", track_source="device", **SEQ)
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, n, total_time=0.4, noise_vision_std=1.0, noise_seed=5, imu_source=src,
                                               imu_noise="philox")
        c = {k: _counters(o) for k, o in outs.items()}
        assert len(outs["device"]["ts"]) == 10 and np.array_equal(outs["device"]["ts"], outs["host"]["ts"])
        assert _books(outs["device"], n) == _books(outs["host"], n)
        assert c["device"] == c["host"] and c["device"]["updates"] > 0
        d = np.abs(_ate(outs["device"]) - _ate(outs["host"])).max()
        print("max |ATE device IMU - ATE host IMU| = %.3e m; counters %s" % (d, c["device"]))
        assert d <= 1e-6
    finally:
        for o in outs.values():
            o["estimator"].close()


def test_python_runner_against_the_cpp_estimator(built):
    """SequenceRunner.frame_world / frame_resident with pool_lifecycle="device" against BatchEstimator::VisualMeasDeviceWorld /
    FrameResident on the same worlds, curves and seeds, 10 frames each: the same books and counters, Tsb within 1e-10 as between
    the two host sides today"""
    from xivo_amd.batch import BatchEstimator
    n, npts, frames = 3, 300, 10
    for imu in ("host", "device"):
        cfg = sequence.SequenceConfig(pool_lifecycle="device", track_source="device", imu_source=imu, npts=npts, tracks_max=npts, **SEQ)
        sims = _sims()
        Xs = frustum_world(cfg, sims, npts, 5)
        poses = sequence.initial_poses(cfg, sims)
        be = sequence.HipBackend(cfg, n, poses, np.repeat(cfg.P_init()[None], n, axis=0))
        est = BatchEstimator(cfg, n, poses, cfg.P_init())
        try:
            be.set_world(Xs)
            est.enable_device_world(Xs)
            if imu == "device":
                be.enable_device_imu(MOTION, RATE, EVERY, frames, IMU_DT, seed=9)
                est.enable_device_imu(MOTION, RATE, EVERY, frames, IMU_DT, seed=9)
            run = sequence.SequenceRunner(be, cfg, n)
            run.noise_px_std, run.noise_seed = 1.0, 3
            Rbc = pcw.so3_exp(cfg.Wbc)
            m0 = [s.meas(0.0) for s in sims]
            feeder = sequence.ImuFeeder(n, 0.0, [m[1] for m in m0], [m[0] for m in m0])
            worst = 0.0
            for f in range(frames):
                if imu == "device":
                    k0, nn = (0, 0) if f == 0 else ((f - 1) * EVERY, EVERY)
                    run.frame_resident(k0, nn, f)
                    est.FrameResident(k0, nn, 1.0, 3)
                else:
                    for k in range(EVERY * f - EVERY + 1 if f else 0, EVERY * f + 1):
                        t = k * IMU_DT
                        m = [s.meas(t) for s in sims] if k > 0 else m0      # (a simulator draws its noise per call)
                        gyro, accel = np.array([x[1] for x in m]), np.array([x[0] for x in m])
                        if k > 0:
                            feeder.imu(t, gyro, accel)
                        est.InertialMeas(t, gyro, accel)
                    t = EVERY * f * IMU_DT
                    feeder.visual(t)
                    gsc = np.array([np.concatenate([(s.gsb(t)[0] @ Rbc).reshape(-1), s.gsb(t)[0] @ cfg.Tbc + s.gsb(t)[1]]) for s in sims])
                    run.frame_world(feeder.take(), gsc, f)
                    est.VisualMeasDeviceWorld(t, gsc, 1.0, 3)
                worst = max(worst, float(np.abs(est.gsb()[1] - be.poses()[1]).max()))
            books = run.books
            for b in range(n):
                fid, fref, gref = est.book(b)
                assert list(fid) == books[b].feat_id and list(fref) == books[b].feat_ref and list(gref) == books[b].group_refs
            st, ps = est.stats(), be.pool_life_stats()
            print("imu %s: updates %d, admitted %d, pool dropped %d, max |Tsb cpp - python| %.3e" % (
                imu, st["updates"], st["admitted"], st["pool_dropped"], worst))
            assert st["updates"] == run.n_updates > 0 and st["mh_rejected"] == run.n_rejected
            assert st["admitted"] == int(ps["admitted"].sum()) > 0 and st["pool_dropped"] == run.n_pool_dropped
            assert worst < 1e-10
        finally:
            be.close(); est.close()


@pytest.mark.parametrize("host", [["-vectorized"], ["-vectorized", "-imu", "device"], []], ids=["host-imu", "device-imu", "python-host"])
def test_run_pcw_cli(built, host):
    """run_pcw.py [-vectorized] -feature_init subfilter -pool-lifecycle device -tracks device [-imu device] runs and reports
    (without -vectorized: sequence.run_pcw, the Python host side)"""
    imu = "-imu" in host
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-sequences", "4", "-total_time", "1.2",
           "-npts", "300", "-feature_init", "subfilter", "-pool-lifecycle", "device", "-tracks", "device"] + host
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["tracks"] == "device" and rep["pool_lifecycle"] == "device" and rep["feature_init"] == "subfilter"
    assert rep.get("imu", "host") == ("device" if imu else "host")
    assert rep["updates"] > 0 and rep["frames_per_sequence"] == 30
