"""GPU: the point-cloud world's track producer on the device (xivo_hip_pcw_*, pcw_kernels.hip) against the numpy restatement of
tests/pcw_restate.py (which tests/test_pcw_tracks_cpu.py holds against the header under a host compiler and against
BatchPCW.generate), the strided track form of the life-cycle kernels against their packed form, and the upper layers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcw_restate as R
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_groups=4, n_features=9, min_new_features=2)      # the layout of tests/test_lifecycle_gpu.py (N = 74)


def _backend(B, npts, tracks_max=None, track_source="device", seed=0, **kw):
    cfg = sequence.SequenceConfig(lifecycle="device", track_source=track_source, npts=npts,
                                  tracks_max=npts if tracks_max is None else tracks_max, **{**SMALL, **kw})
    sims = [pcw.TrajectorySim("lissajous", seed=seed + b) for b in range(B)]
    poses = sequence.initial_poses(cfg, sims, t0=0.4)
    return sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0)), cfg, sims


def _same_tracks(got, want, tag):
    for g, w, k in zip(got, want, ("cnt", "ids", "meas")):
        assert np.array_equal(g, w) and g.tobytes() == w.tobytes(), (tag, k)


@pytest.mark.parametrize("npts", [1, 63, 64, 65, 255, 256, 257, 2048])
def test_scan_boundaries_bit_for_bit(built, npts):
    """B = 3, tracks_max = npts (a world whose every point is visible fills its row), 4 frames, noise off: counts, track ids,
    u, v, z in track order and the worlds' ids / next_id equal the restatement bit for bit. The worlds: every point visible;
    none visible; every point behind the camera; a point that leaves the image and returns with a new id; ids from 2^33 + 5
    (tests/pcw_restate.py edge_case_worlds, whose cases test_pcw_tracks_cpu.py asserts at these sizes)"""
    Xs, next_id, gsc = R.edge_case_worlds(npts, seed=npts)
    rs = R.Restate(Xs, None, next_id)
    be, cfg, _ = _backend(3, npts)
    try:
        be.set_world(Xs, None, next_id)
        steps = []
        for t in range(4):
            be.make_tracks(gsc[t], 0.0, 5, t)
            r = rs.step(gsc[t])
            steps.append(r)
            _same_tracks(be.ctx.pcw_get_tracks(cfg.tracks_max, 0, 3), R.strided(r, cfg.tracks_max), (npts, t))
            ids, nxt = be.world_ids()
            assert np.array_equal(ids, r["ids"]) and np.array_equal(nxt, r["next_id"]), (npts, t)
        R.assert_edge_cases(steps)
    finally:
        be.close()


def test_noise_within_the_derived_bound(built):
    """npts = 257, sigma = 1 px against the restatement with pcw.philox_normal: ids and counts exact, |du|, |dv| <=
    2 ulp(max(imw, imh)) + 1e-13 sigma (|noise| <= 8.6 sigma; log within 1 ulp, sqrt correctly rounded, 2 pi u2 one rounding at
    <= 2 pi, sin / cos within 2 ulp: <= 1.8e-14 sigma, allowed five times over, plus the final addition's rounding); depths exact"""
    npts, sigma = 257, 1.0
    bound = 2 * np.spacing(max(R.CAM["imw"], R.CAM["imh"])) + 1e-13 * sigma
    Xs = R.box_world(3, npts, 4)
    gsc = R.moving_poses(3, 4, 4)
    rs = R.Restate(Xs)
    be, cfg, _ = _backend(3, npts)
    worst, n = 0.0, 0
    try:
        be.set_world(Xs)
        for t in range(4):
            be.make_tracks(gsc[t], sigma, 1234567890123, t)
            cnt, ids, meas = be.ctx.pcw_get_tracks(cfg.tracks_max, 0, 3)
            wc, wi, wm = R.strided(rs.step(gsc[t], sigma, 1234567890123, t), cfg.tracks_max)
            assert np.array_equal(cnt, wc) and np.array_equal(ids, wi)
            assert np.array_equal(meas[..., 2], wm[..., 2])
            worst = max(worst, float(np.abs(meas[..., :2] - wm[..., :2]).max()))
            n += int(cnt.sum())
        print("device noise against pcw.philox_normal: max |du|, |dv| = %.3e px over %d tracks (bound %.3e)" % (worst, n, bound))
        assert n > 50
        assert worst <= bound
    finally:
        be.close()


def test_same_noise_whatever_the_batch(built):
    """a point's noise depends on (seed, frame, filter, point) alone: filters 0 .. 2 of a context of 64 filters produce the
    tracks of a context of 3, byte for byte"""
    npts = 257
    Xs = R.box_world(64, npts, 6)
    gsc = R.moving_poses(64, 2, 6)
    got = {}
    for B in (3, 64):
        be, cfg, _ = _backend(B, npts)
        try:
            be.set_world(Xs[:B])
            got[B] = []
            for t in range(2):
                be.make_tracks(gsc[t, :B], 1.0, 77, t)
                got[B].append(be.ctx.pcw_get_tracks(cfg.tracks_max, 0, 3))
        finally:
            be.close()
    for t in range(2):
        assert got[3][t][0].sum() > 0
        _same_tracks(got[64][t], got[3][t], t)


def _snapshot(be):
    P, scene = be.covariance(), be.scene()
    book = be.life_book()
    return [P.tobytes()] + [x.tobytes() for x in scene] + [x.tobytes() for x in book] + [be.life_stats().tobytes()]


def _packed(cnt, ids, meas):
    off = np.zeros(len(cnt) + 1, dtype=np.int32)
    off[1:] = np.cumsum(cnt)
    return (off, np.concatenate([ids[b, :cnt[b]] for b in range(len(cnt))]),
            np.concatenate([meas[b, :cnt[b]] for b in range(len(cnt))]))


def _frame_poses(sims, cfg, T):
    Rbc = pcw.so3_exp(cfg.Wbc)
    out = []
    for k in range(T):
        g = [np.concatenate([(s.gsb(0.4 + 0.002 * k)[0] @ Rbc).reshape(-1), s.gsb(0.4 + 0.002 * k)[0] @ cfg.Tbc + s.gsb(0.4 + 0.002 * k)[1]])
             for s in sims]
        out.append(np.array(g))
    return out


@pytest.mark.parametrize("alternate", [False, True])
def test_frames_on_device_tracks_equal_frames_on_the_same_tracks_uploaded(built, alternate):
    """6 frames, 2 filters, noise on. Context 1 runs pcw_tracks -> life_begin_tracks -> update -> absorb -> life_end
    (SequenceRunner.frame_world); context 2 is fed context 1's tracks through the host-track xivo_hip_life_begin. After every
    frame P, poses, groups, features, the book and xivo_life_stats are byte-equal. alternate: context 1 takes every other frame
    through xivo_hip_life_begin too (with the tracks it just produced and read back), so that the packed and the strided form
    of the track block follow each other on one context."""
    B, npts, T = 2, 300, 6
    Xs = R.box_world(B, npts, 8) * np.array([0.5, 0.5, 1.0]) + np.array([0.0, 3.0, 0.0])
    one, cfg, sims = _backend(B, npts, tracks_max=320)
    two, _, _ = _backend(B, npts, tracks_max=320, track_source="host")
    try:
        one.set_world(Xs)
        r1 = sequence.SequenceRunner(one, cfg, B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        admitted = 0
        for k, gsc in enumerate(_frame_poses(sims, cfg, T)):
            if alternate and k % 2 == 1:
                one.make_tracks(gsc, 1.0, 21, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)
                one.life_begin(*_packed(*tr))
                one.update(download=False)
                one.life_end()
            else:
                r1.frame_world(None, gsc, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)      # (the frame only read them: still in the block)
            assert tr[0].min() > 0
            two.life_begin(*_packed(*tr))
            two.update(download=False)
            two.life_end()
            assert _snapshot(one) == _snapshot(two), k
            admitted = int(one.life_stats()["admitted"].sum())
        assert admitted > 0 and int(one.life_stats()["updates"].sum()) > 0
    finally:
        one.close(); two.close()


def test_refusals_change_nothing(built):
    """XIVO_HIP_ERR_INVALID and nothing changed: pcw_config without a device life cycle; npts > tracks_max; a value that is not
    finite; life_begin_tracks without produced tracks, with another B, and a second time on the same tracks; pcw_tracks inside
    an open frame"""
    def refused(f, *a, **k):
        with pytest.raises(L.XivoHipError) as e:
            f(*a, **k)
        assert e.value.status == -1

    cam = (275.0, 275.0, 320.0, 240.0, 640.0, 480.0)
    cfg_h = sequence.SequenceConfig(**SMALL)
    sims = [pcw.TrajectorySim("lissajous", seed=b) for b in range(3)]
    H = sequence.HipBackend(cfg_h, 3, sequence.initial_poses(cfg_h, sims, t0=0.4), np.repeat(cfg_h.P_init()[None], 3, axis=0))
    try:
        refused(H.ctx.pcw_config, 64, *cam)
    finally:
        H.close()
    be, cfg, sims = _backend(3, 64, tracks_max=64)
    try:
        Xs = R.box_world(3, 64, 2)
        gsc = R.moving_poses(3, 2, 2)
        be.set_world(Xs)
        be.make_tracks(gsc[0], 0.0, 0, 0)
        before = (be.ctx.pcw_get_tracks(64), be.world_ids(), _snapshot(be))

        def unchanged():
            now = (be.ctx.pcw_get_tracks(64), be.world_ids(), _snapshot(be))
            _same_tracks(now[0], before[0], "tracks")
            assert np.array_equal(now[1][0], before[1][0]) and np.array_equal(now[1][1], before[1][1]) and now[2] == before[2]
        refused(be.ctx.pcw_config, 65, *cam)
        refused(be.ctx.pcw_config, 64, float("nan"), *cam[1:])
        refused(be.ctx.pcw_config, 64, *cam[:5], float("inf"))
        refused(be.ctx.life_begin_tracks, cfg.n_features, B=2)
        unchanged()
        be.life_begin_tracks()
        refused(be.make_tracks, gsc[1], 0.0, 0, 1)               # inside the open frame
        refused(be.ctx.life_begin_tracks, cfg.n_features, B=3)   # (and a frame cannot be opened twice)
        be.update(download=False)
        be.life_end()
        refused(be.ctx.life_begin_tracks, cfg.n_features, B=3)   # consumed: nothing produced since
        ids, nxt = be.world_ids()
        assert np.array_equal(ids, before[1][0]) and np.array_equal(nxt, before[1][1])
        # a host-track frame overwrites the block: no device tracks to read or to begin on
        be.life_begin(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros((0, 3)))
        be.update(download=False)
        be.life_end()
        refused(be.ctx.pcw_get_tracks, 64)
        refused(be.ctx.life_begin_tracks, cfg.n_features, B=3)
        # life_config releases the worlds with the block
        be.enable_device_lifecycle()
        refused(be.make_tracks, gsc[1], 0.0, 0, 1)
    finally:
        be.close()
    # a fresh context that never produced any
    be, cfg, _ = _backend(3, 64, tracks_max=64)
    try:
        refused(be.ctx.life_begin_tracks, cfg.n_features, B=3)
    finally:
        be.close()


def _ate(out):
    return np.sqrt(np.mean(np.sum((out["Tsb"] - out["gt_Tsb"]) ** 2, axis=2), axis=0))


def _books(out, B):
    return [tuple(x.tobytes() for x in out["estimator"].book(b)) for b in range(B)]


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_run_pcw_batch_device_tracks_against_host_tracks(built, sigma):
    """run_pcw_batch (the C++ estimator: VisualMeasDeviceWorld through xivo_amd/batch.py), 4 sequences, 10 frames, device life
    cycle: tracks from the device against BatchPCW(noise="philox") uploaded. Without noise Tsb and the books are byte-equal;
    with noise the books and the counters are equal and the ATE agrees to 1e-6 m (pixel differences of 1e-13 px cannot move
    it by a micrometre unless a decision flipped, which the equal books exclude)"""
    B = 4
    cfg = sequence.SequenceConfig(lifecycle="device")
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, B, total_time=0.4, noise_vision_std=sigma, track_source=src, noise="philox",
                                               noise_seed=5)
        st = {k: o["estimator"].stats() for k, o in outs.items()}
        assert _books(outs["device"], B) == _books(outs["host"], B)
        assert st["device"]["updates"] == st["host"]["updates"] > 0 and st["device"]["mh_rejected"] == st["host"]["mh_rejected"]
        assert len(outs["device"]["ts"]) == 10
        d = np.abs(_ate(outs["device"]) - _ate(outs["host"])).max()
        print("sigma %.1f: max |ATE device tracks - ATE host tracks| = %.3e m" % (sigma, d))
        if sigma == 0.0:
            assert outs["device"]["Tsb"].tobytes() == outs["host"]["Tsb"].tobytes()
        else:
            assert d <= 1e-6
    finally:
        for o in outs.values():
            o["estimator"].close()


def test_python_runner_device_tracks_against_the_cpp_estimator(built):
    """run_pcw with track_source="device" (SequenceRunner.frame_world) against the C++ estimator's VisualMeasDeviceWorld on
    the same worlds, sequences and seed: the same books and counters, Tsb within 1e-10 as between the two host sides today"""
    from xivo_amd.batch import BatchEstimator
    B, npts = 3, 500
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", npts=npts)
    mk = lambda: ([pcw.RandomPCW(npts=npts, seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    w, s = mk()
    py = sequence.run_pcw(sequence.HipBackend, cfg, w, s, total_time=0.4, noise_vision_std=1.0, noise_seed=3)
    w, s = mk()
    est = BatchEstimator(cfg, B, sequence.initial_poses(cfg, s), cfg.P_init())
    try:
        est.enable_device_world(np.array([x.Xs for x in w]))
        Rbc = pcw.so3_exp(cfg.Wbc)
        T = []
        for k in range(160):
            t = k * 0.0025
            m = [x.meas(t) for x in s]
            est.InertialMeas(t, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
            if k % 16 == 0:
                gsc = np.array([np.concatenate([(x.gsb(t)[0] @ Rbc).reshape(-1), x.gsb(t)[0] @ cfg.Tbc + x.gsb(t)[1]]) for x in s])
                est.VisualMeasDeviceWorld(t, gsc, 1.0, 3)
                T.append(est.gsb()[1])
        books = py["runner"].books
        for b in range(B):
            fid, fref, gref = est.book(b)
            assert list(fid) == books[b].feat_id and list(fref) == books[b].feat_ref and list(gref) == books[b].group_refs
        st = est.stats()
        assert st["updates"] == py["runner"].n_updates > 0 and st["mh_rejected"] == py["runner"].n_rejected
        assert np.abs(np.array(T) - py["Tsb"]).max() < 1e-10
    finally:
        py["backend"].close(); est.close()


def test_cpp_estimator_refuses_the_device_world_without_the_device_life_cycle(built):
    from xivo_amd.batch import BatchEstimator
    cfg = sequence.SequenceConfig()
    s = [pcw.TrajectorySim("lissajous", seed=b) for b in range(2)]
    est = BatchEstimator(cfg, 2, sequence.initial_poses(cfg, s), cfg.P_init())
    try:
        with pytest.raises(RuntimeError):
            est.enable_device_world(np.zeros((2, 10, 3)))
        with pytest.raises(RuntimeError):
            est.VisualMeasDeviceWorld(0.0, np.zeros((2, 12)), 0.0, 0)
    finally:
        est.close()


def test_run_pcw_cli_with_device_tracks(built):
    """run_pcw.py -vectorized -sequences 4 -lifecycle device -tracks device runs and reports; what check_lifecycle rejects is
    rejected before anything runs"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-vectorized", "-sequences", "4", "-total_time", "0.4"]
    out = subprocess.run(cmd + ["-lifecycle", "device", "-tracks", "device"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["tracks"] == "device" and rep["lifecycle"] == "device" and rep["updates"] > 0
    assert rep["ate_m"]["max"] < 0.2
    assert abs(rep["simulator_s"] - (rep["sim_imu_s"] + rep["sim_tracks_s"])) < 1e-9
    for bad in (["-tracks", "device"], ["-lifecycle", "device", "-tracks", "device", "-npts", "3000"]):
        out = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and "track_source" in out.stderr, out.stderr[-500:]


def test_map_log_on_device_tracks(built):
    """the landmark log on top of device tracks reads the world's ids from the device every frame: at noise 0 it names the same
    landmarks and gives the same anees_landmark as the host-track arm"""
    cfg = sequence.SequenceConfig(lifecycle="device")
    outs = {}
    for src in ("host", "device"):
        o = sequence.run_pcw_batch(cfg, 3, total_time=0.4, noise_vision_std=0.0, track_source=src, noise="philox", map_log=True)
        o["estimator"].close()
        outs[src] = o
    assert (outs["host"]["map"]["ids"] >= 0).any()
    assert np.array_equal(outs["host"]["map"]["ids"], outs["device"]["map"]["ids"])
    assert np.isfinite(outs["host"]["anees_landmark"])
    assert outs["device"]["anees_landmark"] == outs["host"]["anees_landmark"]
