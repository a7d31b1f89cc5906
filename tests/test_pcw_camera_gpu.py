"""GPU: the track producer through the estimator's camera models (xivo_hip_pcw_camera, pcw_tracks_kernel<model>) against the
restatements of tests/pcw_camera_cases.py - decisions, ids and depths exact, pixels within four times the host build's own
error against the 80-bit restatement (measured here, on these inputs, and itself below 1e-9 px) - and the layers above it: the
pool life cycle on an equidistant camera's tracks against the same tracks uploaded, run_pcw_batch with both track sources."""
import numpy as np
import pytest

import pcw_camera_cases as CC
import test_pool_tracks_gpu as PT
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu


def _context(cam=None, max_radius=np.inf):
    """3 filters with the immediate device life cycle (the smallest that owns a track block) and worlds of 257 points behind
    the default pinhole; cam: xivo_hip_pcw_camera on top"""
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", npts=CC.NPTS, tracks_max=CC.NPTS, n_groups=2,
                                  n_features=4, min_new_features=2)
    sims = [pcw.TrajectorySim("lissajous", seed=b) for b in range(CC.B)]
    be = sequence.HipBackend(cfg, CC.B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], CC.B, axis=0))
    if cam is not None:
        be.ctx.pcw_camera(cam, max_radius)
    return be, cfg


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcw_camera_gpu")
    return d, CC.build_driver(d)


@pytest.mark.parametrize("model", CC.MODELS)
def test_tracks_against_the_restatements(built, driver, model):
    """npts = tracks_max = 257 (two chunks, the second with one point), B = 3, 3 frames, the guard on and removing points:
    counts, track ids, the worlds' ids and next_id equal the restatement exactly, z bit for bit, u and v within the bound. The
    inputs keep every pixel of the 80-bit restatement more than 1e-6 px from the borders and every radius more than 1e-9 from
    max_radius (asserted), so no decision hangs on the last places"""
    tmp, exe = driver
    c = CC.case(model)
    CC.assert_margins(c)
    ref = CC.host_error(exe, tmp, c)
    bound = 4 * ref
    assert 0 < bound <= CC.CAP
    be, cfg = _context(c["cam"], c["max_radius"])
    walk = CC.Walk(c)
    worst, seen, removed = 0.0, 0, 0
    try:
        be.set_world(c["Xs"])
        for t in range(CC.T):
            be.make_tracks(c["gsc"][t], 0.0, 5, t)
            cnt, ids, meas = be.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B)
            r = walk.step(t, cfg.tracks_max)
            wids, nxt = be.world_ids()
            assert np.array_equal(cnt, r["cnt"]) and np.array_equal(ids, r["track_ids"]), t
            assert np.array_equal(wids, r["ids"]) and np.array_equal(nxt, r["next_id"]), t
            assert meas[..., 2].tobytes() == r["meas"][..., 2].tobytes(), t
            vis, u, v, _ = CC.project(c, t, CC.LD)
            for b in range(CC.B):
                k = np.nonzero(vis[b])[0]
                assert len(k) == cnt[b]
                worst = max(worst, float(np.abs(meas[b, :cnt[b], 0] - u[b, k]).max()), float(np.abs(meas[b, :cnt[b], 1] - v[b, k]).max()))
            seen += int(cnt.sum())
            removed += int(CC.project(c, t, max_radius=np.inf)[0].sum() - cnt.sum())
        print("%s: against the 80-bit restatement max |du|, |dv|: host build %.3e px, device %.3e px (bound %.3e px) over %d tracks; "
              "the guard removed %d" % (model, ref, worst, bound, seen, removed))
        assert seen > 50 and removed > 0
        assert worst <= bound
    finally:
        be.close()


def test_noise_and_ranks_are_those_of_the_pinhole_kernel(built):
    """sigma = 1 px through the equidistant camera: the noise added to a track's pixel is the stream of pcw.philox_normal for
    (seed, frame, filter, point), as without a camera (the bound of tests/test_pcw_tracks_gpu.py on the sum, plus the pixel's
    own of this file measured at sigma = 0 on the same context)"""
    c = CC.case("equi")
    be, cfg = _context(c["cam"], c["max_radius"])
    other, _ = _context(c["cam"], c["max_radius"])
    try:
        be.set_world(c["Xs"]); other.set_world(c["Xs"])
        be.make_tracks(c["gsc"][0], 1.0, 1234567890123, 7)
        other.make_tracks(c["gsc"][0], 0.0, 0, 7)
        cnt, ids, meas = be.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B)
        cnt0, ids0, meas0 = other.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B)
        assert np.array_equal(cnt, cnt0) and np.array_equal(ids, ids0) and cnt.sum() > 20
        vis = CC.project(c, 0)[0]
        bound = 2 * np.spacing(640.0) + 1e-13
        for b in range(CC.B):
            k = np.nonzero(vis[b])[0]
            n = pcw.philox_normal(1234567890123, 7, b, k)
            assert np.abs(meas[b, :cnt[b], :2] - (meas0[b, :cnt[b], :2] + 1.0 * n)).max() <= bound
            assert np.array_equal(meas[b, :cnt[b], 2], meas0[b, :cnt[b], 2])
    finally:
        be.close(); other.close()


def test_back_to_the_pinhole(built):
    """cam = NULL after a distorted frame: the tracks of the next frames are byte-equal to those of a context that never set a
    camera and whose worlds were handed the ids the distorted frame left"""
    c = CC.case("equi")
    one, cfg = _context(c["cam"], c["max_radius"])
    two, _ = _context()
    try:
        one.set_world(c["Xs"])
        one.make_tracks(c["gsc"][0], 1.0, 9, 0)
        ids, nxt = one.world_ids()
        two.set_world(c["Xs"], ids, nxt)
        one.ctx.pcw_camera(None)
        for t in (1, 2):
            one.make_tracks(c["gsc"][t], 1.0, 9, t)
            two.make_tracks(c["gsc"][t], 1.0, 9, t)
            a, b = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B), two.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B)
            assert a[0].sum() > 20
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), t
            for x, y in zip(one.world_ids(), two.world_ids()):
                assert np.array_equal(x, y)
    finally:
        one.close(); two.close()


def test_camera_refusals_change_nothing(built):
    """XIVO_HIP_ERR_INVALID: without worlds, inside an open frame, an unknown model, max_radius NaN / 0 / negative, a coefficient
    that is not finite, no image - and the camera in use stays"""
    c = CC.case("atan")
    cam = c["cam"]
    with L.Context(47, 8, 2) as ctx:
        PT._refused(ctx.pcw_camera, cam, 1.0)                       # no worlds
    be, cfg = _context(cam, c["max_radius"])
    try:
        be.set_world(c["Xs"])
        be.make_tracks(c["gsc"][0], 0.0, 0, 0)
        keep = be.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B)
        for bad_r in (float("nan"), 0.0, -1.0):
            PT._refused(be.ctx.pcw_camera, cam, bad_r)
        PT._refused(be.ctx.pcw_camera, dict(cam, model=4), 1.0)
        PT._refused(be.ctx.pcw_camera, dict(cam, d=[float("inf")]), 1.0)
        PT._refused(be.ctx.pcw_camera, dict(cam, fx=float("nan")), 1.0)
        PT._refused(be.ctx.pcw_camera, dict(cam, rows=0), 1.0)
        be.life_begin_tracks()
        PT._refused(be.ctx.pcw_camera, cam, 1.0)                    # inside the open frame
        PT._refused(be.ctx.pcw_camera, None)
        be.update(download=False)
        be.life_end()
        be.set_world(c["Xs"])                                       # the same world again: the same frame must come out
        be.make_tracks(c["gsc"][0], 0.0, 0, 0)
        for x, y in zip(be.ctx.pcw_get_tracks(cfg.tracks_max, 0, CC.B), keep):
            assert x.tobytes() == y.tobytes()
    finally:
        be.close()


EQUI = pcw.SIM_CAMERAS["equi"]


@pytest.mark.parametrize("alternate", [False, True])
def test_pool_life_frames_on_an_equidistant_camera(built, alternate):
    """the scheme of tests/test_pool_tracks_gpu.py end to end with cfg.cam equidistant (the producer, the update's Jacobians and
    the new entries' un-projection all go through it): frames on produced tracks against a second context fed the same tracks
    read back through xivo_hip_pool_life_begin, byte-equal after every frame"""
    one, cfg, sims = PT._backend(cam=EQUI, pcw_max_radius=1.3)
    two, _, _ = PT._backend(track_source="host", cam=EQUI)
    try:
        r1 = sequence.SequenceRunner(one, cfg, PT.B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        for k, (rec, gsc) in enumerate(PT._host_frames(cfg, sims)):
            strict = k + 1 >= cfg.strict_criteria_timesteps
            if alternate and k % 2 == 1:
                one.propagate(rec)
                one.make_tracks(gsc, 1.0, 21, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, PT.B)
                r1.vision_counter += 1
                one.pool_life_begin(*PT._packed(*tr), strict)
                one.update(download=False)
                one.pool_life_end()
            else:
                r1.frame_world(rec, gsc, k)
                tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, PT.B)
            if k == 0:      # the producer saw the equidistant camera: the restatement names the same tracks
                g = gsc
                vis = pcw.project_points_cam(PT.frustum_world(cfg, sims, PT.NPTS, 3), g[:, :9].reshape(-1, 3, 3), g[:, 9:], EQUI, 1.3)[0]
                assert np.array_equal(tr[0], vis.sum(axis=1))
            if rec is not None:
                two.propagate(rec)
            two.pool_life_begin(*PT._packed(*tr), strict)
            two.update(download=False)
            two.pool_life_end()
            PT._same(PT._snapshot(one), PT._snapshot(two), "frame %d" % k)
        st = one.pool_life_stats()
        print("equidistant: admitted %d, pool added %d, updates %d" % (st["admitted"].sum(), st["pool_added"].sum(), st["updates"].sum()))
        assert st["pool_added"].sum() > 0 and st["updates"].sum() > 0
    finally:
        one.close(); two.close()


def test_run_pcw_cli_with_a_camera_model(built):
    """run_pcw.py -cam-model equi runs the sub-filter life cycle on device tracks and reports; a distorted camera with the
    immediate life cycle is refused before anything runs"""
    import json, os, subprocess, sys
    cmd = [sys.executable, os.path.join(CC.ROOT, "scripts", "run_pcw.py"), "-vectorized", "-sequences", "4", "-total_time", "1.2",
           "-npts", "300", "-cam-model", "equi", "-max-radius", "1.3"]
    out = subprocess.run(cmd + ["-feature_init", "subfilter", "-pool-lifecycle", "device", "-tracks", "device"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["cam_model"] == "equi" and rep["tracks"] == "device" and rep["updates"] > 0
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "subfilter" in out.stderr


def test_run_pcw_batch_equidistant_device_tracks_against_host_tracks(built):
    """run_pcw_batch with cfg.cam equidistant, sigma = 1 px: the device's tracks against BatchPCW(noise="philox") projecting
    through the same camera (project_points_cam) - books and counters equal"""
    n = 4
    cfg = sequence.SequenceConfig(pool_lifecycle="device", cam=EQUI, pcw_max_radius=1.3, **PT.SEQ)
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, n, total_time=0.4, noise_vision_std=1.0, track_source=src, noise="philox",
                                               noise_seed=5)
        c = {k: PT._counters(o) for k, o in outs.items()}
        print("equidistant, counters %s" % (c["device"],))
        assert PT._books(outs["device"], n) == PT._books(outs["host"], n)
        assert c["device"] == c["host"] and c["device"]["updates"] > 0
    finally:
        for o in outs.values():
            o["estimator"].close()
