"""GPU: the track faults of the device producer (xivo_hip_pcw_fault_*, the fault instances of pcw_tracks_kernel and
pcw_fault_score_kernel) against the numpy restatement BatchPCW.generate(faults=...) - which tests/test_pcw_faults_cpu.py holds
against the header under a host compiler -, the score against a host recomputation of its four cells, and the layers above."""
import numpy as np
import pytest

import pcw_camera_cases as CC
import pcw_fault_cases as FC
import pcw_restate as R
import test_pool_tracks_gpu as PT
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

SMALL = dict(n_groups=4, n_features=9, min_new_features=2)      # the layout of tests/test_pcw_tracks_gpu.py (N = 74)
FRAMES = 6
SIZES = [1, 63, 64, 65, 255, 256, 257]
RADTAN, RADTAN_R = pcw.SIM_CAMERAS["radtan"], 1.2


def _backend(B, npts, tracks_max=None, track_source="device", seed=0, **kw):
    cfg = sequence.SequenceConfig(lifecycle="device", track_source=track_source, npts=npts,
                                  tracks_max=npts if tracks_max is None else tracks_max, **{**SMALL, **kw})
    sims = [pcw.TrajectorySim("lissajous", seed=seed + b) for b in range(B)]
    poses = sequence.initial_poses(cfg, sims, t0=0.4)
    return sequence.HipBackend(cfg, B, poses, np.repeat(cfg.P_init()[None], B, axis=0)), cfg, sims


def _refused(f, *a, **k):
    with pytest.raises(L.XivoHipError) as e:
        f(*a, **k)
    assert e.value.status == -1


def _read(be, cfg, nb=None):
    nb = be.B if nb is None else nb
    return be.ctx.pcw_get_tracks(cfg.tracks_max, 0, nb) + (be.ctx.pcw_fault_flags(cfg.tracks_max, 0, nb),)


def _counters(be, nb=None):
    st = be.fault_stats()[:nb]
    return np.stack([st[k] for k in pcw.FAULT_COUNTERS], axis=1)


@pytest.fixture(scope="module")
def want():
    """the restatement of every (size, sticky) at noise 0 through the pinhole, computed once; and on it the assertion of
    tests/test_pcw_faults_cpu.py that the inputs hold every case"""
    cases = {n: FC.worlds(n, FRAMES) for n in SIZES}
    out = {(n, s): FC.restate(*cases[n], FC.faults(s)) for n in SIZES for s in (0, 1)}
    for s in (0, 1):
        FC.assert_coverage([out[(n, s)] for n in SIZES], s)
    return cases, out


@pytest.mark.parametrize("cam", ["pinhole", "radtan"])
@pytest.mark.parametrize("npts", SIZES)
def test_producer_against_the_restatement(built, want, npts, cam):
    """B = 3, tracks_max = npts, 6 frames, p_drop = p_outlier = p_tail = 0.2, offsets 20 - 60 px, sticky 0 and 1. At noise 0:
    counts, track ids, the worlds' ids and next_id, flags, z and the producer's five counters equal the restatement exactly, and
    u, v bit for bit through the pinhole. At sigma = 1 px ids, flags and counters are exact and the pixels lie within
    2 ulp(640) + 1e-13 sigma tail_scale (the bound of tests/test_pcw_tracks_gpu.py with sigma scaled by the tail: the sum with
    the offset is exact on both sides, only the normals' libm differs).
    Through the radial-tangential camera the numpy projection is not the device's to the bit: pcw_device.h leaves
    camera_project's statements to the build, which may fuse a product with a sum on the device. The fault path adds nothing to
    the projection but the restated offset, so there u and v are held to the device's own clean projection: a second context
    without faults on the same world, camera and poses gives u, v of every geometrically visible point in point order, and the
    faulty tracks must equal that plus the restated offset by bytes at noise 0, and within the bound above - no more - at
    sigma = 1. Against the numpy projection the pixels keep CC.CAP = 1e-9 px on top, the cap tests/test_pcw_camera_gpu.py holds
    both builds to; everything else stays exact."""
    cases, pin = want
    Xs, next_id, gsc = cases[npts]
    lens = None if cam == "pinhole" else RADTAN
    be, cfg, _ = _backend(3, npts)
    clean, dev_uv = None, []      # the distorted camera: the device's own noise-free u, v per frame, [3, npts, 2] (0: not visible)
    try:
        if lens is not None:
            be.ctx.pcw_camera(lens, RADTAN_R)
            clean, _, _ = _backend(3, npts)
            clean.ctx.pcw_camera(lens, RADTAN_R)
            clean.set_world(Xs, None, next_id)
        for sticky in (0, 1):
            o = FC.faults(sticky)
            for sigma in (0.0, 1.0):
                if lens is None and sigma == 0.0:
                    frames = pin[(npts, sticky)]
                else:
                    frames = FC.restate(Xs, next_id, gsc, o, sigma=sigma, cam=lens, max_radius=np.inf if lens is None else RADTAN_R)
                noise_bound = 0.0 if sigma == 0.0 else 2 * np.spacing(640.0) + 1e-13 * sigma * o["tail_scale"]
                bound = noise_bound + (0.0 if lens is None else CC.CAP)
                be.set_world(Xs, None, next_id)
                be.set_track_faults(o)
                worst, worst_dev = 0.0, 0.0
                for t, w in enumerate(frames):
                    tag = (npts, cam, sticky, sigma, t)
                    if clean is not None and len(dev_uv) == t:
                        clean.make_tracks(gsc[t], 0.0, 0, t)
                        c_cnt, _, c_meas = clean.ctx.pcw_get_tracks(cfg.tracks_max, 0, 3)
                        assert np.array_equal(c_cnt, w["geo"].sum(axis=1)), tag
                        uv = np.zeros((3, npts, 2))
                        for b in range(3):
                            uv[b, w["geo"][b]] = c_meas[b, :c_cnt[b], :2]
                        dev_uv.append(uv)
                    be.make_tracks(gsc[t], sigma, FC.SEED, t)
                    cnt, ids, meas, flags = _read(be, cfg)
                    wc, wi, wm, wf = FC.strided(w, cfg.tracks_max)
                    assert np.array_equal(cnt, wc) and np.array_equal(ids, wi) and np.array_equal(flags, wf), tag
                    wids, nxt = be.world_ids()
                    assert np.array_equal(wids, w["ids"]) and np.array_equal(nxt, w["next_id"]), tag
                    assert np.array_equal(_counters(be), w["counters"]), tag
                    assert meas[..., 2].tobytes() == wm[..., 2].tobytes(), tag
                    if bound == 0.0:
                        assert meas.tobytes() == wm.tobytes(), tag
                    else:
                        worst = max(worst, float(np.abs(meas[..., :2] - wm[..., :2]).max()))
                    if clean is not None:      # the device's projection + the restated offset (+ the restated noise)
                        exp = dev_uv[t] + w["offset"]
                        if sigma != 0.0:
                            exp = exp + (sigma * w["scale"])[..., None] * pcw.philox_normal(FC.SEED, t, np.arange(3)[:, None], np.arange(npts)[None, :])
                        for b in range(3):
                            got, e = meas[b, :cnt[b], :2], exp[b, w["vis"][b]]
                            if sigma == 0.0:
                                assert got.tobytes() == e.tobytes(), tag + (b,)
                            elif cnt[b]:
                                worst_dev = max(worst_dev, float(np.abs(got - e).max()))
                if clean is not None and sigma != 0.0:
                    print("npts %d %s sticky %d sigma %.0f: against the device's projection max |du|, |dv| = %.3e px (bound %.3e)"
                          % (npts, cam, sticky, sigma, worst_dev, noise_bound))
                    assert worst_dev <= noise_bound
                if bound:
                    print("npts %d %s sticky %d sigma %.0f: max |du|, |dv| = %.3e px (bound %.3e)" % (npts, cam, sticky, sigma, worst, bound))
                    assert worst <= bound
    finally:
        be.close()
        if clean is not None:
            clean.close()


def test_off_is_off(built):
    """a context whose faults were never configured, one that ran a faulty frame and then released them, and the restatement
    without faults (tests/pcw_restate.py): the same tracks, bytes, at noise 0; and the two contexts the same at sigma = 1"""
    npts = 257
    Xs, next_id, gsc = FC.worlds(npts, 4)
    never, cfg, _ = _backend(3, npts)
    was, _, _ = _backend(3, npts)
    try:
        was.set_world(Xs, None, next_id)
        was.set_track_faults(FC.faults(1))
        was.stream_share(2)
        was.make_tracks(gsc[0], 1.0, 3, 0)
        assert was.fault_flags().any()
        was.set_track_faults(None)
        was.stream_share(0)
        _refused(was.ctx.pcw_fault_flags, npts)
        _refused(was.ctx.pcw_fault_stats)
        for sigma in (0.0, 1.0):
            never.set_world(Xs, None, next_id); was.set_world(Xs, None, next_id)
            rs = R.Restate(Xs, None, next_id)
            for t in range(4):
                never.make_tracks(gsc[t], sigma, 77, t); was.make_tracks(gsc[t], sigma, 77, t)
                a, b = never.ctx.pcw_get_tracks(npts, 0, 3), was.ctx.pcw_get_tracks(npts, 0, 3)
                assert a[0].sum() > 100
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes(), (sigma, t)
                if sigma == 0.0:
                    for x, y in zip(a, R.strided(rs.step(gsc[t]), npts)):
                        assert x.tobytes() == y.tobytes(), t
                for x, y in zip(never.world_ids(), was.world_ids()):
                    assert np.array_equal(x, y)
    finally:
        never.close(); was.close()


def test_same_tracks_whatever_the_batch_and_shared_streams(built):
    """filters 0 .. 2 of a context of 64 produce the faulty tracks and flags of a context of 3, bytes; with stream_share(3) over
    worlds and poses tiled with period 3, filters b and b + 3 are equal - and filter 3 is then not what it is on its own stream"""
    npts = 257
    Xs3, _, gsc3 = FC.worlds(npts, 3)
    Xs, gsc = np.tile(Xs3, (22, 1, 1))[:64], np.tile(gsc3, (1, 22, 1))[:, :64]
    o = FC.faults(1)
    got = {}
    for B in (3, 64):
        be, cfg, _ = _backend(B, npts)
        try:
            be.set_world(Xs[:B])
            be.set_track_faults(o)
            got[B] = []
            for t in range(3):
                be.make_tracks(gsc[t, :B], 1.0, 77, t)
                got[B].append(_read(be, cfg))
            if B == 64:
                be.set_world(Xs)
                be.set_track_faults(o)
                be.stream_share(3)
                shared = []
                for t in range(3):
                    be.make_tracks(gsc[t], 1.0, 77, t)
                    shared.append(_read(be, cfg))
                st = be.fault_stats()
        finally:
            be.close()
    for t in range(3):
        assert got[3][t][0].sum() > 100 and got[3][t][3].any()
        for x, y in zip(got[64][t], got[3][t]):
            assert x[:3].tobytes() == y.tobytes(), t
        for x, own in zip(shared[t], got[64][t]):
            assert x[3:].tobytes() == x[:-3].tobytes(), t
            assert x[:3].tobytes() == own[:3].tobytes(), t                # (filters 0 .. 2 draw their own words either way)
    assert any(shared[t][3][3].tobytes() != got[64][t][3][3].tobytes() for t in range(3))
    assert st[3:].tobytes() == st[:-3].tobytes()


def _packed(cnt, ids, meas):
    return PT._packed(cnt, ids, meas)


def _snapshot(be):
    P, scene = be.covariance(), be.scene()
    return [P.tobytes()] + [x.tobytes() for x in scene] + [x.tobytes() for x in be.life_book()] + [be.life_stats().tobytes()]


def _frame_poses(sims, cfg, T):
    Rbc = pcw.so3_exp(cfg.Wbc)
    out = []
    for k in range(T):
        g = [s.gsb(0.4 + 0.002 * k) for s in sims]
        out.append(np.array([np.concatenate([(Rsb @ Rbc).reshape(-1), Rsb @ cfg.Tbc + Tsb]) for Rsb, Tsb in g]))
    return out


def _life_world(B, npts):
    return R.box_world(B, npts, 8) * np.array([0.5, 0.5, 1.0]) + np.array([0.0, 3.0, 0.0])   # (tests/test_pcw_tracks_gpu.py)


def test_immediate_frames_on_faulty_device_tracks_equal_the_same_tracks_uploaded(built):
    """6 frames, 2 filters, sigma = 1, sticky faults: context 1 runs pcw_tracks -> life_begin_tracks -> update -> score ->
    life_end (SequenceRunner.frame_world), context 2 is fed context 1's tracks through the host-track xivo_hip_life_begin. After
    every frame P, the scene, the book and xivo_life_stats are byte-equal: the score reads and changes nothing of the frame"""
    B, npts, T = 2, 300, 6
    one, cfg, sims = _backend(B, npts, tracks_max=320, track_faults=FC.faults(1))
    two, _, _ = _backend(B, npts, tracks_max=320, track_source="host")
    try:
        one.set_world(_life_world(B, npts))
        r1 = sequence.SequenceRunner(one, cfg, B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        for k, gsc in enumerate(_frame_poses(sims, cfg, T)):
            r1.frame_world(None, gsc, k)
            tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, B)
            assert tr[0].min() > 0
            two.life_begin(*_packed(*tr)); two.update(download=False); two.life_end()
            assert _snapshot(one) == _snapshot(two), k
        st, fs = one.life_stats(), one.fault_stats()
        assert int(st["admitted"].sum()) > 0 and int(st["updates"].sum()) > 0
        assert int(fs["outlier_events"].sum()) > 0 and int(fs["dropped"].sum()) > 0
        assert int(sum(fs[k].sum() for k in ("outlier_rejected", "outlier_kept", "nominal_rejected", "nominal_kept"))) > 0
    finally:
        one.close(); two.close()


def test_pool_frames_on_faulty_device_tracks_equal_the_same_tracks_uploaded(built):
    """the same on the sub-filter life cycle (the scheme of tests/test_pool_tracks_gpu.py): frames on faulty produced tracks,
    scored, against a second context fed the same tracks through xivo_hip_pool_life_begin, byte-equal after every frame"""
    one, cfg, sims = PT._backend(track_faults=FC.faults(1))
    two, _, _ = PT._backend(track_source="host")
    try:
        r1 = sequence.SequenceRunner(one, cfg, PT.B)
        r1.noise_px_std, r1.noise_seed = 1.0, 21
        for k, (rec, gsc) in enumerate(PT._host_frames(cfg, sims)):
            r1.frame_world(rec, gsc, k)
            tr = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, PT.B)
            if rec is not None:
                two.propagate(rec)
            two.pool_life_begin(*PT._packed(*tr), k + 1 >= cfg.strict_criteria_timesteps)
            two.update(download=False)
            two.pool_life_end()
            PT._same(PT._snapshot(one), PT._snapshot(two), "frame %d" % k)
        st, fs = one.pool_life_stats(), one.fault_stats()
        assert st["pool_added"].sum() > 0 and st["updates"].sum() > 0 and int(fs["outlier_events"].sum()) > 0
    finally:
        one.close(); two.close()


CELLS = ("outlier_rejected", "outlier_kept", "nominal_rejected", "nominal_kept")


@pytest.mark.parametrize("life", ["immediate", "pool"])
def test_score_against_the_host(built, life):
    """10 frames on sticky faulty tracks at sigma = 1: after every update the mask, the book's feat_id and the tracks' ids and
    flags are read, the four cells recomputed on the host (a slot that holds an id, the last track with that id, pcw.fault_cell)
    and compared with the change of the device's counters - integers, exact; the producer's counters do not move under the
    score, and outlier_rejected + outlier_kept > 0 over the run"""
    T = 10
    o = FC.faults(1, p_drop=0.05)
    if life == "immediate":
        B = 4
        be, cfg, sims = _backend(B, 300, tracks_max=320, track_faults=o)
        be.set_world(_life_world(B, 300))
        frames = [(None, g) for g in _frame_poses(sims, cfg, T)]
    else:
        B = PT.B
        be, cfg, sims = PT._backend(track_faults=o)
        frames = list(PT._host_frames(cfg, sims))
        frames = frames + frames[-1:] * (T - len(frames))       # (the camera rests on its last pose: the tracks still change)
        frames = [(rec if k < PT.T else None, g) for k, (rec, g) in enumerate(frames)]
    try:
        total = np.zeros(4, dtype=np.int64)
        for k, (rec, gsc) in enumerate(frames):
            if rec is not None:
                be.propagate(rec)
            be.make_tracks(gsc, 1.0, 21, k)
            cnt, ids, _, flags = _read(be, cfg)
            if life == "immediate":
                be.life_begin_tracks()
            else:
                be.pool_life_begin_tracks(k + 1 >= cfg.strict_criteria_timesteps)
            mask = be.update(download=True)
            feat_id = be.life_book()[0] if life == "immediate" else be.pool_life_book()["feat_id"]
            before = be.fault_stats()
            be.fault_score()
            after = be.fault_stats()
            be.life_end() if life == "immediate" else be.pool_life_end()
            exp = np.zeros((B, 4), dtype=np.int64)
            for b in range(B):
                for j in range(cfg.n_features):
                    hit = np.nonzero(ids[b, :cnt[b]] == feat_id[b, j])[0] if feat_id[b, j] >= 0 else []
                    if len(hit):
                        exp[b, pcw.fault_cell(int(mask[b, j]), int(flags[b, hit[-1]]))] += 1
            got = np.stack([after[c] - before[c] for c in CELLS], axis=1)
            assert np.array_equal(got, exp), (k, got.tolist(), exp.tolist())
            for c in pcw.FAULT_COUNTERS:
                assert np.array_equal(after[c], before[c])
            total += exp.sum(axis=0)
        print("%s: outlier rejected / kept %d / %d, nominal rejected / kept %d / %d" % ((life,) + tuple(total)))
        assert total[0] + total[1] > 0 and total.sum() > 20
    finally:
        be.close()


def test_refusals_change_nothing(built):
    """XIVO_HIP_ERR_INVALID from xivo_hip_pcw_fault_config - no worlds, a frame open, a wrong struct_size, a probability outside
    [0, 1] or a sum above 1, outlier_min_px < 0 or > outlier_max_px, tail_scale < 1 or not finite, any value not finite, sticky
    outside {0, 1} - and from xivo_hip_pcw_fault_score - faults off, no frame open, another B, a frame on uploaded tracks, twice
    in a frame; afterwards the context produces and counts what a twin that never saw the calls does"""
    o = FC.faults(1)
    H, _, _ = _backend(3, 64, track_source="host")
    try:
        _refused(H.ctx.pcw_fault_config, o)                      # no worlds configured
        _refused(H.ctx.pcw_stream_share, 2)
    finally:
        H.close()
    Xs, next_id, gsc = FC.worlds(64, 3)
    be, cfg, _ = _backend(3, 64)
    twin, _, _ = _backend(3, 64)
    try:
        for x in (be, twin):
            x.set_world(Xs, None, next_id)
            x.set_track_faults(o)
            x.make_tracks(gsc[0], 1.0, 9, 0)
        raw = np.zeros(1, dtype=L.pcw_fault_opts_dtype)
        for k, v in o.items():
            raw[k] = v
        raw["struct_size"] = L.pcw_fault_opts_dtype.itemsize - 8
        assert be.ctx.lib.xivo_hip_pcw_fault_config(be.ctx.h, raw.ctypes.data) == -1
        bad = (dict(p_drop=-0.1), dict(p_outlier=1.5), dict(p_drop=0.5, p_outlier=0.4, p_tail=0.2), dict(outlier_min_px=-1.0),
               dict(outlier_min_px=70.0), dict(tail_scale=0.5), dict(tail_scale=float("inf")), dict(tail_scale=float("nan")),
               dict(p_tail=float("nan")), dict(outlier_max_px=float("inf")), dict(sticky=2), dict(sticky=-1))
        for kw in bad:
            _refused(be.ctx.pcw_fault_config, dict(o, **kw))
        _refused(be.ctx.pcw_stream_share, -1)
        _refused(be.fault_score)                                 # no frame open
        for x in (be, twin):
            x.life_begin_tracks()
        _refused(be.ctx.pcw_fault_config, o)                     # a frame open
        _refused(be.ctx.pcw_fault_config, None)
        _refused(be.ctx.pcw_stream_share, 2)
        _refused(be.ctx.pcw_fault_score, 2)                      # not the open frame's B
        for x in (be, twin):
            x.update(download=False)
            x.fault_score()
        _refused(be.fault_score)                                 # twice in a frame
        for x in (be, twin):
            x.life_end()
        _refused(be.fault_score)                                 # the frame is closed
        # a frame on uploaded tracks is not scored
        for x in (be, twin):
            x.life_begin(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros((0, 3)))
            x.update(download=False)
        _refused(be.fault_score)
        for x in (be, twin):
            x.life_end()
            x.make_tracks(gsc[1], 1.0, 9, 1)
        for a, b in zip(_read(be, cfg), _read(twin, cfg)):
            assert a.tobytes() == b.tobytes()
        assert be.fault_stats().tobytes() == twin.fault_stats().tobytes() and int(be.fault_stats()["tracks"].sum()) > 0
        assert _snapshot(be) == _snapshot(twin)
        # with faults off the score is refused inside a frame too
        be.set_track_faults(None)
        be.make_tracks(gsc[2], 1.0, 9, 2)
        be.life_begin_tracks(); be.update(download=False)
        _refused(be.ctx.pcw_fault_score, 3)
        be.life_end()
        # whatever releases the worlds releases the faults
        twin.enable_device_lifecycle()
        _refused(twin.ctx.pcw_fault_stats)
    finally:
        be.close(); twin.close()


def _books(out, B):
    return [tuple(x.tobytes() for x in out["estimator"].book(b)) for b in range(B)]


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_run_pcw_batch_faulty_device_tracks_against_host_tracks(built, sigma):
    """run_pcw_batch (the C++ estimator), 8 sequences, 2 s, lifecycle="device", p_outlier = 0.05 at 20 - 60 px: tracks from the
    device against BatchPCW(noise="philox", faults=...) uploaded. The books and the counters are equal, at sigma = 0 Tsb is
    byte-equal too; both arms report the same producer counters, the device arm the four cells as well. The gate rejects
    (rejected > 0) - and on the same seeds without faults it rejects nothing, the project's measured behaviour on clean tracks"""
    B = 8
    o = dict(p_outlier=0.05, outlier_min_px=20.0, outlier_max_px=60.0)
    cfg = sequence.SequenceConfig(lifecycle="device", track_faults=o)
    outs = {}
    try:
        for src in ("host", "device"):
            outs[src] = sequence.run_pcw_batch(cfg, B, total_time=2.0, noise_vision_std=sigma, track_source=src, noise="philox", noise_seed=5)
        st = {k: x["estimator"].stats() for k, x in outs.items()}
        assert _books(outs["device"], B) == _books(outs["host"], B)
        assert st["device"]["updates"] == st["host"]["updates"] > 0 and st["device"]["mh_rejected"] == st["host"]["mh_rejected"]
        if sigma == 0.0:
            assert outs["device"]["Tsb"].tobytes() == outs["host"]["Tsb"].tobytes()
        fd, fh = outs["device"]["fault_stats"], outs["host"]["fault_stats"]
        for k in pcw.FAULT_COUNTERS:
            assert np.array_equal(fd["per_filter"][k], fh["per_filter"][k]), k
        print("sigma %.0f: rejected %d; %s" % (sigma, st["device"]["mh_rejected"], fd["sum"]))
        assert fd["sum"]["outlier_events"] > 0 and fd["sum"]["outlier_rejected"] + fd["sum"]["outlier_kept"] > 0
        assert st["device"]["mh_rejected"] > 0
        if sigma == 1.0:
            clean = sequence.run_pcw_batch(sequence.SequenceConfig(lifecycle="device"), B, total_time=2.0, noise_vision_std=sigma,
                                           track_source="device", noise_seed=5)
            outs["clean"] = clean
            assert "fault_stats" not in clean and clean["estimator"].stats()["mh_rejected"] == 0
    finally:
        for x in outs.values():
            x["estimator"].close()


def test_sweep_on_device_tracks_equals_plain_runs(built):
    """sweep.run_sweep(track_source="device") at T = 3 tunings x W = 2 worlds, sticky faults on, against three plain device-track
    runs of the same two worlds under stream_share(2) (sweep.run_plain), compared by bytes as tests/test_tune_sequence_gpu.py
    compares the host-track sweep: the final state, the trajectory and innovation logs, the scores, the fault counters; the
    summary carries the four sums of the score and `dropped` per tuning"""
    import test_tune_sequence_gpu as TS
    from xivo_amd import sweep
    o = dict(sticky=1, p_drop=0.02, p_outlier=0.1, outlier_min_px=20.0, outlier_max_px=60.0)
    cfg = sequence.SequenceConfig(lifecycle="device", n_groups=4, n_features=8, tracks_max=128, track_faults=o)
    kw = dict(TS.KW, track_source="device", noise_seed=11)
    sw = sweep.run_sweep(cfg, TS.AXES, TS.W, **kw)
    try:
        final, logs, fs = TS._final(sw), TS._logs(sw), sw["fault_stats"]
    finally:
        sw["backend"].close()
    plain = []
    for c in sw["cfgs"]:
        out = sweep.run_plain(c, TS.W, **kw)
        try:
            plain.append((TS._final(out), TS._logs(out), out["fault_stats"]))
        finally:
            out["backend"].close()
    for k, got in final.items():
        want = np.concatenate([p[0][k] for p in plain])
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    for k, got in logs.items():
        want = np.ascontiguousarray(np.concatenate([p[1][k] for p in plain], axis=1))
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    assert fs.tobytes() == np.concatenate([p[2] for p in plain]).tobytes()
    assert final["P"][:TS.W].tobytes() != final["P"][2 * TS.W:].tobytes()              # the tunings did part
    # every tuning saw the same tracks: the producer's counters repeat with period W
    for k in pcw.FAULT_COUNTERS:
        assert np.array_equal(fs[k].reshape(TS.T, TS.W), np.tile(fs[k][:TS.W], (TS.T, 1))), k
    assert int(fs["outlier_events"].sum()) > 0 and int(fs["dropped"].sum()) > 0
    for t, row in enumerate(sw["summary"]):
        s = slice(t * TS.W, (t + 1) * TS.W)
        for k in CELLS + ("dropped",):
            assert row[k] == int(fs[k][s].sum()), (t, k)
    assert sum(r["outlier_rejected"] + r["outlier_kept"] for r in sw["summary"]) > 0
