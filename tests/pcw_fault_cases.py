"""Shared by tests/test_pcw_faults_cpu.py and tests/test_pcw_faults_gpu.py (not a test module): the options, worlds and frames the
track-fault tests run, the restatement (BatchPCW.generate(faults=...), xivo_amd/pcw.py) frame by frame in the per-point and the
per-track forms the comparisons need, and the assertion that the inputs hold every case they were chosen for."""
import numpy as np

import pcw_restate as R
from xivo_amd import pcw

# the issue's probabilities and offsets; tail_scale 4 makes a tail event visible at sigma = 1 px
FAULTS = dict(p_drop=0.2, p_outlier=0.2, p_tail=0.2, outlier_min_px=20.0, outlier_max_px=60.0, tail_scale=4.0)
SEED = 20240607


def faults(sticky, **kw):
    return pcw.fault_opts(FAULTS, sticky=sticky, **kw)


def worlds(npts, frames, seed=None):
    """3 filters -> (Xs [3, npts, 3], next_id [3], gsc [frames, 3, 12]): filter 0 a box world under a camera that pans and drifts
    (points leave and enter the image on their own), filters 1 and 2 cones in front of cameras that barely move (every point
    geometrically visible in every frame, so that a track ends by a drop alone); ids of filter 0 from 2^33 + 5"""
    seed = npts if seed is None else seed
    rng = np.random.default_rng(seed)
    Xs = np.zeros((3, npts, 3))
    Xs[0] = rng.uniform([-6, -6, 2], [6, 6, 9], size=(npts, 3))
    for b in (1, 2):
        z = rng.uniform(3.0, 6.0, size=npts)
        Xs[b] = np.stack([rng.uniform(-0.5, 0.5, npts) * z, rng.uniform(-0.4, 0.4, npts) * z, z], axis=1)
    gsc = np.zeros((frames, 3, 12))
    for t in range(frames):
        gsc[t, 0] = R.gsc_of(pcw.so3_exp(np.array([0.0, 0.05 * t, 0.01 * t])), [0.05 * t, 0.0, 0.0])[0]
        gsc[t, 1] = R.gsc_of(pcw.so3_exp(np.array([0.01 * t, -0.02 * t, 0.005])), [0.02 * t, -0.01 * t, 0.03 * t])[0]
        gsc[t, 2] = R.gsc_of(pcw.so3_exp(np.array([-0.01 * t, 0.01 * t, 0.0])), [0.0, 0.01 * t, -0.02 * t])[0]
    return Xs, np.array([R.BIG, 10000, 10000], dtype=np.int64), gsc


def restate(Xs, next_id, gsc, opts, seed=SEED, sigma=0.0, stream_mod=0, cam=None, max_radius=np.inf):
    """the frames gsc [T, B, 12] through BatchPCW(noise="philox", faults=opts) -> one dict per frame: off / track_ids / meas /
    track_flags / point (the packed tracks generate() returns, their flag bytes and world points), and per point [B, npts]:
    vis (vis_eff), geo (the geometric visibility), ids, flag, pix [B, npts, 3] (0 where no track), offset [B, npts, 2] (what
    the rules add to a track's pixel: the restated outlier offset or sticky bias, 0 elsewhere) and scale [B, npts] (the factor of
    sigma: tail_scale on a tail event); next_id, cnt [B], bias [B, npts, 2], counters [B, 5] summed over the frames so far.
    Asserts the border condition of tests/pcw_restate.py on the geometric projection."""
    B, npts = Xs.shape[:2]
    w = pcw.BatchPCW(B, Xs=Xs, noise="philox", noise_seed=seed, faults=opts, stream_mod=stream_mod)
    w.next_pt_id = np.array(next_id, dtype=np.int64)
    out = []
    for g in gsc:
        Rsc, Tsc = g[:, :9].reshape(B, 3, 3), g[:, 9:]
        if cam is None:
            geo, u, v, z = pcw.project_points(Xs, Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"])
        else:
            geo, u, v, z = pcw.project_points_cam(Xs, Rsc, Tsc, cam, max_radius)
            d = [Xs[..., i] - Tsc[:, None, i] for i in range(3)]
            Xc = [(Rsc[:, None, 0, i] * d[0] + Rsc[:, None, 1, i] * d[1]) + Rsc[:, None, 2, i] * d[2] for i in range(3)]
            radius = np.hypot(Xc[0] / np.where(Xc[2] > 0, Xc[2], 1.0), Xc[1] / np.where(Xc[2] > 0, Xc[2], 1.0))
            assert np.abs(radius - max_radius).min() >= 1e-9, "a point within 1e-9 of the radius guard"
        assert np.abs(z).min() >= 1e-9, "a point within 1e-9 of the camera plane"
        for x, hi in ((u, R.CAM["imw"]), (v, R.CAM["imh"])):
            assert min(np.abs(x).min(), np.abs(x - hi).min()) >= 1e-9, "a pixel within 1e-9 px of an image border"
        bw = np.arange(B) % stream_mod if stream_mod else np.arange(B)
        draw = pcw.fault_draw(seed, w.frame, bw[:, None], np.arange(npts)[None, :], w.faults)
        off, ids, meas = w.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], sigma, cam=cam, max_radius=max_radius)
        bb = np.repeat(np.arange(B), np.diff(off))
        flag, pix = np.zeros((B, npts), dtype=np.uint8), np.zeros((B, npts, 3))
        flag[bb, w.last_point_index], pix[bb, w.last_point_index] = w.last_fault_flags, meas
        track = w.ids >= 0
        if w.faults["sticky"]:      # after the frame a track's bias is what was added to its pixel
            offset = np.where(track[..., None], w.bias, 0.0)
        else:
            offset = np.where(((flag & pcw.FLAG_OUTLIER) != 0)[..., None], draw["off"], 0.0)
        scale = np.where((flag & pcw.FLAG_TAIL) != 0, w.faults["tail_scale"], 1.0)
        out.append(dict(off=off, track_ids=ids, meas=meas, track_flags=w.last_fault_flags.copy(), point=w.last_point_index.copy(),
                        geo=geo, offset=offset, scale=scale, vis=track, ids=w.ids.copy(), flag=flag, pix=pix, next_id=w.next_pt_id.copy(),
                        cnt=np.diff(off).astype(np.int32), bias=w.bias.copy(),
                        counters=np.stack([w.fault_stats[k] for k in pcw.FAULT_COUNTERS], axis=1).copy()))
    return out


def strided(r, tracks_max):
    """a frame's tracks in the layout of xivo_hip_pcw_get_tracks / _fault_get_flags: (cnt, ids, meas, flags)"""
    cnt, ids, meas = R.strided(r, tracks_max)
    flags = np.zeros((len(cnt), tracks_max), dtype=np.uint8)
    for b in range(len(cnt)):
        flags[b, :cnt[b]] = r["track_flags"][r["off"][b]:r["off"][b + 1]]
    return cnt, ids, meas, flags


def coverage(runs):
    """over runs (lists of frames of restate): how often each case occurs -> dict. outlier / tail / biased: tracks with that flag
    bit; dropped: the counter; returned: a point that held a track, was dropped, and later holds a track under another id;
    cleared: a non-zero bias zeroed because its track ended"""
    n = dict(outlier=0, tail=0, biased=0, dropped=0, returned=0, cleared=0)
    for frames in runs:
        for bit, k in ((pcw.FLAG_OUTLIER, "outlier"), (pcw.FLAG_TAIL, "tail"), (pcw.FLAG_BIASED, "biased")):
            n[k] += sum(int(((f["track_flags"] & bit) != 0).sum()) for f in frames)
        n["dropped"] += int(frames[-1]["counters"][:, 1].sum())
        lost = np.full(frames[0]["ids"].shape, -1, dtype=np.int64)       # the id a point held when it last lost its track
        for a, b in zip(frames[:-1], frames[1:]):
            ended = a["vis"] & ~b["vis"]
            lost = np.where(ended, a["ids"], lost)
            # (filters 1 .. of worlds(): every point is geometrically visible there, so a track that ended was dropped)
            n["returned"] += int((b["vis"] & ~a["vis"] & (lost >= 0) & (b["ids"] != lost))[1:].sum())
            n["cleared"] += int((ended & (a["bias"] != 0.0).any(axis=-1) & (b["bias"] == 0.0).all(axis=-1)).sum())
    return n


def assert_coverage(runs, sticky):
    n = coverage(runs)
    print("cases over the inputs (sticky %d): %s" % (sticky, n))
    assert min(n["outlier"], n["tail"], n["dropped"]) >= 5, n
    assert n["returned"] >= 1, n
    if sticky:
        assert n["biased"] >= 5 and n["cleared"] >= 1, n
    else:
        assert n["biased"] == 0 and n["cleared"] == 0, n
