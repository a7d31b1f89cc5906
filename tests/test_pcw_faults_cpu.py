"""CPU-only: the track-fault rules of the device producer (xivo_amd/csrc/pcw_device.h "Track faults") under a host compiler.
tests/pcw_fault_driver.cpp is compiled with g++ against the header alone - once as the other host drivers are, once with
-fsanitize=address,undefined as a program of its own - and runs the functions the fault instances of the kernel call; the
expectations are the numpy restatement of xivo_amd/pcw.py (fault_draw, BatchPCW.generate(faults=...)).

What this does not cover: the kernel ranks and counts with wave ballots and wave totals in LDS where the driver counts serially;
that both agree is checked on the GPU (tests/test_pcw_faults_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcw_fault_cases as FC
import pcw_restate as R
from xivo_amd import pcw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
FRAMES = 8


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pcw_fault_driver.cpp"
    d = tmp_path_factory.mktemp("pcw_fault_" + request.param)
    exe = str(d / "driver")
    # (as tests/test_pcw_tracks_cpu.py builds pcw_driver.cpp; the sanitized build is the same program with the checks compiled in)
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + CSRC] + extra +
                   [os.path.join(ROOT, "tests", "pcw_fault_driver.cpp"), "-o", exe], check=True)

    def run(mode, *arrays):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.run([exe, mode, fin, fout], check=True)
        with open(fout, "rb") as f:
            return f.read()

    return run


def _thresholds(o):
    t1 = o["p_drop"]; t2 = t1 + o["p_outlier"]; t3 = t2 + o["p_tail"]
    return np.array([t1, t2, t3, o["outlier_min_px"], o["outlier_max_px"], o["tail_scale"]])


def _run_frames(driver, Xs, next_id, gsc, o, seed, sigma, stream_mod=0):
    B, npts, T = Xs.shape[0], Xs.shape[1], gsc.shape[0]
    cam = np.array([R.CAM[k] for k in ("fx", "fy", "cx", "cy", "imw", "imh")])
    raw = driver("frames", np.array([B, npts, T, o["sticky"], stream_mod], dtype=np.int64), np.uint64(seed), np.float64(sigma),
                 _thresholds(o), cam, np.asarray(next_id, dtype=np.int64), Xs, np.full((B, npts), -1, dtype=np.int64), gsc)
    out, p = [], 0

    def take(dtype, shape):
        nonlocal p
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(raw[p:p + n], dtype=dtype).reshape(shape)
        p += n
        return a
    for _ in range(T):
        out.append(dict(vis=take(np.uint8, (B, npts)).astype(bool), ids=take(np.int64, (B, npts)), next_id=take(np.int64, (B,)),
                        cnt=take(np.int32, (B,)), flag=take(np.uint8, (B, npts)), pix=take(np.float64, (B, npts, 3)),
                        bias=take(np.float64, (B, npts, 2)), counters=take(np.int64, (B, 5))))
    assert p == len(raw)
    return out


@pytest.mark.parametrize("sticky", [0, 1])
def test_events_against_the_restatement_bit_for_bit(driver, sticky):
    """worlds of 1, 65 and 257 points, 3 filters, 8 frames, p_drop = p_outlier = p_tail = 0.2, offsets 20 - 60 px, noise 0: the
    header's serial walk and BatchPCW.generate(faults=...) agree on counts, ids, next_id, flags, pixels, the bias state and the
    producer's counters after every frame, bit for bit. First, on the restatement alone: every event class (and "biased" when
    sticky) occurs at least 5 times, a dropped point returns under a new id, a bias is cleared by its track's end."""
    o = FC.faults(sticky)
    cases = {npts: FC.worlds(npts, FRAMES) for npts in (1, 65, 257)}
    want = {npts: FC.restate(*c, o) for npts, c in cases.items()}
    FC.assert_coverage(want.values(), sticky)
    for npts, (Xs, next_id, gsc) in cases.items():
        got = _run_frames(driver, Xs, next_id, gsc, o, FC.SEED, 0.0)
        for t, (g, w) in enumerate(zip(got, want[npts])):
            for k in ("vis", "ids", "next_id", "cnt", "flag", "counters"):
                assert np.array_equal(g[k], w[k]), (npts, t, k)
            for k in ("pix", "bias"):
                assert g[k].tobytes() == w[k].tobytes(), (npts, t, k)
            if not sticky:
                assert not w["bias"].any()


def test_fault_draw_equals_the_header(driver):
    """pcw.fault_draw against pcw_fault_event / pcw_fault_offset over 5 x 300 (filter, point) pairs of three frames: events
    and offsets bit for bit"""
    o = FC.faults(0)
    for frame in (0, 7, (1 << 32) + 3):
        raw = driver("draws", np.array([FC.SEED, frame, 5, 300], dtype=np.uint64), _thresholds(o))
        ev = np.frombuffer(raw[:5 * 300 * 4], dtype=np.int32).reshape(5, 300)
        off = np.frombuffer(raw[5 * 300 * 4:], dtype=np.float64).reshape(5, 300, 2)
        d = pcw.fault_draw(FC.SEED, frame, np.arange(5)[:, None], np.arange(300)[None, :], o)
        assert np.array_equal(ev, d["event"]) and off.tobytes() == d["off"].tobytes()
        assert np.array_equal(d["tail"], ev == pcw.FAULT_TAIL)


def test_the_four_streams_are_disjoint(driver):
    """1000 random (seed, frame, filter, point) quadruples: the counters of draw A, draw B, the pixel noise (philox_words) and the
    trajectory producer (trajsim_normals: word 0 in {0, 1, 2}) are pairwise different, and the words of A and B - from the
    header and from pcw.fault_words - are philox4x32_10 on the counters the header states"""
    rng = np.random.default_rng(9)
    n = 1000
    seed, frame = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64), rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    frame[:100] = np.arange(100)
    b, p = rng.integers(0, 4096, size=n).astype(np.uint64), rng.integers(0, 2048, size=n).astype(np.uint64)
    p[:3] = (0, 1, 2)                                              # (the points whose pixel-noise counters the IMU stream shares)
    lo, hi = (frame & np.uint64(0xFFFFFFFF)).astype(np.uint32), (frame >> np.uint64(32)).astype(np.uint32)
    p32, b32 = p.astype(np.uint32), b.astype(np.uint32)
    ctr = dict(A=np.stack([p32 | np.uint32(0x80000000), b32, lo, hi], 1), B=np.stack([p32 | np.uint32(0x40000000), b32, lo, hi], 1),
               pixel=np.stack([p32, b32, lo, hi], 1))
    for j in range(3):
        ctr["imu%d" % j] = np.stack([np.full(n, j, dtype=np.uint32), b32, lo, hi], 1)
    names = sorted(ctr)
    for i in range(n):
        rows = [tuple(ctr[k][i]) for k in names if not (k.startswith("imu") and p32[i] == int(k[3]))]
        # under one key the IMU stream is the pixel noise of points 0 .. 2 (stated in pcw.trajsim_normals): those aside,
        # no two streams share a counter
        assert len(set(rows)) == len(rows), (i, names)
    assert all((ctr[k][:, 0] >= 0x40000000).all() for k in "AB") and (ctr["pixel"][:, 0] < 2048).all()
    assert not ((ctr["A"][:, 0] ^ ctr["B"][:, 0]) == 0).any()
    key = np.stack([(seed & np.uint64(0xFFFFFFFF)).astype(np.uint32), (seed >> np.uint64(32)).astype(np.uint32)], 1)
    for draw, code in (("A", 0), ("B", 1)):
        want = pcw.philox4x32_10(ctr[draw], key)
        got = np.frombuffer(driver("words", np.int64(n), np.stack([seed, frame, b, p, np.full(n, code, dtype=np.uint64)], 1)),
                            dtype=np.uint32).reshape(n, 4)
        assert np.array_equal(got, want)
        mine = np.array([pcw.fault_words(int(seed[i]), int(frame[i]), int(b[i]), int(p[i]), draw) for i in range(0, n, 10)])
        assert np.array_equal(mine, want[::10])
        # and they are not the pixel noise's words
        assert not np.array_equal(want, pcw.philox4x32_10(ctr["pixel"], key))


@pytest.mark.parametrize("source", ["header", "numpy"])
def test_event_frequencies_and_offsets(driver, source):
    """10^6 draws (500 filters x 2000 points): each event class lies within 5 standard deviations of its binomial expectation,
    |count - n p| <= 5 sqrt(n p (1 - p)); every offset component lies in +-[20, 60] px with both signs present (and about
    evenly: the same bound at p = 1 / 2)"""
    o = FC.faults(0)
    nb, npt = 500, 2000
    if source == "header":
        raw = driver("draws", np.array([FC.SEED, 3, nb, npt], dtype=np.uint64), _thresholds(o))
        ev = np.frombuffer(raw[:nb * npt * 4], dtype=np.int32).reshape(nb, npt)
        off = np.frombuffer(raw[nb * npt * 4:], dtype=np.float64).reshape(nb, npt, 2)
    else:
        d = pcw.fault_draw(FC.SEED, 3, np.arange(nb)[:, None], np.arange(npt)[None, :], o)
        ev, off = d["event"], d["off"]
    n = ev.size
    assert n == 10 ** 6
    for code, prob in ((pcw.FAULT_DROP, 0.2), (pcw.FAULT_OUTLIER, 0.2), (pcw.FAULT_TAIL, 0.2), (pcw.FAULT_NOMINAL, 0.4)):
        k = int((ev == code).sum())
        bound = 5 * np.sqrt(n * prob * (1 - prob))
        print("%s event %d: %d of %d (expected %.0f +- %.0f)" % (source, code, k, n, n * prob, bound))
        assert abs(k - n * prob) <= bound
    a = np.abs(off)
    assert a.min() >= 20.0 and a.max() <= 60.0
    for i in range(2):
        neg = int((off[..., i] < 0).sum())
        assert abs(neg - n / 2) <= 5 * np.sqrt(n / 4), (i, neg)
    assert abs(a.mean() - 40.0) < 5 * (40.0 / np.sqrt(12.0)) / np.sqrt(2 * n)          # uniform on [20, 60]


def test_score_cells(driver):
    """pcw_fault_cell over every (mask, flag) pair against pcw.fault_cell: faulty <=> flag & 5, rejected <=> mask == 0"""
    pairs = np.array([[m, f] for m in (0, 1, 255) for f in range(8)], dtype=np.uint8)
    got = np.frombuffer(driver("cells", np.int64(len(pairs)), pairs), dtype=np.int32)
    assert got.tolist() == [pcw.fault_cell(int(m), int(f)) for m, f in pairs]
    assert pcw.fault_cell(0, 1) == 0 and pcw.fault_cell(1, 4) == 1 and pcw.fault_cell(0, 2) == 2 and pcw.fault_cell(1, 0) == 3


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_zero_probabilities_change_nothing(sigma):
    """generate(faults=...) with every probability 0 returns what generate() returns, bytes (sticky or not), and no flag"""
    Xs, next_id, gsc = FC.worlds(65, 4)
    ws = [pcw.BatchPCW(3, Xs=Xs, noise="philox", noise_seed=5)] + [
        pcw.BatchPCW(3, Xs=Xs, noise="philox", noise_seed=5, faults=dict(sticky=s, outlier_min_px=20.0, outlier_max_px=60.0, tail_scale=3.0))
        for s in (0, 1)]
    for g in gsc:
        outs = [w.generate(g[:, :9].reshape(3, 3, 3), g[:, 9:], R.K, 640.0, 480.0, sigma) for w in ws]
        assert len(outs[0][1]) > 0
        for o in outs[1:]:
            assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(o, outs[0]))
        assert not ws[1].last_fault_flags.any() and len(ws[1].last_fault_flags) == len(outs[0][1])
        assert np.array_equal(ws[1].last_point_index, ws[0].last_point_index)


def test_stream_sharing(driver):
    """stream_mod = 2 over identical worlds: filters 0 and 2 produce identical tracks (and filter 1 others); the header's walk
    agrees with the restatement under the shared stream, noise on the same words"""
    Xs, next_id, gsc = FC.worlds(65, 5)
    Xs, gsc = np.repeat(Xs[1:2], 3, axis=0), np.repeat(gsc[:, 1:2], 3, axis=1)
    o = FC.faults(1)
    fr = FC.restate(Xs, [10000] * 3, gsc, o, sigma=1.0, stream_mod=2)
    own = FC.restate(Xs, [10000] * 3, gsc, o, sigma=1.0)
    got = _run_frames(driver, Xs, [10000] * 3, gsc, o, FC.SEED, 1.0, stream_mod=2)
    differ = False
    for t, f in enumerate(fr):
        for k in ("ids", "flag", "pix", "bias"):
            assert f[k][0].tobytes() == f[k][2].tobytes(), (t, k)
        differ = differ or f["flag"][0].tobytes() != f["flag"][1].tobytes()
        assert f["flag"][0].tobytes() == own[t]["flag"][0].tobytes() and f["flag"][1].tobytes() == own[t]["flag"][1].tobytes()
        for k in ("vis", "ids", "flag", "counters"):
            assert np.array_equal(got[t][k], f[k]), (t, k)
        assert np.abs(got[t]["pix"] - f["pix"]).max() <= 2 * np.spacing(640.0) + 1e-13 * o["tail_scale"]
    assert differ
    assert any(a["flag"][2].tobytes() != f["flag"][2].tobytes() for a, f in zip(own, fr))   # filter 2's own stream is another


def test_refusals_of_the_numpy_side():
    Xs = np.zeros((2, 4, 3))
    with pytest.raises(ValueError):
        pcw.BatchPCW(2, Xs=Xs, faults=FC.FAULTS)                       # the numpy stream has no fault draws
    with pytest.raises(ValueError):
        pcw.BatchPCW(2, Xs=Xs, stream_mod=2)
    with pytest.raises(ValueError):
        pcw.BatchPCW(2, Xs=Xs, noise="philox", stream_mod=-1)
    bad = (dict(p_drop=-0.1), dict(p_tail=1.5), dict(p_drop=0.5, p_outlier=0.4, p_tail=0.2), dict(outlier_min_px=-1.0),
           dict(outlier_min_px=5.0, outlier_max_px=4.0), dict(tail_scale=0.5), dict(tail_scale=float("inf")), dict(p_drop=float("nan")),
           dict(sticky=2), dict(unknown=1.0))
    for kw in bad:
        with pytest.raises(ValueError):
            pcw.fault_opts(**kw)
        with pytest.raises(ValueError):
            pcw.BatchPCW(2, Xs=Xs, noise="philox", faults=kw)
    assert pcw.fault_opts(p_drop=0.5, p_outlier=0.25, p_tail=0.25)["p_tail"] == 0.25      # a sum of exactly 1 is allowed


def test_upper_layers_refuse_faults_they_cannot_run():
    """before anything touches a GPU: scripts/run_pcw.py refuses the fault options on host tracks without the philox stream and
    options xivo_hip_pcw_fault_config would refuse, with a message; run_pcw_batch and run_sweep refuse faults on host tracks
    they could not restate or score"""
    import sys
    from collections import OrderedDict
    from xivo_amd import sequence, sweep
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-sequences", "2", "-total_time", "0.1"]
    for extra, msg in ((["-vectorized", "-outlier-prob", "0.1"], "-pixel-noise philox"),
                       (["-drop-prob", "0.1"], "-pixel-noise philox"),
                       (["-vectorized", "-lifecycle", "device", "-tracks", "device", "-outlier-prob", "1.5"], "track faults"),
                       (["-vectorized", "-lifecycle", "device", "-tracks", "device", "-outlier-prob", "0.1", "-outlier-px", "9", "3"], "track faults"),
                       (["-pixel-noise", "philox"], "-vectorized")):
        out = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and msg in out.stderr, (extra, out.stderr[-500:])
    cfg = sequence.SequenceConfig(lifecycle="device", track_faults=dict(p_drop=0.1))
    with pytest.raises(ValueError):
        sequence.run_pcw_batch(cfg, 2, total_time=0.1)                                  # host tracks on the numpy stream
    with pytest.raises(ValueError):
        sweep.run_sweep(cfg, OrderedDict([("MH_thresh", [3.0])]), 2, total_time=0.1)     # host tracks are not scored
    with pytest.raises(ValueError):
        sweep.run_sweep(sequence.SequenceConfig(lifecycle="device"), OrderedDict([("MH_thresh", [3.0])]), 2, total_time=0.1, track_source="gpu")
    assert sequence.SequenceConfig().track_faults is None
