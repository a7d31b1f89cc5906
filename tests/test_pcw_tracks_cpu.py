"""CPU-only: the rules of the device track producer (xivo_amd/csrc/pcw_device.h) under a host compiler. tests/pcw_driver.cpp is
compiled with g++ against the header alone and runs the functions the kernel calls; the expectations are the numpy generator of
xivo_amd/pcw.py (philox_words / philox_normal), the numpy restatement of the header's evaluation order (tests/pcw_restate.py)
and, behind it, BatchPCW.generate.

What this does not cover: the kernel's two order-preserving ranks come from wave ballots, population counts and wave totals in
LDS; the driver counts serially. That both give the same ranks is checked on the GPU (tests/test_pcw_tracks_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcw_restate as R
from xivo_amd import pcw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
FRAMES = 10


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pcw_driver.cpp"
    d = tmp_path_factory.mktemp("pcw")
    exe = str(d / "driver")
    # (x86-64 without -mfma has no fused multiply-add; -ffp-contract=off says so whatever the target, where g++ does not know
    # the header's clang pragma)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "pcw_driver.cpp"), "-o", exe], check=True)

    def run(mode, *arrays):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.run([exe, mode, fin, fout], check=True)
        with open(fout, "rb") as f:
            return f.read()

    return run


def test_philox_known_answer_and_words(driver):
    """Random123's known-answer vectors of Philox4x32-10 (kat_vectors: all-zero counter and key, all-ones) from the header's
    rounds and from the numpy restatement, and 1000 random (seed, frame, filter, point) counters: the same words exactly"""
    kat = np.array([[0] * 6, [0xffffffff] * 6], dtype=np.uint32)
    want = np.array([[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]], dtype=np.uint32)
    got = np.frombuffer(driver("philox", np.int64(2), kat), dtype=np.uint32).reshape(2, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(pcw.philox4x32_10(kat[:, :4], kat[:, 4:]), want)
    rng = np.random.default_rng(3)
    n = 1000
    seed, frame = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64), rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    frame[:100] = np.arange(100)                                   # (frames as a run counts them)
    b, p = rng.integers(0, 4096, size=n).astype(np.uint64), rng.integers(0, 2048, size=n).astype(np.uint64)
    got = np.frombuffer(driver("words", np.int64(n), np.stack([seed, frame, b, p], axis=1)), dtype=np.uint32).reshape(n, 4)
    want = np.array([pcw.philox_words(int(seed[i]), int(frame[i]), int(b[i]), int(p[i])) for i in range(n)])
    assert np.array_equal(got, want)
    # and vectorised over (filter, point), as BatchPCW(noise="philox") draws them
    grid = pcw.philox_words(int(seed[0]), 7, np.arange(5)[:, None], np.arange(300)[None, :])
    got = np.frombuffer(driver("words", np.int64(1500), np.array([[seed[0], 7, bb, pp] for bb in range(5) for pp in range(300)],
                                                                 dtype=np.uint64)), dtype=np.uint32)
    assert np.array_equal(got.reshape(5, 300, 4), grid)


@pytest.mark.parametrize("source", ["header", "numpy"])
def test_noise_is_standard_normal(driver, source):
    """10^6 draws (500 x 1000 points, both components): |mean| < 5 / sqrt(n), variance within 1 % of 1, all finite; the two
    components do not correlate (|r| < 5 / sqrt(n / 2))"""
    nb, npt = 500, 1000
    if source == "header":
        x = np.frombuffer(driver("normals", np.array([11, 4, nb, npt], dtype=np.uint64)), dtype=np.float64).reshape(nb, npt, 2)
    else:
        x = pcw.philox_normal(11, 4, np.arange(nb)[:, None], np.arange(npt)[None, :])
    n = x.size
    assert n == 10 ** 6 and np.isfinite(x).all()
    print("%s: mean %.3e var %.5f max |x| %.2f" % (source, x.mean(), x.var(), np.abs(x).max()))
    assert abs(x.mean()) < 5 / np.sqrt(n)
    assert abs(x.var() - 1.0) < 0.01
    assert abs(np.mean(x[..., 0] * x[..., 1])) < 5 / np.sqrt(n / 2)
    assert np.abs(x).max() < 8.6


def _run_driver(driver, Xs, ids, next_id, gsc):
    B, npts, T = Xs.shape[0], Xs.shape[1], gsc.shape[0]
    cam = np.array([R.CAM[k] for k in ("fx", "fy", "cx", "cy", "imw", "imh")])
    raw = driver("frames", np.array([B, npts, T], dtype=np.int64), cam, next_id, Xs, ids, gsc)
    out, o = [], 0

    def take(dtype, shape):
        nonlocal o
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(raw[o:o + n], dtype=dtype).reshape(shape)
        o += n
        return a
    for _ in range(T):
        out.append(dict(vis=take(np.uint8, (B, npts)).astype(bool), ids=take(np.int64, (B, npts)), next_id=take(np.int64, (B,)),
                        cnt=take(np.int32, (B,)), uvz=take(np.float64, (B, npts, 3)), rank=take(np.int32, (B, npts))))
    assert o == len(raw)
    return out


def _same(d, r, tag):
    assert np.array_equal(d["vis"], r["vis"]), tag
    assert np.array_equal(d["ids"], r["ids"]) and np.array_equal(d["next_id"], r["next_id"]), tag
    assert np.array_equal(d["cnt"], r["cnt"]), tag
    for i, k in enumerate("uvz"):
        assert d["uvz"][..., i].tobytes() == r[k].tobytes(), (tag, k)      # bit for bit
    rank = np.where(r["vis"], np.cumsum(r["vis"], axis=1) - 1, -1)
    assert np.array_equal(d["rank"], rank), tag


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_driver_equals_the_restatement_bit_for_bit(driver, seed):
    """10 frames of 4 moving cameras over box worlds of 300 points, one world seeded with ids above 2^33 and some points
    tracked already: vis, ids, next_id, counts, the position of every track and the noise-free u, v, z"""
    B, npts = 4, 300
    Xs = R.box_world(B, npts, seed)
    rng = np.random.default_rng(seed)
    ids = np.full((B, npts), -1, dtype=np.int64)
    ids[1, rng.choice(npts, 40, replace=False)] = 500 + np.arange(40)
    next_id = np.array([10000, 10000, R.BIG, 7], dtype=np.int64)
    gsc = R.moving_poses(B, FRAMES, seed)
    rs = R.Restate(Xs, ids, next_id)
    got = _run_driver(driver, Xs, ids, next_id, gsc)
    seen = 0
    for t in range(FRAMES):
        r = rs.step(gsc[t])
        _same(got[t], r, (seed, t))
        seen += int(r["cnt"].sum())
    assert seen > 100 and rs.next_id[2] > R.BIG
    assert (rs.ids[1] >= 10000).any()          # points of world 1 were handed new ids past the seeded ones


@pytest.mark.parametrize("npts", [1, 63, 64, 65, 255, 256, 257, 2048])
def test_edge_case_worlds_hold_their_cases(driver, npts):
    """the worlds and frames of the GPU scan test at every size it runs: the restatement shows the cases they were built for,
    the border condition holds, and the header's serial walk agrees"""
    Xs, next_id, gsc = R.edge_case_worlds(npts, seed=npts)
    rs = R.Restate(Xs, None, next_id)
    got = _run_driver(driver, Xs, rs.ids, next_id, gsc)
    steps = [rs.step(g) for g in gsc]
    R.assert_edge_cases(steps)
    for t, r in enumerate(steps):
        _same(got[t], r, (npts, t))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_batch_pcw(seed):
    """the same 10 frames through BatchPCW.generate (einsum; its own numpy noise at std 0): off and ids exactly, meas to
    rtol 1e-13 - einsum's summation order is not the header's; and through BatchPCW(noise="philox"), which is the restatement:
    everything exactly, noise included"""
    B, npts = 4, 300
    Xs = R.box_world(B, npts, seed)
    gsc = R.moving_poses(B, FRAMES, seed)
    rs, rn = R.Restate(Xs), R.Restate(Xs)
    w = pcw.BatchPCW(B, Xs=Xs)
    wp = pcw.BatchPCW(B, Xs=Xs, noise="philox", noise_seed=99)
    for t in range(FRAMES):
        Rsc, Tsc = gsc[t][:, :9].reshape(B, 3, 3), gsc[t][:, 9:]
        r = rs.step(gsc[t])
        off, ids, meas = w.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], 0.0)
        assert np.array_equal(off, r["off"]) and np.array_equal(ids, r["track_ids"]), (seed, t)
        np.testing.assert_allclose(meas, r["meas"], rtol=1e-13, atol=0)
        assert np.array_equal(w.ids, r["ids"]) and np.array_equal(w.next_pt_id, r["next_id"])
        r = rn.step(gsc[t], 1.0, 99, t)
        off, ids, meas = wp.generate(Rsc, Tsc, R.K, R.CAM["imw"], R.CAM["imh"], 1.0)
        assert np.array_equal(off, r["off"]) and np.array_equal(ids, r["track_ids"]) and meas.tobytes() == r["meas"].tobytes()
    assert r["off"][-1] > 0


def test_check_lifecycle_rejects_a_device_track_source_it_cannot_run():
    from xivo_amd import sequence
    sequence.check_lifecycle(sequence.SequenceConfig(lifecycle="device", track_source="device", npts=1024))
    for kw in (dict(track_source="device"), dict(lifecycle="device", track_source="device", npts=1025),
               dict(lifecycle="device", track_source="device", npts=0), dict(track_source="gpu")):
        with pytest.raises(ValueError):
            sequence.check_lifecycle(sequence.SequenceConfig(**kw))
