"""CPU-only: the rules of the device trajectory producer (xivo_amd/csrc/trajsim_device.h) under a host compiler.
tests/trajsim_driver.cpp is compiled with g++ against the header alone and runs the functions the kernel calls; the expectations
are the numpy restatement of the header's evaluation order (tests/trajsim_restate.py, where the bounds are derived) and, behind
it, BatchTrajectorySim and ImuFeeder.

Largest differences seen (x86-64, glibc, g++ -O2): header under g++ against the restatement 0.0 of the 64-ulp bound in
every field (the same libm on both sides); restatement against BatchTrajectorySim 0.008 of the 16-ulp bound.

What this does not cover: the device's sin / cos / log (tests/test_trajsim_gpu.py holds the kernel to the same bound)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import trajsim_restate as R
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
MOTION = np.array([0, 1, 0, 1, 1], dtype=np.int32)
RATE = np.array([0.08, 0.1, 0.0, 0.12, 0.0])
K0S = (0, 7, 2 ** 32 - 3)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/trajsim_driver.cpp"
    d = tmp_path_factory.mktemp("trajsim")
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "trajsim_driver.cpp"), "-o", exe], check=True)

    def run(mode, *arrays):
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.run([exe, mode, fin, fout], check=True)
        with open(fout, "rb") as f:
            return f.read()

    return run


def _frame(driver, m, motion, rate, k0, n):
    d, seed = m.packed()
    B = len(rate)
    raw = driver("frame", d, np.array([seed, k0], dtype=np.uint64), np.array([B, n], dtype=np.int64),
                 np.asarray(motion, dtype=np.int32), np.asarray(rate, dtype=np.float64))
    nr = B * n * L.imu_dtype.itemsize
    recs = np.frombuffer(raw[:nr], dtype=L.imu_dtype).reshape(B, n)
    rest = np.frombuffer(raw[nr:], dtype=np.float64)
    assert rest.size == 2 * B * 12
    return recs, rest[:B * 12].reshape(B, 12), rest[B * 12:].reshape(B, 12)


def test_times_and_counter_layout_bit_for_bit(driver):
    """t_k, dt_k = t_k - t_{k-1} (not imu_dt), the generator's words and uniforms: no transcendental, so exact - at small k, at
    2^32 - 1 and 2^32 (where the counter's third word wraps into the fourth) and beyond"""
    k = np.array([0, 1, 2, 3, 399, 400, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 5], dtype=np.uint64)
    for imu_dt in (0.0025, 0.01, 1.0 / 3.0):
        raw = np.frombuffer(driver("times", np.float64(imu_dt), np.int64(k.size), k), dtype=np.float64).reshape(2, -1)
        assert raw[0].tobytes() == R.times(k, imu_dt).tobytes()
        assert raw[1][1:].tobytes() == R.dt_of(k[1:], imu_dt).tobytes() and raw[1][0] == 0.0
    assert R.dt_of(np.array([3], dtype=np.uint64), 0.0025)[0] != 0.0025          # (the case the rule exists for)
    rng = np.random.default_rng(5)
    n = 600
    seed = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    kk = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    kk[:8] = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33, 2 ** 32 - 2, 5]
    b = rng.integers(0, 70000, size=n).astype(np.uint64)
    j = rng.integers(0, 3, size=n).astype(np.uint64)
    raw = driver("words", np.int64(n), np.stack([seed, kk, b, j], axis=1))
    w = np.frombuffer(raw[:16 * n], dtype=np.uint32).reshape(n, 4)
    u = np.frombuffer(raw[16 * n:], dtype=np.float64).reshape(n, 2)
    # counter = (pair, filter, k low, k high), key = the halves of the seed
    ctr = np.stack([j, b, kk & np.uint64(0xffffffff), kk >> np.uint64(32)], axis=1).astype(np.uint32)
    key = np.stack([seed & np.uint64(0xffffffff), seed >> np.uint64(32)], axis=1).astype(np.uint32)
    want = pcw.philox4x32_10(ctr, key)
    assert np.array_equal(w, want)
    assert np.array_equal(want[2], pcw.philox_words(int(seed[2]), 2 ** 32 - 1, int(b[2]), int(j[2])))
    assert not np.array_equal(want[2], pcw.philox_words(int(seed[2]), 2 ** 32, int(b[2]), int(j[2])))
    w64 = want.astype(np.uint64)
    for c in range(2):
        uu = (((w64[:, 2 * c] << np.uint64(20)) | (w64[:, 2 * c + 1] >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
        assert u[:, c].tobytes() == uu.tobytes()
    # the pixel stream's layout (point, filter, frame) is this one's with point = pair, frame = k: the documented overlap
    assert np.array_equal(pcw.trajsim_normals(9, 12, np.arange(4))[:, :2], pcw.philox_normal(9, 12, np.arange(4), 0))


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("k0", K0S)
def test_header_under_gxx_against_the_restatement(driver, noise, k0):
    """records k0 + 1 .. k0 + n and both poses at k0 + n of five filters (both curves, rates including 0): dt exact, every other
    value within ULPS ulp of its largest intermediate (the slopes: over dt), as trajsim_restate derives it"""
    m = R.Model(noise_accel=1e-4 if noise else 0.0, noise_gyro=1e-5 if noise else 0.0, Rbc=pcw.so3_exp(np.array([-1.57079633, 0.0, 0.0])),
                Tbc=(0.05, -0.02, 0.1), seed=77)
    worst = 0.0
    for n in (1, 2, 16):
        got, gt, gsc = _frame(driver, m, MOTION, RATE, k0, n)
        want, bound = R.records(m, MOTION, RATE, k0, n)
        assert got["dt"].tobytes() == want["dt"].tobytes()
        w = R.worst(got, want, bound)
        wgt, wgsc, bgt, bgsc = R.truth(m, MOTION, RATE, k0 + n)
        w = max(w, float((np.abs(gt - wgt) / bgt).max()), float((np.abs(gsc - wgsc) / bgsc).max()))
        worst = max(worst, w)
    print("k0 %d noise %s: largest difference %.3f of the bound" % (k0, noise, worst))
    assert worst <= 1.0


def test_restatement_against_the_existing_simulator():
    """noise off: the restatement against BatchTrajectorySim.meas / .gsb at the same times. The two differ in the summation order
    of einsum / @ over three terms, in (d W) W against d (W W), th ** 3 against th th th and numpy's norm against the explicit
    root: a handful of roundings on values the transcendentals do not differ in - 16 ulp of the same largest intermediates"""
    motion = ["lissajous", "trefoil", "lissajous", "trefoil", "trefoil"]
    sim = pcw.BatchTrajectorySim(motion, RATE, noise_accel=0.0, noise_gyro=0.0)
    m = R.Model(noise_accel=0.0, noise_gyro=0.0, rot_w=sim.rot_w, rot_amp=sim.rot_amp, grav_s=sim.grav_s)
    worst = 0.0
    for k0 in K0S:
        k = np.uint64(k0) + np.arange(20, dtype=np.uint64)
        accel, gyro, sa, sg = R.meas(m, MOTION, RATE, k)
        for i, kk in enumerate(k):
            t = float(R.times(kk, m.imu_dt))
            a, g = sim.meas(t)
            worst = max(worst, float((np.abs(a - accel[:, i]) / (16 * R.EPS * sa[:, i])).max()),
                        float((np.abs(g - gyro[:, i]) / (16 * R.EPS * sg[:, i])).max()))
            gt, _, bgt, _ = R.truth(m, MOTION, RATE, int(kk))
            Rsb, Tsb = sim.gsb(t)
            mine = np.concatenate([Rsb.transpose(0, 2, 1).reshape(-1, 9), Tsb], axis=1)
            worst = max(worst, float((np.abs(mine - gt) / (bgt * 16 / R.ULPS)).max()))
    print("largest difference %.3f of the 16-ulp bound" % worst)
    assert worst <= 1.0


def test_restated_records_are_the_host_feeders_bit_for_bit():
    """ImuFeeder.imu driven by the restated samples at the restated times gives the restated records exactly"""
    m = R.Model(seed=5)
    for k0 in K0S:
        n = 9
        k = np.uint64(k0) + np.arange(n + 1, dtype=np.uint64)
        accel, gyro, _, _ = R.meas(m, MOTION, RATE, k)
        t = R.times(k, m.imu_dt)
        f = sequence.ImuFeeder(len(RATE), t[0], gyro[:, 0], accel[:, 0])
        for i in range(1, n + 1):
            f.imu(t[i], gyro[:, i], accel[:, i])
        want, _ = R.records(m, MOTION, RATE, k0, n)
        assert f.take().tobytes() == want.tobytes()


@pytest.mark.parametrize("source", ["header", "numpy"])
def test_noise_moments(driver, source):
    """10^6 draws (500 filters x 334 samples x 6): every one of the six normals has |mean| < 5 / sqrt(n), variance within 1.5 %
    of 1; no two of the six correlate (|r| < 5 / sqrt(n)), in particular none across the three generator calls"""
    nb, nk = 500, 334
    if source == "header":
        x = np.frombuffer(driver("normals", np.array([11, 2 ** 32 - 100, nb, nk, 1, 1], dtype=np.uint64)), dtype=np.float64)
        x = x.reshape(nb * nk, 6)
    else:
        x = np.concatenate([pcw.trajsim_normals(11, 2 ** 32 - 100 + k, np.arange(nb)) for k in range(nk)])
    n = x.shape[0]
    assert x.size >= 10 ** 6 and np.isfinite(x).all() and np.abs(x).max() < R.NORMAL_MAX
    print("%s: mean %s var %s" % (source, x.mean(axis=0), x.var(axis=0)))
    assert (np.abs(x.mean(axis=0)) < 5 / np.sqrt(n)).all()
    assert (np.abs(x.var(axis=0) - 1.0) < 0.015).all()
    c = (x.T @ x) / n
    assert (np.abs(c - np.diag(np.diag(c))) < 5 / np.sqrt(n)).all()


def test_edge_cases(driver):
    """rot_amp = 0: both small-angle branches, R = Jr = I exactly, gyro = 0, accel = d; rate = 0: a stationary body, accel =
    R^T (-g) and Tsb = 0; n = 0: poses only; noise 0 draws nothing (the seed does not matter, wanted-off pairs read 0)"""
    m = R.Model(rot_amp=0.0, noise_accel=0.0, noise_gyro=0.0)
    got, gt, gsc = _frame(driver, m, MOTION, RATE, 40, 3)
    want, _ = R.records(m, MOTION, RATE, 40, 3)
    assert np.array_equal(gt[:, :9], np.tile(np.eye(3).reshape(-1), (5, 1))) and np.array_equal(gsc[:, :9], gt[:, :9])
    assert (got["gyro"] == 0).all() and (got["slope_gyro"] == 0).all()
    assert got.tobytes() == want.tobytes()                     # (no rotation: only the curve's sin / cos, one libm)
    assert np.array_equal(got["accel"][2], np.tile([0.0, 0.0, 9.8], (3, 1)))     # rate 0, R = I: -g
    m = R.Model(noise_accel=0.0, noise_gyro=0.0)
    got, gt, gsc = _frame(driver, m, MOTION, RATE, 40, 3)
    Rm, _, _, _ = R.profile(m, R.times(np.uint64(40) + np.arange(3, dtype=np.uint64), m.imu_dt))
    g = -m.grav_s
    rt = np.stack([Rm[:, 0, i] * g[0] + Rm[:, 1, i] * g[1] + Rm[:, 2, i] * g[2] for i in range(3)], -1)
    for b in (2, 4):                                           # the two stationary filters, one per curve
        assert np.abs(got["accel"][b] - rt).max() <= R.ULPS * R.EPS * 9.8
        assert (gt[b, 9:] == 0).all()
    r0, gt0, gsc0 = _frame(driver, m, MOTION, RATE, 0, 0)
    assert r0.size == 0 and np.array_equal(gt0[:, :9], np.tile(np.eye(3).reshape(-1), (5, 1))) and (gt0[:, 9:] == 0).all()
    m2 = R.Model(noise_accel=0.0, noise_gyro=0.0, seed=123456)
    assert _frame(driver, m2, MOTION, RATE, 40, 3)[0].tobytes() == got.tobytes()
    x = np.frombuffer(driver("normals", np.array([11, 5, 3, 4, 0, 1], dtype=np.uint64)), dtype=np.float64).reshape(-1, 6)
    y = np.frombuffer(driver("normals", np.array([11, 5, 3, 4, 1, 1], dtype=np.uint64)), dtype=np.float64).reshape(-1, 6)
    assert (x[:, :2] == 0).all() and np.array_equal(x[:, 2:], y[:, 2:]) and (y[:, :2] != 0).all()
    z = np.frombuffer(driver("normals", np.array([11, 5, 3, 4, 0, 0], dtype=np.uint64)), dtype=np.float64)
    assert (z == 0).all()
    # only the accelerometer is noisy: the gyro is the noise-free one
    ma = R.Model(noise_accel=1e-3, noise_gyro=0.0)
    ga = _frame(driver, ma, MOTION, RATE, 40, 3)[0]
    assert ga["gyro"].tobytes() == got["gyro"].tobytes() and not np.array_equal(ga["accel"], got["accel"])


def test_entry_points_refuse_bad_arguments_without_a_gpu(built):
    lib = L.load_library()
    o = np.zeros(1, dtype=L.trajsim_opts_dtype)
    p = o.ctypes.data_as(ctypes.c_void_p)
    assert lib.xivo_hip_trajsim_config(None, p) == -1 and lib.xivo_hip_trajsim_config(None, None) == -1
    assert lib.xivo_hip_trajsim_set(None, 0, 1, None, None) == -1
    assert lib.xivo_hip_trajsim_frame(None, 1, 0, 1) == -1
    assert lib.xivo_hip_propagate_resident(None, 1, None) == -1
    assert lib.xivo_hip_pcw_tracks_resident(None, 1, 0.0, 0, 0) == -1
    assert lib.xivo_hip_trajsim_get(None, 0, 1, None, None, None) == -1
    assert lib.xivo_hip_trajsim_get_gt(None, 0, 1, 0, 1, None) == -1
    assert lib.xivo_hip_trajsim_reset(None) == -1 and lib.xivo_hip_trajsim_count(None) == 0


def test_dtypes_match_the_header(tmp_path):
    """sizeof / offsetof of xivo_trajsim_opts as a C compiler lays it out against the numpy mirror"""
    cxx = shutil.which("g++")
    assert cxx
    src = tmp_path / "sz.cpp"
    fields = [n for n in L.trajsim_opts_dtype.names]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "xivo_hip.h"\nint main() { printf("%zu", sizeof(xivo_trajsim_opts));\n'
                   + "".join('printf(" %%zu", offsetof(xivo_trajsim_opts, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.run([cxx, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == L.trajsim_opts_dtype.itemsize == 200
    assert out[1:] == [L.trajsim_opts_dtype.fields[f][1] for f in fields]
    assert L.imu_dtype.itemsize == 13 * 8


def test_configuration():
    cfg = sequence.SequenceConfig()
    assert cfg.imu_source == "host"
    sequence.check_lifecycle(sequence.SequenceConfig(lifecycle="device", track_source="device", imu_source="device", npts=100))
    for kw in (dict(imu_source="device"), dict(lifecycle="device", imu_source="device"), dict(imu_source="gpu")):
        with pytest.raises(ValueError):
            sequence.check_lifecycle(sequence.SequenceConfig(**kw))
    with pytest.raises(ValueError, match="imu_source"):      # the message-by-message driver does not fall back to host IMU
        sequence.run_pcw(None, sequence.SequenceConfig(lifecycle="device", track_source="device", imu_source="device", npts=100),
                         [], [])
    with pytest.raises(ValueError):
        pcw.BatchTrajectorySim(["lissajous"], [0.1], noise="other")
    with pytest.raises(ValueError):
        pcw.BatchTrajectorySim(["lissajous"], [0.1], noise="philox").meas(0.0)        # no sample index
    # the default stream is untouched by the new argument
    a = pcw.BatchTrajectorySim(["lissajous", "trefoil"], [0.1, 0.1], seed=3).meas(0.1)
    rng = np.random.default_rng(3)
    n_a, n_g = rng.standard_normal((2, 3)), rng.standard_normal((2, 3))
    b = pcw.BatchTrajectorySim(["lissajous", "trefoil"], [0.1, 0.1], seed=3, noise_accel=0.0, noise_gyro=0.0).meas(0.1)
    assert a[0].tobytes() == (b[0] + 1e-4 * n_a).tobytes() and a[1].tobytes() == (b[1] + 1e-5 * n_g).tobytes()


def test_run_pcw_batch_refuses_equal_imu_and_pixel_seeds():
    """seed + 1 keys the IMU stream, noise_seed the pixel stream; the same key for both is refused before anything is set up"""
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", n_groups=2, n_features=4)
    with pytest.raises(ValueError, match="seed"):
        sequence.run_pcw_batch(cfg, 2, total_time=0.1, npts=100, seed=4, noise_seed=5, imu_source="device")
    with pytest.raises(ValueError, match="seed"):
        sequence.run_pcw_batch(cfg, 2, total_time=0.1, npts=100, seed=4, noise_seed=5, imu_noise="philox")
