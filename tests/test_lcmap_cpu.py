"""CPU-only: the integer rules of the resident landmark map (xivo_amd/csrc/lcmap_device.h) under a host compiler, against the
numpy restatement (tests/lcmap_restate.py). tests/lcmap_driver.cpp is a stand-alone program built from the header alone -
plain, and under AddressSanitizer and UBSan - that keeps one filter's map as the kernels do and prints every decision of
scripted add / close sequences. Also here, because they need no GPU: the numpy mirrors of the five ABI structs against the
compiler's sizes, the worlds' last_point_index, SequenceConfig's refusals, and the inputs of the GPU update test on the oracle.

What this does not cover: Xs, the rows, gamma and the kernels' own walks (tests/test_lcmap_gpu.py holds them against the same
restatement)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lcmap_cases as LC
import lcmap_restate as R
import xivo_oracle as orc
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "lcmap_driver.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/lcmap_driver.cpp"
    exe = str(tmp_path_factory.mktemp("lcmap_" + request.param) / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, DRIVER, "-o", exe] + BUILDS[request.param], check=True)
    return exe


def _play(exe, map_max, lc_max, min_matches, ops):
    """ops: ("A", [(key, in_state, poor)]) / ("Q", [keys], [kept x lc_max]) -> the driver's lines, held against the restatement;
    returns (the restatement, the per-op results of the restatement)"""
    m = R.MapRestate(map_max, lc_max, min_matches)
    lines, want, res = ["%d %d %d %d" % (map_max, lc_max, min_matches, len(ops))], [], []
    for op in ops:
        if op[0] == "A":
            lines.append("A %d " % len(op[1]) + " ".join("%d %d %d" % r for r in op[1]))
            d = m.add([(k, s, p, None) for k, s, p in op[1]])
            want += [("a " + " ".join(map(str, d))).rstrip(), "c %d" % len(m.keys)]
            res.append(d)
        else:
            keys, kept = op[1], op[2]
            lines.append("Q %d " % len(keys) + " ".join(map(str, keys)) + " " + " ".join(map(str, kept)))
            slots, lst = m.match(keys)
            frame, neutral = m.decide([bool(kept[i]) for i in range(len(lst))])
            want += [("s " + " ".join(map(str, slots))).rstrip(),
                     "l " + " ".join(str(lst[i][1]) if i < len(lst) else "-1" for i in range(lc_max)),
                     "f %d " % frame + " ".join(str(int(v)) for v in neutral)]
            res.append((slots, lst, frame, neutral))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].startswith("S ")
    assert out[1:-3] == want
    assert out[-3] == "p 0 1 0 0"          # poor: equality keeps, one ulp above drops, 0 means no test
    assert out[-2] == "k 1 0 1 0"          # kept: equality keeps, above gates, 0 means no gate, a bad pivot never passes
    assert out[-1] == "n 0 0 0 0 0 0 1"    # kept: NaN and inf never pass, with a gate (5.99) or without (0); DBL_MAX without one does
    return m, res


def test_struct_sizes_equal_the_numpy_mirrors(driver):
    out = subprocess.run([driver], input="1 1 1 0\n", check=True, capture_output=True, text=True).stdout.splitlines()
    sizes = [int(v) for v in out[0].split()[1:]]
    assert sizes == [L.lcmap_opts_dtype.itemsize, L.lcmap_entry_dtype.itemsize, L.lcmap_add_dtype.itemsize,
                     L.lcmap_query_dtype.itemsize, L.lcmap_match_dtype.itemsize, L.lcmap_stats_dtype.itemsize]
    assert L.lcmap_stats_dtype.names == R.STATS == L.LCMAP_STATS_FIELDS


@pytest.mark.parametrize("map_max", [1, 2, 8])
@pytest.mark.parametrize("lc_max", [1, 6])
def test_fuzz_equals_the_restatement(driver, map_max, lc_max):
    """50 scripted sequences per shape (300 in all) of up to 12 calls over ten keys, so that duplicates, a full map and - where
    the map can hold more than lc_max keys or a query repeats one - more matches than lc_max all occur"""
    rng = np.random.default_rng(100 * map_max + lc_max)
    seen = dict.fromkeys(R.STATS, 0)
    for _ in range(50):
        ops = []
        for _ in range(int(rng.integers(2, 13))):
            if rng.uniform() < 0.5:
                ops.append(("A", [(int(rng.integers(-1, 10)), int(rng.uniform() < 0.85), int(rng.uniform() < 0.15))
                                  for _ in range(int(rng.integers(0, 6)))]))
            else:
                ops.append(("Q", [int(rng.integers(-1, 10)) for _ in range(int(rng.integers(0, 15)))],
                            [int(rng.uniform() < 0.8) for _ in range(lc_max)]))
        m, _ = _play(driver, map_max, lc_max, int(rng.integers(1, 4)), ops)
        for k in R.STATS:
            seen[k] += m.stats[k]
    # the fuzz fires every counter at every shape (but seven matches out of one or two stored keys: not asked of the fuzz)
    assert all(seen[k] > 0 for k in R.STATS if not (k == "surplus" and map_max < lc_max)), seen


def test_the_same_key_twice_in_one_call_and_a_key_already_stored(driver):
    _, res = _play(driver, 8, 6, 5, [("A", [(7, 1, 0), (7, 1, 0), (3, 1, 0)]), ("A", [(3, 1, 0), (5, 1, 0)]),
                                    ("A", [(9, 1, 1), (9, 1, 0), (-2, 1, 0), (4, 0, 0)])])
    assert res[0] == [R.ACCEPT, R.DUP, R.ACCEPT] and res[1] == [R.DUP, R.ACCEPT]
    assert res[2] == [R.POOR, R.ACCEPT, R.SKIPPED, R.SKIPPED]     # a poor record stores nothing: its key is still free


def test_the_map_fills_exactly(driver):
    m, res = _play(driver, 2, 6, 5, [("A", [(1, 1, 0), (2, 1, 0), (3, 1, 0), (1, 1, 0)]), ("Q", [3, 2, 1], [1] * 6)])
    assert res[0] == [R.ACCEPT, R.ACCEPT, R.FULL, R.DUP] and m.keys == [1, 2]      # (a stored key is dup even when the map is full)
    assert res[1][0] == [-1, 0, 1] and res[1][1] == [(1, 1), (2, 0)]


def test_exactly_lc_max_and_one_more_matches(driver):
    add = ("A", [(k, 1, 0) for k in range(8)])
    _, res = _play(driver, 8, 6, 5, [add, ("Q", [0, 9, 1, 2, 3, 4, 5], [1] * 6), ("Q", [7, 6, 5, 4, 3, 2, 1], [1] * 6)])
    assert res[1][0] == [0, -1, 1, 2, 3, 4, 5] and res[1][2] == R.CLOSED
    assert res[2][0] == [0, 1, 2, 3, 4, 5, -2] and [e for _, e in res[2][1]] == [7, 6, 5, 4, 3, 2]


def test_one_fewer_than_min_matches_is_short(driver):
    add = ("A", [(k, 1, 0) for k in range(8)])
    _, res = _play(driver, 8, 6, 5, [add, ("Q", list(range(6)), [1, 1, 0, 1, 0, 1]), ("Q", list(range(6)), [1, 1, 0, 1, 1, 1]),
                                    ("Q", [20, 21], [1] * 6)])
    assert res[1][2] == R.SHORT and res[1][3] == [True] * 6                        # 4 kept: every pair neutral
    assert res[2][2] == R.CLOSED and res[2][3] == [False, False, True, False, False, False]
    assert res[3][2] == R.NONE and res[3][3] == [True] * 6


@pytest.mark.parametrize("chi2", [LC.CHI2, 0.0])
def test_a_gamma_that_is_not_finite_is_gated_and_does_not_count(chi2):
    """the restatement's side of the rule the driver prints: a NaN or inf pixel gives finite rows and pivots, no gamma, and a
    match that is not kept with a gate or without one - five of six kept still close, four of five are short"""
    cam = LC.CAMS["equi"]
    c = LC.update_case(cam)
    sc, lay = c["sc"], LC.layout()
    for bad in ((np.nan, 7.0), (7.0, np.nan), (np.inf, 7.0)):
        ms = [dict(Xs=c["Xs"][0, j], Rsb=c["Rsb_p"][0], Tsb=c["Tsb_p"][0], g_sind=-1, xp=np.array(bad) if j == 2 else c["queries"][j][2])
              for j in range(6)]
        H, inn, dR = R.rows(ms, sc["Rbc"][0], sc["Tbc"][0], cam, lay, LC.LC_MAX, LC.RLC)
        assert np.isfinite(H).all() and not np.isfinite(inn[4:6]).all()
        g = [R.gamma(H[2 * m:2 * m + 2], c["P"][0], inn[2 * m:2 * m + 2], LC.RLC) for m in range(6)]
        k = [R.kept(v, chi2) for v in g]
        assert g[2] is None and k == [True, True, False, True, True, True]
        m = R.MapRestate(LC.MAP_MAX, LC.LC_MAX, LC.MIN_MATCHES)
        frame, neutral = m.decide(k)
        assert frame == R.CLOSED and neutral[2] and m.stats["gated"] == 1
        assert np.isfinite(R.neutralise(H, inn, dR, neutral)[1]).all()
        assert R.MapRestate(LC.MAP_MAX, LC.LC_MAX, LC.MIN_MATCHES).decide(k[:5])[0] == R.SHORT     # four kept of five
    assert R.kept(1e300, 0.0) and R.kept(chi2, chi2) and not R.kept(None, chi2)


def test_header_stays_plain_cxx():
    text = open(os.path.join(CSRC, "lcmap_device.h")).read()
    for name in ("lcmap_add_decide", "lcmap_poor", "lcmap_find", "lcmap_match_slot", "lcmap_kept", "lcmap_frame_decide"):
        assert name in text
    body = text.split("#pragma once")[1]
    assert body.count("#include") == 1 and "hip/hip_runtime.h" in body.split("#else")[0]      # HIP's only, under __HIPCC__


# ---- the worlds' point indices
def _poses(t):
    Rsb = pcw.so3_exp(np.array([0.0, 0.9 * np.sin(0.7 * t), 0.0]))
    return Rsb, np.array([0.5 * np.sin(t), 0.0, 0.0])


def test_last_point_index_of_both_worlds():
    K = np.array([[275.0, 0, 320.0], [0, 275.0, 240.0], [0, 0, 1.0]])
    w = pcw.RandomPCW(npts=300, seed=4)
    bw = pcw.BatchPCW(2, npts=300, seed=4)
    by_id, by_id_b, returned = {}, {}, 0
    gone = set()
    for k in range(40):
        Rsc, Tsc = _poses(0.25 * k)
        before = w.ids.copy()
        ids, meas = w.generate_measurements(Rsc, Tsc, K, 640, 480, 0.5)
        idx = w.last_point_index
        assert idx.shape == ids.shape and np.array_equal(w.ids[idx], ids)          # parallel to the returned ids
        assert np.allclose((w.Xs[idx] - Tsc) @ Rsc[:, 2], meas[:, 2])              # ... and to the measurements (depth)
        for i, p in zip(ids.tolist(), idx.tolist()):
            assert by_id.setdefault(i, p) == p                                     # constant over a track's life
            if p in gone and before[p] < 0:
                returned += 1                                                      # a point that left comes back: new id, same index
                assert i not in (None,) and before[p] != i
        gone |= set(np.nonzero((before >= 0) & (w.ids < 0))[0].tolist())
        off, bids, bmeas = bw.generate(np.stack([Rsc, Rsc]), np.stack([Tsc, Tsc]), K, 640, 480, 0.5)
        bidx = bw.last_point_index
        assert bidx.shape == bids.shape
        for b in range(2):
            sl = slice(off[b], off[b + 1])
            assert np.array_equal(bw.ids[b][bidx[sl]], bids[sl])
            for i, p in zip(bids[sl].tolist(), bidx[sl].tolist()):
                assert by_id_b.setdefault((b, i), p) == p
    assert returned > 0
    pts = {}
    for i, p in by_id.items():
        pts.setdefault(p, []).append(i)
    assert any(len(v) > 1 for v in pts.values())                                   # one point, several track ids


# ---- SequenceConfig
def test_sequence_config_defaults_and_refusals():
    C = sequence.SequenceConfig
    c = C()
    assert (c.loop_closure, c.lc_min_matches, c.lc_chi2) == (False, 5, 5.99) and c.M_max() == 2 * c.n_features
    assert abs(c.lc_chi2 - (-2 * np.log(0.05))) < 2e-3
    assert C(loop_closure=True, lc_max=40).M_max() == 80
    for kw in (dict(lifecycle="device"), dict(feature_init="subfilter", pool_lifecycle="device"),
               dict(feature_init="subfilter", use_oos=True), dict(lc_max=L.LCMAP_MAX_MATCHES + 1),
               dict(lc_map_max=L.LCMAP_MAX_ENTRIES + 1), dict(lc_min_matches=0), dict(lc_meas_std=0.0)):
        with pytest.raises(ValueError):
            sequence.SequenceRunner(None, C(loop_closure=True, **kw), 1)
    sequence.SequenceRunner(None, C(loop_closure=True), 1)
    sequence.SequenceRunner(None, C(loop_closure=True, feature_init="subfilter"), 1)
    r = sequence.SequenceRunner(None, C(loop_closure=True), 1)
    with pytest.raises(ValueError):
        r.frame(None, [(np.zeros(0, dtype=np.int64), np.zeros((0, 3)))])          # keys are required
    with pytest.raises(ValueError):
        r.frame(None, [(np.array([10000]), np.zeros((1, 3)))], keys=[[]])          # ... and parallel to the ids


# ---- the inputs of the GPU update test mean something: on the oracle alone
@pytest.mark.parametrize("name", ["pinhole", "equi"])
def test_update_case_moves_the_perturbed_pose_towards_the_truth(name):
    cam = LC.CAMS[name]
    c = LC.update_case(cam)
    sc, lay = c["sc"], LC.layout()
    b = 0
    ms = [dict(Xs=c["Xs"][b, j], Rsb=c["Rsb_p"][b], Tsb=c["Tsb_p"][b], g_sind=-1, xp=xp)
          for j, (bb, _, xp) in enumerate(q for q in c["queries"] if q[0] == b)]
    H, inn, dR = R.rows(ms, sc["Rbc"][b], sc["Tbc"][b], cam, lay, LC.LC_MAX, LC.RLC)
    assert np.abs(inn).max() > 1.0                                                 # the perturbation is visible in the pixels
    g = [R.gamma(H[2 * m:2 * m + 2], c["P"][b], inn[2 * m:2 * m + 2], LC.RLC) for m in range(6)]
    assert all(v is not None and v < LC.CHI2 for v in g), g                        # inside the covariance: the gate keeps all six
    dx, _, _ = orc.update_joseph(H, c["P"][b], inn, dR)
    Rn, Tn = c["Rsb_p"][b] @ orc.so3_exp(dx[0:3]), c["Tsb_p"][b] + dx[3:6]
    ang = lambda Rm: np.linalg.norm(pcw.so3_log(sc["Rsb"][b].T @ Rm))
    # closer to the truth in both parts (how much depends on the camera: six pixels at a focal length of 190 say less than at 580)
    assert ang(Rn) < ang(c["Rsb_p"][b]) and np.linalg.norm(Tn - sc["Tsb"][b]) < np.linalg.norm(c["dT"][b])
    assert ang(Rn) + np.linalg.norm(Tn - sc["Tsb"][b]) < 0.5 * (ang(c["Rsb_p"][b]) + np.linalg.norm(c["dT"][b]))
