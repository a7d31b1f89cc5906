"""CPU-only: the landmark map's visit rule (xivo_amd/csrc/lcmap_device.h) under a host compiler against the numpy restatement
(tests/lcmap_cov_restate.py). tests/lcmap_cov_driver.cpp is a stand-alone program built from the header alone - plain, and
under AddressSanitizer and UBSan - that keeps one filter's map and visit records as lcmap_close_kernel does and prints every
decision of scripted and fuzzed call sequences. Also here, because they need no GPU: the numpy mirrors of the two new ABI
structs against the compiler's sizes, SequenceConfig's new options, and the inputs of the GPU gate / update tests on the
oracle.

What this does not cover: Sigma of an added record, R_e, gamma and the whitening as the kernels compute them
(tests/test_lcmap_cov_gpu.py holds them against the same restatement)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lcmap_cases as LC
import lcmap_cov_cases as CC
import lcmap_cov_restate as CR
import lcmap_restate as R
import xivo_oracle as orc
from xivo_amd import lib as L
from xivo_amd import sequence, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "lcmap_cov_driver.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
GRID = "g 0 %d" % (sum(nm + 1 for nm in range(8)) * 8 * 4 * 2 * 4 * (2 + 16))
NONFINITE = "n 0 0 0 0 1"                  # NaN / inf gamma: not kept without a gate or with one, uses nothing, its pair neutral


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/lcmap_cov_driver.cpp"
    exe = str(tmp_path_factory.mktemp("lcmap_cov_" + request.param) / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, DRIVER, "-o", exe] + BUILDS[request.param], check=True)
    return exe


def _play(exe, map_max, lc_max, min_matches, gap, ops):
    """ops: ("A", [keys]) / ("Q", [keys], [kept x lc_max]) -> the driver's lines held against the restatement; returns (the
    restatement, the result of every Q)"""
    v = CR.VisitRestate(map_max, lc_max, min_matches, gap)
    old = R.MapRestate(map_max, lc_max, min_matches)
    lines, want, res = ["%d %d %d %d %d" % (map_max, lc_max, min_matches, gap, len(ops))], [], []
    for op in ops:
        if op[0] == "A":
            lines.append("A %d " % len(op[1]) + " ".join(map(str, op[1])))
            v.add(op[1]); old.add([(k, True, False, None) for k in op[1]])
            want.append("c %d" % len(v.keys))
        else:
            keys, kept = op[1], op[2]
            lines.append("Q %d " % len(keys) + " ".join(map(str, keys)) + " " + " ".join(map(str, kept)))
            r = v.close(keys, kept)
            n = len(r["entries"])
            want += ["l " + " ".join(str(r["entries"][m]) if m < n else "-1" for m in range(lc_max)),
                     "r " + " ".join(str(r["resting"][m]) if m < n else "0" for m in range(lc_max)),
                     "f %d " % r["frame"] + " ".join(map(str, r["neutral"])),
                     ("v " + " ".join("%d %d" % (a, b) for a, b in zip(v.last_seen, v.used))).rstrip()]
            res.append(r)
            if gap == 0:       # nothing rests, and the frame and the pairs are those of the rules without visits
                _, lst = old.match(keys)
                frame, neutral = old.decide([bool(kept[m]) for m in range(len(lst))])
                assert not any(r["resting"]) and (r["frame"], r["neutral"]) == (frame, [int(x) for x in neutral])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].startswith("S ")
    assert out[1:-2] == want
    assert out[-2] == GRID                 # gap = 0 on the whole grid: no mismatch
    assert out[-1] == NONFINITE
    return v, res


def test_struct_sizes_equal_the_numpy_mirrors(driver):
    out = subprocess.run([driver], input="1 1 1 0 0\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()[1:]] == [L.lcmap_cov_opts_dtype.itemsize, L.lcmap_cov_stats_dtype.itemsize] == [16, 24]
    assert L.lcmap_cov_stats_dtype.names == CR.COV_STATS == L.LCMAP_COV_STATS_FIELDS
    for name in ("xivo_hip_lcmap_cov_config", "xivo_hip_lcmap_set_cov", "xivo_hip_lcmap_get_cov", "xivo_hip_lcmap_get_cov_stats"):
        assert name in L.ALL_SYMBOLS
    assert out[-2] == GRID and out[-1] == NONFINITE


def test_an_entry_of_H_Sigma_Ht_is_rounded_once_where_a_plain_sum_loses_digits(driver):
    """lcmap_quad3 (a^T C b, the entries of R_e - Rlc I) against exact rational arithmetic on 300 nearly rank-one C = s^2 n n^T +
    (1 mm)^2 I with a and b within 1e-1 .. 1e-4 of orthogonal to n: within one ulp of the exact value (plus 2^-100 of the sum of
    the |products|, what two doubles carry), where numpy's plain sums of the same products are tens of ulp off"""
    from fractions import Fraction as Fr
    rng = np.random.default_rng(77)
    cases = []
    for _ in range(300):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        C = 10.0 ** rng.uniform(0, 4) * np.outer(n, n) + 1e-6 * np.eye(3)
        C = np.triu(C) + np.triu(C, 1).T
        v = []
        for _ in range(2):
            t = rng.normal(size=3); t -= (t @ n) * n
            v.append(100.0 * (t / np.linalg.norm(t) + 10.0 ** rng.uniform(-4, -1) * n))
        cases.append((C, v[0], v[0] if rng.uniform() < 0.5 else v[1]))
    lines = ["1 1 1 0 %d" % len(cases)]
    for C, a, b in cases:
        lines.append("C 0 " + " ".join(float(x).hex() for x in [C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2], *a, *b]))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    got = [float.fromhex(l.split()[1]) for l in out[1:-2]]
    assert len(got) == len(cases) and out[-2] == GRID
    worst = plain = 0.0
    for (C, a, b), q in zip(cases, got):
        terms = [Fr(float(C[i, j])) * Fr(float(a[j])) * Fr(float(b[i])) for i in range(3) for j in range(3)]
        exact = sum(terms)
        ulp = Fr(float(np.spacing(abs(float(exact)))))
        assert abs(Fr(q) - exact) <= ulp + sum(abs(t) for t in terms) / 2 ** 100, (C, a, b, q)
        worst = max(worst, float(abs(Fr(q) - exact) / ulp)); plain = max(plain, float(abs(Fr(float(b @ (C @ a))) - exact) / ulp))
    print("lcmap_quad3: worst %.2f ulp; the plain sum: %.0f ulp" % (worst, plain))
    assert plain > 16.0                                                   # (the cases are hard: what the kernel's sums used to lose)


def test_a_gamma_that_is_not_finite_is_never_kept_on_R_e_either():
    """the restatement's side of the rule: a NaN or inf innovation on a definite R_e gives no gamma, with a gate or without"""
    c = CC.gate_case(synth.EQUI)
    H, inn, dR, Res = CC.rows0(c, synth.EQUI)
    assert CR.gamma(H[0:2], c["P"][0], inn[0:2], Res[0]) is not None
    for bad in ((np.nan, inn[1]), (inn[0], np.nan), (np.inf, inn[1]), (-np.inf, np.inf)):
        g = CR.gamma(H[0:2], c["P"][0], np.array(bad), Res[0])
        assert g is None and not R.kept(g, LC.CHI2) and not R.kept(g, 0.0), bad
    v = CR.VisitRestate(8, 6, 1, 2); v.add(range(8))
    r = v.close([0, 1], [R.kept(None, 0.0), True])                        # closes on the other match; the NaN one uses nothing
    assert r["frame"] == CR.CLOSED and r["neutral"][:2] == [1, 0] and v.used[:2] == [0, 1] and v.stats["gated"] == 1


ADD8 = ("A", list(range(8)))


def test_an_entry_is_used_then_rests_and_a_frame_of_resting_matches_is_rested(driver):
    q = ("Q", [0, 1, 2, 3, 4, 5], [1] * 6)
    v, res = _play(driver, 8, 6, 5, 2, [ADD8, q, q, q])
    assert res[0]["frame"] == CR.CLOSED and res[0]["neutral"] == [0] * 6 and res[0]["resting"] == [0] * 6
    for r in res[1:]:                                        # the same six again: they verify the place, nothing is used twice
        assert r["frame"] == CR.RESTED and r["neutral"] == [1] * 6 and r["resting"] == [1] * 6
    assert v.stats["closed_frames"] == 1 and v.stats["rested_frames"] == 2 and v.stats["resting"] == 12
    assert v.last_seen[:6] == [3] * 6 and v.used[:6] == [1] * 6 and v.last_seen[6:] == [0, 0]


def test_a_visit_ends_after_gap_calls_without_a_match(driver):
    gap = 2
    q, other = ("Q", [0, 1, 2, 3, 4], [1] * 6), ("Q", [7], [1] * 6)
    # seen at t = 1, again at t = 1 + gap: t - last_seen == gap is still the same visit
    _, res = _play(driver, 8, 6, 5, gap, [ADD8, q] + [other] * (gap - 1) + [q])
    assert res[0]["frame"] == CR.CLOSED and res[-1]["frame"] == CR.RESTED and res[-1]["resting"][:5] == [1] * 5
    # ... and at t = 1 + gap + 1 a new one: fresh again
    _, res = _play(driver, 8, 6, 5, gap, [ADD8, q] + [other] * gap + [q])
    assert res[-1]["frame"] == CR.CLOSED and res[-1]["resting"][:5] == [0] * 5 and res[-1]["neutral"][:5] == [0] * 5
    assert all(r["frame"] == CR.SHORT for r in res[1:-1])


def test_resting_matches_count_towards_min_matches_and_one_fresh_match_closes(driver):
    v, res = _play(driver, 8, 6, 5, 2, [ADD8, ("Q", [0, 1, 2, 3, 4], [1] * 6), ("Q", [0, 1, 2, 3, 4, 5], [1] * 6),
                                        ("Q", [0, 1, 2, 3, 6], [1, 1, 1, 1, 0, 1])])
    assert res[1]["frame"] == CR.CLOSED and res[1]["resting"] == [1, 1, 1, 1, 1, 0] and res[1]["neutral"] == [1, 1, 1, 1, 1, 0]
    assert res[1]["n_fresh"] == 1 and v.used[5] == 1
    assert res[2]["frame"] == CR.SHORT and v.used[6] == 0 and v.last_seen[6] == 3      # four resting and a gated fresh one
    # a match that was kept in a frame that did not close has not been used
    _, r2 = _play(driver, 8, 6, 5, 2, [ADD8, ("Q", [0, 1, 2, 3], [1] * 6), ("Q", [0, 1, 2, 3, 4], [1] * 6)])
    assert r2[0]["frame"] == CR.SHORT and r2[1]["frame"] == CR.CLOSED and r2[1]["resting"][:5] == [0] * 5
    # ... nor has a match the gate dropped in a frame that closed
    _, r3 = _play(driver, 8, 6, 5, 2, [ADD8, ("Q", [0, 1, 2, 3, 4, 5], [1, 1, 1, 1, 1, 0]), ("Q", [5], [1] * 6)])
    assert r3[0]["frame"] == CR.CLOSED and r3[1]["resting"][0] == 0


def test_the_same_key_twice_in_one_call(driver):
    # both positions see the record from before the call: both fresh, both take part; the entry is used once the frame closes
    v, res = _play(driver, 8, 6, 2, 3, [ADD8, ("Q", [4, 4, 1], [1, 0, 1, 1, 1, 1]), ("Q", [4, 4], [1] * 6)])
    assert res[0]["entries"] == [4, 4, 1] and res[0]["resting"] == [0, 0, 0] and res[0]["neutral"][:3] == [0, 1, 0]
    assert v.used[4] == 1 and res[1]["resting"] == [1, 1] and res[1]["frame"] == CR.RESTED
    # used by the second position alone (the first is gated): used all the same
    v, res = _play(driver, 8, 6, 2, 3, [ADD8, ("Q", [4, 4, 1], [0, 1, 1, 1, 1, 1])])
    assert res[0]["neutral"][:3] == [1, 0, 0] and (v.last_seen[4], v.used[4]) == (1, 1)


@pytest.mark.parametrize("gap", [0, 1, 3])
@pytest.mark.parametrize("lc_max", [1, 6])
def test_fuzz_equals_the_restatement(driver, gap, lc_max):
    """40 sequences per shape of up to 14 calls over ten keys; with gap = 0 every call is also held against the rules
    without visits (tests/lcmap_restate.py)"""
    rng = np.random.default_rng(10 * gap + lc_max)
    seen = dict.fromkeys(("resting", "rested_frames", "closed_frames", "short_frames", "gated"), 0)
    for _ in range(40):
        ops = [("A", [int(k) for k in rng.permutation(10)[:int(rng.integers(3, 9))]])]
        for _ in range(int(rng.integers(2, 14))):
            if rng.uniform() < 0.15:
                ops.append(("A", [int(rng.integers(-1, 10)) for _ in range(int(rng.integers(0, 4)))]))
            else:
                ops.append(("Q", [int(rng.integers(-1, 10)) for _ in range(int(rng.integers(0, 9)))],
                            [int(rng.uniform() < 0.85) for _ in range(lc_max)]))
        v, _ = _play(driver, 8, lc_max, int(rng.integers(1, 4)), gap, ops)
        for k in seen:
            seen[k] += v.stats[k]
    assert all(seen[k] > 0 for k in ("closed_frames", "short_frames", "gated")), seen
    assert (seen["resting"] > 0 and seen["rested_frames"] > 0) == (gap > 0), seen


def test_header_stays_plain_cxx():
    text = open(os.path.join(CSRC, "lcmap_device.h")).read()
    for name in ("lcmap_used_now", "lcmap_resting", "lcmap_frame_decide_visit", "lcmap_pair_neutral_visit", "lcmap_used_next",
                 "LCMAP_FRAME_RESTED = 3"):
        assert name in text
    assert text.split("#pragma once")[1].count("#include") == 1


# ---- SequenceConfig
def test_sequence_config_defaults_and_refusals():
    C = sequence.SequenceConfig
    c = C()
    assert (c.lc_point_cov, c.lc_revisit_gap) == (False, 0)
    for kw in (dict(lc_point_cov=True), dict(lc_revisit_gap=3)):                   # refused without loop_closure
        with pytest.raises(ValueError):
            sequence.SequenceRunner(None, C(**kw), 1)
    for kw in (dict(lc_revisit_gap=-1), dict(lc_revisit_gap=2.5), dict(lc_point_cov=2)):
        with pytest.raises(ValueError):
            sequence.SequenceRunner(None, C(loop_closure=True, **kw), 1)
    sequence.SequenceRunner(None, C(loop_closure=True, lc_point_cov=True, lc_revisit_gap=25), 1)
    sequence.SequenceRunner(None, C(loop_closure=True, lc_revisit_gap=1, feature_init="subfilter"), 1)


# ---- the inputs of the GPU gate and update tests mean something: on the oracle alone
def test_gate_case_is_outside_the_gate_with_exact_points_and_inside_with_their_covariance():
    cam = synth.EQUI
    c = CC.gate_case(cam)
    P = c["P"][0]
    H, inn, dR, Res = CC.rows0(c, cam)
    g0 = [R.gamma(H[2 * m:2 * m + 2], P, inn[2 * m:2 * m + 2], LC.RLC) for m in range(6)]
    g1 = [CR.gamma(H[2 * m:2 * m + 2], P, inn[2 * m:2 * m + 2], Res[m]) for m in range(6)]
    print("gamma exact", np.round(g0, 3), "with Sigma", np.round(g1, 3))
    assert [g <= LC.CHI2 for g in g0] == [m != CC.MOVED for m in range(6)] and g0[CC.MOVED] > 3 * LC.CHI2
    assert all(g is not None and g <= LC.CHI2 for g in g1) and 0.5 * LC.CHI2 < g1[CC.MOVED]
    assert all(np.linalg.cond(Re) < 100 for Re in Res)
    # gamma with Sigma = 0 is the exact-point gamma
    z = [CR.gamma(H[2 * m:2 * m + 2], P, inn[2 * m:2 * m + 2], CR.r_eff(H[2 * m:2 * m + 2], np.zeros((3, 3)), LC.RLC)) for m in range(6)]
    assert np.allclose(z, g0, rtol=1e-14)


def test_the_whitened_update_is_the_full_R_joseph_form_and_the_pose_stays_less_certain():
    cam = synth.EQUI
    c = LC.update_case(cam)
    c["ms0"] = [dict(Xs=c["Xs"][0, j], Rsb=c["Rsb_p"][0], Tsb=c["Tsb_p"][0], g_sind=-1, xp=c["queries"][j][2]) for j in range(6)]
    P = c["P"][0]
    H, inn, dR, Res = CC.rows0(c, cam)
    neutral = [False] * 6
    Hw, iw, dw = CR.whiten(H, inn, dR, Res, neutral)
    assert (dw == 1.0).all()
    e1, P1, _ = orc.update_joseph(Hw, P, iw, dw)
    e2, P2 = CR.joseph_full_R(H, P, inn, CR.block_R(Res, neutral, LC.LC_MAX))
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    print("whitened against full R: dx %.2e P %.2e" % (rel(e1, e2), rel(P1, P2)))
    assert rel(e1, e2) < 1e-13 and rel(P1, P2) < 1e-13
    _, P0, _ = orc.update_joseph(H, P, inn, dR)                                    # exact points
    assert (np.diag(P2)[:6] > np.diag(P0)[:6]).all() and (np.diag(P2)[:6] < np.diag(P)[:6]).all()
    # d xp / d Xs = -H_T, by central differences through the restatement's rows
    sc, m0 = c["sc"], c["ms0"][0]
    J = np.zeros((2, 3))
    for k in range(3):
        d = np.zeros(3); d[k] = 1e-6
        ip = R.rows([dict(m0, Xs=m0["Xs"] + d)], sc["Rbc"][0], sc["Tbc"][0], cam, LC.layout(), LC.LC_MAX, LC.RLC)[1][:2]
        im = R.rows([dict(m0, Xs=m0["Xs"] - d)], sc["Rbc"][0], sc["Tbc"][0], cam, LC.layout(), LC.LC_MAX, LC.RLC)[1][:2]
        J[:, k] = -(ip - im) / 2e-6                                                # inn = obs - xp
    assert np.abs(J + H[0:2, 3:6]).max() < 1e-6 * np.abs(H[0:2, 3:6]).max()
