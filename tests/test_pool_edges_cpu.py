"""The cases of tests/test_pool_edges_gpu.py, checked where no GPU is: the fp64 oracle against the np.longdouble restatement of
Feature::SubfilterUpdate on every family (this computes and prints the bounds the GPU test imports), every threshold case in
both arithmetics (same branch, none excluded; the exact cases bit for bit), that the candidate-order pools really hold the tie
groups the GPU test relies on, and the expected orders and medians from Python alone. Host code only."""
import math

import numpy as np
import pytest

import pool_edge_cases as pe
import subfilter_restate as sr
import xivo_oracle as orc
from xivo_amd import lib as L

LD = np.longdouble
MODES = [False, True]


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("invdepth", MODES)
@pytest.mark.parametrize("family", list(pe.FAMILIES))
def test_oracle_is_within_its_bounds_of_the_restatement(family, invdepth):
    worst, bnd = pe.family_bounds(family, invdepth)          # asserts bound < CAP
    n = n_ex = n_out = 0
    kappa = 0.0
    for cam_name in pe.CAMS:
        ref, f64, err = pe.step_reference(family, cam_name, invdepth)
        ex = pe.excluded(ref)
        n += len(ex); n_ex += int(ex.sum()); n_out += int(ref["outlier"].sum())
        kappa = max(kappa, float(ref["kappa"].max()))
        for k in err:
            assert err[k] <= bnd[k] < pe.CAP
        # the decisions: none of them turns on the arithmetic, no case left out
        assert np.array_equal(f64["status"], ref["status"]) and np.array_equal(f64["ic"], ref["ic"])
        assert np.array_equal(f64["cand"], ref["cand"])
        assert np.array_equal(f64["oc"] > 0, ref["outlier"])
        assert set(ref["cand"]) == {0, 1, 3}, (family, cam_name)       # both sides of the candidate tests, both statuses
    assert n == 4 * pe.PER_CAMERA and n_ex <= 0.01 * n
    if family == "outliers":
        assert n_out >= n / 3 and n - n_out >= n / 3, n_out
    if family == "small_R":
        assert kappa > 1e6
    print("%-9s %s: oracle's worst x %.1e P %.1e oc %.1e | bound x %.1e P %.1e oc %.1e | excluded %d / %d, ratio > 1 in %d, "
          "cond(S) <= %.1e" % (family, "inverse depth" if invdepth else "log depth", worst["x"], worst["P"], worst["oc"], bnd["x"],
                               bnd["P"], bnd["oc"], n_ex, n, n_out, kappa))


@pytest.mark.parametrize("invdepth", MODES)
def test_carried_chain_stays_within_the_cap(invdepth):
    """three steps fed back through the oracle's own output: non-zero counters and non-diagonal P throughout, every step's
    bound below the cap (on the GPU the chain is fed by the device, and its bounds are taken on those inputs)"""
    for cam_name in pe.CAMS:
        chain = pe.carried_oracle_chain(cam_name, invdepth)
        assert len(chain) == 3
        for prior, ref, err in chain:
            assert (np.abs(prior["P"][:, 0, 2]) > 0).all() and (prior["ic"] > 0).all()
            assert pe.excluded(ref).mean() <= 0.01
            for k in err:
                pe.bound(err[k])
        assert (chain[1][0]["oc"] > 0).any() and (chain[2][0]["oc"] > 0).any()


def test_restatement_in_fp64_is_the_oracle():
    """the restatement run in np.float64 follows the oracle's lines: rounding-level agreement on a nominal draw"""
    c = pe.draw("nominal", "radtan", False)
    o = pe.opts_of("nominal")
    for i in range(16):
        args = (c["x"][i], c["P"][i], c["xp"][0, i], c["Rsb"][0, i], c["Tsb"][0, i], pe.RBC, pe.TBC, c["Rsbr"][i], c["Tsbr"][i],
                pe.CAMS["radtan"], o["Rtri"], o["MH_thresh"], o["ready_steps"], int(c["ic"][i]), float(c["oc"][i]), False)
        r = sr.subfilter_update(*args, T=np.float64)
        x, P, st, ic, oc = orc.subfilter_update(*args)
        d = np.sqrt(np.diag(c["P"][i]))
        assert np.abs((r["x"] - x) / d).max() < 1e-12 and np.abs((r["P"] - P) / np.outer(d, d)).max() < 1e-12
        assert (r["status"], r["init_counter"]) == (st, ic) and abs(float(r["outlier_counter"]) - oc) < 1e-12 * max(1.0, oc)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("invdepth", MODES)
def test_exact_cases_reproduce_bit_for_bit_in_the_oracle(invdepth):
    z = pe.exact_z(invdepth)
    for name, pixel, over, (ic, oc), (want_oc, want_st, want_cand) in pe.exact_cases(invdepth):
        o = dict(pe.PERMISSIVE, **over)
        x, P, st, ic2, oc2 = pe.exact_oracle(invdepth, pixel, o["ready_steps"], ic, oc)
        assert x.tobytes() == pe.exact_x(invdepth).tobytes() and not P.any(), name
        assert oc2 == want_oc and st == want_st and ic2 == ic + 1, (name, oc2)
        c1, c2 = orc.candidate_flags(x, st, oc2, o["min_depth"], o["max_depth"], o["max_subfilter_outlier"], invdepth)
        assert (1 if c1 else 0) | (2 if c2 else 0) == want_cand, name
        I3, z3 = np.eye(3), np.zeros(3)
        r = sr.subfilter_update(pe.exact_x(invdepth), np.zeros((3, 3)), pixel, I3, z3, I3, z3, I3, z3, pe.EXACT_CAM, pe.EXACT_RTRI,
                                pe.EXACT_MH, o["ready_steps"], ic, oc, invdepth)
        assert float(r["z"]) == z and r["outlier"] == (pixel == pe.EXACT_OVER)
        # (1/2 + (4 + 2^-40)^2 / 32 is 1 + 2^-42 + 2^-85: the last term is below the 64-bit mantissa too)
        assert r["ratio"] == (LD(pe.EXACT_RATIO_OVER) if r["outlier"] else 1), name
        assert r["status"] == want_st and r["outlier_counter"] == LD(want_oc)
        assert sr.candidate_bits(r["outlier_counter"], r["z"], r["status"], o["min_depth"], o["max_depth"],
                                 o["max_subfilter_outlier"]) == want_cand, name
    assert math.sqrt(pe.EXACT_RATIO_OVER) == 1.0 + 2.0 ** -43


@pytest.mark.parametrize("invdepth", MODES)
def test_straddling_thresholds_decide_alike_in_both_arithmetics(invdepth):
    seen = set()
    for cam_name in pe.CAMS:
        c, prior, ref, idx = pe.straddle_cases(cam_name, invdepth)
        for i in idx:
            for name, side, o, expect in pe.straddle_opts(ref, prior, i):
                args = (prior["x"][i], prior["P"][i], c["xp"][0, i], c["Rsb"][0, i], c["Tsb"][0, i], pe.RBC, pe.TBC, c["Rsbr"][i],
                        c["Tsbr"][i], pe.CAMS[cam_name], o["Rtri"], o["MH_thresh"], o["ready_steps"], int(prior["ic"][i]),
                        float(prior["oc"][i]), invdepth)
                r = sr.subfilter_update(*args)
                x, P, st, ic, oc = orc.subfilter_update(*args)
                cl = sr.candidate_bits(r["outlier_counter"], r["z"], r["status"], o["min_depth"], o["max_depth"], o["max_subfilter_outlier"])
                c1, c2 = orc.candidate_flags(x, st, oc, o["min_depth"], o["max_depth"], o["max_subfilter_outlier"], invdepth)
                if "outlier" in expect:
                    assert r["outlier"] == expect["outlier"] == (oc > 0), (cam_name, i, name, side)
                else:
                    assert bool(cl & 1) == expect["cand0"] == bool(c1), (cam_name, i, name, side)
                    assert bool(cl & 2) == bool(c2)
                seen.add((name, side, expect.get("outlier", expect.get("cand0"))))
    assert len(seen) == 8          # four thresholds, both sides, the two sides deciding differently


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("pm", pe.ORDER_POOL_MAX)
def test_order_pools_hold_their_ties(built, pm):
    sc = pe.order_scene(pm)
    ent, live = pe.simulate_order_scene(sc)
    assert (live == (sc["kind"] != "F")).all()
    for strict in (False, True):
        order, n, keys = pe.python_order(ent, live, strict)
        biggest, crosses = pe.tie_report(keys, pm)
        assert biggest >= min(3, pm), (pm, strict, biggest)          # a tie group of three or more (the whole pool below 3)
        assert crosses or pm < 2, (pm, strict)                       # a tie across position pm // 2
        assert n[1] == pm and list(order[1]) == list(range(pm))      # all ties: entry order
        assert n[2] == (0 if strict else 1) and (strict or order[2, 0] == pm // 2)
        # the host function: the same order, ties in list order, on the same entries
        e2 = ent.copy()
        e2["candidate"] = np.where(live, ent["candidate"], 0)
        oh, nh, _ = L.candidate_order(e2, strict=strict)
        assert np.array_equal(oh, order) and np.array_equal(nh, n)
    if pm >= len(pe.MIX):
        _, n0, keys = pe.python_order(ent, live, False)
        ranks = {k[0] for k in keys[0]}
        assert ranks == {-2, -1}                                     # READY and INITIALIZING both present in the mix
        kinds = set(sc["kind"][0])
        assert kinds == set(pe.MIX)
        wild = sc["kind"][0] == "W"
        assert not (ent[0]["candidate"][wild] & 1).any()             # the wild pixel fails the outlier test
        passing = {e for _, _, e in keys[0]}
        assert all((e in passing) for e in range(pm) if sc["kind"][0, e] in ("T", "Z", "LT", "LZ"))


def test_host_candidate_order_scores(built):
    """the three `comparison_score_type` values on the entries of a tie-laden pool (the order ignores them, as coded)"""
    sc = pe.order_scene(65)
    ent, live = pe.simulate_order_scene(sc)
    base = None
    for t in range(3):
        order, n, score = L.candidate_order(ent, strict=False, score_type=t)
        for b in range(ent.shape[0]):
            for e in range(ent.shape[1]):
                P = ent[b, e]["P"].reshape(3, 3).T
                assert score[b, e] == orc.candidate_scores(P, float(ent[b, e]["outlier_counter"]))[t] or \
                    abs(score[b, e] - orc.candidate_scores(P, float(ent[b, e]["outlier_counter"]))[t]) <= 4e-16 * abs(score[b, e])
        base = order if base is None else base
        assert np.array_equal(order, base)
    with pytest.raises(L.XivoHipError):
        L.candidate_order(ent, score_type=3)


# ---------------------------------------------------------------- D
def test_adapt_scene_holds_its_cases():
    sc = pe.adapt_scene()
    names = sc["names"]
    sim2, sim3 = pe.adapt_sim_entries(sc, 2), pe.adapt_sim_entries(sc, 3)
    n = [len(pe.adapt_depths(sc["feats"][b], sim2, b, 1)) for b in range(sc["B"])]
    assert n[:8] == [0, 1, 2, 3, 255, 256, 257, pe.ADAPT_F + pe.ADAPT_PM]
    med = [pe.adapt_expected(pe.adapt_depths(sc["feats"][b], sim2, b, 1), 0.0, 1.0, -np.inf, np.inf)[0] for b in range(sc["B"])]
    assert med[2] == 1.0 / (1.0 / 3.0) and med[0] == 0.0
    b = names.index("all depths equal")
    assert n[b] == 10 and med[b] == 2.0
    b = names.index("duplicates of the median on both sides of rank n / 2")
    d = np.sort(pe.adapt_depths(sc["feats"][b], sim2, b, 1))
    assert (d[n[b] // 2 - 5:n[b] // 2 + 6] == d[n[b] // 2]).all() and d[n[b] // 2 - 6] < d[n[b] // 2] < d[n[b] // 2 + 6]
    # non-finite depths: left out, and each one would move its filter's median if it were counted
    for name, extra, count in (("+inf depth is left out", np.inf, 7), ("NaN x[2] is left out", None, 7), ("-inf depth is left out", -np.inf, 6)):
        b = names.index(name)
        x2 = sc["feats"][b]["x"][0, 2]
        with np.errstate(all="ignore"):
            assert n[b] == count and not np.isfinite(1.0 / x2) and (extra is None or 1.0 / x2 == extra)
        d = np.sort(pe.adapt_depths(sc["feats"][b], sim2, b, 1))
        counted = np.sort(np.append(d, extra))[(count + 1) // 2] if extra is not None else d[(count + 1) // 2]
        assert counted != d[count // 2] == med[b], name
    # selection: every rule moves the median of its filter
    b = names.index("selection")
    m = lambda sim, life: float(np.sort(pe.adapt_depths(sc["feats"][b], sim, b, life))[len(pe.adapt_depths(sc["feats"][b], sim, b, life)) // 2])
    assert (m(sim2, 1), m(sim2, 0), m(sim2, -1), m(sim3, 1), m(sim3, 0)) == (1.0 / (1.0 / 3.0), 1.0 / (1.0 / 4.5), 1.0 / (1.0 / 4.5),
                                                                          1.0 / (1.0 / 4.5), 1.0 / (1.0 / 4.8))
    assert (sim2["status"][b][sim2["live"][b]] == 0).sum() == 6 and (~sim2["live"][b] & (sim2["init_counter"][b] > 0)).sum() == 4
    # the range rules: the smallest and the largest median of the launch
    lo, hi = names.index("median == min_z"), names.index("median == max_z")
    others = [med[i] for i in range(1, sc["B"]) if i not in (lo, hi)]
    assert med[lo] < min(others) and med[hi] > max(others) and n[lo] % 2 == 1
    assert sum(1 for k in n if k and k % 2 == 0) >= 3 and sum(1 for k in n if k % 2 == 1) >= 3
