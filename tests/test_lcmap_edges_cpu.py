"""CPU-only: the inputs of tests/test_lcmap_edges_gpu.py sit where they claim, on the oracle and the 80-bit restatement alone
(tests/lcmap_edge_cases.py): every derived bound is under the cap, the ill-conditioned families reach their kappa, no gamma is
near chi2, fp64 and 80-bit decide alike at every straddled threshold, the capacity scripts hit the positions they name, and the
pivot case separates its two pivots."""
import numpy as np
import pytest

import lcmap_cases as LC
import lcmap_edge_cases as E
import lcmap_restate as R

LD = E.LD


def test_every_bound_is_derived_and_under_the_cap():
    b = E.bounds()
    for line in E.table_lines():
        print(line)
    print("added: xs %.2e sigma %.2e" % (b["added"]["xs"], b["added"]["sigma"]))
    for name in E.FAMILIES:
        for q in E.QUANTITIES:
            assert E.FLOOR <= b[name][q] < E.CAP, (name, q, b[name][q])
            assert b[name][q] == max(4.0 * E.oracle_worst(name)[q], E.FLOOR)
    assert E.FLOOR <= b["added"]["xs"] < E.CAP and E.FLOOR <= b["added"]["sigma"] < E.CAP


def test_the_ill_conditioned_families_reach_their_kappa():
    kS = np.concatenate([E.reference("illcond", c)["kappa_S"].ravel() for c in E.CAMS])
    kR = np.concatenate([E.reference("aniso", c)["kappa_Re"].ravel() for c in E.CAMS])
    print("kappa_2(S_f): max %.2e, %.0f %% >= 1e5; kappa_2(R_e): max %.2e, %.0f %% >= 1e5"
          % (kS.max(), 100 * (kS >= 1e5).mean(), kR.max(), 100 * (kR >= 1e5).mean()))
    assert kS.max() >= 1e5 and (kS >= 1e5).mean() > 0.25 and kS.max() <= 1.01 * E.KAPPA_S
    assert kR.max() >= 1e5 and (kR >= 1e5).mean() > 0.25 and kR.max() <= 1.01 * E.KAPPA_RE + 1
    for c in E.CAMS:                                                   # the certain filter: S_f is Rlc I
        assert E.reference("certain", c)["kappa_S"].max() < 1 + 1e-6
        assert E.reference("nominal", c)["kappa_Re"].max() == 1.0


@pytest.mark.parametrize("name", E.FAMILIES)
def test_no_gamma_is_near_chi2_and_both_precisions_decide_alike(name):
    near = total = 0
    for c in E.CAMS:
        g80 = E.reference(name, c)["gamma"].astype(np.float64)
        g64 = E.oracle_rows(E.family(name, c))["gamma"]
        assert np.isfinite(g64).all() and (g80 > 0).all()
        close = np.abs(g80 / E.CHI2 - 1) < E.OFF
        near += int(close.sum()); total += g80.size
        assert np.array_equal((g64 <= E.CHI2)[~close], (g80 <= E.CHI2)[~close])
    assert near == 0, near                                             # (the issue allows 1 %: the draw needs none)
    assert total == 4 * E.NB * E.NP


def test_the_families_are_what_they_say():
    for c, cam in E.CAMS.items():
        for name, (lo, hi) in (("nominal", (2.0, 8.0)), ("far", (20.0, 50.0)), ("edge", (0.3, 1.0))):
            f = E.family(name, c)
            assert f["Xs"].shape == (E.NB, E.NP, 3) and set(np.unique(f["g"])) == {-1, 0, 1, 2, 3}
            for b in (0, 17, E.NB - 1):
                for m in range(E.NP):
                    Ro, To = E.observer(f["sc"], b, int(f["g"][b, m]))
                    Xcn = f["sc"]["Rbc"][b].T @ (Ro.T @ (f["Xs"][b, m] - To) - f["sc"]["Tbc"][b])
                    assert lo * (1 - 1e-9) <= Xcn[2] <= hi * (1 + 1e-9), (name, c, b, m, Xcn)
                    if name == "edge":                                 # 0.9 of the way to the nearest border
                        px = E.reference(name, c)["xp"][b, m] - np.array([cam["cx"], cam["cy"]])
                        r = 0.9 * min(cam["cx"], cam["cols"] - cam["cx"], cam["cy"], cam["rows"] - cam["cy"])
                        assert abs(np.linalg.norm(px) / r - 1) < 1e-6
        P = E.family("nominal", c)["P"]
        sd = np.sqrt(np.diagonal(P, axis1=1, axis2=2))
        assert (np.rad2deg(sd[:, 0:3]) >= 1 - 1e-9).all() and (np.rad2deg(sd[:, 0:3]) <= 3 + 1e-9).all()
        assert (sd[:, 3:6] >= 0.01 - 1e-12).all() and (sd[:, 3:6] <= 0.10 + 1e-12).all()
        assert np.abs(E.family("certain", c)["P"]).max() <= 1.0001e-12
        for name in E.COV_FAMILIES:
            S = E.family(name, c)["Sigma"]
            assert np.linalg.eigvalsh(S).min() > 0


@pytest.mark.parametrize("camname", list(E.CAMS))
def test_chi2_straddle_decides_alike_in_both_precisions(camname):
    """chi2 = the 80-bit gamma of a match (1 -+ 1e-6): the oracle's gamma is kept on one side and gated on the other"""
    f = E.family("nominal", camname)
    g80, g64 = E.reference("nominal", camname)["gamma"], E.oracle_rows(f)["gamma"]
    for b in range(E.NB):
        for m in range(E.NP):
            lo, hi = float(g80[b, m] * (1 - LD(E.OFF))), float(g80[b, m] * (1 + LD(E.OFF)))
            assert not R.kept(g64[b, m], lo) and R.kept(g64[b, m], hi)
            assert not (g80[b, m] <= LD(lo)) and g80[b, m] <= LD(hi)
    assert E.bounds()["nominal"]["gamma"] < 0.01 * E.OFF               # the device's bound leaves the margin alone


@pytest.mark.parametrize("map_max", E.ADD_MAP_MAX)
def test_add_scripts_hit_the_positions_they_name(map_max):
    m = R.MapRestate(map_max, 6, 5)
    c1, c2 = E.add_script(map_max, 0)
    d1 = m.add([(k, True, False, None) for _, k in c1])
    assert len(m.keys) == map_max and d1.count(R.FULL) == 2 and d1.count(R.ACCEPT) == map_max
    assert d1.count(R.DUP) == (2 if map_max == 130 else 0)
    if map_max == 130:                                                 # the record behind positions 65 and 127 repeats them
        for p in (65, 127):
            i = [k for _, k in c1].index(m.keys[p])
            assert d1[i] == R.ACCEPT and d1[i + 1] == R.DUP and c1[i + 1][1] == m.keys[p]
    d2 = m.add([(k, True, False, None) for _, k in c2])
    assert d2[:-1] == [R.DUP] * (len(c2) - 1) and d2[-1] == R.FULL
    want = [p for p in (0, 63, 64, map_max - 1) if p < map_max]
    assert sorted(set(m.keys.index(k) for _, k in c2[:-1])) == sorted(set(want))
    assert all(0 <= j < E.NF for j, _ in c1 + c2)


@pytest.mark.parametrize("lc_max", E.MATCH_LC_MAX)
def test_match_scripts_fill_the_list_where_they_say(lc_max):
    seen = dict(last_of_first=0, first_of_second=0, third=0, twice=0, negative=0, absent=0, empty_between=0)
    for b, (n, t) in enumerate(zip(E.MATCH_COUNTS, E.MATCH_FILL_AT)):
        m = R.MapRestate(E.MATCH_ENTRIES, lc_max, 1)
        m.keys = E.match_map_keys(b)
        q = E.match_queries(lc_max, b)
        assert len(q) == n
        slots, lst = m.match(q)
        if t is not None and t < n and t >= lc_max - 1:
            assert slots[t] == lc_max - 1 and len(lst) == lc_max, (b, t)       # query t takes the last list position
            seen["last_of_first"] += t == 63; seen["first_of_second"] += t == 64; seen["third"] += t >= 128
            assert m.stats["surplus"] >= 1 or t == n - 1                       # (no query behind the filling one: no surplus)
        ents = [e for _, e in lst]
        seen["twice"] += len(set(ents)) < len(ents) or any(q.count(k) > 1 and k in m.keys for k in q)
        seen["negative"] += any(k < 0 for k in q); seen["absent"] += any(k >= 0 and k not in m.keys for k in q)
    assert E.MATCH_COUNTS[1] == 0 and E.MATCH_COUNTS[0] > 64 and E.MATCH_COUNTS[2] > 64
    assert set(E.MATCH_COUNTS) == {0, 1, 63, 64, 65, 128, 130, 200}
    assert seen["last_of_first"] and seen["first_of_second"] and seen["third"] and seen["twice"] and seen["negative"] and seen["absent"], seen


def test_pivot_case_separates_the_two_pivots():
    """on the oracle's rows (the GPU test repeats this on the rows the device staged): P = -c I moves s00 through zero on filter 0
    with the Schur pivot positive on the positive side, and on filter 1 leaves s00 positive with a negative Schur pivot"""
    f = E.pivot_case()
    H = E.oracle_rows(f, P=None)["H"]
    cols = E.pair_cols(-1)
    h0, h1 = H[0][:, cols], H[1][:, cols]
    assert h0[0] @ h0[0] > h0[1] @ h0[1] and h1[1] @ h1[1] > h1[0] @ h1[0]
    c_pos, c_neg, mid = E.pivot_cs(h0)
    assert mid is None
    assert E.pivots_ld(h0, c_pos)[:2] == (True, True) and E.pivots_ld(h0, c_neg)[:2] == (False, False)
    _, _, mid = E.pivot_cs(h1)
    assert mid is not None and E.pivots_ld(h1, mid)[:2] == (True, False)
    assert E.pivots_ld(h1, 0.5 * E.RLC / float(h1[1] @ h1[1]))[:2] == (True, True)
    # fp64 agrees with 80-bit on all four signs (margins of 1e-3 against a rounding of 1e-16)
    for h, c in ((h0, c_pos), (h0, c_neg), (h1, mid)):
        S = E.RLC * np.eye(2) - c * (h @ h.T)
        assert (bool(S[0, 0] > 0), bool(S[0, 0] > 0 and S[1, 1] - S[1, 0] ** 2 / S[0, 0] > 0)) == E.pivots_ld(h, c)[:2]


def test_depth_variance_straddle():
    for var in (1e-8, 3.7e-4, 2.0):
        assert not R.is_poor(var, var * (1 + E.OFF)) and R.is_poor(var, var * (1 - E.OFF)) and not R.is_poor(var, var)
