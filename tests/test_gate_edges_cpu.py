"""What tests/test_gate_edges_gpu.py rests on, checked without a GPU: every case of tests/gate_edge_cases.py sits where it claims -
the conditioning class, the margin next to the threshold, the number of relaxations and why the loop stopped, the tie, the RANSAC
frame state and temporary reference - the fp64 oracle and the 80-bit restatement (tests/gate_restate.py) decide alike on every
case, the family-A bounds are the ones written down, and the norm-tie fixture says what the summary says it does. A case whose
preconditions fail fails here; nothing is skipped at run time on the GPU."""
import os

import numpy as np
import pytest

import gate_edge_cases as gc
import gate_restate as gr
import xivo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = gc.LEVELS


# ---------------------------------------------------------------- the restatement itself
def test_restated_loop_is_the_oracle_loop():
    """gate_restate.relax against orc.mh_gate (pinned to the extracted MHGating, test_oracle_pinned.py) wherever the reference's
    loop ends by itself"""
    rng = np.random.default_rng(1)
    for k in range(200):
        F = int(rng.integers(1, 12))
        d = rng.uniform(0, 40, size=F)
        th, mult, mi = float(rng.uniform(0.5, 8)), float(rng.choice([1.1, 1.5, 2.0])), int(rng.integers(1, F + 1))
        rec = gr.relax(d, th, mult, mi)
        m, _, used = orc.mh_gate(d, th, mult, mi)
        assert rec["stop"] == gr.STOP_MIN_INLIERS and np.array_equal(rec["mask"], m) and rec["thresh"] == used, k


def test_fused_and_unfused_norm_differ_as_the_issue_found():
    """about 8 % of random 2-vectors, both directions; the fused form agrees with an exact evaluation rounded once"""
    rng = np.random.default_rng(2)
    r = rng.normal(size=(4000, 2))
    d = np.array([np.sign(gr.norm_fused(a, b) - gr.norm_unfused(a, b)) for a, b in r])
    assert 0.04 < (d != 0).mean() < 0.16 and (d < 0).sum() > 50 and (d > 0).sum() > 50


def test_distance_80_agrees_with_the_oracle_on_easy_inputs():
    ev = gc.evaluate(gc.family_b("update", "easy"))
    assert gc.rel_err(ev["d64"], ev["d80"]).max() < 64 * gc.U and ev["kappa"].max() < 1e3


# ---------------------------------------------------------------- family A
@pytest.mark.parametrize("level", LEVELS)
def test_family_a_classes_sit_where_they_claim(level):
    c = gc.family_a(level)
    ev = gc.evaluate(c)
    for b, cls in enumerate(gc.CLASSES):
        k = ev["kappa"][b]
        if cls in gc.KAPPA_TARGET:
            t = gc.KAPPA_TARGET[cls]
            assert t / 30 < np.median(k) < t * 30 and k.max() > t / 3, (cls, k)
        if cls == "r_dominates":
            for f in range(c.F):
                JPJ = c.J[b, f] @ c.P[b] @ c.J[b, f].T
                assert np.abs(JPJ).max() < c.R / 10, (f, JPJ)
        if cls == "decades":
            v = np.diag(c.P[b])
            assert v.min() < 2e-12 and v.max() > 1e4 and min(np.abs(np.linalg.eigvalsh(c.J[b, f] @ c.P[b] @ c.J[b, f].T)).min() for f in range(c.F)) > 100 * c.R
    assert ev["kappa"].max() > 1e12 / 3 and ev["kappa"][0].min() < 1e3      # 1e2 .. 1e12 in steps of two decades
    mag = np.linalg.norm(c.inn, axis=-1)
    assert mag.min() < 1.01e-6 and mag.max() > 0.99e3
    assert np.isfinite(ev["d64"]).all() and (ev["d80"] > 0).all()


def test_bounds_table_is_the_one_written_down():
    """4 x the oracle's worst error per class, floored - and the table in the case module's docstring and in DESIGN section 5 is
    this one, line by line"""
    b = gc.bounds()
    for level in LEVELS:
        ev = gc.evaluate(gc.family_a(level))
        for k, cls in enumerate(gc.CLASSES):
            assert b[level][cls] == max(4.0 * gc.rel_err(ev["d64"][k], ev["d80"][k]).max(), gc.FLOOR) >= gc.FLOOR
        assert b[level]["easy"] < 64 * gc.U
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    print("\n".join(gc.bounds_table_lines()))
    for line in gc.bounds_table_lines():
        assert line in gc.__doc__, line
        assert line in design, line


# ---------------------------------------------------------------- family B
@pytest.mark.parametrize("cls", gc.B_CLASSES)
@pytest.mark.parametrize("level", LEVELS)
def test_family_b_margins(level, cls):
    c = gc.family_b(level, cls)
    m = c.margin
    assert m == max(1e-6, 100.0 * gc.bounds()[level][cls]) and m < 1e-2
    ev = gc.evaluate(c)
    for b in range(c.B):
        k, inside = c.expect[b]["feature"], c.expect[b]["inlier"]
        ratio = float(ev["d80"][b, k] / gc.LD(c.thresh))
        assert abs(ratio - (1.0 - m if inside else 1.0 + m)) < m / 10, (b, ratio, m)
        rec = ev["rec"][b]
        assert rec["relaxations"] == 0 and rec["stop"] == gr.STOP_MIN_INLIERS
        assert bool(ev["mask"][b, k]) == inside
        # the fp64 oracle decides as the 80-bit restatement does
        assert np.array_equal(gr.relax(ev["d64"][b], c.thresh, c.mult, c.min_inliers)["mask"], ev["mask"][b])
        # no other distance within m of any threshold the loop visits
        for th in rec["visited"]:
            others = np.delete(np.asarray(ev["d80"][b], dtype=np.float64), k)
            assert (np.abs(others / th - 1.0) > 10 * m).all(), (b, th)


# ---------------------------------------------------------------- family D
@pytest.mark.parametrize("name", gc.D_NAMES)
@pytest.mark.parametrize("level", LEVELS)
def test_family_d_branches(level, name):
    c = gc.d_call(name, level)
    ev = gc.evaluate(c)
    got = np.asarray(ev["d80"], dtype=np.float64)
    assert (np.abs(got / c.targets - 1.0)[c.here] < 1e-9).all()
    for b in range(c.B):
        ex, rec = c.expect[b], ev["rec"][b]
        full = c.here[b].all()
        if ex.get("no_gating_feature") and level in gc.SCENE_LEVELS:
            assert rec is None and np.array_equal(ev["mask"][b], c.here[b]) and not ev["dist"][b].any()
            assert c.here[b].sum() == c.min_inliers
            continue
        assert rec is not None
        if level in gc.SCENE_LEVELS:
            assert c.here[b].sum() > c.min_inliers
        if level in gc.SCENE_LEVELS or full:
            assert rec["relaxations"] == ex["relaxations"] and rec["stop"] == ex["stop"], (c.tags[b], rec["relaxations"], rec["stop"])
        for f in ex.get("out", []):
            assert not ev["mask"][b, f] and rec["thresh"] < got[b, f] < rec["thresh"] * c.mult     # between this threshold and the next
        if ex.get("all_in"):
            assert ev["mask"][b].all() and len(rec["visited"]) > 1 and not (got[b] < rec["visited"][-2]).any()
        if rec["stop"] == gr.STOP_MIN_INLIERS and "exact" in c.tags[b]:
            assert ev["mask"][b].sum() == c.min_inliers
        # fp64 and 80 bits decide alike, and nothing sits within 1e-6 of a threshold the loop visits
        d64 = np.where(c.here[b], ev["d64"][b], np.inf) if level in gc.SCENE_LEVELS else ev["d64"][b]
        assert np.array_equal(gr.relax(d64, c.thresh, c.mult, c.min_inliers, int(c.here[b].sum()) if level in gc.SCENE_LEVELS else c.F)["mask"], ev["mask"][b])
        for th in set(rec["visited"]):
            assert (np.abs(got[b][c.here[b]] / th - 1.0) > 1e-6).all(), (c.tags[b], th)
    if name == "branches":
        # present == min_inliers: the two levels differ by construction (the update level takes present = F and gates the zero
        # innovations in); everything present: they agree
        f, u = gc.evaluate(gc.d_call(name, "feature")), gc.evaluate(gc.d_call(name, level if level not in gc.SCENE_LEVELS else "update"))
        tags = gc.d_call(name, "feature").tags
        b0 = next(b for b, t in tags.items() if t == "present_eq_min"); b1 = next(b for b, t in tags.items() if t == "rules_agree")
        assert not np.array_equal(f["mask"][b0], u["mask"][b0]) and f["mask"][b0][0] and not u["mask"][b0][0]
        assert u["mask"][b0][[1, 3, 4, 6, 7]].all()          # the zero innovations of absent entries: distance 0, inliers
        assert np.array_equal(f["mask"][b1], u["mask"][b1])
    if name == "mult_1":
        assert ev["rec"][0]["thresh"] == c.thresh and ev["mask"][0].sum() == 1 < c.min_inliers


def test_wide_calls_put_the_inliers_in_the_second_pass():
    c = gc.d_call("f65", "update")
    ev = gc.evaluate(c)
    assert c.F == 65 and np.nonzero(ev["mask"][0])[0].tolist() == [64] and np.nonzero(ev["mask"][1])[0].tolist() == [63, 64]
    c = gc.d_call("f64", "feature")
    assert c.F == 64 and np.nonzero(gc.evaluate(c)["mask"][0])[0].tolist() == [63]


# ---------------------------------------------------------------- family E
def _host_run(c):
    xp = c.pred + c.noise
    inn = xp - c.pred
    mh = c.host_mh(inn)
    return xp, inn, mh, c.expect(xp, inn, mh)


@pytest.mark.parametrize("make", [gc.e_states, gc.e_ref_ties, gc.e_mask_width], ids=lambda f: f.__name__)
def test_family_e_states_and_references(make):
    c = make()
    xp, inn, mh, ex = _host_run(c)
    for b, e in enumerate(ex):
        dec = e["dec"]
        assert dec["state"] == c.expect_state[b], (c.tags[b], dec["state"])
        kinds = c.kinds[b]
        live = ~(c.absent[b] | c.absent_after[b])
        assert np.array_equal(mh[b], ~c.absent[b] & (kinds != gc.FAR))                 # the gate in front keeps what the case planned
        assert np.array_equal(dec["low"], live & mh[b] & (kinds == gc.LOW))
        # no innovation norm within 0.05 px of the threshold: the device's own innovations decide alike
        n = np.linalg.norm(inn[b], axis=-1)
        assert (np.abs(n - c.thresh) > 0.05).all()
        # no rescue distance within 1e-3 of chi2
        assert all(abs(d / c.chi2 - 1.0) > 1e-3 for d in e["chi"].values()), (c.tags[b], e["chi"])
        if b in c.expect_tmpref:
            assert dec["tmpref"] == c.expect_tmpref[b], (c.tags[b], dec["tmpref"])
    if c.name == "E_states":
        assert 0 in ex[7]["dec"]["zero_groups"] and ex[7]["dec"]["tmpref"] != 0        # the gauge group itself is zeroed
        # the rescue margin (test_rescue_next_to_chi2_and_at_the_tie): chi2 = d80 (1 -+ m) - the fp64 oracle and the 80-bit
        # distance decide alike there, and no other rescue distance of the call lies within m of either chi2
        m = gc.rescue_margin(ex)
        assert m == 1e-6, m                                   # (the oracle is within 2.5e-9 of the 80-bit distance on these priors)
        for b, f in gc.RESCUE_PICKS:
            assert ex[b]["dec"]["state"] == (1 if b == 3 else 2) and f in ex[b]["chi"]
            d80 = float(ex[b]["chi80"][f])
            for chi2, kept in ((d80 * (1 + m), True), (d80 * (1 - m), False)):
                assert bool(gr.rescue(ex[b]["chi"][f], chi2)) == kept == bool(ex[b]["chi80"][f] < chi2)
                for b2, e in enumerate(ex):
                    for f2, d in e["chi80"].items():
                        assert (b2, f2) == (b, f) or abs(float(d) / chi2 - 1.0) > 10 * m, (b, f, b2, f2)
                        assert bool(gr.rescue(e["chi"][f2], chi2)) == bool(d < chi2)
        assert ex[5]["dec"]["mh"].sum() == 6 and not ex[5]["keep"][[1, 2]].any()
        assert sum(len(e["chi"]) for e in ex) > 10 and sum(e["nrej"] for e in ex) >= 1
    if c.name == "E_ref_ties":
        # the chi-square of the rescued features tells which group was zeroed: a wrong choice moves them by far more than the
        # GPU test's 1e-7
        a, b2 = ex[0]["chi"], ex[2]["chi"]
        assert ex[0]["dec"]["tmpref"] != ex[2]["dec"]["tmpref"] and max(abs(a[k] / b2[k] - 1.0) for k in a) > 1e-2
        g = c.lay.group_begin
        for b in (0, 2, 3, 4, 5):
            s1, s2 = gr.group_cov(c.P[b], g, 1), gr.group_cov(c.P[b], g, 2)
            assert (s1 == s2) == (b == 0) and abs(s1 - s2) <= np.spacing(s1)
        assert gr.group_cov(c.P[1], g, 0) == gr.group_cov(c.P[1], g, 1) == gr.group_cov(c.P[1], g, 2)
    if c.name == "E_mask_width":
        assert c.lay.n_groups == 64 and set(np.unique(c.sc["ref"])) == set(gc.WIDE_SLOTS) and ex[0]["dec"]["tmpref"] >= 32
        assert ex[2]["dec"]["zero_groups"] == [32, 63] and ex[3]["dec"]["zero_groups"] == [31, 32, 63] and ex[1]["dec"]["zero_groups"] == []


def test_norm_tie_candidates_exist_in_the_seeded_scene():
    c = gc.e_ties_call()
    found, count = gc.find_tie_pixels(c.pred[0])
    assert count == {-1: 2, 1: 2}, count
    for f, xp, r, u, d in found:
        assert np.array_equal(xp - c.pred[0, f], r)              # one IEEE subtraction: what the Jacobian pass forms
        assert (gr.norm_fused(*r) < u) == (d < 0) and gr.norm_fused(*r) != u
        assert not gr.low_unfused(r, u) and gr.low_unfused(r, np.nextafter(u, np.inf))
        assert gr.low_fused(r, u) == (d < 0)                     # the contracted norm decides differently at the tie where it is smaller
        others = np.delete(np.linalg.norm(c.noise[0], axis=-1), f)
        assert (np.abs(others - u) > 1e-3).all()


# ---------------------------------------------------------------- the norm-tie fixture
def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_gate", os.path.join(ROOT, "tests", "golden", "make_golden_gate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_norm_tie_fixture_outcome():
    """tests/golden/gate_ties.npz (make_golden_gate.py): both extracted builds agree in every bit - decisions and the norm they
    compare - and that norm is NOT a norm of the Jacobian pass's innovation in any of the three forms: the reference evaluates
    Predict a second time (update.cpp:248). Its decision at a one-ulp tie of the device's innovation is therefore not defined
    by the device's inputs; the explicit unfused form is what the project pins."""
    mg = _generator()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gate_ties.npz"))
    assert np.array_equal(g["keep_v3"], g["keep_v4"]) and np.array_equal(g["norm_v3"], g["norm_v4"])
    kinds = set("+".join(g["kinds"]).split("+"))
    assert kinds == set(mg.KINDS)
    off = (g["norm_v3"] - g["U"]) / np.spacing(g["U"])
    forms = np.array([[gr.norm_unfused(*r), gr.norm_fused(*r), mg.norm_fused_b(*r)] for r in g["r"]])
    assert np.abs((forms - g["U"][:, None]) / np.spacing(g["U"])[:, None]).max() == 1.0
    hit = [(g["norm_v3"][k] == forms[k]).any() for k in range(len(off))]
    assert sum(hit) <= 2 and np.abs(off).max() > 100, (off, hit)
    for k, f in enumerate(g["feature"]):
        # the recorded decisions are the recorded norm's: low at U <=> norm < U, low at nextafter(U) <=> norm <= U
        assert g["keep_v3"][k, 0, f] == (g["norm_v3"][k] < g["U"][k]) and g["keep_v3"][k, 1, f] == (g["norm_v3"][k] <= g["U"][k])
        assert not g["keep_v3"][k, :, mg.HIGH].any()


def test_norm_tie_fixture_regenerates_bit_for_bit():
    mg = _generator()
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libxivo_refx_n203_v4.so")):
        pytest.skip("oracle/_ref not built (this test runs against the library only)")
    out = mg.generate()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gate_ties.npz"))
    assert sorted(out) == sorted(g.files)
    for k in g.files:
        assert np.array_equal(out[k], g[k]), k
