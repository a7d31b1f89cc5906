"""The in-state gate (Estimator::MHGating, src/update.cpp:60-96) in all its copies - gate_sparse_kernel, gate_dense_kernel,
gate_ell_kernel, the gate of fused_update_f64_kernel, the prologue of the register Cholesky - and Estimator::OnePointRANSAC
(src/update.cpp:213-393) at thresholds and ties, against the 80-bit restatement of tests/gate_restate.py on the cases of
tests/gate_edge_cases.py (tests/test_gate_edges_cpu.py checks without a GPU that each case sits where it claims).
Every test asserts which gate copy ran from the profile's stage labels / last_route(). The bounds are imported, not typed in."""
import numpy as np
import pytest

import gate_edge_cases as gc
import gate_restate as gr
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from xivo_amd.lib import Context, XivoHipError, FLAG_DENSE_H, FLAG_PROFILE

pytestmark = pytest.mark.gpu
# feature-level gates: name -> (the call's level, context flags, stage label of the gate copy)
# (launches of the gate stage: the calibration gate on dense rows first runs gate_sparse_kernel without gating - the mask of
#  the present entries - then stacks the whole rows and gates them with gate_dense_kernel)
SCENE_GATES = {"mh_gate": ("feature", 0, "gate_sparse_kernel", 1),              # the default build
               "mh_gate_calib": ("calib", 0, "gate_sparse_kernel", 1),          # online calibration: the 43-column form of gate_sparse_kernel
               "mh_gate_calib_dh": ("calib", FLAG_DENSE_H, "gate_dense_kernel", 2)}   # ... on dense rows: gate_dense_kernel counting the scene's entries
GATES = gc.ROUTE_NAMES + list(SCENE_GATES)


# ---------------------------------------------------------------- running a call
def _assert_copy(copy, want_route, prof, route):
    g = prof["mh_gate"]
    if copy == "fused":
        assert route == "fused" and g["launches"] == 0, (route, g)
    elif copy == "chol":
        assert "+gate" in prof["chol_S"]["kernel"] and g["launches"] == 0, (prof["chol_S"], g)
    elif copy == "gate_ell":
        assert g["kernel"] == "gate_ell_kernel" and g["launches"] == 1, g
    elif copy == "gate_dense":
        assert g["kernel"] == "gate_dense_kernel" and g["launches"] == 1, g
    if want_route:
        assert route == want_route, (route, want_route)


def run_update(call, rdef, thresh=None, mult=None, min_inliers=None):
    """an update-level call on one route -> (mask, dist) of the call's filters"""
    name, flags, rows, B, entry, want_route, copy = rdef
    th = call.thresh if thresh is None else thresh
    mu = call.mult if mult is None else mult
    mi = call.min_inliers if min_inliers is None else min_inliers
    idx = np.arange(max(B, call.B)) % call.B if B > call.B else np.arange(call.B)
    H, inn, P, N = call.H()[idx], call.inn.reshape(call.B, 2 * call.F)[idx], call.P[idx], call.N
    nb = len(idx)
    if rows == "rows_n320":                             # the same rows and prior in a wider state: exact zeros in every sum
        N = gc.WIDE_STATE_N
        H = np.concatenate([H, np.zeros(H.shape[:2] + (N - call.N,))], axis=2)
        P = np.tile(np.eye(N), (nb, 1, 1)); P[:, :call.N, :call.N] = call.P[idx]
    with Context(N, 2 * call.F, nb, flags=flags | FLAG_PROFILE) as ctx:
        ctx.upload_P(P); ctx.set_measurements(H, inn, np.full((nb, 2 * call.F), call.R))
        if entry == "g":
            ctx.update_dense_gated(call.F, call.R, th, mu, mi, nb)
            mask, dist = ctx.get_gate(call.F, nb)
        else:
            mask, dist = ctx.mh_gate_dense(call.F, call.R, th, mu, mi, nb)
        prof, route = ctx.profile_get(), ctx.last_route()
    _assert_copy(copy, want_route if entry == "g" else None, prof, route)
    # gate_ell_kernel's two sources of the 2 x 2 blocks. What is asserted is the slab width of the S kernel; the source follows
    # from the launcher's condition, not from an observation of the branch: on these routes (no mixed stacking, no leading block,
    # the T buffer large enough) 64-wide slabs leave the compact copy and the gate is handed it, 32-wide ones leave none
    if copy == "gate_ell":
        assert prof["gemm_S"]["kernel"].split(",")[2] == ("32" if rows == "rows_n320" else "64"), prof["gemm_S"]
    for b in range(call.B, nb):                         # the tiled copies of a large batch: the same bits
        assert np.array_equal(mask[b], mask[b % call.B]) and np.array_equal(dist[b], dist[b % call.B]), b
    return mask[:call.B], dist[:call.B]


def open_scene(call, flags=0):
    """a context with the call's layout (and calibration layout), covariance and scene staged, Jacobians taken"""
    lay, scn = call.scene["lay"], call.scene
    poses, groups, feats, _ = call.feats()
    ctx = Context(lay.N, 2 * call.F, call.B, flags=flags | FLAG_PROFILE)
    ctx.set_layout(lay.N, lay.group_begin, lay.n_groups, lay.feature_begin, lay.n_features, gc.CAM)
    if call.level == "calib":
        ctx.set_calib(lay.td, lay.Cg, lay.cam_begin, lay.cam_dim)
        calib = gc.calib_arrays(scn, poses)
    ctx.upload_P(call.P); ctx.set_scene(poses, groups, feats)
    if call.level == "calib":
        ctx.set_calib_state(calib)
    ctx.jacobians_instate()
    return ctx


def device_rows(ctx, call):
    """whole rows and innovations as the device's Jacobian pass made them (absent entries: zero)"""
    lay, sc = call.scene["lay"], call.scene["sc"]
    J21, inn = ctx.get_jacobians()
    sind = np.where(call.here, sc["sind"], -1)
    if call.level == "calib":
        assert lay.td >= 0 and lay.Cg >= 0 and lay.cam_dim == gc.CALIB_CAM_DIM and lay.group_begin == 48      # 43-column rows: td, Cg / Ca, the intrinsics are state
        J = gc.full_rows_calib(J21, ctx.get_jacobians_calib(F=call.F), lay, sc["ref"], sind)
    else:
        J = gc.full_rows(J21, lay, sc["ref"], sind)
    return J, np.where(call.here[..., None], inn, 0.0)


def run_feature(call, flags=0, label="gate_sparse_kernel", launches=1, thresh=None, mult=None, min_inliers=None):
    """a feature-level call -> (mask, dist, whole rows and innovations as the device's Jacobian pass made them)"""
    with open_scene(call, flags) as ctx:
        J, inn = device_rows(ctx, call)
        ctx.profile_reset()
        mask, dist = ctx.mh_gate(call.R, call.thresh if thresh is None else thresh, call.mult if mult is None else mult,
                                 call.min_inliers if min_inliers is None else min_inliers)
        prof = ctx.profile_get()
    assert prof["mh_gate"]["kernel"].startswith(label) and prof["mh_gate"]["launches"] == launches, prof["mh_gate"]
    return mask, dist, J, inn


def run_gate(make, gate, **kw):
    """the call `make(level)` on `gate` (a ROUTES name or a SCENE_GATES name) -> (call, mask, dist, what the device read)"""
    if gate in SCENE_GATES:
        level, flags, label, launches = SCENE_GATES[gate]
        call = make(level)
        mask, dist, J, inn = run_feature(call, flags, label, launches, **kw)
        return call, mask, dist, J, inn
    call = make(gc.level_of(gate))
    mask, dist = run_update(call, gc.route(gate), **kw)
    return call, mask, dist, None, None


def _level(gate):
    return SCENE_GATES[gate][0] if gate in SCENE_GATES else gc.level_of(gate)


# ---------------------------------------------------------------- A: distance accuracy
@pytest.mark.parametrize("gate", GATES)
def test_distances_within_the_oracles_own_error(built, gate):
    """every conditioning class, |r| from 1e-6 to 1e3 px: the device's distance against the 80-bit restatement within 4 x what the
    fp64 oracle itself loses on the class (gate_edge_cases.bounds: imported, not typed). One stated deviation
    (gate_edge_cases.STATED_DEVIATIONS): the 43-column gate_sparse_kernel at kappa 1e8, measured 1.75 x its bound"""
    call, mask, dist, J, inn = run_gate(gc.family_a, gate)
    ev = gc.evaluate(call, J, inn)
    assert mask.all()
    bound = gc.bounds()[_level(gate)]
    worst = {}
    for b, cls in enumerate(gc.CLASSES):
        worst[cls] = gc.rel_err(dist[b], ev["d80"][b]).max()
        print("gate accuracy %-18s %-12s device %.3g u, bound %.3g u, kappa <= %.1e" % (gate, cls, worst[cls] / gc.U, bound[cls] / gc.U, ev["kappa"][b].max()))
    over = {c: (worst[c] / gc.U, bound[c] / gc.U) for c in gc.CLASSES if worst[c] > bound[c] * gc.STATED_DEVIATIONS.get((gate, c), 1.0)}
    assert not over, (gate, over)


# ---------------------------------------------------------------- B: next to the threshold
@pytest.mark.parametrize("cls", gc.B_CLASSES)
@pytest.mark.parametrize("gate", GATES)
def test_decisions_next_to_the_threshold(built, gate, cls):
    """the chosen feature's 80-bit distance is thresh (1 -+ m), m = max(1e-6, 100 x the class bound): in for the minus, out for the plus"""
    call, mask, dist, J, inn = run_gate(lambda level: gc.family_b(level, cls), gate)
    ev = gc.evaluate(call, J, inn)
    for b in range(call.B):
        k, inside = call.expect[b]["feature"], call.expect[b]["inlier"]
        ratio = float(ev["d80"][b, k] / gc.LD(call.thresh))
        assert abs(ratio - (1.0 - call.margin if inside else 1.0 + call.margin)) < call.margin / 5, (b, ratio)     # (on the device's own rows too)
        assert bool(mask[b, k]) == inside, (gate, cls, b, k, dist[b, k], call.thresh)
    assert np.array_equal(mask, ev["mask"])
    assert gc.rel_err(dist, ev["d80"]).max() <= gc.bounds()[_level(gate)][cls]


# ---------------------------------------------------------------- C: exact ties by two calls
@pytest.mark.parametrize("gate", GATES)
def test_exact_ties_on_the_devices_own_distances(built, gate):
    """The distances are fixed-shape reductions: the same call returns the same bits. thresh = dist[f]: f is out, every smaller
    distance in; nextafter: f in; thresh = dist[f] / 4 with mult 2 and min_inliers = the number of smaller distances: two
    relaxations, and f is out on the third pass's threshold, which is dist[f] again; thresh = dist[f] with one more inlier
    wanted: f is not counted and the loop relaxes."""
    make = lambda level: gc.family_b(level, "easy")
    call, mask0, dist, J, inn = run_gate(make, gate, thresh=gc.HUGE)
    assert mask0.all()
    f = int(np.argsort(dist[0])[3])
    T = float(dist[0, f])
    smaller = dist[0] < T
    assert smaller.sum() == 3 and (dist[0] < T / 2).sum() < 3 and (dist[0] == T).sum() == 1

    def expect(th, mult, mi):
        return np.array([gr.relax(dist[b], th, mult, mi)["mask"] for b in range(call.B)])
    _, mask, d1, _, _ = run_gate(make, gate, thresh=T, mult=2.0, min_inliers=1)
    assert np.array_equal(d1, dist)
    assert not mask[0, f] and np.array_equal(mask[0], smaller) and np.array_equal(mask, expect(T, 2.0, 1))
    up = float(np.nextafter(T, np.inf))
    _, mask, _, _, _ = run_gate(make, gate, thresh=up, mult=2.0, min_inliers=1)
    assert mask[0, f] and np.array_equal(mask[0], dist[0] <= T) and np.array_equal(mask, expect(up, 2.0, 1))
    rec = gr.relax(dist[0], T / 4, 2.0, 3)
    assert rec["relaxations"] == 2 and rec["thresh"] == T
    _, mask, _, _, _ = run_gate(make, gate, thresh=T / 4, mult=2.0, min_inliers=3)
    assert not mask[0, f] and np.array_equal(mask[0], smaller) and np.array_equal(mask, expect(T / 4, 2.0, 3))
    # the tie in the loop's own count: thresh = dist[f] with one inlier more wanted than there are smaller distances - f does not
    # count (update.cpp:84 is strict), the pass falls short and the loop relaxes once; counted, it would stop here
    rec = gr.relax(dist[0], T, 2.0, 4)
    assert rec["relaxations"] == 1 and rec["mask"][f] and rec["mask"].sum() >= 4
    _, mask, _, _, _ = run_gate(make, gate, thresh=T, mult=2.0, min_inliers=4)
    assert mask[0, f] and np.array_equal(mask, expect(T, 2.0, 4))


# ---------------------------------------------------------------- D: the relaxation loop's branches
@pytest.mark.parametrize("name", list(gc.D_SPECS))
@pytest.mark.parametrize("gate", GATES)
def test_relaxation_branches(built, gate, name):
    """present == min_inliers and + 1, a pass that reaches exactly min_inliers, 1 / 2 / 30 relaxations, all out until all in,
    min_inliers <= 0 and mult = 1 as coded (gate_edge_cases.D_SPECS): the mask and the reported distances are the restatement's.
    The update-level gates take present = F (an absent entry is a zero innovation: distance 0, an inlier), the feature-level gate counts."""
    call, mask, dist, J, inn = run_gate(lambda level: gc.d_call(name, level), gate)
    ev = gc.evaluate(call, J, inn)
    assert np.array_equal(mask, ev["mask"]), (gate, name, mask, ev["mask"])
    ref = np.asarray(ev["dist"], dtype=np.float64)
    assert np.array_equal(dist == 0, ref == 0)
    nz = ref != 0
    assert gc.rel_err(dist[nz], ev["d80"][nz]).max() <= gc.bounds()[_level(gate)]["easy"]


@pytest.mark.parametrize("name", list(gc.D_WIDE))
@pytest.mark.parametrize("gate", [r[0] for r in gc.WIDE_ROUTES] + ["mh_gate"])
def test_inliers_beyond_the_first_64_lanes(built, gate, name):
    """F = 65 with the only inliers in entries 63 / 64 (the second pass of the 64-lane count), F = 64 with it in the last lane"""
    if gate == "mh_gate":
        call = gc.d_call(name, "feature")
        mask, dist, J, inn = run_feature(call)
    else:
        call = gc.d_call(name, "update")
        mask, dist = run_update(call, next(r for r in gc.WIDE_ROUTES if r[0] == gate))
        J = inn = None
    ev = gc.evaluate(call, J, inn)
    assert np.array_equal(mask, ev["mask"]) and mask.any(axis=1).all() and not mask[:, :63].any()


# ---------------------------------------------------------------- E: OnePointRANSAC
class _Ransac:
    """one context for a RansacCall: stage pixels -> Jacobians -> MH gate [-> entries made absent] -> OnePointRANSAC, with the
    restoration check and the restatement on what the device read"""

    def __init__(self, c):
        self.c = c
        self.ctx = Context(c.lay.N, 2 * c.F, c.B)
        self.ctx.set_layout(c.lay.N, c.lay.group_begin, c.ng, c.lay.feature_begin, c.F, gc.CAM)
        self.ctx.upload_P(c.P)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def predictions(self):
        poses, groups, feats, _ = self.c.arrays(np.zeros((self.c.B, self.c.F, 2)), self.c.absent)
        self.ctx.set_scene(poses, groups, feats); self.ctx.jacobians_instate()
        return -self.ctx.get_jacobians()[1]

    def run(self, xp, thresh=None, chi2=None, update=False):
        c, ctx = self.c, self.ctx
        thresh = c.thresh if thresh is None else thresh
        chi2 = c.chi2 if chi2 is None else chi2
        ctx.upload_P(c.P)
        poses, groups, feats, _ = c.arrays(xp, c.absent)
        ctx.set_scene(poses, groups, feats); ctx.jacobians_instate()
        mh, _ = ctx.mh_gate(gc.E_R, gc.E_MH, gc.E_MULT, gc.E_MIN)
        if c.absent_after.any():
            poses, groups, feats, _ = c.arrays(xp, c.absent | c.absent_after)
            ctx.set_scene(poses, groups, feats); ctx.jacobians_instate()
        J0, inn0 = ctx.get_jacobians()
        keep, chi, nrej = ctx.one_point_ransac(gc.E_R, thresh, chi2, gauge=c.gauge)
        # RestoreState: covariance, nominal state, Jacobians and innovations are what they were, in every bit
        assert np.array_equal(ctx.download_P(), c.P)
        p2, g2, f2 = ctx.get_scene()
        for k in ("Rsb", "Tsb", "Rbc", "Tbc"):
            assert np.array_equal(p2[k], poses[k]), k
        assert np.array_equal(g2["Rsb"], groups["Rsb"]) and np.array_equal(g2["Tsb"], groups["Tsb"]) and np.array_equal(f2["x"], feats["x"])
        J1, inn1 = ctx.get_jacobians()
        assert np.array_equal(J0, J1) and np.array_equal(inn0, inn1)
        saved = (c.thresh, c.chi2)
        c.thresh, c.chi2 = thresh, chi2
        try:
            ex = c.expect(xp, inn0, mh)
        finally:
            c.thresh, c.chi2 = saved
        out = dict(keep=keep, chi=chi, nrej=nrej, mh=mh, inn=inn0, ex=ex)
        if update:
            ctx.stack(gc.E_R); ctx.update_joseph()
            out["P"], out["err"] = ctx.download_P(), ctx.get_err()
        return out

    def check(self, o, chi_tol=1e-7):
        c = self.c
        for b, e in enumerate(o["ex"]):
            tag = (c.name, b, c.tags.get(b))
            assert np.array_equal(o["keep"][b], e["keep"]), (tag, o["keep"][b], e["keep"], e["dec"])
            assert o["nrej"][b] == e["nrej"], tag
            tested = np.zeros(c.F, dtype=bool); tested[list(e["chi"])] = True
            assert np.array_equal(o["chi"][b] != 0, tested), (tag, o["chi"][b], e["chi"])       # which features went to the rescue test
            for f, d in e["chi"].items():
                assert abs(o["chi"][b, f] - d) < chi_tol * max(1.0, d), (tag, f, o["chi"][b, f], d)

    def check_update(self, o, xp):
        """the update that follows stacks the RANSAC inliers: P+ and dx against the oracle (TOL_P / TOL_DX)"""
        c = self.c
        for b in range(c.B):
            st = gc.state_st(c.sc, b)
            kept = np.nonzero(o["keep"][b])[0]
            if len(kept) == 0:
                continue
            Js, inns = [], []
            for i in kept:
                r = int(st["ref"][i])
                Jf, innf, _ = orc.compute_jacobian(st["x"][i], xp[b, i], st["gR"][r], st["gT"][r], st["Rsb"], st["Tsb"], st["Rbc"], st["Tbc"],
                                                   gc.CAM, c.lay, r, int(st["sind"][i]))
                Js.append(Jf); inns.append(innf)
            H, inn, dR = orc.stack_measurements(np.array(Js), np.array(inns), st["ref"][kept], st["sind"][kept], c.lay, gc.E_R)
            e_ref, P_ref, _ = orc.update_joseph(H, c.P[b], inn, dR)
            assert rel_fro(o["P"][b], P_ref) < TOL_P and rel_fro(o["err"][b], e_ref) < TOL_DX, (c.name, b)


@pytest.mark.parametrize("make", [gc.e_states, gc.e_ref_ties, gc.e_mask_width], ids=lambda f: f.__name__)
def test_ransac_states_gauge_reference_ties_and_mask_width(built, make):
    """frame state 0 / 1 / 2 at their edges, an MH-masked entry with sind < 0, the gauge group with and without a low inlier, gauge
    -1 / >= n_groups / 63 of 64, FindNewRefGroup among bit-equal sums (lowest slot, as coded) and one ulp apart, group slots 31 /
    32 / 63: inlier set, rescue distances, rejected count, the update that follows - and everything restored to the bit"""
    c = make()
    with _Ransac(c) as r:
        xp = r.predictions() + c.noise
        o = r.run(xp, update=True)
        r.check(o)
        for b, e in enumerate(o["ex"]):
            assert e["dec"]["state"] == c.expect_state[b], (c.tags[b], e["dec"])
            if isinstance(c.expect_tmpref.get(b), int):
                assert e["dec"]["tmpref"] == c.expect_tmpref[b], (c.tags[b], e["dec"])
        r.check_update(o, xp)


def test_low_innovation_norm_at_the_tie(built):
    """innovations on which sqrt(fma(r1, r1, r0 r0)) and the unfused norm differ, both ways, found from the device's own
    predictions: ransac_thresh = the unfused norm: not low (strict, update.cpp:249); nextafter: low. A contracted norm that
    comes out one ulp smaller calls the feature low at the tie."""
    c = gc.e_ties_call()
    with _Ransac(c) as r:
        pred = r.predictions()
        found, count = gc.find_tie_pixels(pred[0])
        assert count == {-1: 2, 1: 2}, count
        for f, xpf, rr, u, d in found:
            xp = pred + c.noise
            xp[0, f] = xpf
            for th, low in ((u, False), (float(np.nextafter(u, np.inf)), True)):
                o = r.run(xp, thresh=th)
                assert np.array_equal(o["inn"][0, f], rr)               # the innovation the host planned, to the bit
                assert o["ex"][0]["dec"]["low"][f] == low and o["ex"][0]["dec"]["state"] == 1
                assert (o["chi"][0, f] == 0) == low, (f, d, th, o["chi"][0, f])
                r.check(o)


def test_rescue_next_to_chi2_and_at_the_tie(built):
    """the rescue test d < ransac_chi2 (update.cpp:356, strict) for a feature of a state-1 filter (after the partial update) and
    of a state-2 filter (against the prior): chi2 = d80 (1 -+ m) of the 80-bit distance, m = gate_edge_cases.rescue_margin, then
    chi2 = the device's own returned distance (rejected) and its nextafter (kept)"""
    c = gc.e_states()
    with _Ransac(c) as r:
        xp = r.predictions() + c.noise
        o = r.run(xp)
        r.check(o)
        m = gc.rescue_margin(o["ex"])
        for b, f in gc.RESCUE_PICKS:
            assert o["ex"][b]["dec"]["state"] == (1 if b == 3 else 2)
            d80, d_dev = float(o["ex"][b]["chi80"][f]), float(o["chi"][b, f])
            for chi2, kept in ((d80 * (1 + m), True), (d80 * (1 - m), False), (d_dev, False), (float(np.nextafter(d_dev, np.inf)), True)):
                o2 = r.run(xp, chi2=chi2)
                assert o2["chi"][b, f] == d_dev and bool(o2["keep"][b, f]) == kept, (b, f, chi2, d_dev)
                if chi2 != d_dev and chi2 != float(np.nextafter(d_dev, np.inf)):
                    r.check(o2)


# ---------------------------------------------------------------- the calibration rescue: gate_dense_kernel with no_relax
def _calib_rescue(ctx, call, chi2):
    """OnePointRANSAC of a calibration build with nothing low-innovation (ransac_thresh below every |r|): state 2, every MH inlier
    goes to the rescue test against the prior on its whole 43-column row - the dense-row gate with no_relax - and the returned
    chi is that gate's distance"""
    ctx.upload_P(call.P); ctx.jacobians_instate()
    mh, _ = ctx.mh_gate(call.R, gc.HUGE, 1.1, 2)
    assert np.array_equal(mh, call.here)
    ctx.profile_reset()
    keep, chi, nrej = ctx.one_point_ransac(call.R, 1e-300, chi2, gauge=np.full(call.B, -1, dtype=np.int32))
    g = ctx.profile_get()["mh_gate"]
    assert g["kernel"] == "gate_dense_kernel" and g["launches"] == 1, g
    assert np.array_equal(ctx.download_P(), call.P)
    return keep, chi, nrej


def test_calibration_rescue_distances_margins_and_tie(built):
    """the no_relax form: accuracy on every conditioning class within the class bound; a feature at chi2 (1 -+ m) of its 80-bit
    distance in / out; chi2 = the device's returned distance: rejected, its nextafter: kept"""
    call = gc.family_a("calib")
    with open_scene(call) as ctx:
        J, inn = device_rows(ctx, call)
        keep, chi, nrej = _calib_rescue(ctx, call, gc.HUGE)
    ev = gc.evaluate(call, J, inn)
    assert keep.all() and not nrej.any()
    bound = gc.bounds()["calib"]
    for b, cls in enumerate(gc.CLASSES):
        worst = gc.rel_err(chi[b], ev["d80"][b]).max()
        print("gate accuracy %-18s %-12s device %.3g u, bound %.3g u, kappa <= %.1e" % ("calib_rescue", cls, worst / gc.U, bound[cls] / gc.U, ev["kappa"][b].max()))
        assert worst <= bound[cls], (cls, worst / gc.U, bound[cls] / gc.U)
    for cls in gc.B_CLASSES:
        call = gc.family_b("calib", cls)
        with open_scene(call) as ctx:
            J, inn = device_rows(ctx, call)
            keep, chi, nrej = _calib_rescue(ctx, call, call.thresh)
            d80 = gc.evaluate(call, J, inn)["d80"]
            for b in range(call.B):
                k, inside = call.expect[b]["feature"], call.expect[b]["inlier"]
                assert abs(float(d80[b, k] / gc.LD(call.thresh)) - (1.0 - call.margin if inside else 1.0 + call.margin)) < call.margin / 5
                assert bool(keep[b, k]) == inside, (cls, b, k, chi[b, k])
            assert np.array_equal(keep, np.asarray(d80, dtype=np.float64) < call.thresh) and np.array_equal(nrej, (~keep).sum(axis=1))
            if cls == "easy":
                f = int(np.argsort(chi[0])[3])
                T = float(chi[0, f])
                k2, c2, _ = _calib_rescue(ctx, call, T)
                assert np.array_equal(c2, chi) and not k2[0, f] and np.array_equal(k2, chi < T)
                k3, _, _ = _calib_rescue(ctx, call, float(np.nextafter(T, np.inf)))
                assert k3[0, f] and np.array_equal(k3, chi <= T)


# ---------------------------------------------------------------- refusals
def test_parameters_that_cannot_mean_anything_are_refused(built):
    """a non-finite or non-positive R, a NaN thresh / mult / chi2 / ransac_thresh, mult < 1: XIVO_HIP_ERR_INVALID before anything is
    launched (the mask and distances of the last good call stay as they were); mult = 1 and mult = +inf are accepted"""
    nan, inf = float("nan"), float("inf")
    call = gc.family_b("update", "easy")
    with Context(call.N, 2 * call.F, call.B) as ctx:
        ctx.upload_P(call.P); ctx.set_measurements(call.H(), call.inn.reshape(call.B, -1), np.full((call.B, 2 * call.F), call.R))
        good, gdist = ctx.mh_gate_dense(call.F, call.R, call.thresh, 1.1, 2)
        for R, th, mu in ((0.0, 5.0, 1.1), (-1.0, 5.0, 1.1), (inf, 5.0, 1.1), (nan, 5.0, 1.1), (1.0, nan, 1.1), (1.0, 5.0, nan), (1.0, 5.0, 0.5)):
            with pytest.raises(XivoHipError):
                ctx.mh_gate_dense(call.F, R, th, mu, 2)
            with pytest.raises(XivoHipError):
                ctx.update_dense_gated(call.F, R, th, mu, 2)
        m2, d2 = ctx.get_gate(call.F)
        assert np.array_equal(m2, good) and np.array_equal(d2, gdist)
        ctx.mh_gate_dense(call.F, call.R, call.thresh, 1.0, 2)
        ctx.mh_gate_dense(call.F, call.R, call.thresh, inf, 2)
    c = gc.e_states()
    with _Ransac(c) as r:
        xp = r.predictions() + c.noise
        r.run(xp)
        for R, th, mu in ((0.0, 5.0, 1.1), (inf, 5.0, 1.1), (nan, 5.0, 1.1), (1.0, nan, 1.1), (1.0, 5.0, nan), (1.0, 5.0, 0.99)):
            with pytest.raises(XivoHipError):
                r.ctx.mh_gate(R, th, mu, 2)
            with pytest.raises(XivoHipError):
                r.ctx.filter_update(R, th, mu, 2)
        for R, th, chi2 in ((0.0, 2.0, 5.89), (nan, 2.0, 5.89), (inf, 2.0, 5.89), (1.0, nan, 5.89), (1.0, 2.0, nan)):
            with pytest.raises(XivoHipError):
                r.ctx.one_point_ransac(R, th, chi2, gauge=c.gauge)
        assert np.array_equal(r.ctx.download_P(), c.P)
