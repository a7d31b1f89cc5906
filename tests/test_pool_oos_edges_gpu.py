"""GPU: the pool's MSCKF path through the C ABI (xivo_hip_pool_oos_*) at its shape limits and the gate's branches - the cases of
tests/pool_oos_edge_cases.py, whose scenes tests/test_pool_oos_edges_cpu.py checks without a GPU.

Every frame is the scripted one of tests/test_pool_oos_gpu.py on another shape: the sub-filter is frozen (Rtri = MH_thresh =
1e30), so an entry stays where pool_add put it, and every expectation is computed from the entry as read back with pool_get.
collect_*: the list (order, observations, Xs against the oracle) and the counters for pools past one and two passes of the
wave's lanes, at XIVO_POOL_MAX_ENTRIES, with a full list of 64 positions, under XIVO_HIP_FLAG_INVDEPTH with the depth window on
exact values, and with a slot outside the layout that makes a feature short. gate_*: gamma of features of up to 29 rows and 102
columns against r^T S^-1 r in longdouble over ALL columns of the downloaded rows, bounded per feature by
max(16 e_np, nc eps cond(S)) and never looser than 1e-9; duplicate groups, a threshold 1e-6 either side of gamma, chi2[dof] = 0,
a non-positive pivot. two_frames: a second frame on the same context with fewer in-state rows and a shorter list.

gate_cond: a scalar factor on the prior cannot make S ill-conditioned - cond(S) then stops at cond(H_o P H_o^T), about 50 with
these priors -, so the case puts the groups in other units as well: 2^24 D P D with D = 2^-4(g % 4) on group g's columns, every
factor a power of two (pool_oos_edge_cases.cond_prior); cond(S) is 1.8e6 for the 29-row feature. nc eps cond(S) is then 4e-8, and
the case is held to the 1e-9 of tests/test_pool_oos_gpu.py::test_gamma_equals_numpy instead: no bound here is looser than that.

Measured on one MI355X (relative to the longdouble gamma; every test prints its lines):
  case        rows x columns   cond(S)   e_np      bound     device
  gate_obs16  29 x 102         2.1e+01   1.5e-16   4.8e-13   1.1e-16
  gate_obs16  19 x 72          9.6e+00   8.7e-18   1.5e-13   8.7e-18
  gate_obs16  15 x 60          1.1e+01   2.0e-16   1.5e-13   3.8e-16
  gate_obs16  17 x 66          1.1e+01   1.5e-16   1.6e-13   1.5e-16
  gate_cond   29 x 102         1.8e+06   1.8e-12   1.0e-09   1.6e-12
  gate_cond   19 x 72          8.4e+05   8.1e-12   1.0e-09   4.9e-12
  gate_cond   15 x 60          5.0e+05   1.9e-12   1.0e-09   2.8e-12
  gate_cond   17 x 66          1.7e+05   5.8e-15   1.0e-09   8.0e-14
  gate_dup     5 x 30          4.8e+00   2.0e-17   3.2e-14   1.9e-16
  gate_dup     3 x 24          2.8e+00   1.7e-16   1.5e-14   3.8e-17
  gate_dup     7 x 36          8.9e+00   3.6e-17   7.1e-14   3.9e-16
  gate_dup     5 x 30          4.7e+00   2.9e-17   3.1e-14   2.9e-17
  two_frames   1 x 18          1.0e+00   1.1e-16   4.0e-15   2.7e-17"""
import numpy as np
import pytest

import pool_oos_edge_cases as pc
import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import scene_arrays, oracle_jacobians, cm
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu
CAM, NF, ROOS = pc.CAM, pc.NF, pc.ROOS
R_VIS, MH, MULT = 2.25, 5.991, 1.1
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


class _Frame:
    """one context on a scene, driven step by step"""

    def __init__(self, scene, chi2=None, flags=0, sh=None, M_max=None):
        self.scene, self.sh = scene, dict(scene["sh"] if sh is None else sh)
        sh, sc, lay = self.sh, scene["sc"], scene["lay"]
        self.B, self.ng = sh["B"], sh["ng"]
        self.rows = pc.rows_of(sh["oos_max"], sh["max_obs"])
        self.poses, self.groups, self.feats, self.xp = scene_arrays(sc, CAM)
        self.ctx = ctx = L.Context(lay.N, pc.m_max(sh["oos_max"], sh["max_obs"]) if M_max is None else M_max, self.B, flags=flags)
        ctx.set_layout(lay.N, lay.group_begin, self.ng, lay.feature_begin, NF, CAM)
        ctx.upload_P(pc.prior(scene))
        # the sub-filter's measurement variance is so large that its steps leave x where pool_add put it
        ctx.pool_config(sh["pool_max"], pc.AM, Rtri=1e30, MH_thresh=1e30, ready_steps=1, min_depth=sh.get("min_depth", pc.MIN_DEPTH),
                        max_depth=sh.get("max_depth", pc.MAX_DEPTH), remove_outlier_counter=1e30)
        assert ctx.pool_oos_config(sh["oos_max"], max_obs=sh["max_obs"], min_obs=sh["min_obs"], Roos=ROOS, chi2=chi2) == self.rows

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def populate(self):
        """the anchors at the poses of group slots 0 .. 3 (0 and 1 linked), the entries, two sub-filter steps"""
        ctx, sc, B = self.ctx, self.scene["sc"], self.B
        for a in range(pc.N_ANCHORS):
            pa = self.poses.copy()
            for b in range(B):
                pa[b]["Rsb"] = cm(sc["gR"][b, a]); pa[b]["Tsb"] = sc["gT"][b, a]
            ctx.set_scene(pa, self.groups, self.feats)
            ctx.pool_anchor(np.full(B, a, dtype=np.int32))
        ctx.set_scene(self.poses, self.groups, self.feats)
        ops = np.zeros(2 * B, dtype=L.edit_dtype)
        for b in range(B):
            for a in range(2):
                o = ops[2 * b + a]
                o["b"], o["kind"], o["i0"], o["i1"] = b, L.EDIT_ADD_GROUP_ANCHOR, a, a
        ctx.edit_batch(NF, ops)
        for late in (False, True):
            recs = []
            for (b, e), d in self.scene["ent"].items():
                if d["late"] == late:
                    r = np.zeros((), dtype=L.pool_new_dtype)
                    r["b"], r["entry"], r["anchor"], r["xp"], r["z0"], r["std_xyz"] = b, e, d["anchor"], d["xp0"], d["z0"], [1e-3, 1e-3, 1e-2]
                    recs.append(r)
            ctx.pool_add(np.array(recs, dtype=L.pool_new_dtype))
            ent_d = ctx.pool_get()[0]
            ctx.pool_step(np.where((ent_d["ref_sind"] >= 0)[..., None], ent_d["xp"], np.nan))
        self.entries, self.anchor_poses, self.anchor_slots = ctx.pool_get()
        self.dev_groups = ctx.get_scene()[1]
        return self

    def collect(self, cands):
        self.ctx.pool_oos_collect(cands)
        self.list = self.ctx.pool_oos_get()[0]
        return self

    def stack(self, F=NF, min_inliers=5):
        ctx = self.ctx
        if F != NF:
            ctx.set_scene(self.poses, self.groups, self.feats[:, :F])
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, min_inliers); ctx.stack(R_VIS)
        self.F = F
        return self

    def project_and_gate(self, P_at_gate=None, gate=True):
        """P_at_gate: the prior the gate sees, from the resident one (uploaded behind the projection)"""
        ctx = self.ctx
        ctx.pool_oos_project()
        self.P = ctx.download_P()
        if P_at_gate is not None:
            self.P = P_at_gate(self.P)
            ctx.upload_P(self.P)
        if gate:
            ctx.pool_oos_gate()
        self.gamma = ctx.pool_oos_get()[1]
        self.H = [ctx.get_H(b) for b in range(self.B)]
        self.stats = ctx.pool_oos_stats()
        return self

    def update(self):
        ctx = self.ctx
        ctx.update_joseph()
        self.dx, self.Pn, self.status = ctx.get_err(), ctx.download_P(), ctx.get_status(check=False)
        return self

    # ---- expectations from what is resident
    def facts(self):
        """(READY, depth, valid observations) per scripted entry, from the pool as read back"""
        inv = bool(self.sh.get("invdepth"))
        out = {}
        for (b, e), d in self.scene["ent"].items():
            f = self.entries[b, e]
            assert int(f["ref_sind"]) == d["anchor"], (b, e)
            z = 1.0 / f["x"][2] if inv else float(np.exp(f["x"][2]))
            if not d["exact"]:      # a rounding of exp / the division cannot decide the outcome
                assert min(abs(z / self.sh.get(k, v) - 1) for k, v in (("min_depth", pc.MIN_DEPTH), ("max_depth", pc.MAX_DEPTH))) > 1e-6
            out[b, e] = (int(f["status"]) == 1, z, len(pc.valid_obs(d["obs"], self.ng, self.sh["max_obs"])))
        return out

    def expected_xs(self, b, e):
        sc, f = self.scene["sc"], self.entries[b, e]
        a = int(f["ref_sind"])
        slot = int(self.anchor_slots[b, a])
        assert slot == (a if a < 2 else -1)
        G = self.dev_groups[b, slot] if slot >= 0 else self.anchor_poses[b, a]
        return orc.feature_xs(f["x"], G["Rsb"].reshape(3, 3).T, G["Tsb"], sc["Rbc"][b], sc["Tbc"][b], invdepth=bool(self.sh.get("invdepth")))

    def spans(self, b):
        """[(first row, rows, columns 6 + 6k)] of the list's features in filter b's block"""
        out, r0 = [], 2 * self.F
        for q in range(self.sh["oos_max"]):
            k = int(self.list[b, q]["n_obs"])
            if k >= 2:
                out.append((r0, 2 * k - 3, 6 + 6 * k))
                r0 += 2 * k - 3
        return out


def _check_list(fr, dropped=None, counters=None):
    """the list and the counters of a collect against the rule over the resident entries; -> used [B] lists of (b, e)"""
    scene, sh = fr.scene, fr.sh
    dec, used, cnt = pc.split(sh, scene["dropped"] if dropped is None else dropped, fr.facts())
    lst = fr.list
    assert lst.shape == (sh["B"], sh["oos_max"])
    for b in range(sh["B"]):
        assert [e for _, e in used[b]] == sorted(e for _, e in used[b])           # ascending entry
        for q in range(sh["oos_max"]):
            f = lst[b, q]
            if q >= len(used[b]):
                assert f["n_obs"] == 0, (b, q)
                continue
            key = used[b][q]
            obs = pc.valid_obs(scene["ent"][key]["obs"], sh["ng"], sh["max_obs"])
            k = len(obs)
            assert f["n_obs"] == k, (b, q, key)
            assert f["group_sind"][:k].tolist() == [g for g, _ in obs], (b, q, key)
            assert np.array_equal(f["xp"][:k], np.array([px for _, px in obs])), (b, q, key)
            assert not f["group_sind"][k:].any() and not f["xp"][k:].any(), (b, q, key)      # the tail behind n_obs
            assert np.abs(f["Xs"] - fr.expected_xs(*key)).max() < 1e-10, (b, q, key)
            assert np.abs(f["Xs"] - scene["ent"][key]["Xs"]).max() < 1e-6, (b, q, key)          # ... which is the scripted point
    st = fr.ctx.pool_oos_stats()
    got = (st["oos_used"].tolist(), st["oos_short"].tolist(), st["oos_surplus"].tolist())
    assert got == ([c[pc.USED] for c in cnt], [c[pc.SHORT] for c in cnt], [c[pc.SURPLUS] for c in cnt]), got
    if counters is not None:
        assert got == tuple(counters), got
    assert not st["oos_gated"].any()
    return used


# ---------------------------------------------------------------- collect and list at the limits
@pytest.mark.parametrize("name", ["collect_pool130", "collect_records130", "collect_poolcap", "collect_oos64", "collect_badslot"])
def test_collect_at_the_limits(built, name):
    scene = pc.build(name)
    with _Frame(scene) as fr:
        fr.populate().collect(pc.cands(scene))
        used = _check_list(fr, counters=pc.COUNTERS[name])
    es = [e for u in used for _, e in u]
    if name == "collect_pool130":       # used entries in each of the three passes of the lanes
        assert min(es) == 0 and any(64 <= e < 128 for e in es) and max(es) == 129
    if name == "collect_records130":    # picked from the first and from the third pass over the records
        assert used[1:] == [[(1, e) for e in (0, 1, 2, 3)], [(2, e) for e in (0, 127, 128, 129)]]
    if name == "collect_poolcap":
        assert sorted(es) == [0, 256, 511]
    if name == "collect_oos64":
        assert [len(u) for u in used] == [1, 64, 64] and used[1][-1] == (1, 63) and used[2][0] == (2, 66)
    if name == "collect_badslot":       # the features with a slot outside the layout are the short ones
        assert used == [[], [(1, 64)], [(2, 129)]]


def test_collect_invdepth_and_the_depth_window_on_exact_values(built):
    scene = pc.build("collect_invdepth")
    nxt = np.nextafter
    # (min_depth, max_depth) -> the entries of filter 1 used: (1, 0) sits at z = 2, (1, 129) at z = 4, exactly
    windows = [((pc.MIN_DEPTH, pc.MAX_DEPTH), [0, 64, 128, 129]), ((2.0, 4.0), [64, 128]),
               ((nxt(2.0, 0.0), nxt(4.0, np.inf)), [0, 64, 128, 129]), ((2.0, nxt(4.0, np.inf)), [64, 128, 129]),
               ((nxt(2.0, 0.0), 4.0), [0, 64, 128])]
    for (lo, hi), want in windows:
        sh = dict(scene["sh"], min_depth=float(lo), max_depth=float(hi))
        with _Frame(scene, flags=L.FLAG_INVDEPTH, sh=sh) as fr:
            fr.populate().collect(pc.cands(scene))
            assert 1.0 / fr.entries[1, 0]["x"][2] == 2.0 and 1.0 / fr.entries[1, 129]["x"][2] == 4.0
            assert fr.entries[1, 0]["x"][2] == 0.5
            used = _check_list(fr, counters=pc.COUNTERS["collect_invdepth"] if (lo, hi) == (pc.MIN_DEPTH, pc.MAX_DEPTH) else None)
            assert [e for _, e in used[1]] == want, ((lo, hi), used[1])


# ---------------------------------------------------------------- the gate against an extended-precision reference
def _run_gate(scene, chi2=None, cand=None, P_at_gate=None, update=False):
    with _Frame(scene, chi2=chi2) as fr:
        fr.populate().collect(pc.cands(scene) if cand is None else cand).stack().project_and_gate(P_at_gate)
        if update:
            fr.update()
    return fr


@pytest.fixture(scope="module")
def obs16(built):
    """gate_obs16 without a threshold (gamma is still computed, the rows stay as projected) and with the update behind it"""
    return _run_gate(pc.build("gate_obs16"), update=True)


def _check_gamma(fr, tag, pre=None, want_shapes=None):
    """gamma of every feature against the longdouble reference on the rows of `pre` (the same frame without a threshold)"""
    pre = fr if pre is None else pre
    shapes, table = [], []
    for b in range(fr.B):
        H, inn, _ = pre.H[b]
        sp = fr.spans(b)
        for q, (r0, rr, nc) in enumerate(sp):
            Ho, r = H[r0:r0 + rr], inn[r0:r0 + rr]
            assert len(np.flatnonzero(np.abs(Ho).sum(axis=0))) <= nc
            g, e_np, cond, bound = pc.gate_bound(Ho, fr.P[b], r, nc)
            err = float(abs(pc.LD(fr.gamma[b, q]) - g) / g)
            print("%s filter %d feature %d: rows %d columns %d cond(S) %.3e gamma %.9g e_np %.2e bound %.2e device %.2e"
                  % (tag, b, q, rr, nc, cond, float(g), e_np, bound, err))
            table.append((b, q, rr, nc, cond, e_np, bound, err))
            shapes.append((rr, nc))
        assert not fr.gamma[b, len(sp):].any()
    if want_shapes is not None:
        assert sorted(shapes) == want_shapes
    for b, q, rr, nc, cond, e_np, bound, err in table:
        assert bound <= pc.CAP and err <= bound, (tag, b, q, err, bound)
    return table


def _check_rows_against_the_oracle(fr, F=NF):
    """in-state rows and the block against the oracle on the downloaded list; the rows no feature fills are neutral"""
    scene, sc, lay = fr.scene, fr.scene["sc"], fr.scene["lay"]
    for b in range(fr.B):
        gH, ginn, gdR = fr.H[b]
        assert gH.shape == (2 * F + fr.rows, lay.N)
        scF = dict(sc, x=sc["x"][:, :F], ref=sc["ref"][:, :F], sind=sc["sind"][:, :F])
        Js, inns, _ = oracle_jacobians(scF, CAM, lay, fr.xp, b)
        H, inn, dR = orc.stack_measurements(Js, inns, scF["ref"][b], scF["sind"][b], lay, R_VIS)
        feats = [(fr.list[b, q]["Xs"], [(int(fr.list[b, q]["group_sind"][i]), fr.list[b, q]["xp"][i]) for i in range(int(fr.list[b, q]["n_obs"]))])
                 for q in range(fr.sh["oos_max"]) if fr.list[b, q]["n_obs"] >= 2]
        for Hx, rp in pc.oracle_block(scene, b, feats):
            H = np.vstack([H, Hx]); inn = np.concatenate([inn, rp]); dR = np.concatenate([dR, np.full(len(rp), ROOS)])
        n = len(inn)
        assert n == 2 * F + sum(rr for _, rr, _ in fr.spans(b))
        assert rel_fro(gH[:n], H) < 1e-10 and rel_fro(ginn[:n], inn) < 1e-9 and np.allclose(gdR[:n], dR)
        assert not gH[n:].any() and not ginn[n:].any() and np.array_equal(gdR[n:], np.full(2 * F + fr.rows - n, ROOS)), b


def test_gate_obs16_gamma_at_29_rows_and_102_columns(obs16):
    assert obs16.stats["oos_used"].tolist() == [0, 2, 2] and not obs16.stats["oos_gated"].any()
    _check_gamma(obs16, "gate_obs16", want_shapes=[(15, 60), (17, 66), (19, 72), (29, 102)])
    _check_rows_against_the_oracle(obs16)
    assert (obs16.status == 0).all()
    for b in range(obs16.B):
        gH, ginn, gdR = obs16.H[b]
        e_ref, P_ref, _ = orc.update_joseph(gH, obs16.P[b], ginn, gdR)
        assert rel_fro(obs16.Pn[b], P_ref) < TOL_P and rel_fro(obs16.dx[b], e_ref) < TOL_DX


def test_gate_cond_a_prior_that_dominates_roos(built, obs16):
    scene = obs16.scene
    fr = _run_gate(scene, P_at_gate=lambda P: np.array([pc.cond_prior(P[b], scene["lay"], pc.COND_T) for b in range(len(P))]))
    for b in range(fr.B):       # the rows are those of gate_obs16: only the gate's prior differs
        assert all(np.array_equal(x, y) for x, y in zip(fr.H[b], obs16.H[b]))
    table = _check_gamma(fr, "gate_cond 2^24 D P D, D = 2^-%d(g %% 4)" % pc.COND_T, want_shapes=[(15, 60), (17, 66), (19, 72), (29, 102)])
    assert 1e5 < max(t[4] for t in table) < 1e7         # cond(S) about 1e6


def test_gate_dup_a_group_seen_twice(built):
    fr = _run_gate(pc.build("gate_dup"))
    assert fr.stats["oos_used"].tolist() == [0, 2, 2]
    for b, q in ((1, 0), (2, 0), (2, 1)):
        gs = fr.list[b, q]["group_sind"][:fr.list[b, q]["n_obs"]].tolist()
        assert len(set(gs)) < len(gs) and len(set(gs)) >= 3
    _check_gamma(fr, "gate_dup", want_shapes=[(3, 24), (5, 30), (5, 30), (7, 36)])
    _check_rows_against_the_oracle(fr)


def _chi2(dof, value):
    c = [0.0] * 32
    c[dof] = float(value)
    return c


def test_gate_threshold_either_side_of_gamma(built, obs16):
    scene = obs16.scene
    (r0, rr, nc), (r1, rr1, _) = obs16.spans(1)
    assert (rr, nc) == (29, 102)
    H, inn, _ = obs16.H[1]
    g = pc.gate_bound(H[r0:r0 + rr], obs16.P[1], inn[r0:r0 + rr], nc)[0]
    above = _run_gate(scene, chi2=_chi2(29, g * (1 + pc.LD(1e-6))))
    assert not above.stats["oos_gated"].any()
    for b in range(above.B):
        assert all(np.array_equal(x, y) for x, y in zip(above.H[b], obs16.H[b]))
    assert np.array_equal(above.gamma, obs16.gamma)
    below = _run_gate(scene, chi2=_chi2(29, g * (1 - pc.LD(1e-6))))
    assert below.stats["oos_gated"].tolist() == [0, 1, 0] and np.array_equal(below.gamma, obs16.gamma)
    bH, binn, bdR = below.H[1]
    assert not bH[r0:r0 + rr].any() and not binn[r0:r0 + rr].any() and np.array_equal(bdR[r0:r0 + rr], np.full(rr, ROOS))
    # everything else bit for bit as without a threshold: the other feature's rows, the in-state rows, the other filters
    keep = np.ones(len(binn), dtype=bool); keep[r0:r0 + rr] = False
    assert np.array_equal(bH[keep], H[keep]) and np.array_equal(binn[keep], inn[keep]) and np.array_equal(bdR, obs16.H[1][2])
    assert bH[r1:r1 + rr1].any()
    for b in (0, 2):
        assert all(np.array_equal(x, y) for x, y in zip(below.H[b], obs16.H[b]))
    # chi2[dof] = 0 is no gate for that dof, whatever gamma is
    c = list(L.CHI2_95); c[29] = 0.0
    moved = _run_gate(scene, chi2=c, cand=pc.cands(scene, moved=(1, 0)))
    assert not moved.stats["oos_gated"].any() and moved.gamma[1, 0] > 10 * L.CHI2_95[29]     # (the table's value would gate it)
    assert moved.H[1][0][r0:r0 + rr].any() and 0 < moved.gamma[1, 1] < L.CHI2_95[rr1]


def test_gate_bad_pivot_gates_the_feature_out(built, obs16):
    scene, lay = obs16.scene, obs16.scene["lay"]
    (r0, rr, nc), _ = obs16.spans(1)
    H, inn, _ = obs16.H[1]
    cols = np.flatnonzero(np.abs(H[r0:r0 + rr]).sum(axis=0))
    assert len(cols) == nc == 102

    def bad(P):
        P = P.copy()
        P[1][np.ix_(cols, cols)] = -pc.BAD_PIVOT_C * np.eye(nc)
        return P
    assert pc.gamma_extended(H[r0:r0 + rr], bad(obs16.P)[1], inn[r0:r0 + rr])[2] < -1.0      # the first pivot on the CPU
    fr = _run_gate(scene, P_at_gate=bad)
    # (the k = 11 feature of the filter observes from groups the first one names too: its first pivot is negative as well)
    assert fr.gamma[1].tolist() == [-1.0, -1.0] and fr.stats["oos_gated"].tolist() == [0, 2, 0]
    bH, binn, bdR = fr.H[1]
    assert not bH[r0:].any() and not binn[r0:].any() and np.array_equal(bdR[r0:], np.full(len(bdR) - r0, ROOS))
    assert np.array_equal(bH[:r0], H[:r0]) and np.array_equal(binn[:r0], inn[:r0])
    for b in (0, 2):
        assert all(np.array_equal(x, y) for x, y in zip(fr.H[b], obs16.H[b]))
        assert np.array_equal(fr.gamma[b], obs16.gamma[b])


def test_two_frames_a_shorter_list_and_fewer_in_state_rows(built):
    scene = pc.build("gate_obs16")
    F2 = 4
    with _Frame(scene) as fr:
        fr.populate().collect(pc.cands(scene)).stack().project_and_gate().update()
        assert fr.stats["oos_used"].tolist() == [0, 2, 2] and all(h[0].shape[0] == 2 * NF + fr.rows for h in fr.H)
        assert all(fr.H[b][0][2 * F2:].any() for b in range(fr.B))          # frame 1 wrote rows where frame 2's block lies
        # frame 2: two in-state features fewer, one k = 2 feature in filter 2
        fr.collect(pc.cands(scene, dropped=[(2, 6)])).stack(F=F2, min_inliers=3).project_and_gate()
        assert fr.list["n_obs"].tolist() == [[0, 0], [0, 0], [2, 0]] and fr.list[2, 0]["group_sind"][:2].tolist() == [4, 9]
        assert (fr.stats["oos_used"] - [0, 2, 2]).tolist() == [0, 0, 1]
        _check_rows_against_the_oracle(fr, F=F2)
        for b in range(fr.B):
            gH, ginn, gdR = fr.H[b]
            n = 2 * F2 + (1 if b == 2 else 0)
            assert gH.shape[0] == 2 * F2 + fr.rows and gH[2 * F2:n].any() == (b == 2)
            assert not gH[n:].any() and not ginn[n:].any() and np.array_equal(gdR[n:], np.full(len(gdR) - n, ROOS)), b
        _check_gamma(fr, "two_frames", want_shapes=[(1, 18)])
        fr.update()
        assert (fr.status == 0).all()
        for b in range(fr.B):
            gH, ginn, gdR = fr.H[b]
            e_ref, P_ref, _ = orc.update_joseph(gH, fr.P[b], ginn, gdR)
            print("two_frames filter %d: P %.3e dx %.3e" % (b, rel_fro(fr.Pn[b], P_ref), rel_fro(fr.dx[b], e_ref)))
            assert rel_fro(fr.Pn[b], P_ref) < TOL_P and rel_fro(fr.dx[b], e_ref) < TOL_DX


# ---------------------------------------------------------------- refusals
def _status(call):
    with pytest.raises(L.XivoHipError) as ei:
        call()
    return ei.value.status


def test_refusals_at_the_limits(built):
    scene = pc.build("gate_obs16")
    big = dict(pc.shape("refuse_rows1856"))
    assert pc.rows_of(big["oos_max"], big["max_obs"]) == 1856
    # accepted by the configuration, refused by the projection on a context without those rows - which then changes nothing
    with _Frame(scene, sh=big, M_max=pc.m_max(2, 16)) as fr:
        fr.populate().collect(pc.cands(scene)).stack()
        before = [fr.ctx.get_H(b) for b in range(fr.B)], fr.ctx.pool_oos_stats()
        assert before[0][0][0].shape[0] == 2 * NF and before[1]["oos_used"].tolist() == [0, 2, 2]
        assert _status(fr.ctx.pool_oos_project) in (ERR_UNSUPPORTED, ERR_INVALID)
        after = [fr.ctx.get_H(b) for b in range(fr.B)], fr.ctx.pool_oos_stats()
        assert after[1].tobytes() == before[1].tobytes()
        for x, y in zip(before[0], after[0]):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        assert _status(fr.ctx.pool_oos_gate) == ERR_INVALID                      # nothing was projected
    for name in ("collect_oos65", "refuse_obs17"):
        sh = pc.shape(name)
        with _Frame(scene) as fr:
            st = _status(lambda: fr.ctx.pool_oos_config(sh["oos_max"], max_obs=sh["max_obs"], min_obs=sh["min_obs"]))
            assert st == (ERR_UNSUPPORTED if name == "collect_oos65" else ERR_INVALID), name
    with _Frame(scene, flags=L.FLAG_DENSE_H) as fr:
        fr.populate().collect(pc.cands(scene)).stack()
        assert _status(fr.ctx.pool_oos_project) == ERR_UNSUPPORTED
    with _Frame(scene) as fr:                                                    # online calibration: the td block switched on
        fr.populate().collect(pc.cands(scene)).stack()
        fr.ctx.set_calib(td=23)
        assert _status(fr.ctx.pool_oos_project) == ERR_UNSUPPORTED
