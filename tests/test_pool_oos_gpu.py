"""GPU: the MSCKF update from dropped pool entries through the C ABI (xivo_hip_pool_oos_*): the frame's list against the host's
decisions and the oracle's Xs, the fixed row block against the oracle's OOS rows, the chi-square gate against numpy, the update
against the oracle's Joseph form.

One scripted frame on the smallest shapes: B = 3 filters, 4 group slots, 6 features (N = 65), a pool of 8 entries on 6 anchors,
max_obs = 3, min_obs = 2, oos_max = 2 (a block of 6 rows). Anchors 0..3 sit at the poses of the four in-state groups (0 and 1
linked to their slots, 2 and 3 frozen there), the sub-filter runs with a measurement variance that leaves x as pool_add wrote it,
so the expectation needs no sub-filter restatement. Filter 0 has no OOS feature, filter 1 has oos_max of them plus one surplus, one
short, one INITIALIZING and one out of the depth range, filter 2 has one whose middle observation names a group slot outside the
layout."""
import numpy as np
import pytest

import xivo_oracle as orc
from helpers import rel_fro, TOL_P, TOL_DX
from scene_util import scene_arrays, oracle_jacobians, spd, cm
from xivo_amd import synth
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu
CAM = synth.PINHOLE
NG, NF, B, PM, AM = 4, 6, 3, 8, 6
OOS_MAX, MAX_OBS, MIN_OBS, ROOS = 2, 3, 2, 3.5 ** 2
ROWS = OOS_MAX * (2 * MAX_OBS - 3)
R_VIS, MH, MULT = 2.25, 5.991, 1.1
# (filter, entry): anchor, the observing group slots oldest first (99: outside the layout), added after the first step
# (INITIALIZING at the frame), depth scale
ENTRIES = {(1, 0): (0, [0, 1, 2], False, 1.0), (1, 1): (2, [3], False, 1.0), (1, 2): (1, [2, 3], True, 1.0),
           (1, 3): (3, [0, 1], False, 1.0), (1, 5): (0, [1, 3, 2], False, 8.0), (1, 6): (1, [3, 0], False, 1.0),
           (1, 7): (2, [0, 2, 3], False, 1.0), (2, 4): (3, [1, 99, 0], False, 1.0), (0, 2): (0, [], False, 1.0)}
DROPPED = [(1, 0), (1, 1), (1, 2), (1, 3), (1, 5), (1, 6), (1, 7), (2, 4)]      # (0, 2) keeps its track
USED = {1: [(1, 0), (1, 3)], 2: [(2, 4)], 0: []}       # (1, 1) short, (1, 2) INITIALIZING, (1, 5) too deep, (1, 6) / (1, 7) surplus


def _scene():
    sc = synth.g_level(NG, NF, NF, B, seed=5, cam=CAM)
    lay = orc.Layout(NG, NF, N=sc["N"])
    rng = np.random.default_rng(11)
    ent = {}
    for (b, e), (a, gs, late, zs) in ENTRIES.items():
        Xs = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3, 6) * zs])
        Xc = sc["Rbc"][b].T @ (sc["gR"][b, a].T @ (Xs - sc["gT"][b, a]) - sc["Tbc"][b])     # in the anchor's camera
        assert Xc[2] > 0.5
        xp0 = orc.camera_project(CAM, Xc[:2] / Xc[2])[0]
        obs = []
        for g in gs:
            gg = g if g < NG else 0
            _, _, inn = orc.oos_jacobian_internal(Xs, sc["gR"][b, gg], sc["gT"][b, gg], sc["Rbc"][b], sc["Tbc"][b], [0, 0], CAM, lay, gg)
            obs.append((g, -inn + rng.normal(0, 1.0, 2)))
        ent[b, e] = dict(anchor=a, xp0=xp0, z0=Xc[2], obs=obs, late=late)
    return sc, lay, ent


def _cands(ent, moved=None, without=()):
    """the host's hand-over: every dropped entry, ordered by (b, entry), with its observations; moved: (b, e) whose first pixel
    is off by 200 px; without: entries left out"""
    out = []
    for (b, e) in sorted(DROPPED):
        if (b, e) in without:
            continue
        r = np.zeros((), dtype=L.pool_oos_cand_dtype)
        obs = ent[b, e]["obs"]
        r["b"], r["entry"], r["n_obs"] = b, e, len(obs)
        for q, (g, px) in enumerate(obs):
            r["group_sind"][q] = g
            r["xp"][q] = px + (200.0 if (b, e) == moved and q == 0 else 0.0)
        out.append(r)
    return np.array(out, dtype=L.pool_oos_cand_dtype)


def _frame(sc, lay, ent, cands, chi2, gate=True):
    """the scripted frame -> everything the tests look at"""
    poses, groups, feats, xp = scene_arrays(sc, CAM)
    P0 = np.array([spd(lay.N, 40 + b) * 1e-4 for b in range(B)])
    out = {}
    M_max = 2 * NF + ((ROWS + 16 + 15) // 16) * 16
    with L.Context(lay.N, M_max, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, NG, lay.feature_begin, NF, CAM)
        ctx.upload_P(P0)
        # the sub-filter's measurement variance is so large that its steps leave x where pool_add put it
        ctx.pool_config(PM, AM, Rtri=1e30, MH_thresh=1e30, ready_steps=1, min_depth=0.05, max_depth=10.0, remove_outlier_counter=1e30)
        assert ctx.pool_oos_config(OOS_MAX, max_obs=MAX_OBS, min_obs=MIN_OBS, Roos=ROOS, chi2=chi2) == ROWS
        for a in range(NG):     # anchor a takes the pose of group slot a
            pa = poses.copy()
            for b in range(B):
                pa[b]["Rsb"] = cm(sc["gR"][b, a]); pa[b]["Tsb"] = sc["gT"][b, a]
            ctx.set_scene(pa, groups, feats)
            ctx.pool_anchor(np.full(B, a, dtype=np.int32))
        ctx.set_scene(poses, groups, feats)
        ops = np.zeros(2 * B, dtype=L.edit_dtype)
        for b in range(B):
            for a in range(2):
                o = ops[2 * b + a]
                o["b"], o["kind"], o["i0"], o["i1"] = b, L.EDIT_ADD_GROUP_ANCHOR, a, a
        ctx.edit_batch(NF, ops)

        def add(late):
            recs = []
            for (b, e), d in ent.items():
                if d["late"] == late:
                    r = np.zeros((), dtype=L.pool_new_dtype)
                    r["b"], r["entry"], r["anchor"], r["xp"], r["z0"], r["std_xyz"] = b, e, d["anchor"], d["xp0"], d["z0"], [1e-3, 1e-3, 1e-2]
                    recs.append(r)
            ctx.pool_add(np.array(recs, dtype=L.pool_new_dtype))

        def step():
            ent_d = ctx.pool_get()[0]
            xpp = np.where((ent_d["ref_sind"] >= 0)[..., None], ent_d["xp"], np.nan)
            ctx.pool_step(xpp)
        add(False); step(); add(True); step()
        out["entries"], out["anchor_poses"], out["anchor_slots"] = ctx.pool_get()
        out["groups"] = ctx.get_scene()[1]
        out["P"] = ctx.download_P()
        ctx.pool_oos_collect(cands)
        out["list"] = ctx.pool_oos_get()[0]
        ctx.jacobians_instate(); ctx.mh_gate(R_VIS, MH, MULT, 5); ctx.stack(R_VIS)
        ctx.pool_oos_project()
        if gate:
            ctx.pool_oos_gate()
        out["gamma"] = ctx.pool_oos_get()[1]
        out["rows"] = [ctx.get_H(b) for b in range(B)]
        ctx.update_joseph()
        out["dx"], out["Pn"], out["status"] = ctx.get_err(), ctx.download_P(), ctx.get_status(check=False)
        out["stats"] = ctx.pool_oos_stats()
    out["sc_xp"] = xp
    return out


@pytest.fixture(scope="module")
def world():
    return _scene()


@pytest.fixture(scope="module")
def plain(built, world):
    """the frame without a gate threshold (gamma is still computed): shared by the tests that only read it"""
    sc, lay, ent = world
    return _frame(sc, lay, ent, _cands(ent), chi2=None)


def _expected_obs(ent, key):
    return [(g, px) for g, px in ent[key]["obs"] if g < NG]


def test_list_equals_the_hosts_decisions_and_the_oracles_xs(world, plain):
    sc, lay, ent = world
    lst = plain["list"]
    for b in range(B):
        for q in range(OOS_MAX):
            f = lst[b, q]
            if q >= len(USED[b]):
                assert f["n_obs"] == 0, (b, q)
                continue
            key = USED[b][q]
            obs = _expected_obs(ent, key)
            assert f["n_obs"] == len(obs), (b, q)
            assert f["group_sind"][:len(obs)].tolist() == [g for g, _ in obs], (b, q)
            assert np.array_equal(f["xp"][:len(obs)], np.array([px for _, px in obs])), (b, q)
            # Xs from what is resident: the entry and its anchor's pose (the slot's while linked, the frozen one otherwise)
            e = plain["entries"][b, key[1]]
            a = int(e["ref_sind"])
            assert a == ent[key]["anchor"] and e["status"] == 1
            slot = int(plain["anchor_slots"][b, a])
            assert slot == (a if a < 2 else -1)
            G = plain["groups"][b, slot] if slot >= 0 else plain["anchor_poses"][b, a]
            Xs = orc.feature_xs(e["x"], G["Rsb"].reshape(3, 3).T, G["Tsb"], sc["Rbc"][b], sc["Tbc"][b])
            assert np.abs(f["Xs"] - Xs).max() < 1e-10, (b, q)
    st = plain["stats"]
    assert st["oos_used"].tolist() == [0, 2, 1] and st["oos_surplus"].tolist() == [0, 2, 0]
    assert st["oos_short"].tolist() == [0, 1, 0] and st["oos_gated"].tolist() == [0, 0, 0]


def _oracle_rows(sc, lay, xp, lst, b):
    """the in-state rows and the OOS rows the oracle builds from the downloaded list; -> H, inn, dR, [(row0, rows)] per feature"""
    Js, inns, _ = oracle_jacobians(sc, CAM, lay, xp, b)
    H, inn, dR = orc.stack_measurements(Js, inns, sc["ref"][b], sc["sind"][b], lay, R_VIS)
    spans = []
    for q in range(OOS_MAX):
        f = lst[b, q]
        k = int(f["n_obs"])
        if k < 2:
            continue
        obs = [(int(f["group_sind"][i]), f["xp"][i]) for i in range(k)]
        Hxp, rp, _ = orc.oos_jacobian(f["Xs"], obs, sc["gR"][b], sc["gT"][b], sc["Rbc"][b], sc["Tbc"][b], CAM, lay)
        spans.append((len(inn), len(rp)))
        H = np.vstack([H, Hxp]); inn = np.concatenate([inn, rp]); dR = np.concatenate([dR, np.full(len(rp), ROOS)])
    return H, inn, dR, spans


def test_block_rows_equal_the_oracles_and_unfilled_rows_are_neutral(world, plain):
    sc, lay, ent = world
    for b in range(B):
        gH, ginn, gdR = plain["rows"][b]
        assert gH.shape == (2 * NF + ROWS, lay.N)
        H, inn, dR, spans = _oracle_rows(sc, lay, plain["sc_xp"], plain["list"], b)
        n = len(inn)
        assert n == 2 * NF + sum(2 * len(_expected_obs(ent, k)) - 3 for k in USED[b])
        assert rel_fro(gH[:n], H) < 1e-10 and rel_fro(ginn[:n], inn) < 1e-9 and np.allclose(gdR[:n], dR)
        assert not gH[n:].any() and not ginn[n:].any() and np.array_equal(gdR[n:], np.full(2 * NF + ROWS - n, ROOS))


def test_gamma_equals_numpy(world, plain):
    sc, lay, ent = world
    for b in range(B):
        gH, ginn, gdR = plain["rows"][b]
        _, _, _, spans = _oracle_rows(sc, lay, plain["sc_xp"], plain["list"], b)
        assert len(spans) == len(USED[b])
        for q, (r0, n) in enumerate(spans):
            Ho, ro = gH[r0:r0 + n], ginn[r0:r0 + n]
            S = Ho @ plain["P"][b] @ Ho.T + ROOS * np.eye(n)
            g = float(ro @ np.linalg.solve(S, ro))
            print("filter %d feature %d: gamma %.12g numpy %.12g" % (b, q, plain["gamma"][b, q], g))
            assert abs(plain["gamma"][b, q] - g) <= 1e-9 * g, (b, q)
        assert not plain["gamma"][b, len(spans):].any()


def test_update_with_two_oos_features_equals_the_oracles_joseph_form(world, plain):
    assert (plain["status"] == 0).all()
    for b in range(B):
        gH, ginn, gdR = plain["rows"][b]
        e_ref, P_ref, _ = orc.update_joseph(gH, plain["P"][b], ginn, gdR)
        print("filter %d: P %.3e dx %.3e" % (b, rel_fro(plain["Pn"][b], P_ref), rel_fro(plain["dx"][b], e_ref)))
        assert rel_fro(plain["Pn"][b], P_ref) < TOL_P and rel_fro(plain["dx"][b], e_ref) < TOL_DX


def test_a_pixel_moved_by_200_px_is_gated_out(built, world, plain):
    sc, lay, ent = world
    moved = _frame(sc, lay, ent, _cands(ent, moved=(1, 0)), chi2=L.CHI2_95)
    # the same frame without that feature: (1, 3) alone (the surplus entries would move up into the free position)
    without = _frame(sc, lay, ent, _cands(ent, without=[(1, 0), (1, 6), (1, 7)]), chi2=L.CHI2_95)
    assert moved["stats"]["oos_gated"].tolist() == [0, 1, 0] and without["stats"]["oos_gated"].tolist() == [0, 0, 0]
    assert moved["gamma"][1, 0] > L.CHI2_95[3] and 0 < moved["gamma"][1, 1] < L.CHI2_95[1]
    gH, ginn, gdR = moved["rows"][1]
    r0 = 2 * NF
    assert not gH[r0:r0 + 3].any() and not ginn[r0:r0 + 3].any() and np.array_equal(gdR[r0:r0 + 3], np.full(3, ROOS))
    assert gH[r0 + 3:r0 + 4].any()                                      # the second feature's row stays
    assert np.allclose(gH[r0 + 3], without["rows"][1][0][r0], rtol=1e-12, atol=0)   # ... the row the frame without the first has
    for b in range(B):
        assert rel_fro(moved["Pn"][b], without["Pn"][b]) < TOL_P and rel_fro(moved["dx"][b], without["dx"][b]) < TOL_DX


def test_refusals(built, world):
    sc, lay, ent = world
    with L.Context(lay.N, 2 * NF, B) as ctx:
        ctx.set_layout(lay.N, lay.group_begin, NG, lay.feature_begin, NF, CAM)
        with pytest.raises(L.XivoHipError):
            ctx.pool_oos_config(OOS_MAX, max_obs=MAX_OBS, min_obs=MIN_OBS)          # no pool
        ctx.pool_config(PM, AM)
        for bad in (dict(max_obs=1, min_obs=1), dict(max_obs=L.OOS_MAX_OBS + 1), dict(max_obs=3, min_obs=4), dict(Roos=0.0)):
            with pytest.raises(L.XivoHipError):
                ctx.pool_oos_config(OOS_MAX, **{**dict(max_obs=MAX_OBS, min_obs=MIN_OBS), **bad})
        ctx.pool_oos_config(OOS_MAX, max_obs=MAX_OBS, min_obs=MIN_OBS)
        with pytest.raises(L.XivoHipError):
            ctx.pool_oos_project()                                                  # nothing collected, nothing stacked
        unordered = _cands(ent)[::-1].copy()
        with pytest.raises(L.XivoHipError):
            ctx.pool_oos_collect(unordered)
        assert ctx.pool_oos_config(0) == 0                                          # off: the buffers are released
        with pytest.raises(L.XivoHipError):
            ctx.pool_oos_collect(_cands(ent))
