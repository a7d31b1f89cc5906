"""GPU: the feature pool's kernels (xivo_amd/csrc/pool_kernels.hip) where their decisions turn - the cases of
tests/pool_edge_cases.py, which tests/test_pool_edges_cpu.py checks without a GPU.

A. subfilter_step against the np.longdouble restatement of Feature::SubfilterUpdate (tests/subfilter_restate.py), in units of
   the prior standard deviations, at four times the fp64 oracle's own worst error on the same inputs (no typed-in tolerance).
B. every comparison of the sub-filter and of the pool ON its threshold (exact inputs) and on both sides of it.
C. the candidate order of pool_step_kernel with ties, at the padding edges of its bitonic network.
D. adapt_depth_kernel: the strided loops, the rank n / 2, duplicates, non-finite depths, the selection and range rules."""
import numpy as np
import pytest

import pool_edge_cases as pe
import subfilter_restate as sr
from xivo_amd import lib as L
from xivo_amd import synth
from xivo_amd.lib import Context

pytestmark = pytest.mark.gpu

LD = np.longdouble
MODES = [False, True]


def context(B, cam, invdepth):
    ctx = Context(pe.N, 2 * pe.NF, B, flags=L.FLAG_INVDEPTH if invdepth else 0)
    ctx.set_layout(pe.N, 23, pe.NG, 23 + 6 * pe.NG, pe.NF, cam)
    return ctx


def empty_feats(B):
    f = np.zeros((B, 1), dtype=L.feat_dtype)
    f["sind"] = -1
    return f


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("invdepth", MODES)
@pytest.mark.parametrize("family", list(pe.FAMILIES))
def test_subfilter_step_against_the_long_double_restatement(built, family, invdepth):
    o = pe.opts_of(family)
    worst_oracle, _ = pe.family_bounds(family, invdepth)
    dev = {}
    for cam_name, cam in pe.CAMS.items():
        c = pe.draw(family, cam_name, invdepth)
        prior = pe.prior_of(c)
        with context(pe.PER_CAMERA, cam, invdepth) as ctx:
            for s in range(pe.FAMILIES[family]["steps"]):
                poses, groups, feats = pe.host_arrays(c, s, prior)
                ctx.set_scene(poses, groups, empty_feats(len(poses)))
                out = ctx.subfilter_update(feats, **o)
                if s == 0:
                    ref = pe.step_reference(family, cam_name, invdepth)[0]
                else:         # fed by the device: the references and the oracle's error belong to these inputs
                    ref = pe.reference(c, s, prior, family, cam_name, invdepth, LD)
                    f64 = pe.reference(c, s, prior, family, cam_name, invdepth, np.float64)
                    worst_oracle = pe.merge(worst_oracle, pe.errors(f64, ref, prior))
                assert pe.excluded(ref).mean() <= 0.01
                got = pe.from_feats(out)
                dev = pe.merge(dev, pe.errors(got, ref, prior))
                f = out[:, 0]
                assert same_bits(f["score"], -f["P"][:, 8])                       # Feature::score of the device's own P
                assert np.array_equal(f["status"], ref["status"]) and np.array_equal(f["init_counter"], ref["ic"])
                assert np.array_equal(f["candidate"], ref["cand"]), (family, cam_name, s)
                if family == "carried":
                    assert (np.abs(prior["P"][:, 0, 2]) > 0).all() and (prior["ic"] > 0).all()
                prior = got
    bnd = {k: pe.bound(v) for k, v in worst_oracle.items()}
    print("POOL-EDGES A | %s | %s | oracle's worst x %.1e P %.1e oc %.1e | bound x %.1e P %.1e oc %.1e | cap %.0e | device's worst "
          "x %.1e P %.1e oc %.1e" % (family, "inverse depth" if invdepth else "log depth", worst_oracle["x"], worst_oracle["P"],
                                     worst_oracle["oc"], bnd["x"], bnd["P"], bnd["oc"], pe.CAP, dev["x"], dev["P"], dev["oc"]))
    for k in dev:
        assert dev[k] <= bnd[k], (family, invdepth, k, dev[k], bnd[k])


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("invdepth", MODES)
def test_exact_cases_sit_on_their_thresholds(built, invdepth):
    poses, groups = pe.identity_pose(1)
    with context(1, pe.EXACT_CAM, invdepth) as ctx:
        ctx.set_scene(poses, groups, empty_feats(1))
        for name, pixel, over, (ic, oc), (want_oc, want_st, want_cand) in pe.exact_cases(invdepth):
            o = dict(pe.PERMISSIVE, **over)
            f = ctx.subfilter_update(pe.exact_feat(invdepth, pixel, ic, oc), **o)[0, 0]
            x, P, st, ic2, oc2 = pe.exact_oracle(invdepth, pixel, o["ready_steps"], ic, oc)
            assert same_bits(f["x"], x) and same_bits(f["x"], pe.exact_x(invdepth)), name       # P = 0: K = 0, x comes back
            assert not f["P"].any() and not P.any(), name
            assert same_bits(f["outlier_counter"], oc2) and f["outlier_counter"] == want_oc, (name, f["outlier_counter"])
            assert (f["status"], f["init_counter"], f["candidate"]) == (want_st, ic + 1, want_cand), (name, f)
            assert same_bits(f["score"], -f["P"][8])


@pytest.mark.parametrize("invdepth", MODES)
@pytest.mark.parametrize("cam_name", list(pe.CAMS))
def test_device_takes_the_restatements_branch_on_both_sides(built, cam_name, invdepth):
    c, prior, ref, idx = pe.straddle_cases(cam_name, invdepth)
    poses, groups, feats = pe.host_arrays(c, 0, prior)
    n = len(idx)
    seen = set()
    with context(n, pe.CAMS[cam_name], invdepth) as ctx:
        ctx.set_scene(poses[:n], groups[:n], empty_feats(n))
        for i in idx:
            for name, side, o, expect in pe.straddle_opts(ref, prior, i):
                f = ctx.subfilter_update(feats[i:i + 1], b0=i, **o)[0, 0]
                if "outlier" in expect:      # not an outlier: the counter is reset to 0; an outlier: it grows by sqrt(ratio) > 1
                    assert (f["outlier_counter"] > 1.0) == expect["outlier"], (cam_name, i, name, side, f["outlier_counter"])
                    assert expect["outlier"] or f["outlier_counter"] == 0.0
                else:
                    assert bool(f["candidate"] & 1) == expect["cand0"], (cam_name, i, name, side, f)
                    assert bool(f["candidate"] & 2) == expect["cand0"]           # ready_steps = 0: READY
                seen.add((name, side))
    assert len(seen) == 8


@pytest.mark.parametrize("invdepth", MODES)
def test_pool_thresholds(built, invdepth):
    """the exact case through pool_config / pool_add / pool_step (std_xyz = 0: P = 0, x never moves). Entries 1, 2, 3 of each filter
    are added first, entry 0 one frame later; step 1 gives entry 1 the counter sqrt(1 + 2^-42) = 1 + 2^-43."""
    c1 = 1.0 + 2.0 ** -43
    pm, B = 4, 2
    poses, groups = pe.identity_pose(B)
    x0 = pe.exact_x(invdepth)

    def start(remove):
        ctx = context(B, pe.EXACT_CAM, invdepth)
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.pool_config(pm, 1, remove_outlier_counter=remove, **dict(pe.PERMISSIVE, ready_steps=1))
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        recs = np.zeros(B * 3, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), 3); recs["entry"] = np.tile([1, 2, 3], B)
        recs["xp"] = pe.EXACT_PRED; recs["z0"] = pe.exact_z(invdepth)
        ctx.pool_add(recs)
        xp = np.full((B, pm, 2), np.nan)
        xp[:, 1] = pe.EXACT_OVER; xp[:, 2:] = pe.EXACT_ON
        res = ctx.pool_step(xp, False)
        late = recs[::3].copy()
        late["entry"] = 0
        ctx.pool_add(late)
        return ctx, res

    on = np.full((B, pm, 2), pe.EXACT_ON)
    # remove_outlier_counter == the counter keeps the entry
    ctx, (order, n, live) = start(c1)
    with ctx:
        ent, _, _ = ctx.pool_get()
        assert (ent["outlier_counter"][:, 1] == c1).all() and (ent["outlier_counter"][:, 2:] == 0).all()
        assert live[:, 1:].all() and not live[:, 0].any() and (ent["ref_sind"][:, 1:] == 0).all()
        assert (n == 3).all() and (order == [1, 2, 3, -1]).all()                 # all INITIALIZING (1 > ready_steps is false)
        assert (ent["status"][:, 1:] == sr.FEAT_INITIALIZING).all() and (ent["candidate"][:, 1:] == 1).all()
        # a pixel with only u NaN, only v NaN, or both frees the entry (filter 0); without `strict` READY comes before
        # INITIALIZING, whatever the entry number (filter 1: entry 0 is the late one, every P(2,2) ties at 0)
        xp = on.copy()
        xp[0, 1, 0] = np.nan; xp[0, 2, 1] = np.nan; xp[0, 3] = np.nan
        order, n, live = ctx.pool_step(xp, False)
        ent2, _, _ = ctx.pool_get()
        assert not live[0, 1:].any() and live[0, 0] and (ent2["ref_sind"][0] == [0, -1, -1, -1]).all()
        assert n[0] == 1 and list(order[0]) == [0, -1, -1, -1]
        assert live[1].all() and n[1] == 4 and list(order[1]) == [1, 2, 3, 0]
        assert list(ent2["status"][1]) == [sr.FEAT_INITIALIZING] + [sr.FEAT_READY] * 3 and list(ent2["candidate"][1]) == [1, 3, 3, 3]
        assert (ent2["outlier_counter"][1] == 0).all()                            # ratio == 1 resets entry 1's counter
        for e in range(pm):
            assert same_bits(ent2["x"][1, e], x0) and not ent2["P"][1, e].any()
    # one part in 10^6 below frees it, and the next step does not revive it; `strict` lists READY entries only
    ctx, (order, n, live) = start(c1 * (1 - pe.OFF))
    with ctx:
        ent, _, _ = ctx.pool_get()
        assert not live[:, 1].any() and live[:, 2:].all() and (ent["ref_sind"][:, 1] == -1).all()
        assert (n == 2).all() and (order == [2, 3, -1, -1]).all()
        order, n, live = ctx.pool_step(on, True)
        ent2, _, _ = ctx.pool_get()
        assert not live[:, 1].any() and (ent2["ref_sind"] == [0, -1, 0, 0]).all()
        assert ent2[:, 1].tobytes() == ent[:, 1].tobytes()                        # the dead entry is not stepped
        assert (n == 2).all() and (order == [2, 3, -1, -1]).all()                 # entry 0 is INITIALIZING: not listed
        assert (ent2["status"] == [sr.FEAT_INITIALIZING, sr.FEAT_INITIALIZING, sr.FEAT_READY, sr.FEAT_READY]).all()


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("pm", pe.ORDER_POOL_MAX)
def test_candidate_order_with_ties(built, pm, strict):
    sc = pe.order_scene(pm)
    B = pe.ORDER_B
    nogroups = np.zeros((B, pe.NG), dtype=L.group_dtype)
    with context(B, sc["cam"], False) as ctx:
        ctx.set_scene(sc["poses"][0], nogroups, empty_feats(B))
        ctx.pool_config(pm, 2, remove_outlier_counter=1e9, **pe.ORDER_OPTS)
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        ctx.pool_add(sc["early"])
        ctx.set_scene(sc["poses"][1], nogroups, empty_feats(B))
        ctx.pool_step(sc["xp"][0], strict)
        ctx.pool_anchor(np.ones(B, dtype=np.int32))
        late = sc["late"].copy()
        late["anchor"] = 1
        ctx.pool_add(late)
        ctx.set_scene(sc["poses"][2], nogroups, empty_feats(B))
        order, n, live = ctx.pool_step(sc["xp"][1], strict)
        ent, _, _ = ctx.pool_get()
    assert np.array_equal(live, sc["kind"] != "F")
    # (a) the host function on the downloaded entries, (b) the sort on (-rank, P(2,2), entry) in Python
    masked = ent.copy()
    masked["candidate"] = np.where(live, ent["candidate"], 0)
    order_h, n_h, _ = L.candidate_order(masked, strict=strict)
    order_p, n_p, keys = pe.python_order(ent, live, strict)
    assert np.array_equal(n, n_h) and np.array_equal(n, n_p)
    assert np.array_equal(order, order_h) and np.array_equal(order, order_p), pm
    # the batch holds the ties: three or more alike among the passing entries, and a tie across position pm // 2
    biggest, crosses = pe.tie_report(keys, pm)
    assert biggest >= min(3, pm) and (crosses or pm < 2), (pm, biggest, crosses)
    assert n[1] == pm and n[2] == (0 if strict else 1)
    twins = [e for e in range(pm) if sc["kind"][0, e] == "T" and (e // len(pe.MIX)) % 2 == 0]
    for e in twins[1:]:                                                            # twin tracks are bit-identical entries
        assert ent[0, e]["P"].tobytes() == ent[0, twins[0]]["P"].tobytes() and ent[0, e]["x"].tobytes() == ent[0, twins[0]]["x"].tobytes()
    # the oracle's pool (tests/test_pool_edges_cpu.py builds its tie groups on it) decides alike
    sim, _ = pe.simulate_order_scene(sc)
    assert np.array_equal(sim["candidate"][live], ent["candidate"][live]) and np.array_equal(sim["status"][live], ent["status"][live])


# ---------------------------------------------------------------- D
def _adapt(ctx, B, **cfg):
    ctx.pool_adapt_depth_config(pe.ADAPT_Z0, median_weight=pe.ADAPT_BETA, **cfg)
    return ctx.pool_adapt_depth(B)


def _close(got, want):
    return abs(got - want) <= 4e-16 * max(abs(want), 1.0)       # two roundings


def test_adapt_depth_sets(built):
    sc = pe.adapt_scene()
    B, pm = sc["B"], pe.ADAPT_PM
    names = sc["names"]
    poses, groups = pe.identity_pose(B)
    beta, z0 = pe.ADAPT_BETA, pe.ADAPT_Z0
    with context(B, synth.PINHOLE, True) as ctx:
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.pool_config(pm, 1, ready_steps=0, remove_outlier_counter=1e300)
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        xp = np.zeros((B, pm, 2))
        xp[..., 0], xp[..., 1] = 300.0, 200.0
        ctx.pool_add(sc["early"])
        ctx.pool_step(xp, False)
        ctx.pool_add(sc["late"])
        xp2 = xp.copy()
        xp2[sc["drop"]] = np.nan
        ctx.pool_step(xp2, False)
        ctx.pool_add(sc["fresh"])
        ctx.set_scene(poses, groups, sc["feats"])
        ent, _, _ = ctx.pool_get()
        sim = pe.adapt_sim_entries(sc, 2)
        used = sim["live"] | sc["drop"]
        assert np.array_equal(ent["ref_sind"] >= 0, sim["live"])
        assert same_bits(ent["x"][..., 2][used], sim["x2"][used])                  # P = 0: x[2] is 1 / z0 as pool_add wrote it
        assert np.array_equal(ent["status"][used], sim["status"][used]) and np.array_equal(ent["init_counter"][used], sim["init_counter"][used])

        def expect(sim, life, min_z, max_z, z):
            return [pe.adapt_expected(pe.adapt_depths(sc["feats"][b], sim, b, life), z[b], beta, min_z, max_z) for b in range(B)]

        def check(got, want, tag):
            bad = [(names[b], got[b], want[b]) for b in range(B) if not _close(got[b], want[b][0])]
            # (no update: init_z unchanged, bit for bit)
            bad += [(names[b], "moved") for b in range(B) if want[b][1] != "update" and not same_bits(got[b], z_start[b])]
            assert not bad, (tag, bad)

        lo, hi = names.index("median == min_z"), names.index("median == max_z")
        med = lambda b: float(np.sort(pe.adapt_depths(sc["feats"][b], sim, b, 1))[len(pe.adapt_depths(sc["feats"][b], sim, b, 1)) // 2])
        m_lo, m_hi = med(lo), med(hi)
        # round 1: the median exactly on min_z and exactly on max_z updates (inclusive); two calls compound, a third with
        # init_z_out = NULL too
        z_start = [z0] * B
        z1 = _adapt(ctx, B, min_feature_lifetime=1, min_z=m_lo, max_z=m_hi)
        w1 = expect(sim, 1, m_lo, m_hi, z_start)
        check(z1, w1, "on the range's ends")
        assert [w[1] for w in w1].count("update") == B - 1 and w1[0][1] == "empty" and w1[lo][1] == w1[hi][1] == "update"
        z_start = list(z1)
        z2 = ctx.pool_adapt_depth(B)
        check(z2, expect(sim, 1, m_lo, m_hi, z1), "second call")
        ctx._check(ctx.lib.xivo_hip_pool_adapt_depth(ctx.h, B, None))
        z_start = list(z2)
        check(ctx.pool_get_init_z(), expect(sim, 1, m_lo, m_hi, z2), "third call, no output array")
        # round 2: one ulp outside either end leaves init_z as it is
        z_start = [z0] * B
        z = _adapt(ctx, B, min_feature_lifetime=1, min_z=float(np.nextafter(m_lo, np.inf)), max_z=float(np.nextafter(m_hi, -np.inf)))
        w = expect(sim, 1, np.nextafter(m_lo, np.inf), np.nextafter(m_hi, -np.inf), z_start)
        check(z, w, "one ulp inside")
        assert w[lo][1] == w[hi][1] == "out of range" and same_bits(z[lo], z0) and same_bits(z[hi], z0)
        # rounds 3, 4: init_counter == min_feature_lifetime is excluded (late entries: 1), one less includes them; a live entry that
        # is not READY (never stepped; lifetime -1 lets its counter through) and a freed one stay out
        sel = names.index("selection")
        for life in (0, -1):
            z = _adapt(ctx, B, min_feature_lifetime=life, min_z=0.05, max_z=100.0)
            w = expect(sim, life, 0.05, 100.0, z_start)
            check(z, w, "lifetime %d" % life)
            assert not _close(z[sel], w1[sel][0])
        # one more step: the late entries' counter passes min_feature_lifetime = 1, the fresh ones are READY at counter 1
        ctx.pool_step(xp, False)
        sim3 = pe.adapt_sim_entries(sc, 3)
        ent3, _, _ = ctx.pool_get()
        assert np.array_equal(ent3["init_counter"][sim3["live"]], sim3["init_counter"][sim3["live"]])
        for life in (1, 0):
            z = _adapt(ctx, B, min_feature_lifetime=life, min_z=0.05, max_z=100.0)
            check(z, expect(sim3, life, 0.05, 100.0, z_start), "after a third step, lifetime %d" % life)
        assert not _close(z[sel], w[sel][0])


def test_adapt_depth_log_depth_range(built):
    """log depth: the device's exp is not numpy's to the last bit, so the range's ends sit at median * (1 -+ 1e-6)"""
    B, pm = 3, 8
    depths = [[0.9, 0.7, 1.1], [6.0, 7.5, 5.0, 9.0], [2.0, 3.0, 2.5, 2.25, 4.0]]
    poses, groups = pe.identity_pose(B)
    recs = pe._adapt_recs([(b, e, z) for b in range(B) for e, z in enumerate(depths[b])])
    with context(B, synth.PINHOLE, False) as ctx:
        ctx.set_scene(poses, groups, empty_feats(B))
        ctx.pool_config(pm, 1, ready_steps=0, remove_outlier_counter=1e300)
        ctx.pool_anchor(np.zeros(B, dtype=np.int32))
        ctx.pool_add(recs)
        xp = np.zeros((B, pm, 2))
        xp[..., 0], xp[..., 1] = 300.0, 200.0
        ctx.pool_step(xp, False)
        ent, _, _ = ctx.pool_get()
        med = [float(np.sort(np.exp(ent["x"][b, :len(d), 2]))[len(d) // 2]) for b, d in enumerate(depths)]
        assert med[0] < med[2] < med[1] and all(abs(m - np.sort(d)[len(d) // 2]) < 1e-14 * m for m, d in zip(med, depths))
        for f_lo, f_hi, moved in ((1 - pe.OFF, 1 + pe.OFF, [True, True, True]), (1 + pe.OFF, 1 + pe.OFF, [False, True, True]),
                                  (1 - pe.OFF, 1 - pe.OFF, [True, False, True]), (1 + pe.OFF, 1 - pe.OFF, [False, False, True])):
            z = _adapt(ctx, B, min_feature_lifetime=0, min_z=med[0] * f_lo, max_z=med[1] * f_hi)
            for b in range(B):
                want = (1 - pe.ADAPT_BETA) * pe.ADAPT_Z0 + pe.ADAPT_BETA * med[b] if moved[b] else pe.ADAPT_Z0
                # the two roundings of the update, and beta times the median's own error: the device's exp and numpy's are
                # each within one ulp (2^-52 relative) of the true value
                tol = 4e-16 * max(want, 1.0) + pe.ADAPT_BETA * 2.0 * 2.0 ** -52 * med[b]
                assert abs(z[b] - want) <= tol, (b, z[b], want)
                assert moved[b] or same_bits(z[b], pe.ADAPT_Z0)
