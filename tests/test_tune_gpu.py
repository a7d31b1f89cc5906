"""GPU: the tuning table (xivo_hip_tune_*) against the unchanged scalar path. The yardstick throughout is a context that never
configured a table and is given tuning t through the calls' own arguments - a plain HipBackend of configuration cfg_t; the tuned
context holds T = 3 tunings x W = 2 worlds = 6 filters, filter t * W + w. Everything is compared by bytes: the same operations
run on the same operands, so there is no tolerance.

Shape: n_groups = 4, n_features = 8, tracks_max = 16, a static camera looking at eight scripted points per world (a few of them
pushed off by 4 to 14 pixels from frame 1 on, so that the gates have something to decide), one IMU record per frame that
pushes the body along its x axis."""
import os
import sys

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import pcw, sequence

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import xivo_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

T, W = 3, 2
B = T * W
SHAPE = dict(n_groups=4, n_features=8, tracks_max=16)
# three tunings: R = 0.25 / 1 / 4 (factors of 4), thresholds, new-feature depth std and both noise matrices all differ
TUNINGS = (
    dict(visual_meas_std=0.5, MH_thresh=3.0, initial_std_z=0.05, Qimu=dict(gyro=1e-3, accel=1e-2, gyro_bias=0.0, accel_bias=0.0),
         Qmodel=dict(Wsb=0.005, Wbc=0.0, Wsg=0.0)),
    dict(visual_meas_std=1.0, MH_thresh=5.991, initial_std_z=0.10, Qimu=dict(gyro=5e-3, accel=5e-2, gyro_bias=0.0, accel_bias=0.0),
         Qmodel=dict(Wsb=0.01, Wbc=0.0, Wsg=0.0)),
    dict(visual_meas_std=2.0, MH_thresh=9.0, initial_std_z=0.30, Qimu=dict(gyro=2e-2, accel=2e-1, gyro_bias=1e-4, accel_bias=1e-3),
         Qmodel=dict(Wsb=0.02, Wbc=1e-3, Wsg=0.0)),
)
# pixels a point is pushed off by from frame 1 on (the sign alternates with the frame)
OFFSETS = {2: (3.25, -2.25), 4: (6.0, -4.25), 6: (11.25, 8.75)}


def _cfg(t=1, **kw):
    return sequence.SequenceConfig(lifecycle="device", **dict(SHAPE, **dict(TUNINGS[t], **kw)))


def _table(cfgs):
    return np.repeat(np.array([sequence.HipBackend.tuning_entry(c) for c in cfgs], dtype=L.tune_dtype), W)


def _poses(cfg):
    p = sequence.initial_poses(cfg, [pcw.TrajectorySim("lissajous", seed=40 + w) for w in range(W)])
    p["Vsb"] = 0.0
    return p


def _tracks(t, clean=False):
    """frame t: per world (ids [8], meas [8, 3])"""
    out = []
    for w in range(W):
        meas = []
        for p in range(8):
            rng = np.random.default_rng(1000003 * w + 1009 * t + p)
            u, v = 90.0 + 60.0 * p + 7.0 * w, 110.0 + 35.0 * ((p * 5) % 9)
            du, dv = OFFSETS.get(p, (0.0, 0.0)) if (t >= 1 and not clean) else (0.0, 0.0)
            s = 1.0 if t % 2 else -1.0
            meas.append((u + s * du + rng.uniform(-0.3, 0.3), v + s * dv + rng.uniform(-0.3, 0.3), 1.5 + 0.25 * (p % 5)))
        out.append((np.arange(8, dtype=np.int64) + 100 + 1000 * w, np.array(meas)))
    return out


def _imu(poses, n_imu=1, dt=0.04):
    rec = np.zeros((W, n_imu), dtype=L.imu_dtype)
    for w in range(W):
        Rsb = poses[w]["Rsb"].reshape(3, 3).T
        for k in range(n_imu):
            rec[w, k]["accel"] = Rsb.T @ np.array([0.0, 0.0, 9.8]) + np.array([2.0 + 0.5 * k, 0.1 * w, 0.0])
            rec[w, k]["gyro"] = (0.02 * (k + 1), -0.01, 0.015 * (w + 1))
            rec[w, k]["slope_gyro"] = (0.1, 0.0, -0.05)
    rec["dt"] = dt / n_imu
    return rec


class _Ctxs:
    """the tuned context X (6 filters on `base`) and the scalar contexts S[t] (2 filters on cfgs[t]), with their runners"""

    def __init__(self, cfgs, base, table="cfgs"):
        self.cfgs, self.base, self.open = cfgs, base, []
        poses = _poses(base)
        self.poses = poses
        mk = lambda cfg, n, p: self._add(sequence.HipBackend(cfg, n, p, np.repeat(cfg.P_init()[None], n, axis=0)))
        self.X = mk(base, B, np.tile(poses, T))
        self.S = [mk(c, W, poses) for c in cfgs]
        if table == "cfgs":
            self.X.enable_tuning(_table(cfgs))
        self.rX = sequence.SequenceRunner(self.X, base, B)
        self.rS = [sequence.SequenceRunner(s, c, W) for s, c in zip(self.S, cfgs)]

    def _add(self, be):
        self.open.append(be)
        return be

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for be in self.open:
            be.close()

    def frame(self, t, imu=True, clean=False):
        tr = _tracks(t, clean)
        rec = _imu(self.poses) if (imu and t > 0) else None
        self.rX.frame(None if rec is None else np.tile(rec, (T, 1)), tr * T)
        for r in self.rS:
            r.frame(rec, tr)

    def each(self, fn):
        """fn(backend) of the tuned context, and of the scalar contexts concatenated in filter order"""
        got = fn(self.X)
        want = [fn(s) for s in self.S]
        if isinstance(got, tuple):
            return got, tuple(np.concatenate([w[i] for w in want]) for i in range(len(got)))
        return got, np.concatenate(want)


def _state(be):
    poses, groups, feats = be.scene()
    fid, fref, grefs = be.life_book()
    mask, dist = be.ctx.get_gate(be.F)
    return (be.covariance(), poses, groups, feats, fid, fref, grefs, mask, dist, be.life_stats(), be.ctx.get_status(check=False))


NAMES = ("P", "poses", "groups", "feats", "feat_id", "feat_ref", "group_refs", "mask", "mh_dist", "life stats", "status")


def _same(got, want, tag):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        assert g.tobytes() == w.tobytes(), (tag, name)


def _differs(a, t0=0, t1=2):
    """filters of tuning t0 against those of tuning t1 (same worlds)"""
    a = np.asarray(a)
    return a[t0 * W:(t0 + 1) * W].tobytes() != a[t1 * W:(t1 + 1) * W].tobytes()


# ---------------------------------------------------------------- 1. a table that repeats the scalar arguments
def test_table_of_the_scalar_arguments_changes_nothing():
    cfg = _cfg(1)
    with _Ctxs([cfg] * T, cfg) as c:
        for t in range(4):
            c.frame(t)
            _same(*c.each(_state), "frame %d" % t)
        st = c.X.life_stats()
        assert st["admitted"].sum() > 0 and st["updates"].sum() > 0


# ---------------------------------------------------------------- 2. per filter, stage by stage
@pytest.mark.parametrize("method", ["RK4", "PD"])
@pytest.mark.parametrize("n_imu", [1, 3])
@pytest.mark.parametrize("rng_", [(0, B), (2, 3)])
def test_propagate_per_filter(method, n_imu, rng_):
    """every tuning starts from the same dense P and poses: what differs afterwards is the work of Qimu / Qmodel alone"""
    b0, nb = rng_
    cfgs = [_cfg(t) for t in range(T)]
    with _Ctxs(cfgs, cfgs[1]) as c:
        N = cfgs[0].N
        A = 0.02 * np.random.default_rng(5).standard_normal((W, N, N))
        P = cfgs[0].P_init()[None] + A @ A.transpose(0, 2, 1)
        c.X.ctx.upload_P(np.tile(P, (T, 1, 1)))
        for s in c.S:
            s.ctx.upload_P(P)
        before = c.X.covariance()
        rec = _imu(c.poses, n_imu)
        g, step = cfgs[1].gravity, cfgs[1].stepsize
        c.X.ctx.propagate(np.tile(rec, (T, 1))[b0:b0 + nb], c.X.Qimu, c.X.Qmodel, g, method=method, stepsize=step, b0=b0)
        for t, s in enumerate(c.S):
            ws = [w for w in range(W) if b0 <= t * W + w < b0 + nb]
            if ws:
                s.ctx.propagate(rec[ws[0]:ws[-1] + 1], s.Qimu, s.Qmodel, g, method=method, stepsize=step, b0=ws[0])
        (Px, px), (Ps, ps) = c.each(lambda be: (be.covariance(), be.scene()[0]))
        assert Px.tobytes() == Ps.tobytes() and px.tobytes() == ps.tobytes()
        inside = np.zeros(B, dtype=bool); inside[b0:b0 + nb] = True
        assert Px[~inside].tobytes() == before[~inside].tobytes()
        assert all(Px[b].tobytes() != before[b].tobytes() for b in np.nonzero(inside)[0])
        # the same world under two tunings: equal states and records in, different covariances out
        ta, tb = (0, 2) if nb == B else (1, 2)
        wa = 0 if nb == B else 0          # filters (1, 0) = 2 and (2, 0) = 4 are both inside [2, 5)
        assert Px[ta * W + wa].tobytes() != Px[tb * W + wa].tobytes()
        assert px[ta * W + wa].tobytes() == px[tb * W + wa].tobytes()       # (the nominal state does not read Q)


def _full_J(J, feats, lay):
    """compact 2 x 21 Jacobians -> [F, 2, N] (the column map of the gate: Wsb, Tsb, Wbc, Tbc, group, feature)"""
    F = J.shape[0]
    out = np.zeros((F, 2, lay.N))
    for f in range(F):
        if feats[f]["sind"] < 0:
            continue
        gb = lay.group_begin + 6 * int(feats[f]["ref_sind"]); fb = lay.feature_begin + 3 * int(feats[f]["sind"])
        cols = list(range(0, 6)) + list(range(15, 21)) + list(range(gb, gb + 6)) + list(range(fb, fb + 3))
        out[f][:, cols] = J[f]
    return out


def test_gate_stack_update_life_end_per_filter():
    cfgs = [_cfg(t) for t in range(T)]
    table = _table(cfgs)
    with _Ctxs(cfgs, cfgs[1]) as c:
        assert np.array_equal(c.X.ctx.tune_get(), table)
        # frame 0: no feature in the state yet; life_end admits the eight tracks with diag(var_xyz[b])
        c.frame(0)
        _same(*c.each(_state), "frame 0")
        P, feats = c.X.covariance(), c.X.scene()[2]
        fb = 23 + 6 * SHAPE["n_groups"]
        for b in range(B):
            on = np.nonzero(feats[b]["sind"] >= 0)[0]
            assert on.size == 8
            for j in on:
                blk = P[b][fb + 3 * j:fb + 3 * j + 3, fb + 3 * j:fb + 3 * j + 3]
                assert blk.tobytes() == np.diag(table[b]["var_xyz"]).tobytes(), (b, j)
        assert _differs(P)
        # frame 1, stage by stage
        rec = _imu(c.poses)
        off, ids, meas = c.rX._pack_tracks(_tracks(1) * T)
        c.X.propagate(np.tile(rec, (T, 1))); c.X.life_begin(off, ids, meas)
        for s, r in zip(c.S, c.rS):
            s.propagate(rec); s.life_begin(*r._pack_tracks(_tracks(1)))
        _same(*c.each(_state), "frame 1 begin")
        base = cfgs[1]
        c.X.ctx.jacobians_instate()
        mx, dx = c.X.ctx.mh_gate(base.visual_meas_std ** 2, base.MH_thresh, base.MH_adjust_factor, base.min_inliers)
        ms, ds, omask = [], [], []
        lay = orc.Layout(SHAPE["n_groups"], SHAPE["n_features"])
        for t, (s, cf) in enumerate(zip(c.S, cfgs)):
            s.ctx.jacobians_instate()
            m, d = s.ctx.mh_gate(cf.visual_meas_std ** 2, cf.MH_thresh, cf.MH_adjust_factor, cf.min_inliers)
            ms.append(m); ds.append(d)
            # the premise, on the oracle: the scalar context's P, Jacobians and innovations gated on the CPU with tuning t
            J, inn = s.ctx.get_jacobians()
            Ps, fs = s.covariance(), s.scene()[2]
            for w in range(W):
                dist = orc.mh_distances(_full_J(J[w], fs[w], lay), Ps[w], inn[w], cf.visual_meas_std ** 2)
                om, _, used = orc.mh_gate(dist, cf.MH_thresh, cf.MH_adjust_factor, cf.min_inliers)
                assert used == cf.MH_thresh      # (no relaxation in this case)
                print("tuning %d world %d: oracle distances %s" % (t, w, np.round(dist, 3).tolist()))
                omask.append(om)
        omask = np.array(omask).reshape(T, W, -1)
        assert (omask[0] != omask[2]).any() and omask[2].sum() > omask[0].sum(), "the inputs must part the tunings (oracle)"
        assert mx.tobytes() == np.concatenate(ms).tobytes() and dx.tobytes() == np.concatenate(ds).tobytes()
        assert np.array_equal(mx, omask.reshape(B, -1))
        assert _differs(mx)
        # stack: diagR of an inlier's rows is R_b, everything else of the block stays neutral; H through the re-stacking
        c.X.ctx.stack(base.visual_meas_std ** 2)
        for s, cf in zip(c.S, cfgs):
            s.ctx.stack(cf.visual_meas_std ** 2)
        for b in range(B):
            Hx, ix, rx = c.X.ctx.get_H(b)
            Hs, is_, rs = c.S[b // W].ctx.get_H(b % W)
            assert Hx.tobytes() == Hs.tobytes() and ix.tobytes() == is_.tobytes() and rx.tobytes() == rs.tobytes(), b
            rows = np.repeat(mx[b], 2)
            assert rows.any() and (rx[:rows.size][rows] == table[b]["R"]).all() and (rx[:rows.size][~rows] == 1.0).all(), b
            assert np.abs(Hx[:rows.size][rows]).sum() > 0
        # filter_update (Jacobians, gate, stacking, update in one call): P, err, status
        c.X.ctx.filter_update(base.visual_meas_std ** 2, base.MH_thresh, base.MH_adjust_factor, base.min_inliers, True)
        for s, cf in zip(c.S, cfgs):
            s.ctx.filter_update(cf.visual_meas_std ** 2, cf.MH_thresh, cf.MH_adjust_factor, cf.min_inliers, True)
        (Px, ex, sx), (Ps, es, ss) = c.each(lambda be: (be.covariance(), be.ctx.get_err(), be.ctx.get_status(check=False)))
        assert Px.tobytes() == Ps.tobytes() and ex.tobytes() == es.tobytes() and sx.tobytes() == ss.tobytes()
        assert (sx == 0).all() and np.abs(ex).sum() > 0 and _differs(Px) and _differs(ex)
        for be in [c.X] + c.S:
            be.ctx.absorb_error()
            be.life_end()
        _same(*c.each(_state), "frame 1 end")
        # two more whole frames through the runner
        for t in (2, 3):
            c.frame(t)
            _same(*c.each(_state), "frame %d" % t)
        st = c.X.life_stats()
        assert _differs(st["rejected"]) or st["rejected"][:W].sum() != st["rejected"][2 * W:].sum()


# ---------------------------------------------------------------- 3. the relaxation loop
def test_relaxation_loop_per_filter():
    """tuning 0 and 2: a threshold that leaves fewer than min_inliers, so the loop relaxes it; tuning 1 does not relax"""
    cfgs = [_cfg(0, MH_thresh=0.02), _cfg(1), _cfg(2, MH_thresh=0.05)]
    with _Ctxs(cfgs, cfgs[1]) as c:
        relaxed = []
        for t in range(3):
            c.frame(t)
            got, want = c.each(_state)
            _same(got, want, "frame %d" % t)
            if t != 1:
                continue
            # frame 1 (all eight features in the state), on the oracle: the loop of src/update.cpp:72-96 over the scalar
            # contexts' own distances
            for s, cf in zip(c.S, cfgs):
                mask, dist = s.ctx.get_gate(s.F)
                for w in range(W):
                    assert np.isfinite(dist[w]).all()
                    om, _, used = orc.mh_gate(dist[w], cf.MH_thresh, cf.MH_adjust_factor, cf.min_inliers)
                    print("thresh %g: used %g, distances %s" % (cf.MH_thresh, used, np.round(dist[w], 4).tolist()))
                    relaxed.append(used > cf.MH_thresh)
                    assert np.array_equal(om, mask[w]) and om.sum() >= cf.min_inliers
        relaxed = np.array(relaxed).reshape(T, W)
        assert relaxed[0].all() and not relaxed[1].any(), relaxed.tolist()
        assert c.X.life_stats()["updates"].sum() > 0


# ---------------------------------------------------------------- 4. table handling
def test_table_set_get_release():
    cfgs = [_cfg(t) for t in range(T)]
    cfg = cfgs[1]
    with _Ctxs([cfg] * T, cfg, table=None) as c:
        X = c.X
        with pytest.raises(L.XivoHipError) as e:          # no table yet
            X.ctx.tune_set(_table(cfgs)[:1])
        assert e.value.status == -1
        live0 = X.ctx.ctx_allocs()[0]
        X.enable_tuning(_table([cfg] * T))
        assert X.ctx.ctx_allocs()[0] == live0 + 5
        assert X.ctx.tune_get().tobytes() == _table([cfg] * T).tobytes()
        c.frame(0)
        _same(*c.each(_state), "frame 0")
        # a sub-range: the other rows keep their bits
        new = _table(cfgs)
        X.ctx.tune_set(new[2:5], b0=2)
        got = X.ctx.tune_get()
        want = _table([cfg] * T); want[2:5] = new[2:5]
        assert got.tobytes() == want.tobytes()
        assert X.ctx.tune_get(3, 2).tobytes() == new[3:5].tobytes()
        X.ctx.tune_set(new[:0])                            # an empty range is no error
        assert X.ctx.tune_get().tobytes() == want.tobytes()
        # released: the scalar arguments are back, and the blocks are the owner's no more
        X.enable_tuning(None)
        assert X.ctx.ctx_allocs()[0] == live0
        with pytest.raises(L.XivoHipError):
            X.ctx.tune_get()
        X.ctx.tune_config(None)                            # (twice is no error)
        for t in (1, 2):
            c.frame(t)
            _same(*c.each(_state), "frame %d after release" % t)


# ---------------------------------------------------------------- 5. refusals
def _entry(cfg, **kw):
    e = sequence.HipBackend.tuning_entry(cfg).copy()
    for k, v in kw.items():
        if isinstance(v, tuple):
            e[k][v[0]] = v[1]
        else:
            e[k] = v
    return e


BAD = [dict(R=0.0), dict(R=-1.0), dict(R=np.nan), dict(R=np.inf), dict(mh_thresh=0.0), dict(mh_thresh=-2.0), dict(mh_thresh=np.nan),
       dict(mh_thresh=np.inf), dict(var_xyz=(1, -1e-9)), dict(var_xyz=(2, np.nan)), dict(var_xyz=(0, np.inf)), dict(Qimu=(13, np.nan)),
       dict(Qimu=(143, np.inf)), dict(Qmodel=(0, -np.inf)), dict(Qmodel=(528, np.nan))]


def test_refusals_leave_everything_unchanged():
    cfgs = [_cfg(t) for t in range(T)]
    cfg = cfgs[1]
    with _Ctxs(cfgs, cfg) as c:
        X = c.X
        c.frame(0); c.frame(1)
        snap = lambda: tuple(a.tobytes() for a in _state(X)) + (X.ctx.tune_get().tobytes(),)
        before = snap()

        def refused(status, fn, *a, **kw):
            with pytest.raises(L.XivoHipError) as e:
                fn(*a, **kw)
            assert e.value.status == status, (fn.__name__, a, kw)
            assert snap() == before, (fn.__name__, a, kw)

        good = sequence.HipBackend.tuning_entry(cfgs[2])
        for bad in BAD:
            refused(-1, X.ctx.tune_set, np.array([_entry(cfg, **bad)]), b0=3)
            refused(-1, X.ctx.tune_config, _entry(cfg, **bad))
            # one bad row in the middle of three: none of the three is written
            refused(-1, X.ctx.tune_set, np.array([good, _entry(cfg, **bad), good]), b0=1)
        for b0, nb in ((-1, 1), (B, 1), (B - 1, 2), (0, B + 1)):
            refused(-1, X.ctx.tune_set, np.array([good] * nb), b0=b0)
            with pytest.raises(L.XivoHipError) as e:
                X.ctx.tune_get(b0, nb)
            assert e.value.status == -1
        R, th, mult, mi = cfg.visual_meas_std ** 2, cfg.MH_thresh, cfg.MH_adjust_factor, cfg.min_inliers
        refused(-5, X.ctx.one_point_ransac, R, cfg.ransac_thresh, cfg.ransac_Chi2)
        refused(-5, X.ctx.mh_gate_dense, X.F, R, th, mult, mi)
        refused(-5, X.ctx.update_dense_gated, X.F, R, th, mult, mi)
        refused(-5, X.ctx.propagate_calib, np.tile(_imu(c.poses), (T, 1)), X.Qimu, np.eye(24), cfg.gravity)
        refused(-5, X.ctx.set_calib, td=23)
        # the scalar arguments are still validated
        refused(-1, X.ctx.filter_update, -1.0, th, mult, mi)
        refused(-1, X.ctx.mh_gate, R, np.nan, mult, mi)
        refused(-1, X.ctx.mh_gate, R, th, 0.5, mi)
        # and the context still runs
        c.frame(2)
        _same(*c.each(_state), "frame 2")
    # a context with online calibration takes no table
    with L.Context(cfg.N, cfg.M_max(), 2) as ctx:
        ctx.set_layout(cfg.N, 23, cfg.n_groups, 23 + 6 * cfg.n_groups, cfg.n_features, cfg.cam)
        ctx.set_calib(td=23)
        live = ctx.ctx_allocs()
        with pytest.raises(L.XivoHipError) as e:
            ctx.tune_config(sequence.HipBackend.tuning_entry(cfg))
        assert e.value.status == -5 and ctx.ctx_allocs() == live
        ctx.set_calib()
        ctx.tune_config(sequence.HipBackend.tuning_entry(cfg))
        assert ctx.tune_get().tobytes() == np.repeat(np.array([sequence.HipBackend.tuning_entry(cfg)]), 2).tobytes()


# ---------------------------------------------------------------- 6. the pool life cycle
QUICK = dict(feature_init="subfilter", pool_lifecycle="device", initial_z=5.0, initial_std_z=0.5, max_group_lifetime=3,
             subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=1), n_groups=4, n_features=8, tracks_max=128)
POOL_TUNE = [{k: v for k, v in tn.items() if k != "initial_std_z"} for tn in TUNINGS]


def _pool_run(cfg, n_tunings, table):
    """4 camera frames of run_pcw on two seeded worlds and trajectories, n_tunings times over"""
    worlds = [pcw.RandomPCW(npts=110, seed=20 + w) for _ in range(n_tunings) for w in range(W)]
    sims = [pcw.TrajectorySim("trefoil" if w % 2 else "lissajous", seed=400 + w) for _ in range(n_tunings) for w in range(W)]

    def factory(cfg_, n, poses0, P0):
        be = sequence.HipBackend(cfg_, n, poses0, P0)
        if table is not None:
            be.enable_tuning(table)
        return be
    out = sequence.run_pcw(factory, cfg, worlds, sims, total_time=4 * 0.04, trajectory_log=True, innovation_log=True)
    be = out["backend"]
    try:
        ent, ap, sl = be.ctx.pool_get(0, be.B)
        bk = be.pool_life_book()
        return (be.covariance(),) + tuple(be.scene()) + (ent, ap, sl, bk["feat_id"], bk["ent_id"], be.pool_life_stats(),
                                                         out["trajectory"]["cov"], out["trajectory"]["Tsb"], out["innovation"]["recs"])
    finally:
        be.close()


def test_pool_life_cycle_per_filter():
    cfgs = [sequence.SequenceConfig(**dict(QUICK, **tn)) for tn in POOL_TUNE]
    got = _pool_run(cfgs[1], T, _table(cfgs))
    want = [_pool_run(cf, 1, None) for cf in cfgs]
    names = ("P", "poses", "groups", "feats", "pool entries", "anchor poses", "anchor slots", "feat_id", "ent_id", "stats",
             "logged cov", "logged Tsb", "innovation records")
    for i, name in enumerate(names):
        w = np.concatenate([x[i] for x in want], axis=1 if name.startswith(("logged", "innovation")) else 0)
        assert got[i].shape == w.shape and got[i].tobytes() == np.ascontiguousarray(w).tobytes(), name
    st = got[9]
    assert st["admitted"].sum() > 0 and st["updates"].sum() > 0, "no feature reached the state: R and MH_thresh were never read"
    assert _differs(got[0])
