"""GPU: every device buffer of a context comes from the context's owner (xivo_amd/csrc/device_buffers.h) - checked through the
public API alone: a context whose buffers grew from small to large sizes computes, bit for bit, what a fresh context computes
at the large sizes and owns the same blocks (xivo_hip_selftest_ctx_allocs); re-sizing over and over does not accumulate;
contexts can be created, used and destroyed repeatedly. The owner's failure paths are tests/test_device_buffers_cpu.py: no
test here provokes an out-of-memory condition.

Shapes: N = 59 (3 group slots, 6 feature slots), M_max = 32, B = 3; the scene holds F = 4, then F = 6 features.
(F cannot go past the layout's 6 feature slots, nor past M_max / 2 = 16: every entry point refuses 2 F > M_max. So F never
exceeds Mpmax / 2, and ensure_gate_buffers and the RANSAC scratch allocate once per context, for that size: there is no
re-size of the scene buffers to run. What does grow here: the OOS list, the loop-closure rows, the sub-filter staging, the
edit ops, the pool (the one group that is released and re-allocated) and its per-call staging, the upload staging.)"""
import numpy as np
import pytest

import xivo_oracle as orc
from scene_util import scene_arrays, spd
from xivo_amd import lib as L
from xivo_amd import synth
from xivo_amd.lib import Context

pytestmark = pytest.mark.gpu
NG, NF, B, M_MAX = 3, 6, 3, 32
F_SMALL, F_LARGE = 4, 6
R_VIS, MH, MULT = 1.0, 5.991, 1.1
CAM = synth.PINHOLE


@pytest.fixture(scope="module")
def world():
    """One scene and every input of the sequences below, made once and never written to."""
    sc = synth.g_level(NG, NF, NF, B, seed=21, cam=CAM)
    lay = orc.Layout(NG, NF, N=sc["N"])
    assert lay.N == 59
    poses, groups, feats, xp = scene_arrays(sc, CAM)
    rng = np.random.default_rng(4)
    w = dict(lay=lay, poses=poses, groups=groups, feats=feats, P=np.array([spd(lay.N, 60 + b) * 1e-4 for b in range(B)]))
    oos = np.zeros((B, 2), dtype=L.oos_dtype)          # 3 + 1 rows per filter behind the 12 in-state rows
    for b in range(B):
        for o, k in enumerate((3, 2)):
            oos[b, o]["Xs"] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3, 6)]
            oos[b, o]["n_obs"] = k
            oos[b, o]["group_sind"][:k] = rng.permutation(NG)[:k]
            oos[b, o]["xp"][:k] = rng.uniform(200.0, 400.0, size=(k, 2))
    w["oos"] = oos
    lc = np.zeros((B, 3), dtype=L.lc_dtype)
    for b in range(B):
        for i in range(3):
            lc[b, i]["feat"], lc[b, i]["group_sind"], lc[b, i]["xp"] = i, feats["ref_sind"][b, i], xp[b, i] + 0.5
    w["lc"] = lc
    sub = np.zeros((B, NF), dtype=L.subfilter_dtype)
    sub["x"] = sc["x"] + rng.normal(size=sc["x"].shape) * np.array([0.01, 0.01, 0.15])
    sub["P"] = np.diag([1e-4, 1e-4, 0.25]).reshape(-1)
    sub["ref_sind"] = sc["ref"]; sub["xp"] = xp + rng.normal(size=xp.shape) * 0.8
    w["sub"] = sub
    ops = np.zeros(4, dtype=L.edit_dtype)                # sorted by filter; the first op alone is the small call
    ops["b"] = [0, 1, 2, 2]; ops["kind"] = [L.EDIT_P_ZERO_RC, L.EDIT_P_ZERO_RC, L.EDIT_P_ZERO_RC, L.EDIT_P_COPY_RC]
    ops["i0"] = [50, 44, 41, 53]; ops["i1"] = [3, 3, 3, 47]; ops["i2"] = [0, 0, 0, 3]
    w["ops"] = ops
    for name, pm in (("small", 4), ("large", 8)):
        recs = np.zeros(B * pm, dtype=L.pool_new_dtype)
        recs["b"] = np.repeat(np.arange(B), pm); recs["entry"] = np.tile(np.arange(pm), B); recs["anchor"] = 1
        recs["xp"] = rng.uniform(150.0, 450.0, size=(B * pm, 2)); recs["z0"] = rng.uniform(0.5, 8.0, B * pm)
        recs["std_xyz"] = rng.uniform(0.001, 0.2, (B * pm, 3))
        w["pool_" + name] = (pm, recs, recs["xp"].reshape(B, pm, 2) + rng.normal(size=(B, pm, 2)) * 0.5)
    return w


def context(w):
    ctx = Context(w["lay"].N, M_MAX, B)
    ctx.set_layout(w["lay"].N, w["lay"].group_begin, NG, w["lay"].feature_begin, NF, CAM)
    return ctx


def frame(ctx, w, F, out=None):
    """a step - set scene, Jacobians, gate, stack, update, absorb - from the same prior, then RANSAC and an OOS append on it"""
    ctx.upload_P(w["P"])
    ctx.set_scene(w["poses"], w["groups"], w["feats"][:, :F])
    ctx.jacobians_instate()
    mask, dist = ctx.mh_gate(R_VIS, MH, MULT, 2)
    ctx.stack(R_VIS)
    ctx.update_joseph()
    err = ctx.get_err()
    ctx.absorb_error()
    scene = ctx.get_scene()
    P1 = ctx.download_P()
    ctx.jacobians_instate()
    ctx.mh_gate(R_VIS, MH, MULT, 2, want=False)
    ransac = ctx.one_point_ransac(R_VIS, 2.0, 5.89, gauge=np.zeros(B, dtype=np.int32))
    ctx.stack(R_VIS)
    n_oos = 1 if F == F_SMALL else 2
    rows = ctx.oos_project(w["oos"][:, :n_oos], 3.5 ** 2)
    H = [ctx.get_H(b) for b in range(B)]
    if out is not None:
        out.update(mask=mask, dist=dist, err=err, scene=scene, P1=P1, ransac=ransac, oos_rows=rows, oos_H=H)


def rest(ctx, w, size, out=None):
    """the other buffers that grow on demand, at their small or their large size"""
    large = size == "large"
    ctx.snapshot_P()
    ctx.p_zero_rc(1, 30, 5)
    ctx.restore_P()
    P2 = ctx.download_P()
    ctx.close_loop_stack(w["lc"][:, :3 if large else 1], 1.5 ** 2)
    lcH = [ctx.get_H(b) for b in range(B)]
    sub = ctx.subfilter_update(w["sub"][:, :NF if large else 2], ready_steps=1)
    ctx.edit_batch(F_LARGE if large else F_SMALL, w["ops"][:4 if large else 1])
    P3 = ctx.download_P()
    pm, recs, xp = w["pool_" + size]
    ctx.pool_config(pm, 2)
    ctx.pool_anchor(np.ones(B, dtype=np.int32))
    ctx.pool_add(recs)
    order, n, live = ctx.pool_step(xp)
    pool = ctx.pool_get()
    if out is not None:
        out.update(P2=P2, lc_H=lcH, sub=sub, P3=P3, pool_order=order, pool_n=n, pool_live=live, pool=pool)


def same_bits(a, b, path=""):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, path


def test_buffers_grown_from_small_sizes_equal_a_fresh_context(built, world):
    X, Y = {}, {}
    with context(world) as ctx:                      # X: every size small first, then large
        frame(ctx, world, F_SMALL)
        rest(ctx, world, "small")
        frame(ctx, world, F_LARGE, X)
        rest(ctx, world, "large", X)
        X["allocs"] = ctx.ctx_allocs()
    with context(world) as ctx:                      # Y: fresh, the large sizes only
        frame(ctx, world, F_LARGE, Y)
        rest(ctx, world, "large", Y)
        Y["allocs"] = ctx.ctx_allocs()
    assert sorted(X) == sorted(Y)
    for key in sorted(X):
        same_bits(X[key], Y[key], key)
    # the sequences did what they are meant to do: an update, rows behind the stacked ones, a pool with live entries
    assert np.abs(X["err"]).max() > 0 and not np.array_equal(X["P1"], world["P"]) and np.array_equal(X["P2"], X["P1"])
    assert X["oos_rows"].tolist() == [4] * B and X["oos_H"][0][0].shape[0] == 2 * F_LARGE + 4 and X["lc_H"][0][0].shape[0] == 6
    assert X["pool_live"].any() and X["allocs"][0] > 0 and X["allocs"][1] > 0


def test_repeated_resize_does_not_accumulate(built, world):
    allocs = []
    with context(world) as ctx:
        for _ in range(3):
            for size, F in (("small", F_SMALL), ("large", F_LARGE), ("small", F_SMALL), ("large", F_LARGE)):
                frame(ctx, world, F)
                pm, recs, xp = world["pool_" + size]
                ctx.pool_config(pm, 2)
                ctx.pool_anchor(np.ones(B, dtype=np.int32))
                ctx.pool_add(recs)
                ctx.pool_step(xp)
            allocs.append(ctx.ctx_allocs())
    assert allocs[2] == allocs[0] == allocs[1], allocs


@pytest.mark.parametrize("life", ["pool", "immediate"])
def test_configure_frame_release_cycles_return_to_the_same_blocks(built, world, life):
    """Every area that is configured and released by a call of its own - a device life cycle (the pool's, on a pool of 4 entries
    and 2 anchors, or the immediate one), the point-cloud world, the trajectory producer, the three logs - gives back on its
    zero call what its configure call took: after one resident frame and the zero calls the context owns what it owned after
    the first such cycle. (The pool itself has no zero call: it is configured again, which releases it first.)"""
    rng = np.random.default_rng(8)
    Xs = rng.uniform(-3.0, 3.0, size=(B, 4, 3))
    groups = np.zeros((B, NG), dtype=L.group_dtype)
    groups["Rsb"][:] = np.eye(3).reshape(-1)
    feats = np.zeros((B, NF), dtype=L.feat_dtype)
    feats["sind"] = -1                                 # an empty scene: the life cycle fills it
    prop = L.prop_options(np.eye(12) * 1e-4, np.eye(23) * 1e-6, (0.0, 0.0, -9.8))
    allocs = []
    with context(world) as ctx:
        ctx.upload_P(world["P"])
        ctx.set_scene(world["poses"], groups, feats)
        for _ in range(3):
            if life == "pool":
                ctx.pool_config(4, 2)
                ctx.pool_life_config(8)
            else:
                ctx.life_config(8)
            ctx.pcw_config(4, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["cols"], CAM["rows"])
            ctx.pcw_set_world(Xs)
            ctx.trajsim_config(2, 2)
            ctx.trajsim_set(["lissajous"] * B, np.full(B, 0.5))
            ctx.traj_config(2, range(6)); ctx.map_config(2, NF); ctx.innov_config(2)
            # one resident frame: nothing goes down, nothing comes back
            ctx.trajsim_frame(0, 2)
            ctx.propagate_resident(opts=prop)
            ctx.pcw_tracks_resident(0.5, 3, 0)
            ctx.pool_life_begin_tracks(NF) if life == "pool" else ctx.life_begin_tracks(NF)
            ctx.filter_update(R_VIS, MH, MULT, 2, True)
            ctx.innov_record(0)
            ctx.absorb_error()
            ctx.pool_life_end() if life == "pool" else ctx.life_end()
            ctx.traj_record(0); ctx.map_record(0)
            assert (ctx.traj_count(), ctx.map_count(), ctx.innov_count(), ctx.trajsim_count()) == (1, 1, 1, 1)
            ctx.innov_config(0); ctx.map_config(0); ctx.traj_config(0)
            ctx.trajsim_config(0)
            ctx.pcw_config(0)
            ctx.pool_life_config(0) if life == "pool" else ctx.life_config(0)
            allocs.append(ctx.ctx_allocs())
    assert allocs[1] == allocs[0] and allocs[2] == allocs[0], allocs


def test_create_use_destroy_cycles(built, world):
    with context(world) as a, context(world) as b:
        la, lb = a.ctx_allocs(), b.ctx_allocs()
        assert la == lb and la[0] > 0 and la[1] > 0
    outs = []
    for _ in range(3):
        out = {}
        with context(world) as ctx:
            frame(ctx, world, F_LARGE, out)
            assert (ctx.get_status() == 0).all()
            out["allocs"] = ctx.ctx_allocs()
        outs.append(out)
    for o in outs[1:]:
        for key in sorted(outs[0]):
            same_bits(o[key], outs[0][key], key)
