"""GPU: loop closure inside the device "immediate" life cycle (xivo_hip_lcmap_life_config: SequenceConfig.lc_lifecycle="device")
against the host life cycle with loop closure (lifecycle="host": SequenceRunner.frame's own book, _lc_add / _lc_close), on the
same scripted tracks and keys. The reference is the host life cycle throughout, and everything is compared with np.array_equal /
bytes: P, the scene, the book and its keys, the map, the match lists, the counters.

The scripts: B = 3 filters, n_groups = 4, n_features = 8, tracks_max = 16, a static camera (no IMU records) looking at up to
twelve hand-placed points per filter; a point's track id changes when it comes back, its key does not. Depths: 1.0 in the
log-depth build, so that log z of a new feature is exact whatever library computes it (the one place the two life cycles may
differ in the last bit, tests/test_lifecycle_gpu.py) and whole runs can be held bit for bit; varied in the inverse-depth build.

The device pool life cycle has no keys (ent_key): loop closure stays refused there, and nothing here runs it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_lifecycle_gpu import _same_scene
from xivo_amd import lib as L
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
SHAPE = dict(n_groups=4, n_features=8)
LC = dict(loop_closure=True, lc_map_max=8, lc_max=4, lc_min_matches=2)
INV = dict(use_invdepth=True, initial_std_z=0.05)


def _cfgs(invdepth=True, shape=SHAPE, tracks_max=16, **lc):
    kw = dict(shape, **(INV if invdepth else {}), **dict(LC, **lc))
    return (sequence.SequenceConfig(**kw),
            sequence.SequenceConfig(lifecycle="device", tracks_max=tracks_max, lc_lifecycle="device", **kw))


def _pixel(p, t, b, outlier=False):
    """point p of filter b in frame t: a grid in the image, a fraction of a pixel of scripted jitter"""
    rng = np.random.default_rng(1000003 * b + 1009 * t + p)
    u, v = 80.0 + 45.0 * (p % 12) + 3.0 * b, 100.0 + 35.0 * ((p * 5) % 9) + 0.5 * (p // 12)
    if outlier:
        u, v = u + 90.0, v - 70.0
    return u + rng.uniform(-0.3, 0.3), v + rng.uniform(-0.3, 0.3)


def _frames(script, invdepth):
    """script: per frame, per filter a list of (track id, key, point[, "outlier"]) -> per frame (tracks, keys)"""
    out = []
    for t, per in enumerate(script):
        tracks, keys = [], []
        for b, lst in enumerate(per):
            ids = np.array([x[0] for x in lst], dtype=np.int64)
            meas = np.array([_pixel(x[2], t, b, len(x) > 3) + ((1.5 + 0.25 * (x[2] % 5)) if invdepth else 1.0,) for x in lst],
                            dtype=float).reshape(-1, 3)
            tracks.append((ids, meas)); keys.append(np.array([x[1] for x in lst], dtype=np.int64))
        out.append((tracks, keys))
    return out


def _revisit(n_frames=8, short_keys=True, leave=(4, 5, 6, 7), n_pts=8, new_keys=False):
    """filter 0: points `leave` are hidden in frame 1 and back from frame 2 on under new track ids with their old keys; filter 1:
    the same, but only the first of them keeps its key (one match: short); filter 2: no tracks at all. new_keys: every track's
    key is its track id - no key ever repeats."""
    script = []
    for t in range(n_frames):
        per = []
        for b in range(2):
            lst = []
            for p in range(n_pts):
                if p in leave and t == 1:
                    continue
                back = p in leave and t >= 2
                tid = 100 + 1000 * b + p + (100 if back else 0)
                key = p if not (b == 1 and back and p != leave[0] and short_keys) else 5000 + p
                lst.append((tid, tid if new_keys else key, p))
            per.append(lst)
        per.append([])
        script.append(per)
    return script


class _Host(sequence.HipBackend):
    """the host life cycle's backend, keeping what the resident state and the map look like between the stages of a frame"""

    def lcmap_add(self, recs):
        super().lcmap_add(recs)
        self.snap["add"] = _map(self)

    def update(self, download=True):
        self.snap["begin"] = (self.covariance(), self.scene())
        mask = super().update(download=True)
        self.snap["update"] = (self.covariance(), self.scene(), mask)
        return mask

    def lcmap_close(self, queries):
        n = super().lcmap_close(queries)
        self.snap["close"] = (self.covariance(), self.scene(), _map(self), n)
        return n


def _map(be):
    ent, cnt = be.ctx.lcmap_get(0, be.B)
    out = dict(entries=ent.tobytes(), count=cnt.tolist(), matches=be.ctx.lcmap_matches(0, be.B).tobytes(), stats=be.lcmap_stats().tobytes())
    if getattr(be, "lc_cov_on", False):
        out["cov_stats"] = be.lcmap_cov_stats().tobytes()
        if be.cfg.lc_point_cov:
            out["cov"] = be.ctx.lcmap_get_cov(0, be.B).tobytes()
    return out


def _poses(cfg):
    return sequence.initial_poses(cfg, [pcw.TrajectorySim("lissajous", seed=40 + b) for b in range(B)])


def _push(poses, a0=2.0, dt=0.04):
    """one IMU record per filter: no rotation, the specific force of a body at rest plus a0 m/s^2 along its x axis for dt
    seconds - the estimate moves a few millimetres a frame, enough for the depth variances to part"""
    rec = np.zeros((B, 1), dtype=L.imu_dtype)
    for b in range(B):
        Rsb = poses[b]["Rsb"].reshape(3, 3).T
        rec[b, 0]["accel"] = Rsb.T @ np.array([0.0, 0.0, 9.8]) + np.array([a0, 0.0, 0.0])
    rec["dt"] = dt
    return rec


def _open(cfg_h, cfg_d, host_cls=sequence.HipBackend, still=False):
    poses = _poses(cfg_h)
    if still:
        poses["Vsb"] = 0.0
    P0 = np.repeat(cfg_h.P_init()[None], B, axis=0)
    H = host_cls(cfg_h, B, poses, P0)
    try:
        D = sequence.HipBackend(cfg_d, B, poses, P0)
    except Exception:
        H.close()
        raise
    return H, D, sequence.SequenceRunner(H, cfg_h, B), sequence.SequenceRunner(D, cfg_d, B)


def _same(H, D, rh, tag, x2_ulp=0):
    assert np.array_equal(D.covariance(), H.covariance()), (tag, "P")
    _same_scene(D.scene(), H.scene(), x2_ulp, tag)
    fid, fref, grefs = D.life_book()
    keys = D.ctx.lcmap_life_get_keys(0, B)
    for b in range(B):
        bk = rh.books[b]
        assert fid[b].tolist() == bk.feat_id and fref[b].tolist() == bk.feat_ref and grefs[b].tolist() == bk.group_refs, (tag, b)
        # the book's key of every held slot; a free slot reads -1 (the host's list keeps what it last held there)
        assert keys[b].tolist() == [k if i >= 0 else -1 for i, k in zip(bk.feat_id, bk.feat_key)], (tag, b)
    assert _map(D) == _map(H), (tag, "map")
    st = D.life_stats()
    assert int(st["rejected"].sum()) == rh.n_rejected and int(st["not_spd"].sum()) == getattr(H, "n_not_spd", 0), tag


def _run(script, invdepth=True, every_frame=True, push=False, **lc):
    """both life cycles over the script, equal after every frame -> (the map counters, the device's life counters, the map's
    entries and counts, the host's P of every frame). push: the filters start at rest and every frame but the first brings the
    record of _push"""
    cfg_h, cfg_d = _cfgs(invdepth, **lc)
    H, D, rh, rd = _open(cfg_h, cfg_d, still=push)
    try:
        Ps = []
        rec = _push(_poses(cfg_h)) if push else None
        for t, (tracks, keys) in enumerate(_frames(script, invdepth)):
            rh.frame(rec if t else None, tracks, keys)
            rd.frame(rec if t else None, tracks, keys)
            if every_frame or t == len(script) - 1:
                _same(H, D, rh, "frame %d" % t)
            Ps.append(H.covariance())
        assert getattr(rd, "n_lc_closed", 0) == getattr(rh, "n_lc_closed", 0)
        st = D.lcmap_stats()
        print({k: st[k].tolist() for k in st.dtype.names}, "closed", getattr(rd, "n_lc_closed", 0))
        return st, D.life_stats(), D.ctx.lcmap_get(0, B), Ps
    finally:
        H.close(); D.close()


# ---- 1. stage by stage
@pytest.mark.parametrize("invdepth", [False, True])
def test_one_frame_stage_by_stage(built, invdepth):
    """Frames 0..2 of the revisit bring the state to where frame 3 has everything: in filter 0 the four returned points are in
    the state and match the map, in filter 1 one does. Frame 1 (four features leave in filters 0 and 1) and frame 3 (queries,
    a closure, a short frame) are taken stage by stage on the device - begin, add, update, close, end - and held against what
    the host life cycle's backend saw between its calls."""
    cfg_h, cfg_d = _cfgs(invdepth)
    H, D, rh, rd = _open(cfg_h, cfg_d, _Host)
    try:
        H.snap = {}
        for t, (tracks, keys) in enumerate(_frames(_revisit(4), invdepth)):
            H.snap.clear()
            rh.frame(None, tracks, keys)
            if t not in (1, 3):
                rd.frame(None, tracks, keys)
                _same(H, D, rh, "frame %d" % t)
                continue
            before = (D.covariance(), D.scene(), _map(D))
            D.life_begin_keys(*rd._pack_tracks(tracks), rd._pack_keys(tracks, keys))
            # begin decides only: P, the scene's state (the tracked features' pixels aside) and the map are as they were
            assert np.array_equal(D.covariance(), before[0]) and _map(D) == before[2]
            assert np.array_equal(D.scene()[2]["x"], before[1][2]["x"]) and np.array_equal(D.scene()[2]["sind"], before[1][2]["sind"])
            D.lcmap_add_resident()
            if t == 1:
                assert _map(D) == H.snap["add"], "map after add"
                assert np.frombuffer(H.snap["add"]["stats"], dtype=L.lcmap_stats_dtype)["added"].tolist() == [4, 4, 0]
            else:
                assert "add" not in H.snap and _map(D) == before[2]      # nobody leaves: the host makes no call, the device an empty one
            assert np.array_equal(D.covariance(), H.snap["begin"][0]), "P after add"
            _same_scene(D.scene(), H.snap["begin"][1], 0, "scene after add")
            mask = D.update(download=True)
            assert np.array_equal(mask, H.snap["update"][2])
            assert np.array_equal(D.covariance(), H.snap["update"][0]), "P after update"
            _same_scene(D.scene(), H.snap["update"][1], 0, "scene after update")
            n = D.lcmap_close_resident(wait=True)
            assert n == H.snap["close"][3] == (1 if t == 3 else 0)
            assert np.array_equal(D.covariance(), H.snap["close"][0]), "P after close"
            _same_scene(D.scene(), H.snap["close"][1], 0, "scene after close")
            assert _map(D) == H.snap["close"][2], "map after close"
            D.life_end()
            _same(H, D, rh, "frame %d after end" % t, 0 if invdepth else 2)
        st = D.lcmap_stats()
        assert st["closed_frames"].tolist() == [1, 0, 0] and st["short_frames"].tolist() == [0, 1, 0] and st["matched"].tolist() == [4, 1, 0]
    finally:
        H.close(); D.close()


# ---- 2. a scripted revisit
def test_revisit_closes_where_enough_points_return(built):
    st, life, (ent, cnt), _ = _run(_revisit(8))
    assert cnt.tolist() == [4, 4, 0] and st["added"].tolist() == [4, 4, 0]
    assert st["closed_frames"][0] == 5 and st["short_frames"][0] == 0          # frames 3..7: four matches each
    assert st["closed_frames"][1] == 0 and st["short_frames"][1] == 5          # one returning key: fewer than lc_min_matches
    assert all(int(st[k][2]) == 0 for k in st.dtype.names)                     # no tracks at all: untouched
    assert life["updates"][2] == 0 and life["admitted"][2] == 0
    assert sorted(ent[0]["key"][:4].tolist()) == [4, 5, 6, 7]


def test_keys_that_never_repeat_change_nothing(built):
    """the same script with every key its track id: nothing ever matches, and P, the scene and the book of every frame equal,
    bit for bit, a device life cycle's run with loop closure off"""
    script = _revisit(8, new_keys=True)
    st, _, _, Ps = _run(script)
    assert not st["matched"].any() and not st["closed_frames"].any() and st["queries"][:2].all()
    cfg = sequence.SequenceConfig(lifecycle="device", tracks_max=16, **SHAPE, **INV)
    be = sequence.HipBackend(cfg, B, _poses(cfg), np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        r = sequence.SequenceRunner(be, cfg, B)
        for t, (tracks, _) in enumerate(_frames(script, True)):
            r.frame(None, tracks)
            assert np.array_equal(be.covariance(), Ps[t]), t
    finally:
        be.close()


# ---- 3. edges
def test_more_leaving_features_than_free_map_entries(built):
    st, _, (_, cnt), _ = _run(_revisit(5), lc_map_max=2)
    assert st["full"].tolist() == [2, 2, 0] and cnt.tolist() == [2, 2, 0]


def test_two_slots_with_one_key_leave_in_one_frame(built):
    script = _revisit(5)
    for t in range(len(script)):
        script[t][0] = [(i, 4 if (p == 5 and t < 2) else k, p) for i, k, p in script[t][0]]      # points 4 and 5 share key 4 while they are first seen
    st, _, (ent, cnt), _ = _run(script)
    assert st["dup"][0] == 1 and cnt[0] == 3 and ent[0]["key"][:3].tolist() == [4, 6, 7]       # the first kept, in slot order


def test_a_key_of_minus_one_is_skipped(built):
    script = _revisit(5)
    for t in range(len(script)):
        script[t][0] = [(i, -1 if p == 6 else k, p) for i, k, p in script[t][0]]
    st, _, (_, cnt), _ = _run(script)
    assert st["skipped"][0] == 1 and cnt[0] == 3 and st["matched"][0] == 3 * 2


def test_one_leaver_is_poor(built):
    """lc_max_depth_var between the depth variances two leavers of filter 0 have when they leave, read from a run of the host
    life cycle alone (the reference): one is stored, the other counted poor - in both life cycles"""
    script = [_revisit(1)[0]] + _revisit(5)      # (frame 0 twice: the leavers have been through two updates when they leave)
    cfg_h, _ = _cfgs(True)
    poses = _poses(cfg_h)
    poses["Vsb"] = 0.0
    be = sequence.HipBackend(cfg_h, B, poses, np.repeat(cfg_h.P_init()[None], B, axis=0))
    try:
        r = sequence.SequenceRunner(be, cfg_h, B)
        for t, (tracks, keys) in enumerate(_frames(script, True)[:2]):
            r.frame(_push(poses) if t else None, tracks, keys)
        P = be.covariance()[0]
        var = sorted(P[23 + 24 + 3 * j + 2, 23 + 24 + 3 * j + 2] for j in (4, 5, 6, 7))
    finally:
        be.close()
    print("depth variances of the four leavers", var)
    assert var[1] > var[0], var                  # (with the estimate at rest all four keep the variance they entered with)
    st, _, (_, cnt), _ = _run(script, push=True, lc_max_depth_var=float(0.5 * (var[0] + var[1])))
    assert st["poor"][0] == 3 and st["added"][0] == 1 and cnt[0] == 1


def _with_outlier(script, frames, b=0, p=1):
    for t in frames:
        script[t][b] = [x + ("outlier",) if x[2] == p else x for x in script[t][b]]
    return script


def test_a_gate_rejected_feature_never_reaches_the_map(built):
    """point 1 of filter 0 jumps in frame 2: the gate rejects it, life_end frees its slot and its key - no record then, and none
    later: its track goes on and it enters the state again"""
    st, life, (ent, cnt), _ = _run(_with_outlier(_revisit(6), [2]))
    assert life["rejected"][0] >= 1
    assert 1 not in ent[0]["key"][:cnt[0]].tolist() and cnt[0] == 4


def test_a_closure_and_a_rejection_in_one_frame(built):
    """frame 4: filter 0 closes (second update, which rewrites the status) while the gate rejects point 1; `rejected` and
    `not_spd` of xivo_hip_life_stats equal the host's counts (_same, after every frame). life_end counts the status the close
    call kept from the first update."""
    st, life, _, _ = _run(_with_outlier(_revisit(6), [4]))
    assert life["rejected"][0] >= 1 and st["closed_frames"][0] == 3
    print("not_spd", life["not_spd"].tolist())


def test_more_than_64_feature_slots_and_a_surplus(built):
    """n_features = 72 (test_launch_shape_limits' largest layout has 30): filter 0 holds 72 features, twelve of which (slots 60 ..
    71, the second 64-wide chunk of the query kernel) left and came back - twelve matching queries for lc_max = 4: eight surplus"""
    shape = dict(n_groups=4, n_features=72)
    script = _revisit(4, leave=tuple(range(60, 72)), n_pts=72, short_keys=False)
    cfg_h, cfg_d = _cfgs(True, shape=shape, tracks_max=80, lc_map_max=16)
    H, D, rh, rd = _open(cfg_h, cfg_d)
    try:
        for t, (tracks, keys) in enumerate(_frames(script, True)):
            rh.frame(None, tracks, keys); rd.frame(None, tracks, keys)
        _same(H, D, rh, "72 slots")
        st = D.lcmap_stats()
        assert st["queries"][0] == 72 + 60 * 2 and st["surplus"][0] == 8 and st["matched"][0] == 4 and st["added"][0] == 12
        m = D.ctx.lcmap_matches(0, 1)[0]
        assert m["entry"].tolist() == [0, 1, 2, 3]                              # the first four in slot order: slots 60 .. 63
    finally:
        H.close(); D.close()


class _Recording(sequence.HipBackend):
    """the host life cycle's backend, keeping every add record and query it hands down"""

    def lcmap_add(self, recs):
        self.__dict__.setdefault("said", []).append(("A", recs.copy()))
        super().lcmap_add(recs)

    def lcmap_close(self, queries):
        self.__dict__.setdefault("said", []).append(("Q", queries.copy()))
        return super().lcmap_close(queries)


def test_all_72_slots_leave_in_one_frame_and_return(built):
    """the row / count form of the records past 64 entries: n_features = 72, every slot of filters 0 and 1 leaves in frame 1 into
    lc_map_max = 80 - the add kernel's duplicate search takes its second pass from entry 64 on - and returns under its key. Both
    life cycles agree, and the map's keys and counters are those of tests/lcmap_restate.py's MapRestate on the records and
    queries the host life cycle handed down: the comparison is not between two runs of the same kernels only."""
    import lcmap_restate as R
    shape = dict(n_groups=4, n_features=72)
    lc = dict(lc_map_max=80, lc_max=64, lc_min_matches=2)
    script = _revisit(4, leave=tuple(range(72)), n_pts=72, short_keys=False)
    cfg_h, cfg_d = _cfgs(True, shape=shape, tracks_max=80, **lc)
    H, D, rh, rd = _open(cfg_h, cfg_d, host_cls=_Recording)
    try:
        for t, (tracks, keys) in enumerate(_frames(script, True)):
            rh.frame(None, tracks, keys); rd.frame(None, tracks, keys)
            _same(H, D, rh, "72 leave, frame %d" % t)
        want = [R.MapRestate(80, 64, 2) for _ in range(B)]
        for kind, a in getattr(H, "said", []):
            for b in range(B):
                mine = a[a["b"] == b]
                if kind == "A":
                    want[b].add([(int(k), True, False, None) for k in mine["key"]])
                else:
                    want[b].match([int(k) for k in mine["key"]])
        st, (ent, cnt) = D.lcmap_stats(), D.ctx.lcmap_get(0, B)
        print({k: st[k].tolist() for k in ("added", "dup", "full", "queries", "matched", "surplus")})
        assert cnt.tolist() == [72, 72, 0]
        for b in range(B):
            assert ent["key"][b, :cnt[b]].tolist() == want[b].keys, b
            for k in ("added", "dup", "full", "poor", "skipped", "queries", "matched", "surplus"):
                assert st[k][b] == want[b].stats[k], (b, k)
        assert want[0].keys == list(range(72)) and st["added"].tolist() == [72, 72, 0]       # slot order: the key is the point
        assert st["matched"][0] > 0 and st["surplus"][0] > 0                                 # 72 returning keys, 64 list positions
    finally:
        H.close(); D.close()


def test_lc_max_smaller_than_the_matching_queries(built):
    st, _, _, _ = _run(_revisit(5), lc_max=2)
    assert st["surplus"][0] == 2 * 2 and st["matched"][0] == 2 * 2


# ---- 4. the map's two options
def test_both_cov_options(built):
    st, _, _, _ = _run(_revisit(8), lc_point_cov=True, lc_revisit_gap=2)      # (_map compares lcmap_get_cov and lcmap_cov_stats too)
    assert st["closed_frames"][0] >= 1


# ---- 5. waiting against non-waiting close
def test_the_close_call_that_does_not_wait(built):
    """the same script with the waiting close (second update only in a frame some filter closes, and then for all) and the
    non-waiting one (second update in every frame, on neutral rows for who does not close): P, scene, book, map, counters"""
    script = _revisit(6)
    cfg_h, cfg_d = _cfgs(True)
    poses, P0 = _poses(cfg_d), np.repeat(cfg_d.P_init()[None], B, axis=0)
    W, N = sequence.HipBackend(cfg_d, B, poses, P0), None
    try:
        N = sequence.HipBackend(cfg_d, B, poses, P0)
        rw, rn = sequence.SequenceRunner(W, cfg_d, B), sequence.SequenceRunner(N, cfg_d, B)
        rn.lc_wait = False
        for t, (tracks, keys) in enumerate(_frames(script, True)):
            rw.frame(None, tracks, keys); rn.frame(None, tracks, keys)
            dP = np.abs(W.covariance() - N.covariance()).max()
            print("frame %d: max |dP| waiting - non-waiting %.3e" % (t, dP))
            assert np.array_equal(W.covariance(), N.covariance()), t
            for x, y in zip(W.scene(), N.scene()):
                assert x.tobytes() == y.tobytes(), t
            assert _map(W) == _map(N) and W.life_stats().tobytes() == N.life_stats().tobytes(), t
            assert [x.tobytes() for x in W.life_book()] == [x.tobytes() for x in N.life_book()]
        assert W.lcmap_stats()["closed_frames"][0] == 3
    finally:
        W.close()
        if N is not None:
            N.close()


# ---- 7. device tracks
def test_device_tracks_carry_the_point_index(built):
    """track_source="device": the keys pcw_tracks_kernel leaves equal BatchPCW.generate's last_point_index on the same poses;
    frame_world equals the host-track device frame fed those tracks and keys; and frame_resident (non-waiting close) leaves the
    map counters frame_world leaves on the same records, poses and seeds"""
    import pcw_restate as PR
    from test_trajsim_gpu import _backend
    npts, n = 300, 16
    Xs = PR.box_world(2, npts, 8)
    lc = dict(LC, lc_map_max=64, lc_lifecycle="device")
    one, cfg = _backend(2, npts, **lc)
    two, _ = _backend(2, npts, imu=False, **lc)
    three, cfg3 = _backend(2, npts, track_source="host", imu=False, **lc)
    try:
        one.set_world(Xs); two.set_world(Xs)
        r1, r2, r3 = (sequence.SequenceRunner(be, c, 2) for be, c in ((one, cfg), (two, cfg), (three, cfg3)))
        for r in (r1, r2):
            r.noise_px_std, r.noise_seed = 1.0, 21
        world = pcw.BatchPCW(2, npts=npts, Xs=Xs, noise="philox", noise_seed=21)
        K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
        for f in range(6):
            k0, nn = (0, 0) if f == 0 else ((f - 1) * n, n)
            r1.frame_resident(k0, nn, f)
            recs, gsc = one.ctx.trajsim_get(0, 2)
            cnt, ids, meas = one.ctx.pcw_get_tracks(cfg.tracks_max, 0, 2)
            keys = one.ctx.lcmap_life_get_track_keys(cfg.tracks_max, 0, 2)
            off, wids, wmeas = world.generate(gsc[:, :9].reshape(2, 3, 3), gsc[:, 9:], K, cfg.cam["cols"], cfg.cam["rows"], 1.0)
            assert off.tolist() == [0] + np.cumsum(cnt).tolist()
            for b in range(2):
                assert np.array_equal(keys[b, :cnt[b]], world.last_point_index[off[b]:off[b + 1]]) and (keys[b, cnt[b]:] == -1).all()
                assert np.array_equal(ids[b, :cnt[b]], wids[off[b]:off[b + 1]])
            r2.frame_world(recs if nn else None, gsc, f)
            tracks = [(ids[b, :cnt[b]], meas[b, :cnt[b]]) for b in range(2)]
            r3.frame(recs if nn else None, tracks, [keys[b, :cnt[b]] for b in range(2)])
            assert np.array_equal(two.covariance(), three.covariance()), f
            assert _map2(two) == _map2(three), f
            assert [x.tobytes() for x in two.life_book()] == [x.tobytes() for x in three.life_book()]
            assert two.ctx.lcmap_life_get_keys(0, 2).tobytes() == three.ctx.lcmap_life_get_keys(0, 2).tobytes()
            assert one.lcmap_stats().tobytes() == two.lcmap_stats().tobytes(), f
        st = one.lcmap_stats()
        print({k: st[k].tolist() for k in st.dtype.names})
        assert st["queries"].all()
    finally:
        one.close(); two.close(); three.close()


def _map2(be):
    ent, cnt = be.ctx.lcmap_get(0, 2)
    return ent.tobytes(), cnt.tolist(), be.ctx.lcmap_matches(0, 2).tobytes(), be.lcmap_stats().tobytes()


# ---- 8. refusals
def test_refusals_leave_everything_unchanged(built):
    cfg_h, cfg_d = _cfgs(True)
    poses, P0 = _poses(cfg_h), np.repeat(cfg_h.P_init()[None], B, axis=0)
    tracks, keys = _frames(_revisit(1), True)[0]
    # without a life cycle (a map alone), and without a map (a life cycle alone)
    H = sequence.HipBackend(cfg_h, B, poses, P0)
    try:
        P = H.covariance().tobytes()
        with pytest.raises(L.XivoHipError) as e:
            H.ctx.lcmap_life_config(True)
        assert e.value.status == -1 and H.covariance().tobytes() == P and H.ctx.lcmap_get(0, B)[1].tolist() == [0] * B
    finally:
        H.close()
    cfg_l = sequence.SequenceConfig(lifecycle="device", tracks_max=16, **SHAPE, **INV)
    D = sequence.HipBackend(cfg_l, B, poses, P0)
    try:
        r = sequence.SequenceRunner(D, cfg_l, B)
        packed = r._pack_tracks(tracks)
        before = (D.covariance().tobytes(), [x.tobytes() for x in D.life_book()])
        for call in (lambda: D.ctx.lcmap_life_config(True),                                                  # no map
                     lambda: D.ctx.life_begin_keys(D.F, *packed, np.concatenate(keys)),                      # the option is off
                     lambda: D.ctx.lcmap_add_resident(B), lambda: D.ctx.lcmap_close_resident(B)):
            with pytest.raises(L.XivoHipError) as e:
                call()
            assert e.value.status == -1
            assert (D.covariance().tobytes(), [x.tobytes() for x in D.life_book()]) == before
    finally:
        D.close()
    # the option on: inside an open frame, the resident calls before a begin and out of order
    D = sequence.HipBackend(cfg_d, B, poses, P0)
    try:
        r = sequence.SequenceRunner(D, cfg_d, B)
        r.frame(None, tracks, keys)
        state = lambda: (D.covariance().tobytes(), [x.tobytes() for x in D.life_book()], D.ctx.lcmap_life_get_keys(0, B).tobytes(), _map(D))
        before = state()
        for call in (lambda: D.ctx.lcmap_add_resident(B), lambda: D.ctx.lcmap_close_resident(B)):      # no frame is open
            with pytest.raises(L.XivoHipError) as e:
                call()
            assert e.value.status == -1 and state() == before
        D.life_begin_keys(*r._pack_tracks(tracks), r._pack_keys(tracks, keys))
        opened = state()
        for call in (lambda: D.ctx.lcmap_life_config(False), lambda: D.ctx.lcmap_life_config(True),      # a frame is open
                     lambda: D.ctx.lcmap_close_resident(B),                                             # the add call has not run
                     lambda: D.ctx.life_end(B)):                                                        # nor have the removals it makes
            with pytest.raises(L.XivoHipError) as e:
                call()
            assert e.value.status == -1 and state() == opened
        D.lcmap_add_resident()
        with pytest.raises(L.XivoHipError):
            D.ctx.lcmap_add_resident(B)                                                                 # once per frame
        D.update(download=False)
        D.lcmap_close_resident(wait=True)
        with pytest.raises(L.XivoHipError):
            D.ctx.lcmap_close_resident(B)
        D.life_end()
        # the plain begin call with the option on: every track's key is -1
        D.life_begin(*r._pack_tracks(tracks)); D.lcmap_add_resident(); D.update(download=False); D.lcmap_close_resident(wait=True); D.life_end()
        # releasing the map or the life cycle releases the option: the calls are refused again
        D.ctx.lcmap_config(0)
        with pytest.raises(L.XivoHipError):
            D.ctx.lcmap_life_get_keys(0, B)
    finally:
        D.close()


# ---- 9. the command line
def test_run_pcw_cli_reports_the_same_map_counters(built):
    outs = []
    for extra in (["-lifecycle", "host"], ["-lifecycle", "device", "-lc-lifecycle", "device"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_pcw.py"), "-sequences", "4", "-total_time", "1.0",
                            "-loop-closure", "-lc-min-matches", "2"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    h, d = outs
    assert d["lc_lifecycle"] == "device" and h["lc_lifecycle"] == "host"
    lc = {k: v for k, v in h.items() if k.startswith("lcmap_")}
    print(lc)
    assert lc and lc["lcmap_queries"] > 0 and lc == {k: v for k, v in d.items() if k.startswith("lcmap_")}
