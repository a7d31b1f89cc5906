"""GPU: the device-resident feature life cycle (xivo_hip_life_*, lifecycle_kernels.hip) against the host life cycle
(SequenceRunner.frame + xivo_hip_edit_batch / xivo_hip_set_pixels): stage by stage on seeded states, at the launch shape's
limits, and over whole sequences."""
import numpy as np
import pytest

from xivo_amd import pcw, sequence
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu

BIG = 1 << 33      # ids above 2^32


def _state(cfg, B, seed):
    rng = np.random.default_rng(seed)
    sims = [pcw.TrajectorySim("lissajous", seed=seed + b) for b in range(B)]
    poses = sequence.initial_poses(cfg, sims, t0=0.4)
    P0 = []
    for b in range(B):
        A = rng.uniform(-1, 1, size=(cfg.N, cfg.N))
        P = A @ A.T / cfg.N * 1e-3 + 1e-5 * np.eye(cfg.N)
        P0.append(0.5 * (P + P.T))
    return poses, np.array(P0), rng


def _filter(cfg, rng, groups, keep, new, bounds=False, dup=False, big=False, n_tracks=None):
    """one filter's seeded state and frame. groups: features per group slot (-1: free slot); keep: how many of the in-state
    features the tracker still sees; new: tracks that are not in the state. -> (feat_id [F], feat_ref [F], ids, meas)"""
    F = cfg.n_features
    base = BIG if big else 0
    n_in = sum(g for g in groups if g > 0)
    slots = np.sort(rng.choice(F, size=n_in, replace=False))
    feat_id, feat_ref = np.full(F, -1, dtype=np.int64), np.full(F, -1, dtype=np.int32)
    in_ids = base + 1000 + rng.choice(500, size=n_in, replace=False)
    refs = np.concatenate([[g] * c for g, c in enumerate(groups) if c > 0]).astype(np.int32) if n_in else np.zeros(0, np.int32)
    feat_id[slots], feat_ref[slots] = in_ids, rng.permutation(refs)
    new_ids = base + np.concatenate([rng.choice(1000, size=new // 2, replace=False), 1500 + rng.choice(1000, size=new - new // 2, replace=False)])
    ids = np.concatenate([rng.permutation(in_ids)[:keep], new_ids]).astype(np.int64)
    depth = rng.uniform(0.5, 5.0, size=len(ids))
    if bounds and new >= 4:        # exactly on either bound (no candidates), and out of range on either side
        depth[keep:keep + 4] = [cfg.min_depth, cfg.max_depth, 0.01, 12.0]
    order = rng.permutation(len(ids))
    ids, depth = ids[order], depth[order]
    if dup and keep > 0:           # an in-state id a second time, with another pixel: the last occurrence counts
        k = int(np.nonzero(np.isin(ids, in_ids))[0][0])
        ids, depth = np.append(ids, ids[k]), np.append(depth, 1.0)
    if n_tracks is not None:
        assert len(ids) == n_tracks, (len(ids), n_tracks)
    meas = np.column_stack([rng.uniform(0, 640, len(ids)), rng.uniform(0, 480, len(ids)), depth])
    return feat_id, feat_ref, ids, meas


def _scene(cfg, rng, books):
    B = len(books)
    groups = np.zeros((B, cfg.n_groups), dtype=L.group_dtype)
    feats = np.zeros((B, cfg.n_features), dtype=L.feat_dtype)
    feats["sind"] = -1
    for b, (fid, fref) in enumerate(books):
        for g in range(cfg.n_groups):
            groups[b, g]["Rsb"] = pcw.so3_exp(rng.normal(size=3) * 0.3).T.reshape(-1)
            groups[b, g]["Tsb"] = rng.normal(size=3)
        for j in np.nonzero(fid >= 0)[0]:
            feats[b, j]["x"] = [rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), np.log(rng.uniform(1.0, 4.0))]
            feats[b, j]["xp"] = [rng.uniform(0, 640), rng.uniform(0, 480)]
            feats[b, j]["sind"], feats[b, j]["ref_sind"] = j, fref[j]
    return groups, feats


class _Staged(sequence.HipBackend):
    """the product backend that keeps what the resident state looks like between the stages of a frame"""

    def update(self, download=True):
        self.pre = (self.covariance(), self.scene())
        self.mask = super().update(download=True)
        return self.mask


def _ulps(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _same_scene(sa, sb, x2_ulp, tag):
    (pa, ga, fa), (pb, gb, fb) = sa, sb
    assert pa.tobytes() == pb.tobytes(), tag
    assert ga.tobytes() == gb.tobytes(), tag                     # group poses
    for k in ("xp", "sind", "ref_sind"):
        assert np.array_equal(fa[k], fb[k]), (tag, k)
    assert np.array_equal(fa["x"][..., :2], fb["x"][..., :2]), tag
    on = fa["sind"] >= 0
    u = _ulps(fa["x"][..., 2][on], fb["x"][..., 2][on])
    print("%s: x[2] differs by at most %.1f ulp over %d features" % (tag, u.max(initial=0.0), int(on.sum())))
    assert (u <= x2_ulp).all(), (tag, u.max())


def _run_both(cfg_kw, specs, seed, tracks_max=64):
    """the same seeded state and frame through the host life cycle (op lists) and the device life cycle; asserts the stages
    equal and returns the device backend's counters and both books"""
    B = len(specs)
    cfg_h = sequence.SequenceConfig(**cfg_kw)
    cfg_d = sequence.SequenceConfig(lifecycle="device", tracks_max=tracks_max, **cfg_kw)
    poses, P0, rng = _state(cfg_h, B, seed)
    filt = [_filter(cfg_h, rng, **s) for s in specs]
    groups, feats = _scene(cfg_h, rng, [(f[0], f[1]) for f in filt])
    tracks = [(f[2], f[3]) for f in filt]
    A = _Staged(cfg_h, B, poses, P0)
    D = sequence.HipBackend(cfg_d, B, poses, P0)
    try:
        for be in (A, D):
            be.ctx.set_scene(poses, groups, feats)
        ra, rd = sequence.SequenceRunner(A, cfg_h, B), sequence.SequenceRunner(D, cfg_d, B)
        for b, (fid, fref, _, _) in enumerate(filt):
            bk = ra.books[b]
            bk.feat_id, bk.feat_ref = [int(i) for i in fid], [int(r) for r in fref]
            bk.id2slot = {int(i): j for j, i in enumerate(fid) if i >= 0}
            bk.group_refs = [int((fref == g).sum()) if (fref == g).any() else -1 for g in range(cfg_h.n_groups)]
        D.ctx.life_set_book(np.array([f[0] for f in filt]))
        got = D.ctx.life_get_book()
        assert np.array_equal(got[0], [f[0] for f in filt]) and np.array_equal(got[1], [f[1] for f in filt])
        assert got[2].tolist() == [bk.group_refs for bk in ra.books]
        # host: the whole frame (its stages are kept by _Staged); device: stage by stage
        ra.frame(None, tracks)
        off = np.zeros(B + 1, dtype=np.int32); off[1:] = np.cumsum([len(t[0]) for t in tracks])
        D.life_begin(off, np.concatenate([t[0] for t in tracks]), np.concatenate([t[1] for t in tracks]))
        assert np.array_equal(D.covariance(), A.pre[0]), "P after life_begin"
        _same_scene(D.scene(), A.pre[1], 0, "scene after life_begin")
        mask = D.update(download=True)
        assert np.array_equal(mask, A.mask)
        D.life_end()
        assert np.array_equal(D.covariance(), A.covariance()), "P after life_end"
        _same_scene(D.scene(), A.scene(), 0 if cfg_kw.get("use_invdepth") else 2, "scene after life_end")
        books = rd.books
        for b in range(B):
            assert books[b].feat_id == ra.books[b].feat_id and books[b].feat_ref == ra.books[b].feat_ref, b
            assert books[b].group_refs == ra.books[b].group_refs, b
        assert rd.n_updates == ra.n_updates and rd.n_rejected == ra.n_rejected
        return D.life_stats(), ra.books, A.mask
    finally:
        A.close(); D.close()


SIX = [
    dict(groups=[-1, -1, -1, -1], keep=0, new=0),                               # empty state, no tracks at all
    dict(groups=[5, 4, -1, -1], keep=9, new=8, dup=True),                       # all slots full; a duplicated id
    dict(groups=[2, 1, 1, 1], keep=5, new=6),                                   # free slots but no free group
    dict(groups=[4, 4, -1, -1], keep=8, new=5),                                 # 1 free slot < min_new_features, state not empty
    dict(groups=[3, -1, -1, -1], keep=0, new=16, bounds=True, big=True),        # everything dropped; more candidates than slots
    dict(groups=[2, -1, 2, -1], keep=4, new=2),                                 # fewer candidates than slots
]


@pytest.mark.parametrize("invdepth", [False, True])
def test_one_frame_stage_by_stage_bit_for_bit(built, invdepth):
    """n_groups = 4, n_features = 9 (N = 74), six filters that hit the cases of tests/test_lifecycle_cpu.py: after life_begin P
    and the scene equal those after the host's op list and pixels bit for bit, the same update gives the same mask, after
    life_end P, x[0..1], xp, sind, ref_sind, the group poses and the books are equal bit for bit and x[2] = log z to 2 ulp
    (libm and the device library: each within 1 ulp) - bit for bit too in the inverse-depth build"""
    kw = dict(n_groups=4, n_features=9, min_new_features=2)
    if invdepth:
        kw.update(use_invdepth=True, initial_std_z=0.05)
    st, books, mask = _run_both(kw, SIX, seed=5)
    assert st["dropped"].tolist()[4] == 3 and st["admitted"][4] == 9 and st["groups_added"][4] == 1
    assert all(i >= BIG for i in books[4].feat_id)
    assert st["admitted"][0] == 0 and st["admitted"][2] == 0
    assert st["updates"].tolist() == [0, 1, 1, 1, 0, 1]


def test_launch_shape_limits(built):
    """the default layout (N = 203: more columns than the workgroup has threads), a filter with 300 tracks (more than one pass
    of 256 threads), one with exactly tracks_max, one with none; tracks_max + 1 is refused with nothing changed"""
    kw = dict()
    tm = 320
    specs = [dict(groups=[4, 3] + [-1] * 13, keep=5, new=295, bounds=True, n_tracks=300),
             dict(groups=[2, 2, 2] + [-1] * 12, keep=6, new=tm - 6, n_tracks=tm),
             dict(groups=[3, 1] + [-1] * 13, keep=0, new=0, n_tracks=0)]
    st, books, _ = _run_both(kw, specs, seed=9, tracks_max=tm)
    assert st["admitted"][0] > 0 and st["admitted"][1] > 0 and st["dropped"][2] == 4
    # limits of the calls themselves
    cfg = sequence.SequenceConfig(lifecycle="device", tracks_max=tm)
    poses, P0, rng = _state(cfg, 3, 2)
    D = sequence.HipBackend(cfg, 3, poses, P0)
    try:
        P_before, scene_before = D.covariance(), D.scene()
        off = np.array([0, 10, 10 + tm + 1, 10 + tm + 1], dtype=np.int32)
        n = int(off[-1])
        ids, meas = np.arange(n, dtype=np.int64), np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n), np.full(n, 2.0)])
        with pytest.raises(L.XivoHipError) as e:
            D.life_begin(off, ids, meas)
        assert e.value.status == -1
        assert np.array_equal(D.covariance(), P_before)
        for x, y in zip(D.scene(), scene_before):
            assert x.tobytes() == y.tobytes()
        assert (D.ctx.life_get_book()[0] == -1).all()
    finally:
        D.close()
    # a context with a feature pool, and one that is not configured
    cfg_h = sequence.SequenceConfig()
    H = sequence.HipBackend(cfg_h, 3, poses, P0)
    try:
        with pytest.raises(L.XivoHipError) as e:
            H.ctx.life_begin(cfg_h.n_features, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros((0, 3)))
        assert e.value.status == -1
        H.enable_pool()
        with pytest.raises(L.XivoHipError) as e:
            H.ctx.life_config(64)
        assert e.value.status == -1
    finally:
        H.close()
    # beyond the LDS plan
    G = sequence.HipBackend(cfg_h, 3, poses, P0)
    try:
        with pytest.raises(L.XivoHipError) as e:
            G.ctx.life_config(L.LIFE_MAX_TRACKS + 1)
        assert e.value.status == -1
        G.ctx.life_config(L.LIFE_MAX_TRACKS)
        G.ctx.life_config(0)
    finally:
        G.close()


def _sequences(cfg_kw, world0, sim0, B=4):
    mk = lambda: ([pcw.RandomPCW(seed=world0 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=sim0 + b) for b in range(B)])
    w1, s1 = mk()
    host = sequence.run_pcw(sequence.HipBackend, sequence.SequenceConfig(**cfg_kw), w1, s1, total_time=1.0)
    w2, s2 = mk()
    dev = sequence.run_pcw(sequence.HipBackend, sequence.SequenceConfig(lifecycle="device", **cfg_kw), w2, s2, total_time=1.0)
    return host, dev


def _same_run(host, dev, bound):
    try:
        hb, db = host["runner"].books, dev["runner"].books
        for b in range(len(hb)):
            assert db[b].feat_id == hb[b].feat_id and db[b].feat_ref == hb[b].feat_ref and db[b].group_refs == hb[b].group_refs, b
        assert dev["runner"].n_updates == host["runner"].n_updates and dev["runner"].n_rejected == host["runner"].n_rejected
        dT, dW = np.abs(host["Tsb"] - dev["Tsb"]).max(), np.abs(host["Wsb"] - dev["Wsb"]).max()
        print("device vs host life cycle: max |dTsb| %.3e, max |dWsb| %.3e" % (dT, dW))
        if bound == 0:
            assert np.array_equal(host["Tsb"], dev["Tsb"]) and np.array_equal(host["Wsb"], dev["Wsb"])
        else:
            assert dT < bound and dW < bound
        st = dev["backend"].life_stats()
        assert int(st["not_spd"].sum()) == getattr(host["backend"], "n_not_spd", 0)
        return int(host["runner"].n_rejected)
    finally:
        host["backend"].close(); dev["backend"].close()


def test_sequences_defaults(built):
    """whole sequences, device against host life cycle: same books and counters, poses within 1e-9 (the bound between the
    project's two host sides: log z of a new feature may differ in the last place)"""
    _same_run(*_sequences({}, 20, 400), 1e-9)


def test_sequences_under_rejections(built):
    assert _same_run(*_sequences(dict(MH_thresh=0.02), 60, 500), 1e-9) > 50


def test_sequences_invdepth_bit_for_bit(built):
    """all host arithmetic is then - and /: Tsb, Wsb and the books are equal bit for bit"""
    _same_run(*_sequences(dict(use_invdepth=True, initial_std_z=0.05), 60, 500), 0)


def test_sequences_one_point_ransac(built):
    _same_run(*_sequences(dict(use_1pt_RANSAC=True), 20, 400), 1e-9)


def test_cpp_batch_estimator_with_the_device_life_cycle_equals_the_python_runner(built):
    """xivo::hip::BatchEstimator::EnableDeviceLifecycle against SequenceRunner with lifecycle="device": books, counters, Tsb
    within 1e-10 as between the two host sides today"""
    B = 4
    cfg = sequence.SequenceConfig(lifecycle="device")
    mk = lambda: ([pcw.RandomPCW(seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    w1, s1 = mk()
    py = sequence.run_pcw(sequence.HipBackend, cfg, w1, s1, total_time=1.0)
    w2, s2 = mk()
    cp = sequence.run_pcw_cpp(cfg, w2, s2, total_time=1.0)
    try:
        books = py["runner"].books
        for b in range(B):
            fid, fref, gref = cp["estimator"].book(b)
            assert list(fid) == books[b].feat_id and list(fref) == books[b].feat_ref and list(gref) == books[b].group_refs
        st = cp["estimator"].stats()
        assert st["updates"] == py["runner"].n_updates > 0 and st["mh_rejected"] == py["runner"].n_rejected
        assert np.abs(py["Tsb"] - cp["Tsb"]).max() < 1e-10 and np.abs(py["Wsb"] - cp["Wsb"]).max() < 1e-10
    finally:
        py["backend"].close(); cp["estimator"].close()


@pytest.mark.parametrize("extra", [[], ["-vectorized"]])
def test_run_pcw_cli_with_the_device_life_cycle(built, extra):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    reps = {}
    for life in ("host", "device"):
        cmd = [sys.executable, os.path.join(root, "scripts", "run_pcw.py"), "-sequences", "6", "-total_time", "0.6",
               "-lifecycle", life] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        reps[life] = json.loads(out.stdout.strip().splitlines()[-1])
        assert reps[life]["lifecycle"] == life
    assert reps["device"]["ate_m"]["max"] < 0.2
    assert reps["device"]["updates"] == reps["host"]["updates"] > 0


def test_map_log_reads_its_ids_from_the_device_book(built):
    """the landmark log of a run with the device life cycle (one life_get_book read per recorded frame) names the same tracks
    as with the host life cycle, through the Python runner and through the C++ estimator"""
    B = 2
    mk = lambda: ([pcw.RandomPCW(seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    outs = {}
    for life in ("host", "device"):
        w, s = mk()
        outs[life] = sequence.run_pcw(sequence.HipBackend, sequence.SequenceConfig(lifecycle=life), w, s, total_time=0.4, map_log=True)
        outs[life]["backend"].close()
    assert (outs["host"]["map"]["ids"] >= 0).any()
    assert np.array_equal(outs["host"]["map"]["ids"], outs["device"]["map"]["ids"])
    assert np.array_equal(outs["host"]["map"]["n_pts"], outs["device"]["map"]["n_pts"])
    batch = {}
    for life in ("host", "device"):
        batch[life] = sequence.run_pcw_batch(sequence.SequenceConfig(lifecycle=life), 3, total_time=0.4, map_log=True)
        batch[life]["estimator"].close()
    assert (batch["host"]["map"]["ids"] >= 0).any()
    assert np.array_equal(batch["host"]["map"]["ids"], batch["device"]["map"]["ids"])


def test_cpp_estimator_switches_the_device_life_cycle_off_and_on(built):
    """EnableDeviceLifecycle(0) reads books and counters home and goes on with the host life cycle, enabling it again adopts
    the book: a run that switches twice ends like one that never did; EnableSubfilter is refused while it is on"""
    from xivo_amd.batch import BatchEstimator
    B = 3
    cfg = sequence.SequenceConfig()
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    Rbc = pcw.so3_exp(cfg.Wbc)
    res = {}
    for switch in (False, True):
        worlds = [pcw.RandomPCW(seed=20 + b) for b in range(B)]
        sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]
        est = BatchEstimator(cfg, B, sequence.initial_poses(cfg, sims), cfg.P_init())
        try:
            for k in range(200):
                t = k * 0.0025
                m = [s.meas(t) for s in sims]
                est.InertialMeas(t, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
                if k % 16 == 0:
                    if switch and k == 48:
                        est.enable_device_lifecycle(cfg.tracks_max); est.want_mask = False
                        with pytest.raises(RuntimeError):
                            _subfilter(est, cfg)
                    if switch and k == 128:
                        est.enable_device_lifecycle(0); est.want_mask = True
                    tracks = []
                    for b in range(B):
                        Rsb, Tsb = sims[b].gsb(t)
                        tracks.append(worlds[b].generate_measurements(Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb, K, 640, 480, 1.0))
                    est.VisualMeasPointCloud(t, tracks)
            res[switch] = ([tuple(map(tuple, est.book(b))) for b in range(B)], est.stats()["updates"], est.stats()["mh_rejected"],
                           est.poses()["Tsb"].copy())
        finally:
            est.close()
    assert res[True][0] == res[False][0] and res[True][1:3] == res[False][1:3] and res[False][1] > 0
    assert np.abs(res[True][3] - res[False][3]).max() < 1e-9


def _subfilter(est, cfg):
    from xivo_amd import batch
    sc = np.zeros(1, dtype=batch.batch_subfilter_cfg_dtype)
    sc["pool_max"], sc["anchor_max"] = 8, 4
    if est.host.xivo_batch_enable_subfilter(est.h, sc.ctypes.data) != 0:
        raise RuntimeError("xivo_batch_enable_subfilter failed")
