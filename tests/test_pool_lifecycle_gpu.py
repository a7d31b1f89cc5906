"""GPU: the device-resident life cycle of the "subfilter" mode (xivo_hip_pool_life_*, pool_lifecycle_kernels.hip) against the
host life cycle (SequenceRunner._frame_subfilter: xivo_hip_pool_step + op lists + set_pixels + pool_anchor + pool_add): stage by
stage over simulated sequences, at the launch shape's limits, over whole runs, and its refusals. Both arms execute the same
device functions in the same order, so every comparison is for equal bytes."""
import numpy as np
import pytest

from xivo_amd import pcw, sequence
from xivo_amd import lib as L

pytestmark = pytest.mark.gpu

# the sub-filter set-up of tests/test_feature_pool_gpu.py: tracks pass the candidate test within a few frames
QUICK = dict(feature_init="subfilter", initial_z=5.0, initial_std_z=0.5, max_group_lifetime=3,
             subfilter=dict(visual_meas_std=3.5, MH_thresh=8.991, ready_steps=2))


class _Staged(sequence.HipBackend):
    """the product backend that keeps what is resident between the stages of a frame"""

    def snapshot(self):
        ent, ap, sl = self.ctx.pool_get(0, self.B)
        z = self.ctx.pool_get_init_z(0, self.B) if self.cfg.adaptive_initial_depth else np.zeros(0)
        return (self.covariance(),) + tuple(self.scene()) + (ent, ap, sl, z)

    def update(self, download=True):
        self.pre = self.snapshot()
        self.mask = super().update(download=True)
        self.post = self.snapshot()
        return self.mask


NAMES = ("P", "poses", "groups", "feats", "pool entries", "anchor poses", "anchor slots", "init_z")


def _same(a, b, tag):
    for x, y, name in zip(a, b, NAMES):
        assert x.tobytes() == y.tobytes(), (tag, name)


def _same_books(host, D, tag):
    """the host runner's books against the device's (the entries' anchors and the anchors' links are the resident ones)"""
    bk = D.pool_life_book()
    ent, _, slots = D.ctx.pool_get(0, D.B)
    for b in range(D.B):
        hb, hp = host.books[b], host.pools[b]
        assert bk["feat_id"][b].tolist() == hb.feat_id and bk["feat_ref"][b].tolist() == hb.feat_ref, (tag, b)
        assert bk["group_refs"][b].tolist() == hb.group_refs, (tag, b)
        assert bk["ent_id"][b].tolist() == hp.ent_id, (tag, b)
        held = bk["ent_id"][b] >= 0
        assert np.array_equal(np.where(held, ent["ref_sind"][b], -1), hp.ent_anchor), (tag, b)
        assert np.array_equal(bk["ent_born"][b][held], np.array(hp.ent_born)[held]), (tag, b)
        assert bk["anc_used"][b].astype(bool).tolist() == [bool(u) for u in hp.anc_used], (tag, b)
        used = bk["anc_used"][b] > 0
        assert np.array_equal(bk["anc_life"][b][used], np.array(hp.anc_life)[used]), (tag, b)
        assert np.array_equal(np.where(used, slots[b], -1), np.where(used, hp.anc_link, -1)), (tag, b)


def _same_counters(host, st, tag):
    assert int(st["updates"].sum()) == host.n_updates and int(st["rejected"].sum()) == host.n_rejected, tag
    assert int(st["pool_dropped"].sum()) == host.n_pool_dropped and int(st["admitted"].sum()) == len(host.admitted), tag
    assert int(st["admit_steps"].sum()) == sum(a[3] for a in host.admitted), tag


def _lockstep(cfg_kw, frames_of, B, n_frames, tracks_max=256, seed=0, host_tracks=None):
    """the same frames through the host life cycle (whole frames, its stages kept by _Staged) and the device life cycle stage by
    stage; frames_of(t) -> (imu records or None, tracks). host_tracks(t, tracks) (default: the same tracks): what the host
    life cycle gets of the frame. Returns (host runner, device counters)."""
    cfg_h = sequence.SequenceConfig(**cfg_kw)
    cfg_d = sequence.SequenceConfig(pool_lifecycle="device", tracks_max=tracks_max, **cfg_kw)
    sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + seed + b) for b in range(B)]
    poses0 = sequence.initial_poses(cfg_h, sims)
    P0 = np.repeat(cfg_h.P_init()[None], B, axis=0)
    A, D = _Staged(cfg_h, B, poses0, P0), sequence.HipBackend(cfg_d, B, poses0, P0)
    try:
        ra, rd = sequence.SequenceRunner(A, cfg_h, B), sequence.SequenceRunner(D, cfg_d, B)
        for t in range(n_frames):
            rec, tracks = frames_of(t, sims)
            ra.frame(rec, tracks if host_tracks is None else host_tracks(t, tracks))
            if rec is not None:
                D.propagate(rec)
            off, ids, meas = rd._pack_tracks(tracks)
            D.pool_life_begin(off, ids, meas, t + 1 >= cfg_d.strict_criteria_timesteps)
            tag = "frame %d" % t
            _same(_Staged.snapshot(D), A.pre, tag + " after begin")
            mask = D.update(download=True)
            assert np.array_equal(mask, A.mask), tag
            _same(_Staged.snapshot(D), A.post, tag + " after the update")
            D.pool_life_end()
            _same(_Staged.snapshot(D), A.snapshot(), tag + " after end")
            _same_books(ra, D, tag)
            _same_counters(ra, D.pool_life_stats(), tag)
        return ra, D.pool_life_stats()
    finally:
        A.close(); D.close()


def _sim_frames(cfg, B, npts, seed=20):
    """frames of the point-cloud simulator: the IMU records since the last frame and the tracks of B small worlds"""
    worlds = [pcw.RandomPCW(npts=npts, seed=seed + b) for b in range(B)]
    K = np.array([[cfg.cam["fx"], 0, cfg.cam["cx"]], [0, cfg.cam["fy"], cfg.cam["cy"]], [0, 0, 1.0]])
    Rbc = pcw.so3_exp(cfg.Wbc)
    state = {}

    def frames_of(t, sims):
        if t == 0:
            m0 = [s.meas(0.0) for s in sims]
            state["feeder"] = sequence.ImuFeeder(B, 0.0, [m[1] for m in m0], [m[0] for m in m0])
        feeder = state["feeder"]
        for k in range(16 * t - 15 if t else 0, 16 * t + 1):
            if k > 0:
                m = [s.meas(k * 0.0025) for s in sims]
                feeder.imu(k * 0.0025, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
        tt = 16 * t * 0.0025
        feeder.visual(tt)
        tracks = []
        for b in range(B):
            Rsb, Tsb = sims[b].gsb(tt)
            tracks.append(worlds[b].generate_measurements(Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb, K, cfg.cam["cols"], cfg.cam["rows"], 1.0))
        return feeder.take(), tracks
    return frames_of


@pytest.mark.parametrize("extra", [dict(triangulate_pre_subfilter=True), dict(use_invdepth=True, adaptive_initial_depth=True),
                                   dict(adaptive_initial_depth=True, triangulate_pre_subfilter=True, MH_thresh=0.3),
                                   dict(use_invdepth=True, MH_thresh=0.3)],
                         ids=["log-tri", "invdepth-adaptive", "log-adaptive-tri-tight", "invdepth-tight"])
def test_stage_by_stage_bit_for_bit(built, extra):
    """B = 3 sequences of 24 frames over worlds of 400 points with small tables (9 feature slots, 4 group slots, 24 pool entries,
    4 anchors: every table fills): after begin, after the update and after end P, the scene, the pool entries, the anchors'
    poses and slots and init_z are byte-equal to the op-list path's, and so are the books and the counters; two of the four
    runs under a tight gate, whose rejections empty groups under live pool entries"""
    kw = dict(dict(QUICK, n_groups=4, n_features=9, pool_max=24, anchor_max=4, MH_thresh=1.5), **extra)
    cfg = sequence.SequenceConfig(**kw)
    ra, st = _lockstep(kw, _sim_frames(cfg, 3, 400), 3, 24, tracks_max=400)
    print("admitted %d, rejected %d, pool-dropped %d, outliers %d, anchors created / freed %d / %d" % (
        st["admitted"].sum(), st["rejected"].sum(), st["pool_dropped"].sum(), st["pool_outliers"].sum(),
        st["anchors_created"].sum(), st["anchors_freed"].sum()))
    # the run reaches what it is for
    assert st["admitted"].sum() > 10 and st["pool_dropped"].sum() > 0 and (st["groups_added"] > 0).all()
    assert st["anchors_created"].sum() > 4 and st["pool_added"].sum() > 30


def _synthetic_frames(counts_of, pool_max, seed):
    """frames without a simulator, for the launch shapes: filter b brings counts_of(t)[b] tracks whose ids drift by three per
    frame (three leave, three are new) at pixels that move a little per frame; in frame 1 the lowest id - which has sat in the
    pool since frame 0 - comes twice, and the last occurrence supplies the pixel"""
    rng = np.random.default_rng(seed)

    def frames_of(t, sims):
        tracks = []
        for b, n in enumerate(counts_of(t)):
            ids = (1 << 33) * (b % 2) + 3 * t + np.arange(n, dtype=np.int64)       # ids above 2^32 in every other filter
            if t == 1 and n >= 5 and pool_max >= 5 and counts_of(0)[b] >= 5:
                ids[-1] = ids[0]
            px = np.column_stack([(ids * 37 % 600) + 20.0 + 0.3 * t, (ids * 91 % 440) + 20.0 - 0.2 * t])
            tracks.append((ids, np.column_stack([px + rng.normal(size=px.shape) * 0.2, np.full(n, 2.0)])))
        return None, tracks
    return frames_of


SHAPES = [
    # (B, pool_max, anchor_max, tracks per filter by frame, tracks_max)
    (1, 1, 1, lambda t: [1], 4),
    (3, 63, L.POOL_LIFE_MAX_ANCHORS, lambda t: [0, 255, 63], 255),
    (3, 64, 3, lambda t: [256, 1, 257], 257),
    (2, 65, 2, lambda t: [0, L.LIFE_MAX_TRACKS], L.LIFE_MAX_TRACKS),              # a filter with no track next to a full one
    (70, L.POOL_MAX_ENTRIES, 2, lambda t: [(7 * b + 3 * t) % 41 for b in range(70)], 64),
    (2, L.POOL_MAX_ENTRIES, 3, lambda t: [700, 513], 700),                         # more new tracks than the largest pool holds
]


def test_repeated_ids_through_the_parallel_rules(built):
    """what tests/test_pool_lifecycle_cpu.py checks through the serial forms, through the kernels' parallel ones, with more
    tracks than the workgroup has threads (347 and more) and the occurrences of an id in different passes of 256. From frame 1
    on every one of twenty always-tracked ids comes twice, the second time at the tail with another pixel: some of them sit in
    feature slots by then and the others in pool entries, and the last occurrence supplies the pixel (the LDS maxima of the
    begin kernel). In frames 0 and 2 brand-new ids come three times and twice: only the first occurrence takes part (the
    first-occurrence pass of the end kernel) - the host life cycle, which has no rule for such a frame, gets it without the
    later occurrences. No gating and no outlier removal, so that a repeated held id never turns into a new track."""
    B = 2
    kw = dict(QUICK, n_groups=4, n_features=9, pool_max=64, anchor_max=8, use_MH_gating=False, remove_outlier_counter=1e9)
    steady = np.arange(1000, 1020, dtype=np.int64)
    filler = np.arange(3000, 3300, dtype=np.int64)
    new_twice = {0: [(2000, 3), (2001, 2)], 2: [(2020, 2), (2021, 3)]}     # frame -> (brand-new id, occurrences)

    def px(ids, shift):
        return np.column_stack([(ids * 37 % 600) + 20.0 + shift, (ids * 91 % 440) + 20.0 - shift, np.full(len(ids), 2.0)])

    def frames_of(t, sims):
        tracks = []
        for b in range(B):
            fresh = np.arange(2000 + 10 * t, 2000 + 10 * t + 5, dtype=np.int64)
            earlier = np.concatenate([np.arange(2000 + 10 * q, 2000 + 10 * q + 5, dtype=np.int64) for q in range(t)] + [fresh])
            ids = np.concatenate([steady, earlier[:3], filler[:270], earlier[3:], filler[270:]])
            meas = px(ids, 0.0)
            tail = [np.full(c - 1, i, dtype=np.int64) for i, c in new_twice.get(t, [])] + ([steady] if t >= 1 else [])
            tail = np.concatenate(tail) if tail else np.zeros(0, dtype=np.int64)
            ids, meas = np.concatenate([ids, tail]), np.concatenate([meas, px(tail, 1.5)])
            assert len(ids) > 256 and (np.nonzero(ids == 2000)[0].max() > 256 if t == 0 else True)
            tracks.append((ids + (1 << 33) * b, meas))
        return None, tracks

    def host_tracks(t, tracks):
        out = []
        for b, (ids, meas) in enumerate(tracks):
            keep = np.ones(len(ids), dtype=bool)
            for i, _ in new_twice.get(t, []):
                keep[np.nonzero(ids == i + (1 << 33) * b)[0][1:]] = False
            out.append((ids[keep], meas[keep]))
        return out
    ra, st = _lockstep(kw, frames_of, B, 5, tracks_max=512, host_tracks=host_tracks)
    for b in range(B):
        held_state = set(ra.books[b].feat_id) & set((steady + (1 << 33) * b).tolist())
        held_pool = set(ra.pools[b].ent_id) & set((steady + (1 << 33) * b).tolist())
        assert held_state and held_pool and len(held_state | held_pool) == len(steady), b    # repeated ids in both places
        assert 2000 + (1 << 33) * b in set(ra.books[b].feat_id) | set(ra.pools[b].ent_id), b   # the thrice-seen id was taken once
    assert st["rejected"].sum() == 0 and st["pool_outliers"].sum() == 0 and st["pool_dropped"].sum() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=["pool1", "pool63-anchorcap", "pool64", "pool65-trackcap", "B70-poolcap", "poolcap-full"])
def test_launch_shape_limits(built, shape):
    """four frames at the limits of the launch shapes, device against host stage by stage: pool_max 1 / 63 / 64 / 65 / the cap,
    anchor_max 1 / the cap, 0 / 1 / 255 / 256 / 257 / XIVO_LIFE_MAX_TRACKS tracks per filter, B = 1 and B = 70"""
    B, pm, am, counts, tm = shape
    kw = dict(QUICK, n_groups=4, n_features=9, pool_max=pm, anchor_max=am)
    ra, st = _lockstep(kw, _synthetic_frames(counts, pm, 3), B, 4, tracks_max=tm)
    n0 = counts(0)
    assert st["pool_added"].sum() >= sum(min(n, pm) for n in n0)
    if max(n0) > pm:
        assert st["pool_dropped"].sum() > 0


def _runs(cfg_kw, B=4, total_time=1.2, npts=300):
    mk = lambda: ([pcw.RandomPCW(npts=npts, seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    w1, s1 = mk()
    host = sequence.run_pcw(sequence.HipBackend, sequence.SequenceConfig(**cfg_kw), w1, s1, total_time=total_time)
    w2, s2 = mk()
    dev = sequence.run_pcw(sequence.HipBackend, sequence.SequenceConfig(pool_lifecycle="device", tracks_max=npts, **cfg_kw), w2, s2,
                           total_time=total_time)
    return host, dev


def _same_run(host, dev):
    try:
        assert np.array_equal(host["Tsb"], dev["Tsb"]) and np.array_equal(host["Wsb"], dev["Wsb"])
        _same_books(host["runner"], dev["backend"], "end of the run")
        st = dev["backend"].pool_life_stats()
        _same_counters(host["runner"], st, "end of the run")
        assert int(st["not_spd"].sum()) == getattr(host["backend"], "n_not_spd", 0)
        assert np.array_equal(host["backend"].covariance(), dev["backend"].covariance())
        r = dev["runner"]
        assert (r.n_updates, r.n_rejected, r.n_pool_dropped) == (host["runner"].n_updates, host["runner"].n_rejected, host["runner"].n_pool_dropped)
        assert [bk.feat_id for bk in r.books] == [bk.feat_id for bk in host["runner"].books]
        return st
    finally:
        host["backend"].close(); dev["backend"].close()


SEQ = dict(QUICK, pool_max=64, anchor_max=16)


@pytest.mark.parametrize("extra", [dict(), dict(MH_thresh=0.02), dict(use_invdepth=True),
                                   dict(cam=dict(model=L.CAM_EQUI, rows=480, cols=640, fx=275.0, fy=275.0, cx=320.0, cy=240.0,
                                                 d=[0.01, -0.005, 0.002, -0.001]))],
                         ids=["defaults", "tight-gate", "invdepth", "equidistant"])
def test_sequences_equal_the_host_life_cycle(built, extra):
    """run_pcw, B = 4, 30 frames, worlds of 300 points: trajectories, P, books and counters are equal"""
    st = _same_run(*_runs(dict(SEQ, **extra)))
    assert st["admitted"].sum() > 0 and st["updates"].sum() > 0
    if "MH_thresh" in extra:
        assert st["rejected"].sum() > 20


def test_cpp_batch_estimator_equals_the_python_runner(built):
    """xivo::hip::BatchEstimator::EnableDevicePoolLifecycle against SequenceRunner with pool_lifecycle="device": books,
    counters, and Tsb within 1e-10 as between the two host sides in the host life cycle (the initial std is divided by the
    focal length on each host: hypot vs sqrt)"""
    B = 4
    cfg = sequence.SequenceConfig(pool_lifecycle="device", tracks_max=300, **SEQ)
    mk = lambda: ([pcw.RandomPCW(npts=300, seed=20 + b) for b in range(B)],
                  [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)])
    w1, s1 = mk()
    py = sequence.run_pcw(sequence.HipBackend, cfg, w1, s1, total_time=1.2)
    w2, s2 = mk()
    cp = sequence.run_pcw_cpp(cfg, w2, s2, total_time=1.2)
    try:
        assert cp["estimator"].device_pool_lifecycle
        books = py["runner"].books
        for b in range(B):
            fid, fref, gref = cp["estimator"].book(b)
            assert list(fid) == books[b].feat_id and list(fref) == books[b].feat_ref and list(gref) == books[b].group_refs
        st, ps = cp["estimator"].stats(), py["backend"].pool_life_stats()
        assert st["updates"] == py["runner"].n_updates > 0 and st["mh_rejected"] == py["runner"].n_rejected
        assert st["admitted"] == int(ps["admitted"].sum()) > 0 and st["pool_dropped"] == py["runner"].n_pool_dropped
        assert np.abs(py["Tsb"] - cp["Tsb"]).max() < 1e-10 and np.abs(py["Wsb"] - cp["Wsb"]).max() < 1e-10
    finally:
        py["backend"].close(); cp["estimator"].close()


def test_cpp_estimator_refuses_the_wrong_order(built):
    """EnableDevicePoolLifecycle throws before EnableSubfilter and next to the immediate device life cycle; EnableSubfilter
    still throws while the immediate device life cycle is on"""
    from xivo_amd.batch import BatchEstimator
    cfg = sequence.SequenceConfig()
    sims = [pcw.TrajectorySim("lissajous", seed=1)]
    est = BatchEstimator(cfg, 1, sequence.initial_poses(cfg, sims), cfg.P_init())
    try:
        with pytest.raises(RuntimeError):
            est.enable_device_pool_lifecycle(64)
        est.enable_device_lifecycle(64)
        with pytest.raises(RuntimeError):
            est.enable_device_pool_lifecycle(64)
    finally:
        est.close()


@pytest.mark.parametrize("extra", [[], ["-vectorized"]])
def test_run_pcw_cli_with_the_device_pool_life_cycle(built, extra):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    reps = {}
    for life in ("host", "device"):
        cmd = [sys.executable, os.path.join(root, "scripts", "run_pcw.py"), "-sequences", "4", "-total_time", "0.6", "-npts", "300",
               "-feature_init", "subfilter", "-pool-lifecycle", life] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        reps[life] = json.loads(out.stdout.strip().splitlines()[-1])
        assert reps[life]["pool_lifecycle"] == life and reps[life]["feature_init"] == "subfilter"
    assert reps["device"]["updates"] == reps["host"]["updates"] and reps["device"]["mh_rejected"] == reps["host"]["mh_rejected"]
    assert reps["device"]["ate_m"] == reps["host"]["ate_m"]
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "run_pcw.py"), "-pool-lifecycle", "device"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "subfilter" in out.stderr      # refused before anything runs


# device blocks of xivo_hip_pool_life_config: the two books (2 + 4), the counters, slot_track / ent_track, the step's xp / order /
# n / live, the track block
CONFIG_BLOCKS = 14


def _one_frame(D, t, n=12):
    ids = np.arange(100 + t, 100 + t + n, dtype=np.int64)
    meas = np.column_stack([(ids * 37 % 600) + 20.0, (ids * 91 % 440) + 20.0, np.full(n, 2.0)])
    return np.array([0, n], dtype=np.int32), ids, meas


def test_refusals_leave_everything_as_it_was(built):
    """while the pool life cycle is configured the host pool calls and the two pool ops are refused, and so are a filter above
    tracks_max, begin twice and a config over a non-empty pool - each with P and the pool unchanged; the configuration's
    blocks are gone after release"""
    kw = dict(QUICK, n_groups=4, n_features=9, pool_max=16, anchor_max=4)
    cfg = sequence.SequenceConfig(pool_lifecycle="device", tracks_max=16, **kw)
    sims = [pcw.TrajectorySim("lissajous", seed=3)]
    poses0, P0 = sequence.initial_poses(cfg, sims), cfg.P_init()[None]
    H = sequence.HipBackend(sequence.SequenceConfig(**kw), 1, poses0, P0)
    live0, _ = H.ctx.ctx_allocs()
    H.close()
    D = sequence.HipBackend(cfg, 1, poses0, P0)
    try:
        ctx = D.ctx
        assert ctx.ctx_allocs()[0] >= live0 + CONFIG_BLOCKS
        for t in range(2):
            D.pool_life_begin(*_one_frame(D, t), False)
            D.update(download=False)
            D.pool_life_end()
        state = lambda: (D.covariance().tobytes(),) + tuple(x.tobytes() for x in ctx.pool_get(0, 1)) + tuple(
            v.tobytes() for v in D.pool_life_book().values())
        before = state()
        bk = D.pool_life_book()                # (nine of the first frame's tracks are in the state by now, the others wait)
        assert (bk["ent_id"] >= 0).sum() > 0 and (bk["feat_id"] >= 0).sum() > 0

        def refused(call, status=-1):
            with pytest.raises(L.XivoHipError) as e:
                call()
            assert e.value.status == status and state() == before
        rec = np.zeros(1, dtype=L.pool_new_dtype)
        rec["entry"], rec["anchor"], rec["xp"], rec["z0"], rec["std_xyz"] = 15, 0, [100.0, 100.0], 2.0, [0.1, 0.1, 0.1]
        refused(lambda: ctx.pool_anchor(np.array([3], dtype=np.int32)))
        refused(lambda: ctx.pool_add(rec))
        refused(lambda: ctx.pool_add_ex(rec, 0))
        refused(lambda: ctx.pool_step(np.full((1, 16, 2), np.nan), False))
        refused(lambda: ctx.edit_batch(9, np.array([sequence._op(0, L.EDIT_ADD_GROUP_ANCHOR, 0, 0)], dtype=L.edit_dtype)))
        refused(lambda: ctx.edit_batch(9, np.array([sequence._op(0, L.EDIT_ADMIT_POOL, 0, 0, 0)], dtype=L.edit_dtype)))
        off = np.array([0, 17], dtype=np.int32)
        ids17 = np.arange(17, dtype=np.int64)
        refused(lambda: ctx.pool_life_begin(9, off, ids17, np.zeros((17, 3))))                     # above tracks_max
        refused(lambda: ctx.pool_life_begin(9, np.array([1, 3], dtype=np.int32), ids17[:3], np.zeros((3, 3))))   # malformed off
        refused(lambda: ctx.pool_life_end(1))                                                      # no frame open
        refused(lambda: ctx.pool_life_config(16))                                                  # configured already
        refused(lambda: ctx.life_config(16))                                                       # a context with a pool
        D.pool_life_begin(*_one_frame(D, 2), False)
        before = state()                                                                           # (the frame is open)
        refused(lambda: D.pool_life_begin(*_one_frame(D, 2), False))                               # begin twice
        D.update(download=False)
        D.pool_life_end()
        # beyond the LDS plan, and the pool's reads that keep working
        before = state()
        refused(lambda: ctx.pool_life_config(L.LIFE_MAX_TRACKS + 1))
        ctx.pool_tri_counts()
        resident = lambda: (D.covariance().tobytes(),) + tuple(x.tobytes() for x in ctx.pool_get(0, 1))
        before = resident()
        # release: the blocks are gone, the host calls work again, and a config over the non-empty pool is refused
        live_on = ctx.ctx_allocs()[0]          # (the frames above made the context allocate its update buffers)
        ctx.pool_life_config(0)
        assert ctx.ctx_allocs()[0] == live_on - CONFIG_BLOCKS
        assert resident() == before                                                                # release changes nothing resident
        with pytest.raises(L.XivoHipError) as e:                                                   # config over a non-empty pool
            ctx.pool_life_config(16)
        assert e.value.status == -1 and resident() == before
        assert ctx.ctx_allocs()[0] == live_on - CONFIG_BLOCKS                                      # and it allocated nothing
        ctx.pool_step(np.full((1, 16, 2), np.nan), False)
    finally:
        D.close()
    # more anchors than the LDS plan holds
    big = sequence.SequenceConfig(pool_lifecycle="device", **dict(kw, anchor_max=L.POOL_LIFE_MAX_ANCHORS + 1))
    with pytest.raises(L.XivoHipError) as e:
        sequence.HipBackend(big, 1, poses0, P0)
    assert e.value.status == -5


def test_release_hands_the_life_cycle_back_to_the_host(built):
    """ten frames on the device, release, then ten frames of the host life cycle on the books read back: the end state equals
    a run of twenty host frames that never switched"""
    kw = dict(QUICK, n_groups=4, n_features=9, pool_max=24, anchor_max=4)
    B = 2
    cfg_h = sequence.SequenceConfig(**kw)
    cfg_d = sequence.SequenceConfig(pool_lifecycle="device", tracks_max=256, **kw)
    sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]
    poses0, P0 = sequence.initial_poses(cfg_h, sims), np.repeat(cfg_h.P_init()[None], B, axis=0)
    frames_of = _sim_frames(cfg_h, B, 300)
    A, D = sequence.HipBackend(cfg_h, B, poses0, P0), sequence.HipBackend(cfg_d, B, poses0, P0)
    try:
        ra, rd = sequence.SequenceRunner(A, cfg_h, B), sequence.SequenceRunner(D, cfg_d, B)
        def same_state():
            assert np.array_equal(A.covariance(), D.covariance())
            for x, y in zip(A.scene() + A.ctx.pool_get(0, B), D.scene() + D.ctx.pool_get(0, B)):
                assert x.tobytes() == y.tobytes()
        for t in range(10):
            rec, tracks = frames_of(t, sims)
            ra.frame(rec, tracks); rd.frame(rec, tracks)
        same_state()
        # the books come home, then the device life cycle is released
        bk = D.pool_life_book()
        ent, _, slots = D.ctx.pool_get(0, B)
        D.ctx.pool_life_config(0)
        rh = sequence.SequenceRunner(D, cfg_h, B)
        rh.vision_counter = rd.vision_counter
        rh.pools = [sequence._PoolBook(cfg_h.pool_max, cfg_h.anchor_max) for _ in range(B)]
        for b in range(B):
            hb, hp = rh.books[b], rh.pools[b]
            hb.feat_id, hb.feat_ref, hb.group_refs = bk["feat_id"][b].tolist(), bk["feat_ref"][b].tolist(), bk["group_refs"][b].tolist()
            hb.id2slot = {i: j for j, i in enumerate(hb.feat_id) if i >= 0}
            hp.ent_id = bk["ent_id"][b].tolist()
            hp.ent_anchor = np.where(bk["ent_id"][b] >= 0, ent["ref_sind"][b], -1).tolist()
            hp.ent_born = bk["ent_born"][b].tolist()
            hp.id2ent = {i: e for e, i in enumerate(hp.ent_id) if i >= 0}
            hp.anc_used = [bool(u) for u in bk["anc_used"][b]]
            hp.anc_life = bk["anc_life"][b].tolist()
            hp.anc_link = np.where(bk["anc_used"][b] > 0, slots[b], -1).tolist()
        for t in range(10, 20):
            rec, tracks = frames_of(t, sims)
            ra.frame(rec, tracks); rh.frame(rec, tracks)
        same_state()
        assert [b_.feat_id for b_ in ra.books] == [b_.feat_id for b_ in rh.books]
        assert [p.ent_id for p in ra.pools] == [p.ent_id for p in rh.pools]
        assert len(ra.admitted) > 0
    finally:
        A.close(); D.close()
