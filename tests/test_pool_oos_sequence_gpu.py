"""GPU: sequences with use_oos on both pool life cycles - the host's (SequenceRunner._frame_subfilter ->
xivo_hip_pool_oos_collect) and the device's (xivo_hip_pool_life_begin / _end select and record themselves) -, which must leave
the same bytes: list, P, scene, pool, observation rings, counters.

The point-cloud simulator alone never fires the selection in a short run: a new anchor is linked to a group slot only once one of
its own tracks enters the state, which takes the sub-filter's warm-up, while the ring of an entry keeps its LAST observations -
the ones from the youngest anchors. So the 12 frames here are scripted on top of the simulator's tracks, B = 4: of the tracks
visible in frame 0, five are shown from frame 0 on, three more from frame 3 and three from frame 6 (each batch creates one anchor
and, once admitted, links it), and two "bystanders" are shown from frame 0 with pixels 40 px off in every later frame - their
sub-filter counts them as outliers, so they never become candidates, stay in the pool and are observed by all three anchors.
Their tracks end in frame 10: READY, three observations, anchors linked by then - used."""
import numpy as np
import pytest

from helpers import rel_fro
from test_pool_lifecycle_gpu import QUICK, _sim_frames
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu
B, N_FRAMES, DROP_AT = 4, 12, 10
SHAPE = dict(n_groups=4, n_features=12, pool_max=16, anchor_max=6, remove_outlier_counter=1e9)
OOS = dict(use_oos=True, oos_max=2, oos_max_obs=3, oos_min_observations=2)


def _script(tracks0, cfg):
    """per filter: {track id: first frame it is shown in} and the bystanders' ids, from the central tracks of frame 0"""
    shown, by = [], []
    for ids, meas in tracks0:
        c = [int(i) for i, m in sorted(zip(ids, meas), key=lambda t: t[0])
             if abs(m[0] - cfg.cam["cx"]) < 160 and abs(m[1] - cfg.cam["cy"]) < 120]
        assert len(c) >= 13
        shown.append({**{i: 0 for i in c[:7]}, **{i: 3 for i in c[7:10]}, **{i: 6 for i in c[10:13]}})
        by.append(c[5:7])
    return shown, by


def _run(cfg_kw, device=False):
    cfg = sequence.SequenceConfig(**QUICK, **SHAPE, **cfg_kw, **(dict(pool_lifecycle="device", tracks_max=300) if device else {}))
    sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]
    frames_of = _sim_frames(cfg, B, 300)
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    out = dict(P=[], poses=[], stats=None)
    try:
        runner = sequence.SequenceRunner(be, cfg, B)
        for t in range(N_FRAMES):
            rec, tracks = frames_of(t, sims)
            if t == 0:
                shown, by = _script(tracks, cfg)
            ft = []
            for b, (ids, meas) in enumerate(tracks):
                keep = [k for k, i in enumerate(ids)
                        if shown[b].get(int(i), 1 << 30) <= t and not (t >= DROP_AT and int(i) in by[b])]
                m = np.array(meas, dtype=float)[keep]
                for r, k in enumerate(keep):
                    if t > 0 and int(ids[k]) in by[b]:
                        m[r, :2] += 40.0 if t % 2 else -40.0
                ft.append((np.array(ids)[keep], m))
            runner.frame(rec, ft)
            out["P"].append(be.covariance()); out["poses"].append(be.scene()[0])
            if cfg.use_oos and t == DROP_AT:
                out["list"], out["gamma"] = be.ctx.pool_oos_get(0, B)
        out["pools"], out["books"], out["bystanders"] = runner.pools, runner.books, by
        out["pool"] = be.ctx.pool_get(0, B)
        out["scene"] = be.scene()
        if cfg.use_oos:
            out["stats"] = be.oos_stats()
            if device:
                out["rings"] = be.ctx.pool_oos_get_rings(0, B)
                out["book"] = be.pool_life_book()
    finally:
        be.close()
    return out


@pytest.fixture(scope="module")
def runs(built):
    return _run({}), _run(OOS)


def test_dropped_bystanders_are_used_once(runs):
    off, on = runs
    st = on["stats"]
    print({k: st[k].tolist() for k in st.dtype.names}, on["list"]["n_obs"].tolist(), on["gamma"].round(2).tolist())
    assert int(st["oos_used"].sum()) > 0
    assert (st["oos_used"] + st["oos_short"] <= 2).all()          # the two bystanders of every filter: nothing else is dropped
    assert (st["oos_gated"] <= st["oos_used"]).all() and not st["oos_surplus"].any()
    assert ((on["list"]["n_obs"] >= 2).sum(axis=1) == st["oos_used"]).all()
    for b in range(B):      # a used entry is freed as before
        assert not set(on["bystanders"][b]) & set(on["pools"][b].id2ent)


def test_empty_block_rows_change_nothing_before_the_drop(runs):
    """until a feature is used the block holds H = 0, inn = 0 rows only: P+ is the same update with more rows (other kernels, so
    not bit for bit: the bound is fp64 round-off over the frames, P is ~1e-3 .. 1)"""
    off, on = runs
    for t in range(DROP_AT):
        for b in range(B):
            assert rel_fro(on["P"][t][b], off["P"][t][b]) < 1e-9, (t, b)
            assert np.abs(on["poses"][t][b]["Tsb"] - off["poses"][t][b]["Tsb"]).max() < 1e-9, (t, b)


def _same_state(a, b, tag):
    for t in range(N_FRAMES):
        assert a["P"][t].tobytes() == b["P"][t].tobytes(), (tag, "P", t)
        assert a["poses"][t].tobytes() == b["poses"][t].tobytes(), (tag, "poses", t)
    for x, y, name in zip(a["scene"] + a["pool"], b["scene"] + b["pool"], ("poses", "groups", "feats", "entries", "anchor poses", "slots")):
        assert x.tobytes() == y.tobytes(), (tag, name)


def test_device_life_cycle_equals_the_host_life_cycle_bit_for_bit(built, runs):
    """the same 12 scripted frames with pool_lifecycle="device": the list of the frame the bystanders end in, P and the poses of
    every frame, the scene and the pool at the end, the counters, and the device's rings against the host's _PoolBook"""
    _, host = runs
    dev = _run(OOS, device=True)
    assert int(dev["stats"]["oos_used"].sum()) > 0
    assert dev["stats"].tobytes() == host["stats"].tobytes()
    assert dev["list"].tobytes() == host["list"].tobytes() and dev["gamma"].tobytes() == host["gamma"].tobytes()
    _same_state(dev, host, "use_oos")
    r, mo = dev["rings"], OOS["oos_max_obs"]
    for b in range(B):
        pb = host["pools"][b]
        assert dev["book"]["ent_id"][b].tolist() == pb.ent_id, b
        used = np.array(pb.anc_used, dtype=bool)
        assert np.array_equal(r["anc_born"][b][used], np.array(pb.anc_born)[used]), b
        for e, fid in enumerate(pb.ent_id):
            if fid < 0:
                continue
            assert r["hist_cnt"][b, e] == pb.hist_cnt[e] > 0, (b, e)
            for s_ in range(min(pb.hist_cnt[e], mo)):
                a, born, px = pb.hist[e][s_]
                assert (r["hist_anchor"][b, e, s_], r["hist_born"][b, e, s_]) == (a, born), (b, e, s_)
                assert tuple(r["hist_xp"][b, e, s_]) == px, (b, e, s_)


def test_the_option_off_on_the_device_life_cycle_is_the_host_life_cycle_without_it(built, runs):
    off, _ = runs
    _same_state(_run(dict(use_oos=False), device=True), off, "off")


def test_unsupported_combinations_are_refused():
    with pytest.raises(ValueError):
        sequence.check_lifecycle(sequence.SequenceConfig(use_oos=True))                       # needs the pool
    sequence.check_lifecycle(sequence.SequenceConfig(**QUICK, pool_lifecycle="device", tracks_max=300, **OOS))
    with pytest.raises(ValueError):
        sequence.check_lifecycle(sequence.SequenceConfig(**QUICK, **{**OOS, "oos_min_observations": 1}))


def test_run_pcw_cli_reports_the_four_counters(built):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts", "run_pcw.py"), "-sequences", "2", "-total_time", "0.4", "-npts", "200",
           "-feature_init", "subfilter", "-use-oos", "-oos-min-obs", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert all(isinstance(rep[k], int) for k in ("oos_used", "oos_gated", "oos_surplus", "oos_short"))
    # the C++ host side (BatchEstimator::EnableOosUpdates) on the device life cycle and the device's tracks
    vec = [sys.executable, os.path.join(root, "scripts", "run_pcw.py"), "-sequences", "4", "-total_time", "0.4", "-npts", "200",
           "-feature_init", "subfilter", "-vectorized", "-pool-lifecycle", "device", "-tracks", "device", "-use-oos"]
    out = subprocess.run(vec, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert all(isinstance(rep[k], int) for k in ("oos_used", "oos_gated", "oos_surplus", "oos_short", "oos_sequences_with_used"))
    for bad in (["-vectorized"], ["-innov-log"], ["-host", "cpp"]):
        r = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "error" in r.stderr, (bad, r.stderr[-500:])


# ---- the same on tracks the device produces (track_source="device"): xivo_hip_pool_life_begin_tracks -> pool_oos_select_kernel on
# the strided track block. The producer's tracks are steered through its world, which is uploaded again before every frame with
# the ids it handed out: a point that is not shown yet, or no longer, stands 50 m behind the first camera; a bystander jumps
# 40 px sideways and back from frame to frame, so its sub-filter counts it as an outlier. The host life cycle runs in a second
# context on exactly those tracks, read back.
NPTS_W = 13     # points 0 - 4 from frame 0, 5 - 6 the bystanders, 7 - 9 from frame 3, 10 - 12 from frame 6


def _world_frames(cfg, sims):
    """per frame: the IMU records, the ground-truth camera poses gsc [B, 12] and the world Xs [B, NPTS_W, 3] of that frame"""
    Rbc = pcw.so3_exp(cfg.Wbc)
    rng = np.random.default_rng(7)
    cam = cfg.cam
    true, side, hidden = np.zeros((B, NPTS_W, 3)), np.zeros((B, NPTS_W, 3)), np.zeros((B, 3))
    for b, s in enumerate(sims):
        Rsb, Tsb = s.gsb(0.0)
        Rsc, Tsc = Rsb @ Rbc, Rsb @ cfg.Tbc + Tsb
        z = rng.uniform(3.0, 6.0, NPTS_W)
        u, v = rng.uniform(cam["cx"] - 150, cam["cx"] + 150, NPTS_W), rng.uniform(cam["cy"] - 110, cam["cy"] + 110, NPTS_W)
        Xc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], axis=1)
        true[b] = Xc @ Rsc.T + Tsc
        side[b] = np.outer(40.0 / cam["fx"] * z, Rsc[:, 0])             # 40 px along the first camera's x axis
        hidden[b] = Rsc @ np.array([0.0, 0.0, -50.0]) + Tsc
    first = np.array([0] * 7 + [3] * 3 + [6] * 3)
    m0 = [s.meas(0.0) for s in sims]
    feeder = sequence.ImuFeeder(B, 0.0, [m[1] for m in m0], [m[0] for m in m0])
    for t in range(N_FRAMES):
        for k in range(16 * t - 15 if t else 0, 16 * t + 1):
            if k > 0:
                m = [s.meas(k * 0.0025) for s in sims]
                feeder.imu(k * 0.0025, np.array([x[1] for x in m]), np.array([x[0] for x in m]))
        tt = 16 * t * 0.0025
        feeder.visual(tt)
        g = [s.gsb(tt) for s in sims]
        gsc = np.array([np.concatenate([(R @ Rbc).reshape(-1), R @ cfg.Tbc + p]) for R, p in g])
        Xs = true.copy()
        if t > 0:
            Xs[:, 5:7] += side[:, 5:7] * (1.0 if t % 2 else -1.0)
        Xs[:, first > t] = hidden[:, None]
        if t >= DROP_AT:
            Xs[:, 5:7] = hidden[:, None]
        yield feeder.take(), gsc, Xs


def test_device_tracks_and_life_cycle_equal_the_host_life_cycle_on_the_same_tracks(built):
    kw = dict(**QUICK, **SHAPE, **OOS)
    cfg_d = sequence.SequenceConfig(pool_lifecycle="device", track_source="device", npts=NPTS_W, tracks_max=NPTS_W, **kw)
    cfg_h = sequence.SequenceConfig(**kw)
    sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]
    poses0, P0 = sequence.initial_poses(cfg_h, sims), np.repeat(cfg_h.P_init()[None], B, axis=0)
    dev, host = sequence.HipBackend(cfg_d, B, poses0, P0), sequence.HipBackend(cfg_h, B, poses0, P0)
    try:
        rd, rh = sequence.SequenceRunner(dev, cfg_d, B), sequence.SequenceRunner(host, cfg_h, B)
        rd.noise_px_std, rd.noise_seed = 1.0, 21
        ids, next_id = None, None
        for t, (rec, gsc, Xs) in enumerate(_world_frames(cfg_d, sims)):
            dev.set_world(Xs, ids, next_id)
            rd.frame_world(rec, gsc, t)
            cnt, tid, meas = dev.ctx.pcw_get_tracks(cfg_d.tracks_max, 0, B)      # (the frame only read them: still in the block)
            ids, next_id = dev.world_ids()
            rh.frame(rec, [(tid[b, :cnt[b]], meas[b, :cnt[b]]) for b in range(B)])
            snap = lambda be: [be.covariance()] + list(be.scene()) + list(be.ctx.pool_get(0, B))
            for x, y, name in zip(snap(dev), snap(host), ("P", "poses", "groups", "feats", "entries", "anchor poses", "slots")):
                assert x.tobytes() == y.tobytes(), (t, name)
            if t == DROP_AT:
                ld, lh = dev.ctx.pool_oos_get(0, B), host.ctx.pool_oos_get(0, B)
                assert ld[0].tobytes() == lh[0].tobytes() and ld[1].tobytes() == lh[1].tobytes()
                assert cnt.tolist() == [NPTS_W - 2] * B                            # every point but the bystanders is tracked
        sd, sh = dev.oos_stats(), host.oos_stats()
        print({k: sd[k].tolist() for k in sd.dtype.names}, ld[0]["n_obs"].tolist(), ld[1].round(2).tolist())
        assert sd.tobytes() == sh.tobytes() and int(sd["oos_used"].sum()) > 0
        r, book, mo = dev.ctx.pool_oos_get_rings(0, B), dev.pool_life_book(), OOS["oos_max_obs"]
        for b in range(B):
            pb = rh.pools[b]
            assert book["ent_id"][b].tolist() == pb.ent_id, b
            used = np.array(pb.anc_used, dtype=bool)
            assert np.array_equal(r["anc_born"][b][used], np.array(pb.anc_born)[used]), b
            for e, fid in enumerate(pb.ent_id):
                if fid >= 0:
                    assert r["hist_cnt"][b, e] == pb.hist_cnt[e], (b, e)
                    for s_ in range(min(pb.hist_cnt[e], mo)):
                        a, born, px = pb.hist[e][s_]
                        assert (r["hist_anchor"][b, e, s_], r["hist_born"][b, e, s_], tuple(r["hist_xp"][b, e, s_])) == (a, born, px)
    finally:
        dev.close(); host.close()
