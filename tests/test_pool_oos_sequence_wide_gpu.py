"""GPU: the device pool life cycle's MSCKF kernels past one wave of entries - pool_oos_select_kernel and pool_oos_record_kernel
with pool_max = 130, where their lane-strided loops over the entries take a second and a third pass and sCase[] / the rings are
indexed past 64 and 128 (tests/test_pool_oos_sequence_gpu.py runs a pool of 16).

The 12 scripted frames of that file on a fuller pool, B = 3: of the simulator's tracks that stay visible throughout, 130 are
shown from frame 0 on - they take entries 0 .. 129 in the order of their ids -, five of them as they are (admitted in frame 3,
their anchor linked) and 125 as a "crowd" with pixels 40 px off in every later frame: the sub-filter counts them as outliers, so
they never become candidates and keep their entries. Three more tracks are shown from each of frames 3, 6 and 9 (one anchor
each; the first two are linked by frame 9), so a crowd entry is observed by four anchors and its ring of three has wrapped. In
frame 10 five crowd tracks end, which hold one entry below 64, one from 64 on and three around 128 (up to 129): READY, the two
observations of the linked anchors still valid - one more than oos_max = 4. The same frames run in log depth and with
use_invdepth (XIVO_HIP_FLAG_INVDEPTH: feature_depth / feature_unproject of the select kernel), where fewer of the ending
entries keep a depth inside the window.

Required: the device life cycle leaves the bytes of the host life cycle on the same tracks (list, P, scene, pool, counters), and
its rings and anc_born equal a restatement kept here that shares nothing with either - a list per entry, one append per created
anchor, reset at birth - driven by the tracks shown and the books read back after every frame."""
import numpy as np
import pytest

from test_pool_lifecycle_gpu import QUICK, _sim_frames
from test_pool_oos_sequence_gpu import _same_state, N_FRAMES, DROP_AT
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu
B, NPTS = 3, 900
SHAPE = dict(n_groups=4, n_features=12, pool_max=130, anchor_max=6, remove_outlier_counter=1e9)
OOS = dict(use_oos=True, oos_max=4, oos_max_obs=3, oos_min_observations=2)
# entries (= ranks among the ids shown in frame 0) whose crowd tracks end in DROP_AT: the first of the low and of the middle ranks
# and the first three of the high ones that are crowd tracks - five, so that with oos_max = 4 the used ones reach past 128
ENDING = ((1, 2, 3, 4, 5, 6), (64, 65, 66, 67, 68, 69), (129, 128, 127, 126, 125, 124))


def _sims():
    return [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]


@pytest.fixture(scope="module")
def script():
    """per frame (IMU records, per filter (ids, meas) of the tracks shown), and per filter the ids that end in DROP_AT"""
    cfg = sequence.SequenceConfig(**QUICK, **SHAPE, **OOS)
    sims, frames_of = _sims(), _sim_frames(cfg, B, NPTS)
    raw = [frames_of(t, sims) for t in range(N_FRAMES)]
    first, crowd, ending = [], [], []
    for b in range(B):
        always = set.intersection(*[set(int(i) for i in raw[t][1][b][0]) for t in range(N_FRAMES)])
        ids0, meas0 = raw[0][1][b]
        central = [int(i) for i, m in sorted(zip(ids0, meas0), key=lambda p: p[0]) if int(i) in always
                   and abs(m[0] - cfg.cam["cx"]) < 160 and abs(m[1] - cfg.cam["cy"]) < 120]
        assert len(central) >= 14
        rest = sorted(always - set(central[:14]))
        assert len(rest) >= 125
        f = {**{i: 0 for i in central[:5]}, **{i: 3 for i in central[5:8]}, **{i: 6 for i in central[8:11]},
             **{i: 9 for i in central[11:14]}, **{i: 0 for i in rest[:125]}}
        shown0 = sorted(i for i, t0 in f.items() if t0 == 0)
        assert len(shown0) == SHAPE["pool_max"]
        first.append(f); crowd.append(set(rest[:125]))
        ending.append({shown0[e] for band, n in zip(ENDING, (1, 1, 3)) for e in [e for e in band if shown0[e] in crowd[b]][:n]})
        assert len(ending[b]) == 5 > OOS["oos_max"]
    frames = []
    for t, (rec, tracks) in enumerate(raw):
        ft = []
        for b, (ids, meas) in enumerate(tracks):
            keep = [k for k, i in enumerate(ids) if first[b].get(int(i), 1 << 30) <= t and not (t >= DROP_AT and int(i) in ending[b])]
            m = np.array(meas, dtype=float)[keep]
            for r, k in enumerate(keep):
                if t > 0 and int(ids[k]) in crowd[b]:
                    m[r, :2] += 40.0 if t % 2 else -40.0
            ft.append((np.array(ids)[keep], m))
        frames.append((rec, ft))
    return frames, ending


def _run(frames, device, extra):
    cfg = sequence.SequenceConfig(**QUICK, **SHAPE, **OOS, **extra, **(dict(pool_lifecycle="device", tracks_max=300) if device else {}))
    sims = _sims()
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    out = dict(P=[], poses=[], books=[], anchors=[], extra=extra)
    try:
        runner = sequence.SequenceRunner(be, cfg, B)
        for t, (rec, ft) in enumerate(frames):
            runner.frame(rec, ft)
            out["P"].append(be.covariance()); out["poses"].append(be.scene()[0])
            if device:      # what the restatement is driven by: who is in the state and in the pool, and the entries' anchors
                out["books"].append(be.pool_life_book()); out["anchors"].append(be.ctx.pool_get(0, B)[0]["ref_sind"].copy())
                if t == DROP_AT - 1:
                    out["rings_before"] = be.ctx.pool_oos_get_rings(0, B)
            if t == DROP_AT:
                out["list"], out["gamma"] = be.ctx.pool_oos_get(0, B)
                out["stats_drop"] = be.oos_stats()
        out["pool"], out["scene"], out["stats"] = be.ctx.pool_get(0, B), be.scene(), be.oos_stats()
        if device:
            out["rings"] = be.ctx.pool_oos_get_rings(0, B)
        else:
            out["pools"] = runner.pools
    finally:
        be.close()
    return out


# log depth, and the USE_INVDEPTH build (XIVO_HIP_FLAG_INVDEPTH: feature_depth and feature_unproject of the select kernel)
@pytest.fixture(scope="module", params=[{}, dict(use_invdepth=True)], ids=["logdepth", "invdepth"])
def runs(built, script, request):
    frames, _ = script
    return _run(frames, False, request.param), _run(frames, True, request.param)


def test_the_script_drops_entries_past_64_and_128_with_wrapped_rings(script, runs):
    """the preconditions, from the device's books: which entries the ending tracks hold, their rings, and that they are used"""
    _, ending = script
    host, dev = runs
    book, r = dev["books"][DROP_AT - 1], dev["rings_before"]
    for b in range(B):
        es = sorted(e for e, fid in enumerate(book["ent_id"][b]) if int(fid) in ending[b])
        assert len(es) == len(ending[b]) > OOS["oos_max"], (b, es)
        assert es[0] < 64 and any(64 <= e < 128 for e in es) and es[-1] >= 128, (b, es)
        assert all(r["hist_cnt"][b, e] > OOS["oos_max_obs"] for e in es), (b, r["hist_cnt"][b, es])
        gone = dev["books"][DROP_AT]["ent_id"][b]
        assert all(gone[e] < 0 for e in es)                                  # used or not, a dropped entry is freed
    st = dev["stats_drop"]
    print({k: st[k].tolist() for k in st.dtype.names}, dev["list"]["n_obs"].tolist(), dev["gamma"].round(2).tolist())
    # which entries were used: a list position's first pixel is one of its entry's ring
    mo, all_used = OOS["oos_max_obs"], []
    for b in range(B):
        es = [e for e, fid in enumerate(book["ent_id"][b]) if int(fid) in ending[b]]
        used = []
        for f in dev["list"][b]:
            if f["n_obs"] >= 2:
                m = [e for e in es if any(tuple(r["hist_xp"][b, e, s_]) == tuple(f["xp"][0]) for s_ in range(mo))]
                assert len(m) == 1, (b, m)
                used.append(m[0])
        print("filter %d: ending entries %s used %s" % (b, sorted(es), used))
        assert used == sorted(used) and len(used) == st["oos_used"][b], (b, used)
        all_used += used
    # used entries from each of the three passes of the lanes (which filter has them depends on the sub-filters' depths)
    assert min(all_used) < 64 and any(64 <= e < 128 for e in all_used) and max(all_used) >= 128, all_used
    if not dev["extra"]:        # log depth: every ending entry of filters 0 and 1 is eligible, the fifth - entry 129 - is surplus
        assert st["oos_used"].tolist()[:2] == [4, 4] and st["oos_surplus"].tolist()[:2] == [1, 1]
    assert (st["oos_used"] + st["oos_surplus"] + st["oos_short"] <= 5).all()       # nothing else is dropped


def test_device_life_cycle_equals_the_host_life_cycle_bit_for_bit_past_one_wave(runs):
    host, dev = runs
    assert dev["stats"].tobytes() == host["stats"].tobytes() and dev["stats_drop"].tobytes() == host["stats_drop"].tobytes()
    assert dev["list"].tobytes() == host["list"].tobytes() and dev["gamma"].tobytes() == host["gamma"].tobytes()
    _same_state(dev, host, "pool_max 130")
    r, mo = dev["rings"], OOS["oos_max_obs"]
    for b in range(B):
        pb = host["pools"][b]
        assert dev["books"][-1]["ent_id"][b].tolist() == pb.ent_id, b
        used = np.array(pb.anc_used, dtype=bool)
        assert np.array_equal(r["anc_born"][b][used], np.array(pb.anc_born)[used]), b
        for e, fid in enumerate(pb.ent_id):
            if fid < 0:
                continue
            assert r["hist_cnt"][b, e] == pb.hist_cnt[e] > 0, (b, e)
            for s_ in range(min(pb.hist_cnt[e], mo)):
                a, born, px = pb.hist[e][s_]
                assert (r["hist_anchor"][b, e, s_], r["hist_born"][b, e, s_], tuple(r["hist_xp"][b, e, s_])) == (a, born, px), (b, e, s_)


def test_rings_equal_a_restatement_from_the_tracks_and_the_books(script, runs):
    """a list per entry: reset when the entry takes a new track, one (anchor, frame, pixel) appended per frame that creates an
    anchor, to every entry live at the end of the frame. The anchor a frame creates is the one its new tracks' entries hang on."""
    frames, _ = script
    _, dev = runs
    mo, pm = OOS["oos_max_obs"], SHAPE["pool_max"]
    ring = [[[] for _ in range(pm)] for _ in range(B)]
    born = [dict() for _ in range(B)]                                       # anchor -> frame it was created in
    created = 0
    for t, (_, ft) in enumerate(frames):
        frame = t + 1                                                        # the life cycle counts frames from 1
        book, anchors = dev["books"][t], dev["anchors"][t]
        prev = dev["books"][t - 1] if t else None
        for b in range(B):
            ids, meas = ft[b]
            px = {int(i): (float(m[0]), float(m[1])) for i, m in zip(ids, meas)}
            known = set() if prev is None else {int(i) for i in prev["feat_id"][b] if i >= 0} | {int(i) for i in prev["ent_id"][b] if i >= 0}
            new = set(px) - known
            took = [e for e in range(pm) if int(book["ent_id"][b, e]) in new]
            assert (len(took) > 0) == (len(new) > 0), (t, b)                 # (a frame's new tracks find a free entry)
            for e in took:
                ring[b][e] = []
            if not new:
                continue
            a = {int(anchors[b, e]) for e in took}
            assert len(a) == 1, (t, b, a)
            a = a.pop()
            born[b][a] = frame
            created += 1
            for e in range(pm):
                fid = int(book["ent_id"][b, e])
                if fid >= 0:
                    ring[b][e].append((a, frame, px[fid]))
    assert created >= 4 * B         # (one more where the pool was full: the track left over is new again in the next frame)
    r, last = dev["rings"], dev["books"][-1]
    wrapped = 0
    for b in range(B):
        for a, frame in born[b].items():
            if last["anc_used"][b, a]:
                assert r["anc_born"][b, a] == frame, (b, a)
        for e in range(pm):
            if last["ent_id"][b, e] < 0:
                continue
            h = ring[b][e]
            assert r["hist_cnt"][b, e] == len(h) > 0, (b, e)
            wrapped += len(h) > mo
            for i in range(max(0, len(h) - mo), len(h)):
                s_ = i % mo
                got = (int(r["hist_anchor"][b, e, s_]), int(r["hist_born"][b, e, s_]), tuple(r["hist_xp"][b, e, s_].tolist()))
                assert got == h[i], (b, e, i)
    assert wrapped >= 100 * B                                                # the crowd's rings, entries up to 129
