"""CPU-only: the OOS rules of xivo_amd/csrc/pool_lifecycle_device.h (observation ring, validity of an observation, which dropped
entries are used) under a host compiler, against the host life cycle. tests/pool_oos_driver.cpp is a stand-alone program built
from the header alone - plain, and under AddressSanitizer and UBSan - that keeps the rings itself and replays, per frame and
filter, the anchor tables at selection time, the dropped entries and the frame's appends. The expectation is
SequenceRunner._frame_subfilter with use_oos over the recording backend double of tests/test_pool_lifecycle_cpu.py, which here
also plays the device's part of the decision (an entry's status and depth) and restates plife_oos_decide in Python.

What this does not cover: Xs, the rows and the gate (tests/test_pool_oos_gpu.py), and the kernel's walk itself, which calls the
same plife_oos_decide (tests/test_pool_oos_gpu.py holds its list and counters against these rules)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_pool_lifecycle_cpu import _RecordingBackend, _cfg, _fuzz_frames, _tracks
from xivo_amd import lib as L
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "pool_oos_driver.cpp")
NONE, USED, SHORT, SURPLUS = range(4)


def _oos_cfg(**kw):
    base = dict(use_oos=True, oos_max=1, oos_max_obs=3, oos_min_observations=2)
    base.update(kw)
    return _cfg(**base)


class _Double(_RecordingBackend):
    """the recording double plus the device's side of the OOS selection: what it is handed (with the books at that moment) and
    its answer - READY and depth in range per entry from the script (not_ready / deep sets of (b, e)) or at random (85 % / 90 %)"""

    runner = None

    def pool_oos_collect(self, cands):
        cfg, B = self.cfg, self.B
        rec = dict(books=[(list(map(int, pb.anc_used)), list(pb.anc_born), list(pb.anc_link)) for pb in self.runner.pools],
                   live=[[(e, 0 if fid in self.pos[b] else -1) for e, fid in enumerate(pb.ent_id) if fid >= 0]
                         for b, pb in enumerate(self.runner.pools)], dropped=[[] for _ in range(B)], decisions=[])
        n_used = [0] * B
        assert [(int(c["b"]), int(c["entry"])) for c in cands] == sorted((int(c["b"]), int(c["entry"])) for c in cands)
        for c in cands:
            b, e, k = int(c["b"]), int(c["entry"]), int(c["n_obs"])
            assert self.live[b, e]
            if self.script is not None:
                ready, depth = (b, e) not in self.script.get("not_ready", ()), (b, e) not in self.script.get("deep", ())
            else:
                ready, depth = bool(self.rng.uniform() < 0.85), bool(self.rng.uniform() < 0.9)
            d = NONE if not ready else SHORT if k < cfg.oos_min_observations else NONE if not depth else \
                USED if n_used[b] < cfg.oos_max else SURPLUS
            n_used[b] += d == USED
            self.stats[b][d] += 1
            rec["dropped"][b].append((e, int(ready), int(depth)))
            rec["decisions"].append((b, e, k, d, tuple(int(g) for g in c["group_sind"][:k]), [tuple(p) for p in c["xp"][:k]]))
        self.oos = rec


def _build(tmp, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pool_oos_driver.cpp"
    exe = str(tmp / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, DRIVER, "-o", exe] + flags, check=True)
    return exe


BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pool_oos_" + request.param), BUILDS[request.param])


def _play(exe, cfg, B, frames, scripts=None, seed=7):
    """the host life cycle over the double, then the same frames through the driver; everything the driver prints must equal what
    the host life cycle did. -> (per frame the decisions [(b, e, k, decision, groups, pixels)], counters [B][4], runner)"""
    be = _Double(cfg, B, seed)
    runner = sequence.SequenceRunner(be, cfg, B)
    be.runner, be.stats = runner, [[0] * 4 for _ in range(B)]
    lines = ["%d %d %d %d %d %d %d %d" % (cfg.pool_max, cfg.anchor_max, cfg.n_groups, cfg.oos_max_obs, cfg.oos_min_observations,
                                          cfg.oos_max, B, len(frames))]
    want, per_frame = [], []
    for t, tracks in enumerate(frames):
        be.script = None if scripts is None else scripts.get(t, {})
        be.pos = [set(int(i) for i in tracks[b][0]) for b in range(B)]
        before = [list(pb.hist_cnt) for pb in runner.pools] if runner.pools else [[0] * cfg.pool_max for _ in range(B)]
        runner.frame(None, tracks)
        rec, frame = be.oos, runner.vision_counter
        per_frame.append(rec["decisions"])
        rows = []
        for b in range(B):
            pb = runner.pools[b]
            used, born, link = rec["books"][b] if t else ([0] * cfg.anchor_max, [0] * cfg.anchor_max, [-1] * cfg.anchor_max)
            for row in (used, born, link):
                lines.append(" ".join(str(int(v)) for v in row))
            live = rec["live"][b] if t else []
            lines.append("%d %s" % (len(live), " ".join("%d %d" % p for p in live)))
            lines.append("%d %s" % (len(rec["dropped"][b]), " ".join("%d %d %d" % p for p in rec["dropped"][b])))
            for (bb, e, k, d, groups, _) in rec["decisions"]:
                if bb == b:
                    rows.append("D %d %d %d %d" % (b, e, k, d) + "".join(" %d" % g for g in groups))
            rows.append("C %d %d %d %d" % (b, be.stats[b][USED], be.stats[b][SHORT], be.stats[b][SURPLUS]))
            made = [a for a in range(cfg.anchor_max) if pb.anc_used[a] and pb.anc_born[a] == frame and pb.anc_life[a] == 0]
            assert len(made) <= 1
            lines.append("%d %d" % (made[0] if made else -1, frame))
            taken = [e for e, fid in enumerate(pb.ent_id) if fid >= 0 and pb.ent_born[e] == frame]
            seen = [e for e, fid in enumerate(pb.ent_id) if fid >= 0]
            lines.append("%d %s" % (len(taken), " ".join(map(str, taken))))
            lines.append("%d %s" % (len(seen), " ".join(map(str, seen))))
            for e in seen:
                if made:
                    a, fb, px = pb.hist[e][(pb.hist_cnt[e] - 1) % cfg.oos_max_obs]
                    assert (a, fb) == (made[0], frame) and px == tuple(tracks[b][1][list(tracks[b][0]).index(pb.ent_id[e]), :2])
                    rows.append("H %d %d %d %d" % (b, e, pb.hist_cnt[e], (pb.hist_cnt[e] - 1) % cfg.oos_max_obs))
                else:
                    assert pb.hist_cnt[e] == before[b][e]          # a frame without a new anchor records nothing
        want.append(rows)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "R %d" % cfg.oos_rows()
    got, cur = [], []
    for ln in out[1:]:
        if ln == "E":
            got.append(cur); cur = []
        else:
            # the driver prints the ring slots behind the groups: the host keeps no slot numbers, so they are cut off here
            p = ln.split()
            cur.append(" ".join(p[:5 + int(p[3])]) if p[0] == "D" else ln)
    assert got == want
    return per_frame, be.stats, runner


def _case(exe, cfg, id_lists, scripts):
    rng = np.random.default_rng(5)
    frames = [[_tracks(ids, rng)] for ids in id_lists]
    dec, stats, runner = _play(exe, cfg, 1, frames, scripts={t: s for t, s in enumerate(scripts)})
    return [[d[1:5] for d in fr] for fr in dec], stats[0], runner, frames


# tracks 1 and 2 are seen by anchor 0 (frame 1); track 1 is admitted and links it, track 3 arrives with anchor 1 (frame 2), which
# sees track 2 as well; track 3 is admitted and links anchor 1 (frame 3) unless the case says otherwise; track 2 ends in frame 4
BASE_IDS = [[1, 2], [1, 2, 3], [1, 2, 3], [1, 3]]
BASE = [dict(order={0: []}), dict(order={0: [0]}), dict(order={0: [0]}), dict(order={0: []})]


def test_exactly_min_obs_observations_are_used_and_one_fewer_is_short(driver):
    dec, st, runner, _ = _case(driver, _oos_cfg(), BASE_IDS, BASE)
    assert dec[3] == [(1, 2, USED, (0, 1))] and st == [0, 1, 0, 0]
    assert runner.pools[0].ent_id[1] == -1                              # freed as before: used once
    # anchor 1 is never linked: one valid observation
    dec, st, _, _ = _case(driver, _oos_cfg(), BASE_IDS, BASE[:2] + [dict(order={0: []})] * 2)
    assert dec[3] == [(1, 1, SHORT, (0,))] and st == [0, 0, 1, 0]


def test_a_wrapped_ring_forgets_the_oldest_observation(driver):
    """track 1 is seen by the anchors of frames 1 - 4, max_obs = 3: the first is gone; tracks 2 - 4 are admitted in frame 5 and link
    anchors 1 - 3; track 1 ends in frame 6 with the three youngest observations, oldest first"""
    cfg = _oos_cfg(n_features=3, anchor_max=5)
    dec, st, runner, frames = _case(driver, cfg, [[1], [1, 2], [1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4], [2, 3, 4]],
                                    [dict(order={0: []})] * 4 + [dict(order={0: [1, 2, 3]}), dict(order={0: []})])
    assert dec[5] == [(0, 3, USED, (0, 1, 2))] and st[USED] == 1
    assert runner.pools[0].hist_cnt[0] == 4


def test_a_stale_observation_of_a_reused_anchor_index_does_not_count(driver):
    """anchor 1 (frame 2, track 3) loses its only entry in frame 3, expires at the end of frame 4 (max_group_lifetime = 1) and
    its index is created again in frame 5 with track 4; tracks 1 and 4 are admitted in frame 6 and link anchors 0 and 1. Track 2,
    seen by (0, frame 1), (1, frame 2) and (1, frame 5), ends in frame 7: the middle observation names an anchor that is gone"""
    cfg = _oos_cfg(max_group_lifetime=1)
    dec, st, runner, _ = _case(driver, cfg, [[1, 2], [1, 2, 3], [1, 2], [1, 2], [1, 2, 4], [1, 2, 4], [1, 4]],
                               [dict(order={0: []})] * 5 + [dict(order={0: [0, 2]}), dict(order={0: []})])
    assert runner.pools[0].anc_born[1] == 5
    assert dec[2] == [(2, 0, SHORT, ())]                               # (track 3 itself: its one observation hangs on an unlinked anchor)
    assert dec[6] == [(1, 2, USED, (0, 1))] and st == [0, 1, 1, 0]


def test_an_observation_from_a_group_that_left_the_state_does_not_count(driver):
    """as the base case, but track 1 - the only feature of anchor 0's group - ends in frame 4 too: the group is discarded before
    the selection and its observation no longer counts"""
    dec, st, _, _ = _case(driver, _oos_cfg(), BASE_IDS[:3] + [[3]], BASE)
    assert dec[3] == [(1, 1, SHORT, (1,))] and st == [0, 0, 1, 0]


def test_more_eligible_entries_than_oos_max_are_counted_as_surplus(driver):
    ids = [[1, 2, 5], [1, 2, 3, 5], [1, 2, 3, 5], [1, 3]]
    dec, st, _, _ = _case(driver, _oos_cfg(), ids, BASE)
    assert dec[3] == [(1, 2, USED, (0, 1)), (2, 2, SURPLUS, (0, 1))] and st == [0, 1, 0, 1]
    dec, st, _, _ = _case(driver, _oos_cfg(oos_max=2), ids, BASE)
    assert [d[2] for d in dec[3]] == [USED, USED] and st == [0, 2, 0, 0]


def test_an_entry_dropped_in_a_frame_without_a_new_anchor(driver):
    """frames 3 and 4 of the base case create no anchor: nothing is recorded in them (_play checks every ring), and the entry that
    ends in frame 4 is used with what the earlier frames recorded"""
    dec, st, runner, _ = _case(driver, _oos_cfg(), BASE_IDS, BASE)
    assert [a for a in range(3) if runner.pools[0].anc_used[a]] == [0, 1] and runner.pools[0].anc_born[:2] == [1, 2]
    assert dec[3][0][2] == USED


def test_a_subfilter_outlier_is_never_used(driver):
    """track 2 stays, but the step kills its entry in frame 4: it was never handed over"""
    dec, st, runner, _ = _case(driver, _oos_cfg(), BASE_IDS[:3] + [[1, 2, 3]], BASE[:3] + [dict(kill={(0, 1)}, order={0: []})])
    assert dec[3] == [] and st == [0, 0, 0, 0]


def test_not_ready_and_out_of_depth_entries_are_not_used(driver):
    dec, st, _, _ = _case(driver, _oos_cfg(), BASE_IDS, BASE[:3] + [dict(order={0: []}, not_ready={(0, 1)})])
    assert dec[3] == [(1, 2, NONE, (0, 1))] and st == [1, 0, 0, 0]
    dec, st, _, _ = _case(driver, _oos_cfg(), BASE_IDS, BASE[:3] + [dict(order={0: []}, deep={(0, 1)})])
    assert dec[3] == [(1, 2, NONE, (0, 1))] and st == [1, 0, 0, 0]


def test_fuzz_fires_and_equals_the_host_life_cycle(driver):
    """random track sets over small tables, min_obs = 2 of max_obs = 4, two features per frame at most; the seed is pinned and
    the configuration fires: at least a quarter of the filters use an entry"""
    cfg = _oos_cfg(oos_max=2, oos_max_obs=4, anchor_max=6, max_group_lifetime=3)
    B = 8
    frames = _fuzz_frames(B, 150, np.random.default_rng(11), p_toggle=0.06)
    dec, stats, _ = _play(driver, cfg, B, frames, seed=3)
    used = [s[USED] for s in stats]
    assert sum(u > 0 for u in used) * 4 >= B, used
    assert sum(s[SHORT] for s in stats) > 0
    assert any(d[2] == 4 for fr in dec for d in fr) or any(d[2] == 3 for fr in dec for d in fr)     # longer histories occur too


def test_chi2_table_equals_scipy():
    st = pytest.importorskip("scipy.stats")
    assert len(L.CHI2_95) == 32 and L.CHI2_95[0] == 0.0 and L.CHI2_95[30:] == (0.0, 0.0)
    assert np.abs(np.array(L.CHI2_95[1:30]) - st.chi2.ppf(0.95, np.arange(1, 30))).max() < 1e-10


def test_config_and_row_reservation():
    C = sequence.SequenceConfig
    c = C()
    assert (c.use_oos, c.oos_min_observations, c.oos_meas_std, c.oos_max, c.oos_max_obs) == (False, 5, 3.5, 4, 6)
    assert c.oos_rows() == 0 and c.M_max() == 2 * c.n_features                    # off: the context is sized as before
    c = C(use_oos=True, feature_init="subfilter")
    assert c.oos_rows() == 36 and c.M_max() == 60 + 64                            # 36 rows + 16 of padding, rounded up to 16
    for kw in (dict(use_oos=True),
               dict(use_oos=True, feature_init="subfilter", oos_max_obs=L.OOS_MAX_OBS + 1),
               dict(use_oos=True, feature_init="subfilter", oos_min_observations=7)):
        with pytest.raises(ValueError):
            sequence.SequenceRunner(None, C(**kw), 1)


def test_header_stays_plain_cxx():
    text = open(os.path.join(CSRC, "pool_lifecycle_device.h")).read()
    for name in ("plife_hist_append", "plife_hist_slot", "plife_obs_group", "plife_valid_obs", "plife_oos_decide", "plife_oos_rows"):
        assert name in text
    assert "hip/" not in text.split("#pragma once")[1]
