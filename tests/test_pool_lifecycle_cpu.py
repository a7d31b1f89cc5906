"""CPU-only: the decisions of the device pool life cycle (xivo_amd/csrc/pool_lifecycle_device.h) under a host compiler, against
the host life cycle of the "subfilter" mode. tests/pool_lifecycle_driver.cpp is compiled with g++ against the header (and
lifecycle_device.h, which it includes) alone and replays a scripted run - per frame and filter the tracks, what the pool step
answered (live flags, candidate order) and the gating outcome per slot - through the functions the kernels call, in the
kernels' order. The expectation is SequenceRunner._frame_subfilter over a recording backend double that gives the same answers:
the op sequences, the track that feeds every slot and entry, the anchors and entries created, both books and the counters must
be identical frame by frame.

What this does not cover: the kernels reach the slot / entry -> track association with one thread per track and an LDS maximum,
the new-track flags and ranks with one thread per track; the driver uses the serial forms of the same rules. That the parallel
forms agree is checked on the GPU (tests/test_pool_lifecycle_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "pool_lifecycle_driver.cpp")
POOL_OPS = (L.EDIT_ADD_GROUP_ANCHOR, L.EDIT_ADMIT_POOL)


def _cfg(**kw):
    base = dict(feature_init="subfilter", n_features=6, n_groups=3, pool_max=8, anchor_max=3, max_group_lifetime=2)
    base.update(kw)
    return sequence.SequenceConfig(**base)


class _RecordingBackend:
    """Backend double of the "subfilter" host life cycle: keeps a shadow of what is resident (in-state slots, live pool entries
    and their anchors, the anchors' links), checks every call against it, records what it is asked and answers pool_step and
    update from a script or at random (10 % of the live entries killed, a random subset in random order as candidates, 15 %
    of the features rejected)."""

    def __init__(self, cfg, B, seed):
        self.cfg, self.B = cfg, B
        self.rng = np.random.default_rng(seed)
        self.sind = np.full((B, cfg.n_features), -1)
        self.live = np.zeros((B, cfg.pool_max), dtype=bool)
        self.anchor = np.full((B, cfg.pool_max), -1)
        self.link = np.full((B, cfg.anchor_max), -2)         # -2: never created
        self.script = None           # dict(kill={(b, e)}, order={b: [e]}, reject={(b, j)}) of the next frame, None: random
        self.cur = None

    def propagate(self, imu):
        pass

    def pool_step(self, xp, strict):
        B, pm = self.B, self.cfg.pool_max
        self.cur = dict(xpp=xp.copy(), edits=[], slots=None, recs=[])
        fed = ~np.isnan(xp[..., 0])
        assert not (fed & ~self.live).any()                  # only live entries get a pixel
        was = self.live.copy()
        self.live &= fed                                     # dropped by the tracker
        order = np.full((B, pm), -1, dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        for b in range(B):
            ents = np.nonzero(self.live[b])[0]
            if self.script is not None:
                kill = [e for e in ents if (b, int(e)) in self.script.get("kill", ())]
                cand = self.script.get("order", {}).get(b)
            else:
                kill = [e for e in ents if self.rng.uniform() < 0.10]
                cand = None
            self.live[b, kill] = False
            ents = np.nonzero(self.live[b])[0]
            if cand is None:
                cand = list(self.rng.permutation(ents)[:self.rng.integers(0, len(ents) + 1)]) if self.script is None else list(ents)
            assert all(self.live[b, e] for e in cand)
            n[b] = len(cand)
            order[b, :len(cand)] = cand
        self.cur.update(order=order.copy(), n=n.copy(), live=self.live.copy(), outliers=int((was & fed & ~self.live).sum()))
        return order, n, self.live.copy()

    def edit(self, ops):
        rec = []
        for o in ops[np.argsort(ops["b"], kind="stable")] if len(ops) else ():
            b, k, i0, i1, i2 = int(o["b"]), int(o["kind"]), int(o["i0"]), int(o["i1"]), int(o["i2"])
            rec.append((b, k, i0, i1, i2))
            if k == L.EDIT_REMOVE_FEATURE:
                assert self.sind[b, i0] >= 0
                self.sind[b, i0] = -1
            elif k == L.EDIT_REMOVE_GROUP:
                self.link[b][self.link[b] == i0] = -1
            elif k == L.EDIT_ADD_GROUP_ANCHOR:
                assert self.link[b, i1] == -1 and not (self.link[b] == i0).any()
                self.link[b, i1] = i0
            else:
                assert k == L.EDIT_ADMIT_POOL and self.live[b, i2] and self.link[b, self.anchor[b, i2]] >= 0 and self.sind[b, i0] < 0
                self.sind[b, i0] = i1
                self.live[b, i2] = False
        self.cur["edits"].append(rec)

    def set_pixels(self, xp):
        self.cur["xp"] = xp.copy()

    def update(self):
        present = self.sind >= 0
        if self.script is not None:
            rej = np.zeros_like(present)
            for b, j in self.script.get("reject", ()):
                rej[b, j] = True
            mask = present & ~rej
        else:
            mask = present & (self.rng.uniform(size=present.shape) > 0.15)
        self.cur["mask"] = mask.copy()
        return mask

    def pool_anchor(self, slots):
        self.cur["slots"] = slots.copy()
        for b, a in enumerate(slots):
            if a >= 0:
                assert self.link[b, a] < 0
                self.link[b, a] = -1

    def pool_add(self, recs):
        for r in recs:
            b, e, a = int(r["b"]), int(r["entry"]), int(r["anchor"])
            assert not self.live[b, e] and self.link[b, a] == -1
            self.live[b, e] = True; self.anchor[b, e] = a
        self.cur["recs"] = list(recs)


def _build(tmp, flags, name):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pool_lifecycle_driver.cpp"
    exe = str(tmp / name)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, DRIVER, "-o", exe] + flags, check=True)
    return exe


def _run_driver(exe, cfg, B, frames, answers):
    """frames: per frame the tracks [(ids, meas)] * B; answers: per frame the double's record -> per frame dict of tag -> rows"""
    lines = ["%d %d %d %d %d %d %d" % (cfg.n_features, cfg.n_groups, cfg.pool_max, cfg.anchor_max, cfg.max_group_lifetime, B,
                                       len(frames))]
    for tracks, ans in zip(frames, answers):
        for b in range(B):
            ids = tracks[b][0]
            lines.append(str(len(ids)))
            lines.append(" ".join(str(int(i)) for i in ids))
            lines.append(" ".join(str(int(v)) for v in ans["live"][b]))
            lines.append(str(int(ans["n"][b])))
            lines.append(" ".join(str(int(e)) for e in ans["order"][b, :ans["n"][b]]))
            lines.append(" ".join(str(int(v)) for v in ans["mask"][b]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    res, cur = [], {k: [] for k in "PXQTRANBC"}
    for ln in out.splitlines():
        if ln == "E":
            res.append(cur); cur = {k: [] for k in "PXQTRANBC"}
        elif ln[0] == "B":
            cur["B"].append(tuple(tuple(int(v) for v in part.split()) for part in ln.split("|")[1:]))
        else:
            cur[ln[0]].append(tuple(int(v) for v in ln.split()[1:]))
    assert len(res) == len(frames)
    return res


BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    """the driver as a stand-alone program, built twice: plain, and under AddressSanitizer and UBSan (a report ends the program
    with a non-zero status, which fails the run). Every test that takes the driver - the fuzz and every scripted case, the
    degenerate tables among them - runs under both builds."""
    exe = _build(tmp_path_factory.mktemp("pool_lifecycle_" + request.param), BUILDS[request.param], "driver")
    return lambda cfg, B, frames, answers: _run_driver(exe, cfg, B, frames, answers)


def _expect(cfg, B, frames, seed=7, scripts=None, host_frames=None):
    """the host life cycle over the double -> (per frame the rows the driver prints, the double's answers, runner). frames: what
    the driver gets; host_frames (default: the same): what the host life cycle gets - the pixels of both are looked up in
    `frames`, where every track has its own."""
    be = _RecordingBackend(cfg, B, seed)
    runner = sequence.SequenceRunner(be, cfg, B)
    out, answers = [], []
    dropped = np.zeros(B, dtype=int); gadd = np.zeros(B, dtype=int); padd = np.zeros(B, dtype=int); outl = 0; created = np.zeros(B, dtype=int)
    for t, tracks in enumerate(frames):
        be.script = None if scripts is None else scripts.get(t, {})
        runner.frame(None, (host_frames or frames)[t])
        fr = be.cur
        answers.append(fr)

        def track_of(b, px):
            meas = tracks[b][1]
            k = [k for k in range(len(meas)) if meas[k, 0] == px[0] and meas[k, 1] == px[1]]
            assert len(k) == 1          # the scripts give every track of a frame its own pixel
            return k[0]
        first, post = fr["edits"]
        row = dict(P=[o for o in first if o[1] not in POOL_OPS], Q=[o for o in first if o[1] in POOL_OPS], R=post)
        row["X"] = [(b, e, track_of(b, fr["xpp"][b, e])) for b in range(B) for e in range(cfg.pool_max) if not np.isnan(fr["xpp"][b, e, 0])]
        row["T"] = [(b, j, track_of(b, fr["xp"][b, j])) for b in range(B) for j in range(cfg.n_features) if not np.isnan(fr["xp"][b, j, 0])]
        row["A"] = [(b, int(a)) for b, a in enumerate(fr["slots"] if fr["slots"] is not None else []) if a >= 0]
        row["N"] = [(int(r["b"]), int(r["entry"]), int(r["anchor"]), track_of(int(r["b"]), r["xp"])) for r in fr["recs"]]
        outl += fr["outliers"]
        for o in row["P"]:
            dropped[o[0]] += o[1] == L.EDIT_REMOVE_FEATURE
        for o in row["Q"]:
            gadd[o[0]] += o[1] == L.EDIT_ADD_GROUP_ANCHOR
        for b, _ in row["A"]:
            created[b] += 1
        for r in row["N"]:
            padd[r[0]] += 1
        row["B"] = [(tuple(bk.feat_id), tuple(bk.feat_ref), tuple(bk.group_refs), tuple(pb.ent_id), tuple(pb.ent_anchor),
                     tuple(born if fid >= 0 else 0 for born, fid in zip(pb.ent_born, pb.ent_id)),
                     tuple(int(u) for u in pb.anc_used), tuple(pb.anc_life), tuple(pb.anc_link))
                    for bk, pb in zip(runner.books, runner.pools)]
        row["totals"] = dict(updates=runner.n_updates, rejected=runner.n_rejected, dropped=int(dropped.sum()),
                             admitted=len(runner.admitted), groups_added=int(gadd.sum()), pool_added=int(padd.sum()),
                             pool_dropped=runner.n_pool_dropped, pool_outliers=outl, anchors_created=int(created.sum()),
                             anchors_freed=int(created.sum()) - sum(int(sum(pb.anc_used)) for pb in runner.pools),
                             admit_steps=sum(a[3] for a in runner.admitted))
        out.append(row)
    return out, answers, runner


COUNTERS = ("updates", "rejected", "dropped", "admitted", "groups_added", "pool_added", "pool_dropped", "pool_outliers",
            "anchors_created", "anchors_freed", "admit_steps")


def _compare(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        for key in "PXQTRANB":
            assert g[key] == w[key], (t, key, g[key], w[key])
        tot = {k: sum(c[1 + i] for c in g["C"]) for i, k in enumerate(COUNTERS)}
        assert tot == w["totals"], (t, tot, w["totals"])


def _tracks(ids, rng):
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    # every track its own pixel, so that the track behind a pixel can be read back
    u = rng.permutation(640)[:n] + rng.uniform(0, 0.5, n)
    return ids, np.column_stack([u, rng.uniform(0, 480, n), np.full(n, 2.0)])


def _fuzz_frames(B, T, rng, n_ids=24, p_toggle=0.12):
    """track sets that change slowly - every id of a filter's own range appears or vanishes with probability p_toggle per
    frame - so that features live long enough for all group slots to fill; now and then a filter loses all its tracks"""
    seen = rng.uniform(size=(B, n_ids)) < 0.3
    frames = []
    for t in range(T):
        seen ^= rng.uniform(size=seen.shape) < p_toggle
        tracks = []
        for b in range(B):
            ids = 100 * b + np.nonzero(seen[b])[0] if rng.uniform() > 0.03 else []
            tracks.append(_tracks(ids, rng))
        frames.append(tracks)
    return frames


def _case(driver, cfg, id_lists, scripts, host_id_lists=None):
    """one filter through scripted frames -> (want rows, runner) after the comparison with the driver"""
    rng = np.random.default_rng(5)
    frames = [[_tracks(ids, rng)] for ids in id_lists]
    host_frames = None
    if host_id_lists is not None:    # the host gets a subset of the frame's tracks, with the full frame's pixels
        host_frames = []
        for fr, keep in zip(frames, host_id_lists):
            ids, meas = fr[0]
            host_frames.append([(ids[keep], meas[keep])])
    want, answers, runner = _expect(cfg, 1, frames, scripts={t: s for t, s in enumerate(scripts)}, host_frames=host_frames)
    _compare(driver(cfg, 1, frames, answers), want)
    return want, runner


def test_header_is_plain_cxx_for_a_host_compiler():
    """HIP's header only under hipcc (through lifecycle_device.h), no project header but lifecycle_device.h"""
    text = open(os.path.join(CSRC, "pool_lifecycle_device.h")).read().split("#pragma once")[1]
    assert [ln for ln in text.splitlines() if ln.startswith("#include")] == ['#include "lifecycle_device.h"']
    assert "hip/" not in text and "__global__" not in text


def test_fuzz_decisions_equal_the_host_life_cycle(driver):
    """random track sets over small tables (6 feature slots, 3 group slots, 8 pool entries, 3 anchors) so that every table
    fills: tracks appear, vanish and come back; the step kills 10 % of the entries and names random candidates in random order;
    15 % of the features are rejected"""
    cfg = _cfg()
    B = 3
    rng = np.random.default_rng(11)
    frames = _fuzz_frames(B, 150, rng)
    want, answers, runner = _expect(cfg, B, frames)
    tot = want[-1]["totals"]
    # the fuzz reaches what it is for: every table was full at some point and every kind of event occurred
    assert tot["pool_dropped"] > 20 and tot["admitted"] > 50 and tot["rejected"] > 20 and tot["pool_outliers"] > 20
    assert tot["anchors_freed"] > 10 and tot["dropped"] > 20 and tot["groups_added"] > 20
    assert any(all(f >= 0 for f in w["B"][b][0]) for w in want for b in range(B))            # no free feature slot
    assert any(all(r >= 0 for r in w["B"][b][2]) for w in want for b in range(B))            # no free group slot
    assert any(all(e >= 0 for e in w["B"][b][3]) for w in want for b in range(B))            # no free entry
    assert any(all(u for u in w["B"][b][6]) for w in want for b in range(B))                 # no free anchor
    _compare(driver(cfg, B, frames, answers), want)


def test_no_free_group_slot_skips_the_entry_and_the_walk_goes_on(driver):
    """one group slot, taken by anchor 0's group; the best candidate hangs on the unlinked anchor 1 and waits, the next one
    hangs on anchor 0 and is admitted all the same"""
    cfg = _cfg(n_groups=1)
    want, _ = _case(driver, cfg, [[1, 2], [1, 2, 3], [1, 2, 3]],
                    [dict(order={0: []}), dict(order={0: [0]}), dict(order={0: [0, 1]})])
    assert want[1]["Q"] == [(0, L.EDIT_ADD_GROUP_ANCHOR, 0, 0, 0), (0, L.EDIT_ADMIT_POOL, 0, 0, 0)]
    assert want[1]["N"] == [(0, 0, 1, 2)]                                # track 3 takes the entry just freed, on anchor 1
    assert want[2]["Q"] == [(0, L.EDIT_ADMIT_POOL, 1, 1, 1)]             # entry 0 skipped, entry 1 admitted
    assert want[2]["B"][0][3][0] == 3                                    # track 3 still waits in entry 0


def test_no_free_anchor_drops_all_new_tracks(driver):
    cfg = _cfg(anchor_max=1)
    want, runner = _case(driver, cfg, [[1], [1, 2, 3]], [dict(order={0: []}), dict(order={0: []})])
    assert want[1]["A"] == [] and want[1]["N"] == [] and runner.n_pool_dropped == 2


def test_more_new_tracks_than_free_entries(driver):
    cfg = _cfg(pool_max=2)
    want, runner = _case(driver, cfg, [[5, 3, 4, 9], [3, 4, 5, 9]], [dict(order={0: []})] * 2)
    assert want[0]["N"] == [(0, 0, 0, 1), (0, 1, 0, 2)] and runner.n_pool_dropped == 2 + 2    # ids 3, 4 enter; 5, 9 twice dropped
    assert want[1]["A"] == [(0, 1)] and want[1]["N"] == []               # the anchor is created even with no entry to give


def test_an_entry_freed_and_taken_again_in_the_same_frame(driver):
    """entry 0's track vanishes: freed before the step, taken by a new track after the update; entry 1 is killed by the step
    and its own track, new again, takes it back"""
    cfg = _cfg()
    want, _ = _case(driver, cfg, [[1, 2], [2, 3], [2, 3]], [dict(order={0: []}), dict(order={0: []}), dict(kill={(0, 1)}, order={0: []})])
    assert want[1]["X"] == [(0, 1, 0)] and want[1]["N"] == [(0, 0, 1, 1)]
    assert want[2]["N"] == [(0, 1, 2, 0)] and want[2]["totals"]["pool_outliers"] == 1


def test_group_removed_under_live_entries_freezes_the_anchor_which_admits_into_a_new_slot(driver):
    """anchor 0's group enters slot 0 with track 1; track 1 vanishes, the group leaves and anchor 0 is unlinked while entry 1
    still hangs on it; entry 1 is then admitted - in the frame of the removal (one op list) and, in a second run, a frame
    later - through ADD_GROUP_ANCHOR of the frozen anchor"""
    cfg = _cfg()
    want, _ = _case(driver, cfg, [[1, 2], [1, 2], [2]], [dict(order={0: []}), dict(order={0: [0]}), dict(order={0: [1]})])
    assert want[2]["P"] == [(0, L.EDIT_REMOVE_FEATURE, 0, 0, 0), (0, L.EDIT_REMOVE_GROUP, 0, 0, 0)]
    assert want[2]["Q"] == [(0, L.EDIT_ADD_GROUP_ANCHOR, 0, 0, 0), (0, L.EDIT_ADMIT_POOL, 0, 0, 1)]
    want, _ = _case(driver, cfg, [[1, 2], [1, 2], [2], [2]],
                    [dict(order={0: []}), dict(order={0: [0]}), dict(order={0: []}), dict(order={0: [1]})])
    assert want[2]["B"][0][8][0] == -1 and want[2]["B"][0][4][1] == 0    # unlinked, entry 1 still on anchor 0
    assert want[3]["Q"] == [(0, L.EDIT_ADD_GROUP_ANCHOR, 0, 0, 0), (0, L.EDIT_ADMIT_POOL, 0, 0, 1)]


def test_anchor_expires_after_max_group_lifetime_and_not_a_frame_earlier(driver):
    cfg = _cfg(max_group_lifetime=2)
    want, _ = _case(driver, cfg, [[1], [], [], [], []], [dict(order={0: []})] * 5)
    assert [w["B"][0][6][0] for w in want] == [1, 1, 1, 0, 0] and [w["B"][0][7][0] for w in want[:4]] == [0, 1, 2, 3]
    assert [w["totals"]["anchors_freed"] for w in want] == [0, 0, 0, 1, 1]


def test_a_rejected_features_track_returns_to_the_pool_in_the_same_frame(driver):
    cfg = _cfg()
    want, _ = _case(driver, cfg, [[1, 2], [1, 2], [1, 2]],
                    [dict(order={0: []}), dict(order={0: [0, 1]}), dict(order={0: []}, reject={(0, 0)})])
    assert want[2]["R"] == [(0, L.EDIT_REMOVE_FEATURE, 0, 0, 0)] and want[2]["N"] == [(0, 0, 1, 0)]
    assert want[2]["B"][0][0][:2] == (-1, 2) and want[2]["B"][0][3][0] == 1


def test_repeated_ids_in_the_state_in_the_pool_and_among_new_tracks(driver):
    """of a repeated id the last occurrence feeds a feature slot or a pool entry; among new tracks the first takes part and the
    others are ignored: the host life cycle, which fails on such a frame, gets it with the later duplicates removed"""
    cfg = _cfg()
    id_lists = [[1, 2], [1, 2, 2, 1],            # 1: both ids twice while in the pool; entry 0 is admitted
                [2, 1, 1, 2, 1],                 # 2: 1 is in the state, 2 in the pool
                [7, 1, 7, 2, 6, 7, 6]]           # 3: 7 three times and 6 twice among the new tracks
    keep = [[0, 1], [0, 1, 2, 3], [0, 1, 2, 3, 4], [0, 1, 3, 4]]
    want, _ = _case(driver, cfg, id_lists, [dict(order={0: []}), dict(order={0: [0]}), dict(order={0: []}), dict(order={0: []})],
                    host_id_lists=keep)
    assert want[1]["X"] == [(0, 0, 3), (0, 1, 2)] and want[1]["T"] == [(0, 0, 3)]
    assert want[2]["T"] == [(0, 0, 4)] and want[2]["X"] == [(0, 1, 3)]
    assert want[3]["N"] == [(0, 0, 1, 4), (0, 2, 1, 0)]                  # id 6 (track 4) before id 7 (track 0): ascending id


def test_pool_lifecycle_option_checks():
    """the new switch raises before anything is allocated; the immediate mode's switch is unchanged"""
    C = sequence.SequenceConfig
    assert C().pool_lifecycle == "host"
    for kw in (dict(pool_lifecycle="device"), dict(pool_lifecycle="device", feature_init="immediate"),
               dict(pool_lifecycle="gpu", feature_init="subfilter"),
               dict(pool_lifecycle="device", feature_init="subfilter", lifecycle="device"),
               dict(pool_lifecycle="device", feature_init="subfilter", tracks_max=L.LIFE_MAX_TRACKS + 1),
               dict(lifecycle="device", feature_init="subfilter")):
        with pytest.raises(ValueError):
            sequence.SequenceRunner(None, C(**kw), 1)
        with pytest.raises(ValueError):
            sequence.HipBackend(C(**kw), 1, None, None)
    sequence.check_lifecycle(C(pool_lifecycle="device", feature_init="subfilter"))
    assert sequence.SequenceRunner(None, C(pool_lifecycle="device", feature_init="subfilter"), 1).device_pool_lifecycle
