"""CPU-only: the decisions of the device life cycle (xivo_amd/csrc/lifecycle_device.h) under a host compiler, against the host
life cycle. tests/lifecycle_driver.cpp is compiled with g++ against the header alone and replays a scripted run - per frame the
tracks of each filter and the gating outcome per slot - through the functions the kernels call, in the kernels' order. The
expectation is SequenceRunner.frame with lifecycle="host" over a recording backend double: the op sequences (kind, i0, i1, i2),
the slot -> track association and the books must be identical frame by frame.

What this does not cover: the kernel reaches the slot -> track association with one thread per track and an LDS maximum per
slot over life_slot_holds; the driver uses the serial form of the same rule, life_track_of_slot. That the parallel form picks
the last occurrence of a repeated id is checked on the GPU only (the duplicated id of tests/test_lifecycle_gpu.py).
Everything else the driver calls is what the kernels call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")


class _RecordingBackend:
    """Backend double: keeps a shadow of which slots are in the state, records per frame the op lists, the pixels and the
    gating outcome it answered `update` with - random (15 % rejected), or the slots a script asked to reject."""

    def __init__(self, cfg, B, seed):
        self.cfg, self.B = cfg, B
        self.rng = np.random.default_rng(seed)
        self.sind = np.full((B, cfg.n_features), -1)
        self.frames = []
        self.reject = None           # scripted: [B, F] bool, the slots the next update rejects
        self._cur = None

    def propagate(self, imu):
        pass

    def edit(self, ops):
        assert (np.diff(ops["b"]) >= 0).all() if len(ops) else True
        rec = []
        for o in ops:
            b, k, i0, i1, i2 = int(o["b"]), int(o["kind"]), int(o["i0"]), int(o["i1"]), int(o["i2"])
            rec.append((b, k, i0, i1, i2))
            if k == L.EDIT_ADD_FEATURE:
                assert self.sind[b, i0] < 0
                self.sind[b, i0] = i1
            elif k == L.EDIT_REMOVE_FEATURE:
                assert self.sind[b, i0] >= 0
                self.sind[b, i0] = -1
            else:
                assert k in (L.EDIT_ADD_GROUP, L.EDIT_REMOVE_GROUP)
        if self._cur is None:
            self._cur = dict(pre=rec)
        else:
            self._cur["post"] = rec
            self.frames.append(self._cur)
            self._cur = None

    def set_pixels(self, xp):
        self._cur["xp"] = xp.copy()

    def update(self):
        present = self.sind >= 0
        if self.reject is not None:
            mask = present & ~self.reject
            self.reject = None
        else:
            mask = present & (self.rng.uniform(size=present.shape) > 0.15)
        self._cur["mask"] = mask.copy()
        return mask


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/lifecycle_driver.cpp"
    exe = str(tmp_path_factory.mktemp("lifecycle") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(ROOT, "tests", "lifecycle_driver.cpp"),
                    "-o", exe], check=True)

    def run(cfg, B, frames, masks):
        """frames: per frame the tracks [(ids, meas)] * B; masks: per frame [B, F] -> per frame dict(T, P, Q, B)"""
        lines = ["%d %d %d %s %s %d %d" % (cfg.n_features, cfg.n_groups, cfg.min_new_features, float(cfg.min_depth).hex(),
                                            float(cfg.max_depth).hex(), B, len(frames))]
        for tracks, mask in zip(frames, masks):
            for b in range(B):
                ids, meas = tracks[b]
                lines.append(str(len(ids)))
                lines += ["%d %s" % (int(i), float(z).hex()) for i, z in zip(ids, meas[:, 2])]
                lines.append(" ".join(str(int(v)) for v in mask[b]))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
        res, cur = [], dict(T=[], P=[], Q=[], B=[])
        for ln in out.splitlines():
            if ln == "E":
                res.append(cur); cur = dict(T=[], P=[], Q=[], B=[])
            elif ln[0] == "B":
                cur["B"].append(tuple(tuple(int(v) for v in part.split()) for part in ln.split("|")[1:]))
            else:
                cur[ln[0]].append(tuple(int(v) for v in ln.split()[1:]))
        assert len(res) == len(frames)
        return res
    return run


def _expect(cfg, B, frames, seed=7, rejects=None):
    """the host life cycle over the double -> (per frame dict(T, P, Q, B) as the driver prints them, masks, runner)"""
    be = _RecordingBackend(cfg, B, seed)
    runner = sequence.SequenceRunner(be, cfg, B)
    out = []
    for t, tracks in enumerate(frames):
        if rejects is not None:
            rej = np.zeros((B, cfg.n_features), dtype=bool)
            for b, j in rejects.get(t, ()):
                rej[b, j] = True
            be.reject = rej
        runner.frame(None, tracks)
        fr = be.frames[-1]
        assoc = []
        for b in range(B):
            ids, meas = tracks[b]
            for j in range(cfg.n_features):
                if not np.isnan(fr["xp"][b, j, 0]):
                    k = [k for k in range(len(ids)) if meas[k, 0] == fr["xp"][b, j, 0] and meas[k, 1] == fr["xp"][b, j, 1]]
                    assert len(k) == 1          # the scripts give every track of a frame its own pixel
                    assoc.append((b, j, k[0]))
        books = [(tuple(bk.feat_id), tuple(bk.feat_ref), tuple(bk.group_refs)) for bk in runner.books]
        out.append(dict(T=assoc, P=fr["pre"], Q=fr["post"], B=books))
    return out, [fr["mask"] for fr in be.frames], runner


def _compare(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        for key in ("T", "P", "Q", "B"):
            assert g[key] == w[key], (t, key, g[key], w[key])


def _tracks(ids, depths, rng):
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    # every track its own pixel, so that the slot -> track association can be read back from the pixels
    u = rng.permutation(640)[:n] + rng.uniform(0, 0.5, n)
    return ids, np.column_stack([u, rng.uniform(0, 480, n), np.asarray(depths, dtype=float)])


def test_header_is_plain_cxx_for_a_host_compiler():
    """HIP's header only under hipcc, no header of the project: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "lifecycle_device.h")).read().split("#pragma once")[1]
    assert '#include "' not in text
    assert text.count("hip/") == 1 and text.index("#if defined(__HIPCC__)") < text.index("hip/") < text.index("#else")


def test_fuzz_decisions_equal_the_host_life_cycle(driver):
    """the fuzz of test_life_cycle_fuzz_against_a_shadow_of_the_resident_slots: random track sets (tracks appear, vanish and
    come back, depths in and out of range), 15 % random rejections"""
    cfg = sequence.SequenceConfig(n_groups=4, n_features=9, min_new_features=2)
    B = 5
    rng = np.random.default_rng(11)
    pool = [np.arange(100 * b, 100 * b + 40) for b in range(B)]
    frames = []
    for _ in range(120):
        tracks = []
        for b in range(B):
            ids = np.sort(rng.choice(pool[b], size=int(rng.integers(0, 25)), replace=False))
            tracks.append(_tracks(ids, rng.uniform(0.01, 14.0, size=len(ids)), rng))
        frames.append(tracks)
    want, masks, runner = _expect(cfg, B, frames)
    assert runner.n_rejected > 100 and sum(len(w["Q"]) + len(w["P"]) for w in want) > 2000
    _compare(driver(cfg, B, frames, masks), want)


def test_scripted_edge_cases_equal_the_host_life_cycle(driver):
    """one filter through: no tracks at all; ids above 2^32; depth exactly at either bound; more candidates than slots; all
    slots full; fewer free slots than min_new_features with a non-empty state; a rejected feature re-admitted in the same
    frame, and into a group slot freed in that frame; fewer candidates than slots; no free group; a duplicated id"""
    cfg = sequence.SequenceConfig(n_groups=4, n_features=9, min_new_features=2)
    rng = np.random.default_rng(3)
    base = 1 << 33
    first = [base + i for i in range(1, 13)]
    d_first = [cfg.min_depth, cfg.max_depth] + [2.0] * 10      # the two lowest ids sit exactly on the bounds: no candidates
    keep = [base + 3, base + 4]
    frames = [
        [_tracks([], [], rng)],                                  # 0: no tracks, empty state
        [_tracks(first, d_first, rng)],                          # 1: 10 candidates for 9 slots: base+3 .. base+11 enter
        [_tracks(first, d_first, rng)],                          # 2: all slots full
        [_tracks(first, d_first, rng)],                          # 3: slot 3 rejected: 1 free < 2, state not empty
        [_tracks(first, d_first, rng)],                          # 4: slot 5 rejected: 2 free, group 1 takes base+6 and base+8
        [_tracks(first, d_first, rng)],                          # 5: slots 3, 5 rejected: group 1 freed and re-used at once
        [_tracks(keep + [base + 20], [2.0] * 3, rng)],           # 6: most tracks vanish; one candidate for 7 free slots
        [_tracks(keep + [base + 20, base + 21], [2.0] * 4, rng)],            # 7: group 2
        [_tracks(keep + [base + 20, base + 21, base + 22], [2.0] * 5, rng)],  # 8: group 3
        [_tracks(keep + [base + 20, base + 21, base + 22, base + 23], [2.0] * 6, rng)],   # 9: no free group
        [_tracks([base + 3] + keep + [base + 20, base + 21, base + 22, base + 3], [2.0] * 7, rng)],   # 10: base+3 three times
        [_tracks([], [], rng)],                                  # 11: no tracks, full-ish state: everything leaves
    ]
    rejects = {3: [(0, 3)], 4: [(0, 5)], 5: [(0, 3), (0, 5)]}
    for t in range(len(frames)):
        rejects.setdefault(t, [])
    want, masks, runner = _expect(cfg, 1, frames, rejects=rejects)
    # the script reaches what it is written for
    assert want[1]["B"][0][0] == tuple(base + i for i in range(3, 12)) and want[1]["B"][0][2] == (9, -1, -1, -1)
    assert want[2]["Q"] == [] and want[3]["Q"] == [(0, L.EDIT_REMOVE_FEATURE, 3, 0, 0)]
    assert want[4]["Q"][-3:] == [(0, L.EDIT_ADD_GROUP, 1, 0, 0), (0, L.EDIT_ADD_FEATURE, 3, 3, 1), (0, L.EDIT_ADD_FEATURE, 5, 5, 1)]
    assert want[4]["B"][0][0][5] == base + 8                       # rejected in this frame, back in this frame
    assert want[5]["Q"] == [(0, L.EDIT_REMOVE_FEATURE, 3, 0, 0), (0, L.EDIT_REMOVE_FEATURE, 5, 0, 0), (0, L.EDIT_REMOVE_GROUP, 1, 0, 0),
                            (0, L.EDIT_ADD_GROUP, 1, 0, 0), (0, L.EDIT_ADD_FEATURE, 3, 3, 1), (0, L.EDIT_ADD_FEATURE, 5, 5, 1)]
    assert want[6]["Q"] == [(0, L.EDIT_ADD_GROUP, 1, 0, 0), (0, L.EDIT_ADD_FEATURE, 2, 2, 1)]
    assert want[8]["B"][0][2] == (2, 1, 1, 1) and want[9]["Q"] == [] and want[9]["B"] == want[8]["B"]
    assert (0, 0, 6) in want[10]["T"]                              # the last of the three occurrences feeds slot 0
    assert want[11]["B"][0][2] == (-1, -1, -1, -1)
    _compare(driver(cfg, 1, frames, masks), want)


def test_admission_into_an_empty_state_ignores_min_new_features(driver):
    """fewer free slots than min_new_features (10 > the 9 there are): an empty state admits all the same, a non-empty one does
    not"""
    cfg = sequence.SequenceConfig(n_groups=4, n_features=9, min_new_features=10)
    rng = np.random.default_rng(4)
    frames = [[_tracks([7, 5, 6], [1.0] * 3, rng)], [_tracks([7, 5, 6, 8, 9], [1.0] * 5, rng)]]
    want, masks, _ = _expect(cfg, 1, frames, rejects={0: [], 1: []})
    assert want[0]["B"][0][0][:3] == (5, 6, 7) and want[1]["Q"] == [] and want[1]["B"] == want[0]["B"]
    _compare(driver(cfg, 1, frames, masks), want)


def test_device_lifecycle_needs_the_immediate_mode():
    """lifecycle="device" with feature_init="subfilter" is refused before anything is allocated"""
    with pytest.raises(ValueError):
        sequence.SequenceRunner(None, sequence.SequenceConfig(lifecycle="device", feature_init="subfilter"), 1)
    with pytest.raises(ValueError):
        sequence.HipBackend(sequence.SequenceConfig(lifecycle="device", feature_init="subfilter"), 1, None, None)
    with pytest.raises(ValueError):
        sequence.SequenceRunner(None, sequence.SequenceConfig(lifecycle="gpu"), 1)
