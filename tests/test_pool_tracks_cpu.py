"""CPU-only: the upper layers of the "subfilter" device life cycle on tracks the device produces. check_lifecycle takes
track_source="device" (and imu_source="device" on top) with either device life cycle and with neither still raises;
SequenceRunner.frame_world / frame_resident over the recording double of tests/test_pool_lifecycle_cpu.py issue the produced-tracks
calls of the pool life cycle in order, with CandidateStrict turning on at strict_criteria_timesteps; the new entry point is
declared in the public header and bound in xivo_amd/lib.py. What the calls compute is checked on the GPU
(tests/test_pool_tracks_gpu.py)."""
import os
import re

import numpy as np
import pytest

from test_pool_lifecycle_cpu import _RecordingBackend, _cfg
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _life(**kw):
    base = dict(feature_init="subfilter", pool_lifecycle="device", tracks_max=300, npts=300, track_source="device")
    base.update(kw)
    return sequence.SequenceConfig(**base)


def test_check_lifecycle_takes_device_tracks_with_either_device_life_cycle():
    sequence.check_lifecycle(_life())
    sequence.check_lifecycle(_life(imu_source="device"))
    sequence.check_lifecycle(sequence.SequenceConfig(lifecycle="device", track_source="device", npts=300, tracks_max=300))
    sequence.check_lifecycle(sequence.SequenceConfig(lifecycle="device", track_source="device", imu_source="device", npts=300,
                                                     tracks_max=300))


@pytest.mark.parametrize("kw", [dict(track_source="device", npts=300, tracks_max=300),
                                dict(feature_init="subfilter", track_source="device", npts=300, tracks_max=300),
                                dict(feature_init="subfilter", pool_lifecycle="host", track_source="device", imu_source="device",
                                     npts=300, tracks_max=300)],
                         ids=["immediate-host", "subfilter-host", "subfilter-host-imu"])
def test_check_lifecycle_still_refuses_device_tracks_with_neither_device_life_cycle(kw):
    with pytest.raises(ValueError, match="track_source"):
        sequence.check_lifecycle(sequence.SequenceConfig(**kw))


@pytest.mark.parametrize("kw", [dict(feature_init="subfilter", pool_lifecycle="device", tracks_max=300, imu_source="device"),
                                dict(lifecycle="device", imu_source="device")], ids=["pool", "immediate"])
def test_check_lifecycle_still_refuses_device_imu_without_device_tracks(kw):
    with pytest.raises(ValueError, match="imu_source"):
        sequence.check_lifecycle(sequence.SequenceConfig(**kw))


def test_check_lifecycle_still_bounds_npts_by_tracks_max():
    with pytest.raises(ValueError, match="npts"):
        sequence.check_lifecycle(_life(npts=301))


class _Calls(_RecordingBackend):
    """the recording double with the produced-tracks calls of both device life cycles: every call is noted in order"""

    def __init__(self, cfg, B):
        super().__init__(cfg, B, 0)
        self.calls = []

    def _note(self, name, *a):
        self.calls.append((name,) + a)

    def propagate(self, imu):
        self._note("propagate")

    def make_tracks(self, gsc, noise_px_std, seed, frame):
        self._note("make_tracks", float(noise_px_std), int(seed), int(frame))

    def make_imu(self, k0, n):
        self._note("make_imu", int(k0), int(n))

    def propagate_resident(self):
        self._note("propagate_resident")

    def make_tracks_resident(self, noise_px_std, seed, frame):
        self._note("make_tracks_resident", float(noise_px_std), int(seed), int(frame))

    def pool_life_begin_tracks(self, strict):
        self._note("pool_life_begin_tracks", bool(strict))

    def pool_life_end(self):
        self._note("pool_life_end")

    def life_begin_tracks(self):
        self._note("life_begin_tracks")

    def life_end(self):
        self._note("life_end")

    def update(self, download=True):
        self._note("update", bool(download))
        return None


def test_frame_world_issues_the_pool_life_cycle_on_produced_tracks():
    """make_tracks -> pool_life_begin_tracks(strict) -> update -> pool_life_end, frame after frame; vision_counter counts the
    frames and strict turns on with the frame at which it reaches strict_criteria_timesteps"""
    B = 2
    cfg = _cfg(pool_lifecycle="device", tracks_max=300, npts=300, track_source="device", strict_criteria_timesteps=3)
    be = _Calls(cfg, B)
    r = sequence.SequenceRunner(be, cfg, B)
    r.noise_px_std, r.noise_seed = 0.5, 9
    gsc = np.zeros((B, 12))
    for t in range(5):
        be.calls.clear()
        r.frame_world(None if t == 0 else object(), gsc, t)
        want = [("propagate",)] if t else []
        want += [("make_tracks", 0.5, 9, t), ("pool_life_begin_tracks", t + 1 >= 3), ("update", False), ("pool_life_end",)]
        assert be.calls == want, t
        assert r.vision_counter == t + 1


def test_frame_resident_issues_the_pool_life_cycle_on_produced_tracks():
    """make_imu -> propagate_resident (n > 0) -> make_tracks_resident -> pool_life_begin_tracks(strict) -> update -> pool_life_end"""
    B = 2
    cfg = _cfg(pool_lifecycle="device", tracks_max=300, npts=300, track_source="device", imu_source="device",
               strict_criteria_timesteps=2)
    be = _Calls(cfg, B)
    r = sequence.SequenceRunner(be, cfg, B)
    r.noise_px_std, r.noise_seed = 1.0, 4
    for t in range(4):
        be.calls.clear()
        k0, n = (16 * (t - 1), 16) if t else (0, 0)
        r.frame_resident(k0, n, t)
        want = [("make_imu", k0, n)] + ([("propagate_resident",)] if n else [])
        want += [("make_tracks_resident", 1.0, 4, t), ("pool_life_begin_tracks", t + 1 >= 2), ("update", False), ("pool_life_end",)]
        assert be.calls == want, t
    assert r.vision_counter == 4


def test_the_immediate_life_cycle_keeps_its_pair():
    """frame_world / frame_resident with lifecycle="device" call life_begin_tracks / life_end as before and count no frames"""
    B = 2
    cfg = sequence.SequenceConfig(lifecycle="device", track_source="device", imu_source="device", npts=300, tracks_max=300,
                                  n_features=6, n_groups=3)
    be = _Calls(cfg, B)
    r = sequence.SequenceRunner(be, cfg, B)
    r.frame_world(None, np.zeros((B, 12)), 0)
    r.frame_resident(0, 16, 1)
    assert [c[0] for c in be.calls] == ["make_tracks", "life_begin_tracks", "update", "life_end", "make_imu", "propagate_resident",
                                        "make_tracks_resident", "life_begin_tracks", "update", "life_end"]
    assert r.vision_counter == 0


def test_frame_world_needs_device_tracks_and_frame_resident_the_device_imu():
    cfg = _cfg(pool_lifecycle="device", tracks_max=300)
    r = sequence.SequenceRunner(_Calls(cfg, 1), cfg, 1)
    with pytest.raises(ValueError, match="track_source"):
        r.frame_world(None, np.zeros((1, 12)), 0)
    with pytest.raises(ValueError, match="imu_source"):
        r.frame_resident(0, 0, 0)
    assert r.vision_counter == 0


def test_the_new_entry_point_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "xivo_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+xivo_hip_pool_life_begin_tracks\(xivo_hip_ctx\*\s*ctx,\s*int B,\s*int F,\s*int strict\);", header)
    with open(os.path.join(ROOT, "xivo_amd", "lib.py")) as f:
        binding = f.read()
    assert '"xivo_hip_pool_life_begin_tracks": [C.c_void_p, C.c_int, C.c_int, C.c_int]' in binding
    assert "def pool_life_begin_tracks(self, F, strict=False, B=None)" in binding
    assert hasattr(sequence.HipBackend, "pool_life_begin_tracks")
