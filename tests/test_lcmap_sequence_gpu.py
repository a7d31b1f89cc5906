"""GPU: sequences with loop_closure on both host life cycles (SequenceRunner.frame / _frame_subfilter -> xivo_hip_lcmap_*).

B = 2 sequences of 16 frames, scripted on top of the point-cloud simulator's tracks: twelve central points of frame 0 are
shown from frame 0 on; six of them are hidden in frames LEAVE .. RETURN - 1 and shown again from frame RETURN on under new
track ids - what the tracker makes of a point that comes back. Their keys are the script's to choose:
  (a) keys that never repeat (the track id): loop closure on must change nothing, bit for bit;
  (b) the old keys: the six features go to the map when they leave and close the loop once they are back in the state."""
import copy

import numpy as np
import pytest

from test_pool_lifecycle_gpu import QUICK, _sim_frames
from xivo_amd import pcw, sequence

pytestmark = pytest.mark.gpu
B, N_FRAMES, LEAVE, RETURN, NEW_ID = 2, 16, 7, 9, 500000
SHAPE = dict(n_groups=4, n_features=12)
CYCLES = {"immediate": dict(feature_init="immediate"),
          "subfilter": dict(**QUICK, pool_max=16, anchor_max=6, remove_outlier_counter=1e9)}
LC = dict(loop_closure=True, lc_map_max=8, lc_max=8, lc_min_matches=5)
# the Context calls that change resident state or staged rows: what a replay by hand has to repeat
MUTATING = ("propagate", "edit_batch", "set_pixels", "filter_update", "absorb_error", "update_joseph", "lcmap_add", "lcmap_close",
            "pool_step", "pool_anchor", "pool_add_ex")


class _Recorder:
    """a Context that writes down every state-changing call (arguments copied) before passing it on"""

    def __init__(self, ctx, log):
        self.__dict__["_ctx"], self.__dict__["_log"] = ctx, log

    def __getattr__(self, name):
        fn = getattr(self._ctx, name)
        if name not in MUTATING:
            return fn

        def call(*a, **kw):
            self._log.append((name, copy.deepcopy(a), copy.deepcopy(kw)))
            return fn(*a, **kw)
        return call

    def __setattr__(self, name, v):
        setattr(self._ctx, name, v)


def _frames(cfg, repeat_keys):
    """-> per frame (imu records, tracks, keys) of the script"""
    sims = [pcw.TrajectorySim("trefoil" if b % 2 else "lissajous", seed=400 + b) for b in range(B)]
    frames_of = _sim_frames(cfg, B, 300)
    out = []
    for t in range(N_FRAMES):
        rec, tracks = frames_of(t, sims)
        if t == 0:
            shown = []
            for ids, meas in tracks:
                c = [int(i) for i, m in sorted(zip(ids, meas), key=lambda v: v[0])
                     if abs(m[0] - cfg.cam["cx"]) < 160 and abs(m[1] - cfg.cam["cy"]) < 120]
                assert len(c) >= 12
                shown.append(c[:12])
        ft, fk = [], []
        for b, (ids, meas) in enumerate(tracks):
            pos = {int(i): k for k, i in enumerate(ids)}
            assert all(i in pos for i in shown[b])                       # (the script's points stay in view for the whole run)
            rid, rows, keys = [], [], []
            for n, i in enumerate(shown[b]):
                leaves = n < 6
                if leaves and LEAVE <= t < RETURN:
                    continue
                back = leaves and t >= RETURN
                rid.append(i + NEW_ID if back else i)
                keys.append(i if (repeat_keys or not back) else i + NEW_ID)
                rows.append(meas[pos[i]])
            ft.append((np.array(rid, dtype=np.int64), np.array(rows, dtype=float))); fk.append(np.array(keys, dtype=np.int64))
        out.append((rec, ft, fk))
    return sims, out


def _run(cycle, lc, repeat_keys, log=None):
    cfg = sequence.SequenceConfig(**CYCLES[cycle], **SHAPE, **(LC if lc else {}))
    sims, frames = _frames(cfg, repeat_keys)
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    out = dict(P=[], poses=[], cfg=cfg, sims=sims)
    try:
        if log is not None:
            be.ctx = _Recorder(be.ctx, log)
        runner = sequence.SequenceRunner(be, cfg, B)
        for t, (rec, ft, fk) in enumerate(frames):
            if log is not None:
                log.append(("frame", t, None))
            runner.frame(rec, ft, fk if lc else None)
            out["P"].append(be.covariance()); out["poses"].append(be.scene()[0])
        if lc:
            out["stats"] = be.lcmap_stats()
            out["map"] = be.ctx.lcmap_get(0, B)
    finally:
        be.close()
    return out


@pytest.mark.parametrize("cycle", list(CYCLES))
def test_keys_that_never_repeat_change_nothing(built, cycle):
    off, on = _run(cycle, False, False), _run(cycle, True, False)
    st = on["stats"]
    print(cycle, {k: st[k].tolist() for k in st.dtype.names})
    assert not st["matched"].any() and not st["closed_frames"].any() and st["queries"].all()
    for t in range(N_FRAMES):
        assert on["P"][t].tobytes() == off["P"][t].tobytes(), t
        assert on["poses"][t].tobytes() == off["poses"][t].tobytes(), t


@pytest.mark.parametrize("cycle", list(CYCLES))
def test_points_that_return_close_the_loop_and_the_runner_is_its_context_calls(built, cycle):
    log = []
    on = _run(cycle, True, True, log)
    st = on["stats"]
    print(cycle, {k: st[k].tolist() for k in st.dtype.names})
    assert st["added"].tolist() == [6] * B and (st["closed_frames"] >= 1).all()
    assert (on["map"][1] == 6).all() and not st["dup"].any() and not st["full"].any()
    # the order of a frame: the map takes the leaving features before the edit that removes them; the close call comes right
    # behind the frame's update and AbsorbError, and the second update and AbsorbError right behind a close call
    names = [c[0] for c in log]
    i_add = names.index("lcmap_add")
    assert names[i_add + 1:].index("edit_batch") < names[i_add + 1:].index("filter_update")
    removed = log[i_add + 1 + names[i_add + 1:].index("edit_batch")][1][1]
    assert int((removed["kind"] == sequence.L.EDIT_REMOVE_FEATURE).sum()) == 6 * B and len(log[i_add][1][0]) == 6 * B
    for i, n in enumerate(names):
        if n == "lcmap_close":
            assert names[i - 2:i] == ["filter_update", "absorb_error"]
    closes = [i for i, n in enumerate(names) if n == "lcmap_close" and names[i + 1:i + 3] == ["update_joseph", "absorb_error"]]
    assert len(closes) >= int(st["closed_frames"].max())
    # the same frames by hand: a fresh context, the recorded calls in order - P and the poses of every frame, bit for bit
    cfg, sims = on["cfg"], on["sims"]
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    try:
        P, poses = [], []
        for name, a, kw in log[1:] + [("frame", N_FRAMES, None)]:
            if name == "frame":
                P.append(be.ctx.download_P()); poses.append(be.ctx.get_scene()[0])
            else:
                getattr(be.ctx, name)(*a, **kw)
    finally:
        be.close()
    for t in range(N_FRAMES):
        assert P[t].tobytes() == on["P"][t].tobytes() and poses[t].tobytes() == on["poses"][t].tobytes(), t
