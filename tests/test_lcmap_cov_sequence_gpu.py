"""GPU: sequences with the landmark map's two options (SequenceConfig.lc_point_cov, lc_revisit_gap) on both host life cycles.
The script is tests/test_lcmap_sequence_gpu.py's: B = 2 sequences of 16 frames, six of twelve shown points hidden in frames
LEAVE .. RETURN - 1 and shown again under new track ids with their old keys."""
import numpy as np
import pytest

import test_lcmap_sequence_gpu as S
from xivo_amd import sequence

pytestmark = pytest.mark.gpu
B, N_FRAMES = S.B, S.N_FRAMES
GAP = 25            # longer than the run: a returning point closes once


def _run(cycle, extra, log=None, explicit_off=False):
    cfg = sequence.SequenceConfig(**S.CYCLES[cycle], **S.SHAPE, **S.LC, **extra)
    sims, frames = S._frames(cfg, True)
    be = sequence.HipBackend(cfg, B, sequence.initial_poses(cfg, sims), np.repeat(cfg.P_init()[None], B, axis=0))
    out = dict(P=[], poses=[], cfg=cfg, sims=sims)
    try:
        if explicit_off:
            be.ctx.lcmap_cov_config(point_cov=False, revisit_gap=0)
        if log is not None:
            be.ctx = S._Recorder(be.ctx, log)
        runner = sequence.SequenceRunner(be, cfg, B)
        for t, (rec, ft, fk) in enumerate(frames):
            if log is not None:
                log.append(("frame", t, None))
            runner.frame(rec, ft, fk)
            out["P"].append(be.covariance()); out["poses"].append(be.scene()[0])
        out["stats"], out["cov_stats"] = be.lcmap_stats(), be.lcmap_cov_stats()
    finally:
        be.close()
    return out


@pytest.mark.parametrize("cycle", list(S.CYCLES))
def test_options_at_their_defaults_change_no_bit(built, cycle):
    a, b = _run(cycle, {}), _run(cycle, dict(lc_point_cov=False, lc_revisit_gap=0), explicit_off=True)
    assert (a["stats"]["closed_frames"] >= 1).all() and a["stats"].tobytes() == b["stats"].tobytes()
    assert not a["cov_stats"]["resting"].any() and not a["cov_stats"]["rested_frames"].any()
    for t in range(N_FRAMES):
        assert a["P"][t].tobytes() == b["P"][t].tobytes() and a["poses"][t].tobytes() == b["poses"][t].tobytes(), t


@pytest.mark.parametrize("cycle", list(S.CYCLES))
def test_both_options_close_the_loop_once_and_the_runner_is_its_context_calls(built, cycle):
    log = []
    on = _run(cycle, dict(lc_point_cov=True, lc_revisit_gap=GAP), log)
    st, cst = on["stats"], on["cov_stats"]
    print(cycle, {k: st[k].tolist() for k in st.dtype.names}, {k: cst[k].tolist() for k in cst.dtype.names})
    assert st["added"].tolist() == [6] * B and (st["closed_frames"] >= 1).all()      # returning points close the loop
    assert (cst["resting"] > 0).all() and not cst["bad_cov"].any()                   # ... and then rest while they stay in view
    off = _run(cycle, {})
    assert any(not np.array_equal(on["P"][t], off["P"][t]) for t in range(N_FRAMES))
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
        assert be.ctx.lcmap_cov_stats(0, B).tobytes() == cst.tobytes()
    finally:
        be.close()
    for t in range(N_FRAMES):
        assert P[t].tobytes() == on["P"][t].tobytes() and poses[t].tobytes() == on["poses"][t].tobytes(), t
