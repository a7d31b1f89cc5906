"""GPU: sweep.run_sweep (T = 3 tunings x W = 2 worlds in one context) against three plain runs of cfg_t on the same two worlds
(sweep.run_plain: the same driver, no tuning table), compared by bytes; the per-tuning summary against numpy on the per-filter
arrays; scripts/run_sweep.py end to end."""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

from xivo_amd import sequence, sweep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, W = 3, 2
KW = dict(total_time=8 * 0.04, npts=110, seed=3)           # 8 camera frames; at most 110 tracks a frame
AXES = OrderedDict([("visual_meas_std", [0.5, 1.0, 2.0])])
AXES2 = OrderedDict([("MH_thresh", [2.0, 9.0]), ("Qimu.gyro", [1e-3]), ("initial_std_z", [0.3])])


def _cfg():
    return sequence.SequenceConfig(lifecycle="device", n_groups=4, n_features=8, tracks_max=128)


def _final(out):
    be = out["backend"]
    poses, groups, feats = be.scene()
    fid, fref, grefs = be.life_book()
    return dict(P=be.covariance(), poses=poses, groups=groups, feats=feats, feat_id=fid, feat_ref=fref, group_refs=grefs,
                life_stats=out["life_stats"])


def _logs(out):
    tr = out["trajectory"]
    d = {"traj " + k: tr[k] for k in ("Rsb", "Tsb", "Vsb", "bg", "ba", "status", "cov")}
    d["innovation"] = out["innovation"]["recs"]
    for k in ("ate_aligned", "ate_raw", "rpe_pos", "rpe_rot", "nis_per_dof_seq"):
        d[k] = out[k][None]
    d["nees"] = out["nees"]
    return d


@pytest.fixture(scope="module")
def runs():
    """the sweep and the three plain runs, made once and read by the tests below"""
    cfg = _cfg()
    sw = sweep.run_sweep(cfg, AXES, W, **KW)
    keep = dict(sw=sw, final=_final(sw), logs=_logs(sw), plain=[])
    sw["backend"].close()
    for c in sw["cfgs"]:
        out = sweep.run_plain(c, W, **KW)
        keep["plain"].append((_final(out), _logs(out)))
        out["backend"].close()
    return keep


def test_sweep_equals_plain_runs_final_state(runs):
    assert runs["sw"]["T"] == T and runs["sw"]["W"] == W and runs["sw"]["frames"] == 8
    for k, got in runs["final"].items():
        want = np.concatenate([p[0][k] for p in runs["plain"]])
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    st = runs["final"]["life_stats"]
    assert st["updates"].sum() > 0 and st["admitted"].sum() > 0
    P = runs["final"]["P"]
    assert P[:W].tobytes() != P[2 * W:].tobytes()              # the tunings did part


def test_sweep_equals_plain_runs_logs(runs):
    for k, got in runs["logs"].items():
        want = np.ascontiguousarray(np.concatenate([p[1][k] for p in runs["plain"]], axis=1))     # [frames, filters, ...]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), k
    assert runs["logs"]["innovation"].shape == (8, T * W)


def test_summary_is_the_per_filter_arrays(runs):
    sw = runs["sw"]
    st = sw["innovation"]["stats"]
    assert len(sw["summary"]) == T
    for t, row in enumerate(sw["summary"]):
        s = slice(t * W, (t + 1) * W)
        assert row["ate_aligned_m"] == float(np.median(sw["ate_aligned"][s]))
        assert row["ate_aligned_p90"] == float(np.percentile(sw["ate_aligned"][s], 90))
        assert row["rpe_pos_m"] == float(np.median(sw["rpe_pos"][s])) and row["rpe_rot_m"] == float(np.median(sw["rpe_rot"][s]))
        nees = sw["nees"][:, s]
        assert np.isfinite(nees).all()
        assert row["anees_pose"] == pytest.approx(float(nees.mean(axis=1).mean()), rel=1e-12)
        assert row["nis_per_dof"] == float(st["filt_nis"][s].sum() / st["filt_dof"][s].sum())
        assert row["rejected"] == int(sw["life_stats"]["rejected"][s].sum()) and row["not_spd"] == int(sw["life_stats"]["not_spd"][s].sum())
        # a plain run of cfg_t summarises to the same row
        plain = runs["plain"][t][1]
        assert row["ate_aligned_m"] == float(np.median(plain["ate_aligned"][0]))
    assert len({row["nis_per_dof"] for row in sw["summary"]}) == T


def test_sweep_two_axes_against_plain():
    """a second grid (threshold x noise x depth std: 2 tunings), final state only"""
    cfg = _cfg()
    sw = sweep.run_sweep(cfg, AXES2, W, **KW)
    try:
        got = _final(sw)
        assert sw["T"] == 2 and [c.MH_thresh for c in sw["cfgs"]] == [2.0, 9.0]
    finally:
        sw["backend"].close()
    want = []
    for c in sw["cfgs"]:
        out = sweep.run_plain(c, W, **KW)
        want.append(_final(out))
        out["backend"].close()
    for k in got:
        w = np.concatenate([x[k] for x in want])
        assert got[k].tobytes() == w.tobytes(), k


def test_run_sweep_script_writes_its_json(tmp_path):
    out = tmp_path / "sweep.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_sweep.py"), "-axis", "visual_meas_std=0.5:2:2", "-axis",
                        "MH_thresh=3,9", "-worlds", "2", "-total_time", "0.16", "-npts", "110", "-out", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    rep = json.loads(line)
    assert out.read_text().strip() == line.strip()
    assert rep["tunings"] == 4 and rep["worlds"] == 2 and rep["filters"] == 8 and rep["contexts"] == 1 and rep["runs"] == 1
    assert [(r_["visual_meas_std"], r_["MH_thresh"]) for r_ in rep["table"]] == [(0.5, 3.0), (0.5, 9.0), (2.0, 3.0), (2.0, 9.0)]
    for r_ in rep["table"]:
        assert {"ate_aligned_m", "ate_aligned_p90", "rpe_pos_m", "anees_pose", "nis_per_dof", "rejected", "not_spd"} <= set(r_)
    assert rep["best"]["ate_aligned_m"] in rep["table"] and rep["best"]["nis_per_dof"] in rep["table"]
