"""No GPU: the tuning table's record (lib.tune_dtype against xivo_tune_in of include/xivo_hip.h), sweep.grid (order, the rows
against what HipBackend passes for the same configuration, refusals), every configuration run_sweep refuses, and the argument
parser of scripts/run_sweep.py."""
import argparse
import importlib.util
import os
import shutil
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import sequence, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_sweep_script():
    spec = importlib.util.spec_from_file_location("run_sweep_script", os.path.join(ROOT, "scripts", "run_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tune_record_size_and_symbols(tmp_path):
    assert L.tune_dtype.itemsize == 5424
    assert [L.tune_dtype.fields[k][1] for k in ("R", "mh_thresh", "var_xyz", "Qimu", "Qmodel")] == [0, 8, 16, 40, 40 + 144 * 8]
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile against include/xivo_hip.h"
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "xivo_hip.h"\nint main() { printf("%zu %zu %zu\\n", '
                   'sizeof(xivo_tune_in), offsetof(xivo_tune_in, var_xyz), offsetof(xivo_tune_in, Qmodel)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(v) for v in out] == [5424, 16, 40 + 144 * 8]
    for name in ("xivo_hip_tune_config", "xivo_hip_tune_set", "xivo_hip_tune_get"):
        assert name in L.ALL_SYMBOLS and name in L._SIGS
    assert hasattr(L.Context, "tune_config") and hasattr(L.Context, "tune_set") and hasattr(L.Context, "tune_get")
    assert hasattr(sequence.HipBackend, "enable_tuning")


def test_grid_order_last_axis_fastest():
    cfg = sequence.SequenceConfig(lifecycle="device")
    axes = OrderedDict([("visual_meas_std", [0.5, 1.0, 2.0]), ("MH_thresh", [3.0, 9.0]), ("Qimu.gyro", [1e-3, 5e-3])])
    cfgs, table = sweep.grid(cfg, axes)
    assert len(cfgs) == 12 and table.shape == (12,) and table.dtype == L.tune_dtype
    got = [(c.visual_meas_std, c.MH_thresh, c.Qimu["gyro"]) for c in cfgs]
    want = [(a, b, c) for a in (0.5, 1.0, 2.0) for b in (3.0, 9.0) for c in (1e-3, 5e-3)]
    assert got == want
    # the base configuration keeps its own values, and every other field is the base's
    assert cfg.visual_meas_std == 1.0 and cfg.Qimu["gyro"] == 5e-3
    assert all(c.Qimu["accel"] == cfg.Qimu["accel"] and c.n_features == cfg.n_features for c in cfgs)


def test_grid_rows_are_what_the_backend_passes():
    """row t against the expressions of HipBackend.update / propagate / enable_device_lifecycle for cfg_t, byte for byte"""
    cfg = sequence.SequenceConfig(lifecycle="device")
    axes = OrderedDict([("visual_meas_std", [0.3, 1.7]), ("MH_thresh", [5.991]), ("initial_std_z", [0.1, 0.35]),
                        ("initial_std_x", [1.0, 3.0]), ("Qimu.gyro", [1e-3, 7e-3]), ("Qimu.accel", [3e-2]), ("Qmodel.Wsb", [0.01, 0.02])])
    cfgs, table = sweep.grid(cfg, axes)
    assert len(cfgs) == 32
    for c, row in zip(cfgs, table):
        R = c.visual_meas_std ** 2                                  # HipBackend.update
        assert np.float64(R).tobytes() == row["R"].tobytes() and np.float64(c.MH_thresh).tobytes() == row["mh_thresh"].tobytes()
        o = L.prop_options(c.Qimu_matrix(), c.Qmodel_matrix(), c.gravity)          # Context.propagate
        assert o["Qimu"][0].tobytes() == row["Qimu"].tobytes() and o["Qmodel"][0].tobytes() == row["Qmodel"].tobytes()
        fl = c.focal_length()                                       # HipBackend.enable_device_lifecycle
        std = np.array([c.initial_std_x / fl, c.initial_std_y / fl, c.initial_std_z])
        assert (std * std).tobytes() == row["var_xyz"].tobytes()
        assert row.tobytes() == sequence.HipBackend.tuning_entry(c).tobytes()
    assert len({r.tobytes() for r in table}) == 32


def test_grid_refuses_unknown_axis():
    cfg = sequence.SequenceConfig(lifecycle="device")
    for name in ("min_inliers", "MH_adjust_factor", "Qimu.nothing", "gravity", "subfilter.visual_meas_std", "nonsense"):
        with pytest.raises(ValueError):
            sweep.grid(cfg, OrderedDict([(name, [1.0])]))
        with pytest.raises(ValueError):
            sweep.run_sweep(cfg, OrderedDict([(name, [1.0])]), 2, total_time=0.1)
    with pytest.raises(ValueError):
        sweep.grid(cfg, OrderedDict([("MH_thresh", [])]))


@pytest.mark.parametrize("kw,axes", [
    (dict(lifecycle="device", feature_init="immediate", use_1pt_RANSAC=True), {"MH_thresh": [3.0]}),
    (dict(feature_init="subfilter", pool_lifecycle="device", use_oos=True), {"MH_thresh": [3.0]}),
    (dict(lifecycle="device", loop_closure=True, lc_lifecycle="device"), {"MH_thresh": [3.0]}),
    (dict(lifecycle="device", track_source="device", npts=500), {"MH_thresh": [3.0]}),
    (dict(feature_init="subfilter", pool_lifecycle="device"), {"initial_std_z": [0.1, 0.2]}),
    (dict(feature_init="subfilter", pool_lifecycle="device"), {"MH_thresh": [3.0], "initial_std_x": [1.0]}),
    (dict(lifecycle="host"), {"MH_thresh": [3.0]}),
    (dict(feature_init="subfilter", pool_lifecycle="host"), {"MH_thresh": [3.0]}),
])
def test_run_sweep_refusals(kw, axes):
    """refused before a context exists: nothing here needs a GPU"""
    cfg = sequence.SequenceConfig(**kw)
    with pytest.raises(ValueError):
        sweep.run_sweep(cfg, OrderedDict(axes), 2, total_time=0.2)


def test_run_sweep_accepts_what_it_should():
    sweep.check_sweep(sequence.SequenceConfig(lifecycle="device"), {"initial_std_z": [0.1], "Qmodel.Wsb": [0.01]})
    sweep.check_sweep(sequence.SequenceConfig(feature_init="subfilter", pool_lifecycle="device"), {"visual_meas_std": [1.0], "Qimu.accel": [0.05]})
    with pytest.raises(ValueError):
        sweep.run_sweep(sequence.SequenceConfig(lifecycle="device"), {"MH_thresh": [3.0]}, 0)


def test_run_sweep_script_parser():
    rs = _run_sweep_script()
    ap = rs.make_parser()
    a = ap.parse_args(["-axis", "visual_meas_std=0.5:4:8", "-axis", "MH_thresh=3,5.991,9", "-worlds", "16", "-total_time", "4",
                       "-out", "x.json"])
    axes = rs.axes_of(a)
    assert list(axes) == ["visual_meas_std", "MH_thresh"]
    assert axes["visual_meas_std"] == [float(v) for v in np.linspace(0.5, 4.0, 8)] and axes["MH_thresh"] == [3.0, 5.991, 9.0]
    assert a.worlds == 16 and a.total_time == 4.0 and a.out == "x.json"
    assert rs.parse_axis("Qimu.gyro=1e-3") == ("Qimu.gyro", [1e-3])
    assert rs.parse_axis("MH_thresh=2:2:1") == ("MH_thresh", [2.0])
    for bad in ("visual_meas_std", "=1,2", "MH_thresh=", "MH_thresh=1:2", "MH_thresh=1:2:0", "MH_thresh=a,b", "MH_thresh=1:2:x"):
        with pytest.raises(argparse.ArgumentTypeError):
            rs.parse_axis(bad)
        with pytest.raises(SystemExit):
            ap.parse_args(["-axis", bad])
    with pytest.raises(ValueError):
        rs.axes_of(ap.parse_args(["-axis", "MH_thresh=1", "-axis", "MH_thresh=2"]))
    s = [dict(ate_aligned_m=0.3, nis_per_dof=2.0), dict(ate_aligned_m=0.1, nis_per_dof=0.2), dict(ate_aligned_m=0.2, nis_per_dof=1.1)]
    assert rs.best_rows(s) == {"ate_aligned_m": 1, "nis_per_dof": 2}
