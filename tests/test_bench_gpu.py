"""bench.py end to end on the GPU box at a small batch: one JSON line with the contract's keys; with --full the default and the
opt-in symmetric-form figure, the in-bench parity check, roofline and the per-stage times (the hand-over stage inside the timed
step); a plain run times the headline and nothing else, and dumps what a --full run dumps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, full=True, plain=False):
    """bench.py --full (plain=True: without it) -> the verbose record (--full-out) by default, the printed compact line with
    full=False."""
    import tempfile
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "full.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "512", "--steps", "2", "--warmup", "1",
                            *([] if plain else ["--full"]), "--no-cpu-baseline", "--full-out", path, *extra], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        assert len(lines[0]) < 6144          # the driver keeps the last 8 KB of stdout: the whole line has to fit
        return json.load(open(path)) if full else json.loads(lines[0])


def test_default_line(built):
    d = _run("--no-configs", "--no-dropin")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "f64" and d["unit"] == "updates/s" and d["value"] > 0
    assert "workload" in d["config"] and "precision" in d["config"] and "hand_over" in d["config"]
    assert d["config"]["pipeline"].startswith("sparse-H") and d["config"]["not_spd_filters"] == 0
    # the two modes, each with its own figure (no speed ordering asserted here: two timed steps on a box that has just
    # been handed over can stall for tens of milliseconds - the ordering is a bench result, profiles/r03_bench_n1.json)
    assert d["value_symmetric_form"] > 0 and d["config"]["route"] == "sparse_in_solve"
    assert d["parity_check"]["ok"] and d["parity_check"]["rel_fro_P_max"] < 1e-6 and d["parity_check"]["inlier_masks_equal"]
    assert d["symmetric_form"]["parity_check"]["ok"]
    # round 3: the state the timed loop left behind is checked too, every rank reports its own checks and its core binding
    assert d["parity_check_last_timed_step"]["ok"] and d["parity_check_last_timed_step"]["updates_in_a_row"] == 3
    assert [p["ok"] for p in d["per_rank_parity"]] == [True] and len(d["per_rank_affinity"]) == 1
    assert "pipeline_frac_note" in d["roofline"] and d["config"]["precision"]["value"].startswith("library default = all fp64")
    st = d["stage_ms_per_step"]
    assert st["stack_H"] > 0 and st["trsm_gain"] > 0 and st["gemm_HP"] > 0      # hand-over is a timed stage
    assert not ({"gemm_AP", "gemm_KH_I", "gemm_Pnew"} & set(st))                # the covariance update lives in the solve kernel
    assert "gemm_KH_I" not in d["symmetric_form"]["stage_ms_per_step"]          # no T / G pass in the symmetric form
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] < 1 and r["kernel"] and r["avg_launch_ms"] > 0
    assert len(d["per_rank_updates_per_s"]) == 1


def test_printed_line_is_compact_and_complete(built):
    """What the driver's 8 KB tail keeps: contract keys, roofline, parity maxima, stage times, the drop-in medians mirrored
    into `config` as flat scalars, one short row per sub-configuration (the child runs at their own batch sizes)."""
    d = _run(full=False)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "parity_check", "parity_last", "stage_ms", "dropin", "configs"):
        assert k in d, k
    assert d["parity_check"]["ok"] and d["parity_last"]["ok"] and d["parity_last"]["n"] == 3
    assert all(len(v) <= 120 for v in d["config"].values() if isinstance(v, str))
    assert d["config"]["dropin_ms_250_160"] > 0 and d["config"]["dropin_ok_250_160"] is True and d["config"]["dropin_ms_203_60"] > 0
    keys = [r["k"] for r in d["configs"]]
    assert keys[:5] == ["cfg2", "cfg3", "cfg3_m260", "cfg4_f64", "cfg4_f32w"] and {"calib", "tumvi", "glevel", "ransac", "frame_rk4", "frame_pd", "b1"} <= set(keys)
    for r in d["configs"]:
        assert "error" not in r, r
        assert r.get("skipped") or (r["v"] > 0 and r["ok"] in (True, None)), r
        if r["k"] != "b1":           # (round 6: the RANSAC and whole-frame rows carry an in-bench parity too)
            assert r["ok"] is True, r
    assert d["config"]["cfg2_upd_s"] == [r for r in d["configs"] if r["k"] == "cfg2"][0]["v"]


def test_dump_outputs_repeat_bit_for_bit(built, tmp_path):
    """--dump-outputs: the last timed step's dx / status / gate of every filter and P+ of a seeded sample, under 64 MB; two runs
    with the same arguments write the same arrays (the inputs are seeded), and the state they come from passes parity_last."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        rec = _run("--no-configs", "--no-dropin", "--no-mixed", "--dump-outputs", str(d))
        assert rec["parity_check_last_timed_step"]["ok"] and rec["dumped_outputs"]["bytes"] <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert set(a) == {"dx", "status", "inlier_mask", "mh_distance", "P", "P_filters"}
    assert a["dx"].shape == (512, 250) and a["inlier_mask"].shape == (512, 80) and a["P"].shape[1:] == (250, 250)
    assert all(a[k].dtype in (np.float32, np.float64) for k in a)
    assert (a["status"] == 0).all() and np.abs(a["dx"]).max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_feature_level_and_config3_lines(built):
    d = _run("--level", "G", "--ransac")
    assert d["value"] > 0 and "OnePointRANSAC" in d["config"]["workload"]
    d = _run("--level", "G", "--oos", "20")
    assert d["value"] > 0 and "QR-compressed" in d["config"]["workload"] and "mixed stacking" in d["config"]["pipeline"]
    d = _run("--level", "G", "--oos", "20", "--no-compression")
    assert d["value"] > 0 and "QR-compressed" not in d["config"]["workload"] and d["parity_check"]["ok"]


def test_plain_run_is_the_headline_only(built, tmp_path):
    """Without --full: the contract keys, the per-stage times and the roofline of the timed steps - no parity, no second figure,
    no measured peak, no CPU baseline, no drop-in, no configurations - and --dump-outputs writes, array for array and bit for
    bit, what a --full run writes (the dump is taken before anything else runs the path again)."""
    import numpy as np
    rec = _run("--dump-outputs", str(tmp_path / "plain"), plain=True)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline"):
        assert k in rec, k
    assert rec["value"] > 0 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["dtype"] == "f64" and rec["unit"] == "updates/s"
    assert rec["config"]["not_spd_filters"] == 0 and rec["stage_ms_per_step"]["stack_H"] > 0
    assert rec["parity_check"] is None and rec["parity_check_last_timed_step"] is None and rec["symmetric_form"] is None
    assert rec["roofline"]["mfma_peak_measured_tflops"] is None
    assert not ({"cpu_baseline", "dropin", "configs"} & set(rec))
    _run("--no-configs", "--no-dropin", "--dump-outputs", str(tmp_path / "full"))
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    for f in names:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
