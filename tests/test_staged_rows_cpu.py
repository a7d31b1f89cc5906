"""CPU-only: the transitions of StagedRows (xivo_amd/csrc/staged_rows.h) against the table of what every producer of the C ABI
left in the loose fields of xivo_hip_ctx before the record existed. tests/staged_rows_driver.cpp replays each producer
sequence as transitions (g++ -std=c++17 against the header alone) and prints the whole record after every step.

A line of the table is
  sequence/step: M Mp dense from_compressed ht clean mixed_row0 lead oos_row0 oos_max_rows oos_R stack_B stack_R gate | over | nc | pw | nc_max pw_max any_over
written from the host code as it was, site by site (stage_measurements and its two exits, xivo_hip_stack, calib_gate, the two
stackings of xivo_hip_one_point_ransac, xivo_hip_oos_project_ex, xivo_hip_compress_oos, xivo_hip_close_loop_stack, the fast
path of xivo_hip_update_joseph_host, ensure_dense, ensure_HT). Where the record deliberately differs, WAS holds what the old
code left and the fields that may differ:
  - every producer of new rows resets oos_row0 / lead (a hand-over after an OOS append; the one-filter call after a
    calibration stacking),
  - calib_gate's whole-row stacking now marks its filters "do not fit" with the slot counts of whole rows, as RANSAC's does
    (it used to leave over / nc / pw of whatever was staged before).
The invariants of the header comment are asserted after every step.

What this pins is the header's transitions. The driver restates the host decisions around them (the mixed predicate of
xivo_hip_oos_project, the branch order of ensure_dense, which stackings RANSAC makes) in test code, so a call site in
capi_glevel.hip / capi_update.hip that passed the wrong kind, calibration columns or dense flag to a transition would not show
here: the sequences of tests/test_staging_gpu.py cover the call sites."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")

FIELDS = ("M", "Mp", "dense", "from_compressed", "ht", "clean", "mixed_row0", "lead", "oos_row0", "oos_max_rows", "oos_R",
          "stack_B", "stack_R", "gate")

TABLE = """
    handover_fit/hand_over: 40 48 0 1 1 1 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_fit/update: 40 48 0 1 1 1 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_fit/get_H: 40 48 1 1 1 0 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_fit/hand_over_again: 40 48 0 1 1 0 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_mixed_batch/hand_over: 40 48 0 1 1 0 -1 0 -1 0 0 0 0 P | 0 1 0 | 12 16 12 | 6 13 6 | 16 13 1
    handover_mixed_batch/update_dense: 40 48 1 1 1 0 -1 0 -1 0 0 0 0 P | 0 1 0 | 12 16 12 | 6 13 6 | 16 13 1
    handover_mixed_batch/hand_over_sub_range: 40 48 0 1 1 0 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_none_fit/hand_over: 40 48 1 1 1 0 -1 0 -1 0 0 0 0 P | 1 1 1 | 16 16 16 | 13 13 13 | 16 13 1
    handover_none_fit/update_dense: 40 48 1 1 1 0 -1 0 -1 0 0 0 0 P | 1 1 1 | 16 16 16 | 13 13 13 | 16 13 1
    stack_oos/mh_gate: 0 0 1 0 1 1 -1 0 -1 0 0 0 0 S | 1 1 1 | 16 16 16 | 12 12 12 | 16 12 1
    stack_oos/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    stack_oos/oos_project: 60 64 0 0 0 1 40 0 40 20 12.25 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    stack_oos/compress_oos: 49 64 0 0 0 1 40 0 40 9 12.25 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    stack_oos/get_H: 49 64 1 0 0 0 40 0 40 9 12.25 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    stack_oos/oos_project_2: 59 64 1 0 0 0 -1 0 49 10 12.25 3 1 S | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    stack_oos/update_dense: 59 64 1 0 1 0 -1 0 49 10 12.25 3 1 S | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    stack_oos/stack_next_frame: 40 48 0 0 1 0 -1 0 -1 10 12.25 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    stack_oos/oos_project_resident: 50 64 0 0 0 1 40 0 40 10 12.25 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    oos_no_spare_rows/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    oos_no_spare_rows/oos_project: 60 64 1 0 1 0 -1 0 40 20 12.25 3 1 P | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    stack_dense_h/stack: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 9 9 9 | 12 9 0
    stack_dense_h/gated_update: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 9 9 9 | 12 9 0
    stack_dense_h/oos_project: 60 64 1 0 1 0 -1 0 40 20 12.25 3 1 P | 1 1 1 | 12 12 12 | 9 9 9 | 12 9 1
    calib_lead/mh_gate: 0 0 1 0 1 1 -1 0 -1 0 0 0 0 S | 1 1 1 | 16 16 16 | 12 12 12 | 16 12 1
    calib_lead/stack: 40 48 0 0 1 1 -1 1 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    calib_lead/update: 40 48 0 0 1 1 -1 1 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    calib_lead/get_H: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 S | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    calib_lead/stack_again: 40 48 0 0 1 0 -1 1 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    calib_lead/update_dense_gated: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 P | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    calib_lead/set_calib: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 P | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    calib_dense/mh_gate: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 S | 1 1 1 | 12 12 12 | 9 9 9 | 12 9 1
    calib_dense/stack: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 S | 1 1 1 | 12 12 12 | 6 6 6 | 12 6 1
    calib_dense/ransac: 40 48 1 0 1 0 -1 0 -1 0 0 3 1 S | 1 1 1 | 12 12 12 | 9 9 9 | 12 9 1
    ransac/hand_over: 40 48 0 1 1 1 -1 0 -1 0 0 0 0 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    ransac/ransac: 40 48 0 1 1 1 -1 0 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 9 9 9 | 12 9 0
    ransac/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    ransac/ransac_again: 40 48 0 1 1 1 -1 0 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 9 9 9 | 12 9 0
    ransac/get_H: 40 48 1 1 1 0 -1 0 -1 0 0 3 1 S | 0 0 0 | 12 12 12 | 9 9 9 | 12 9 0
    close_loop/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    close_loop/oos_project: 60 64 0 0 0 1 40 0 40 20 12.25 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    close_loop/close_loop_stack: 8 16 0 1 1 1 -1 0 -1 20 12.25 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_after_oos/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_after_oos/oos_project: 60 64 0 0 0 1 40 0 40 20 12.25 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    handover_after_oos/hand_over: 40 48 0 1 1 1 -1 0 -1 20 12.25 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    dropin_after_lead/stack: 40 48 0 0 1 1 -1 1 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    dropin_after_lead/dropin: 30 32 0 1 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    dropin_after_lead/stack_again: 40 48 0 0 1 1 -1 1 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    dropin_and_batch/dropin: 30 32 0 1 1 1 -1 0 -1 0 0 0 0 P | 1 0 1 | 16 12 16 | 12 6 12 | 16 12 1
    dropin_and_batch/stack: 40 48 0 0 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
    dropin_and_batch/dropin_again: 30 32 0 1 1 1 -1 0 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0
"""

# step -> (what the old code left, the fields that are allowed to differ)
WAS = {
    "handover_after_oos/hand_over": ("40 48 0 1 1 1 -1 0 40 20 12.25 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0", {"oos_row0"}),
    "dropin_after_lead/dropin": ("30 32 0 1 1 1 -1 1 -1 0 0 3 1 P | 0 0 0 | 12 12 12 | 6 6 6 | 12 6 0", {"lead"}),
    "calib_dense/mh_gate": ("40 48 1 0 1 0 -1 0 -1 0 0 3 1 S | 1 1 1 | 16 16 16 | 12 12 12 | 16 12 1", {"nc", "pw", "slots"}),
}


def parse(line):
    name, rest = line.split(": ", 1)
    head, over, nc, pw, slots = [p.split() for p in rest.split("|")]
    rec = dict(zip(FIELDS, head))
    for k in FIELDS[:10] + ("stack_B",):
        rec[k] = int(rec[k])
    rec.update(over=[int(x) for x in over], nc=[int(x) for x in nc], pw=[int(x) for x in pw], slots=[int(x) for x in slots])
    return name, rec


EXPECTED = dict(parse(l.strip()) for l in TABLE.strip().splitlines())
SEQUENCES = sorted({k.split("/")[0] for k in EXPECTED})


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/staged_rows_driver.cpp"
    exe = str(tmp_path_factory.mktemp("staged_rows") / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(ROOT, "tests", "staged_rows_driver.cpp"),
                    "-o", exe], check=True)
    return exe


def replay(driver, seq):
    out = subprocess.run([driver, seq], check=True, capture_output=True, text=True).stdout
    return [parse(l) for l in out.strip().splitlines()]


def check_invariants(name, r, prev):
    assert r["Mp"] == (r["M"] + 15) // 16 * 16, name
    if r["mixed_row0"] >= 0:
        assert not r["from_compressed"] and not r["lead"] and r["oos_row0"] == r["mixed_row0"], name
        if prev is not None and prev["mixed_row0"] < 0:      # the append itself
            assert not prev["dense"] and not r["dense"] and not r["ht"], name
    if r["lead"]:
        assert not r["dense"] and r["mixed_row0"] < 0 and not any(r["over"][:r["stack_B"]]), name
    if r["oos_row0"] >= 0:
        assert r["M"] <= r["oos_row0"] + r["oos_max_rows"], name
    assert r["slots"] == [max(r["nc"]), max(1, max(r["pw"])), int(any(r["over"]))], name


def test_header_is_plain_cxx():
    """The record includes neither HIP headers nor the context: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "staged_rows.h")).read()
    assert "hip/" not in text and "capi_internal.h" not in text.split("#pragma once")[1]
    assert "friend" not in text


@pytest.mark.parametrize("seq", SEQUENCES)
def test_producer_leaves_what_the_old_code_left(driver, seq):
    steps = replay(driver, seq)
    assert steps[0][0] == seq + "/created"
    want = [k for k in EXPECTED if k.startswith(seq + "/")]
    assert [n for n, _ in steps[1:]] == want
    prev = None
    for name, rec in steps:
        check_invariants(name, rec, prev)
        prev = rec
        if name.endswith("/created"):
            continue
        assert rec == EXPECTED[name], name
        if name in WAS:
            old = parse(name + ": " + WAS[name][0])[1]
            assert {k for k in rec if rec[k] != old[k]} == WAS[name][1], name


@pytest.mark.parametrize("seq", SEQUENCES)
def test_new_rows_reset_what_the_previous_rows_left(driver, seq):
    """oos_row0 >= 0 only between an OOS append and the next producer of rows; no producer of new rows inherits a lead block
    or the mixed mode."""
    producers = ("hand_over", "stack", "ransac", "dropin", "close_loop_stack")
    for name, rec in replay(driver, seq):
        step = name.split("/")[1]
        if step.startswith(producers):
            assert rec["oos_row0"] == -1 and rec["mixed_row0"] == -1, name
            if not step.startswith("stack"):
                assert not rec["lead"], name
