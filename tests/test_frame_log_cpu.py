"""CPU-only: the host bookkeeping of a per-frame device log (xivo_amd/csrc/frame_log.h) at its edges.
tests/frame_log_driver.cpp is compiled with g++ -std=c++17 -Wall -Wextra against the header alone, once plainly and once with
-fsanitize=address,undefined; every scenario runs on both and prints "step key=value ..." lines.

What the entry points of the four logs do with the type (status codes, what a refused call leaves behind) is in
tests/test_traj_log_gpu.py, test_map_log_gpu.py, test_innov_log_gpu.py and test_trajsim_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/frame_log_driver.cpp"
    exe = str(tmp_path_factory.mktemp("frame_log") / "driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", *extra, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "frame_log_driver.cpp"), "-o", exe], check=True)
    return exe


def run(driver, scenario):
    """a sanitizer report ends the program with a non-zero status (no recovery) and writes to stderr: both must stay clean"""
    r = subprocess.run([driver, scenario], check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr
    steps = {}
    for line in r.stdout.strip().splitlines():
        name, *kv = line.split()
        assert name not in steps, name
        steps[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    return steps


def test_header_is_plain_cxx():
    """No HIP header, no header of the project: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "frame_log.h")).read().split("#pragma once")[1]
    assert "hip/" not in text and '#include "' not in text


def test_capacity_zero_is_not_configured(driver):
    s = run(driver, "life")
    assert s["fresh"] == dict(configured=0, full=1, capacity=0, count=0)
    assert s["fresh_commit"] == dict(index=-1, count=0)
    assert s["released"] == dict(configured=0, full=1, capacity=0, count=0)


def test_capacity_one_is_full_after_one_commit_and_refuses_the_next(driver):
    s = run(driver, "life")
    assert s["one"] == dict(configured=1, full=0, capacity=1, count=0)
    assert s["one_full"] == dict(configured=1, full=1, capacity=1, count=1)
    assert s["one_refused"] == dict(first=0, again=-1, count=1, stamp=11)    # the refused stamp is not kept either


def test_commit_counts_up_and_a_middle_slice_has_its_stamps_in_order(driver):
    s = run(driver, "life")
    assert s["order"] == dict(i0=0, i1=1, i2=2, i3=3, mid0=110, mid1=120)


def test_reset_keeps_the_capacity_and_reuses_index_zero(driver):
    s = run(driver, "life")
    assert s["reset"] == dict(configured=1, full=0, capacity=5, count=0)
    assert s["reuse"] == dict(index=0, count=1, stamp=7)
    assert s["reconfigured"] == dict(configured=1, full=0, capacity=3, count=0)


def test_slice_check(driver):
    """3 frames recorded (capacity 8). Accepted: the empty slice at each end, all, a middle one; refused: the five shapes the GPU
    tests send - (INT_MAX, INT_MAX) is the one the overflow-safe form is for - and an empty slice behind the end."""
    s = run(driver, "slices")
    for name in ("empty_front", "empty_back", "all", "middle"):
        assert s[name] == dict(ok=1), name
    for name in ("too_long", "past_end", "neg_t0", "neg_nt", "int_max", "empty_past", "empty_far"):
        assert s[name] == dict(ok=0), name
    assert s["after"] == dict(configured=1, full=0, capacity=8, count=3)         # a check changes nothing
    assert s["at"] == dict(small=2 * 7 + 3, big=INT_MAX * INT_MAX + INT_MAX)


def test_sizing_guard(driver):
    s = run(driver, "sizing")
    assert s["below"] == dict(ok=1, entries=2 ** 40)         # 2^40 entries of 2^23 - 1 bytes: 2^63 - 2^40
    assert s["exact"] == dict(ok=0, entries=2 ** 40)         # 2^63 itself does not fit 63 bits
    T, B, per = 7 * 73 * 127 * 337, 7 * 92737, 649657
    assert T * B * per == 2 ** 63 - 1 and T <= INT_MAX and B <= INT_MAX
    assert s["last"] == dict(ok=1, entries=T * B)            # 2^63 - 1 bytes: the largest that fits
    assert s["over"] == dict(ok=0, entries=T * B)            # one byte more per entry
    assert s["int_max_bytes"] == dict(ok=1, entries=INT_MAX * INT_MAX)
    assert s["int_max"] == dict(ok=0, entries=INT_MAX * INT_MAX)   # refused, and the entry count did not wrap
