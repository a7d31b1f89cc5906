"""CPU-only: the owner of a context's device memory (xivo_amd/csrc/device_buffers.h) against a counting allocator.
tests/device_buffers_driver.cpp is compiled with g++ -std=c++17 against the header alone; its allocator counts live blocks,
logs every free and fails the k-th allocation on request. Each scenario prints "step key=value ..." lines.

What a step reports: owner_live / owner_bytes (what the owner says it holds), alloc_live / alloc_bytes (what the allocator
has handed out and not got back), frees (distinct blocks freed), max_freed (the most often any one block was freed),
bad_frees (frees of something that was not live).

The failure paths of the call sites (a re-size that runs out of memory half way) are covered here and only here: no GPU test
provokes an out-of-memory condition. That the call sites go through the owner is tests/test_ctx_buffers_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/device_buffers_driver.cpp"
    exe = str(tmp_path_factory.mktemp("device_buffers") / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(ROOT, "tests", "device_buffers_driver.cpp"),
                    "-o", exe], check=True)
    return exe


def run(driver, *args):
    out = subprocess.run([driver, *map(str, args)], check=True, capture_output=True, text=True).stdout
    steps = {}
    for line in out.strip().splitlines():
        name, *kv = line.split()
        assert name not in steps, name
        steps[name] = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (x.split("=") for x in kv)}
    return steps


def consistent(s):
    """the owner and the allocator agree, nothing was freed twice, nothing foreign was freed"""
    assert s["owner_live"] == s["alloc_live"] and s["owner_bytes"] == s["alloc_bytes"], s
    assert s["max_freed"] <= 1 and s["bad_frees"] == 0, s


def test_header_is_plain_cxx():
    """No HIP header, no header of the project: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "device_buffers.h")).read().split("#pragma once")[1]
    assert "hip/" not in text and '#include "' not in text


def test_free_everything_after_a_mix_of_fixed_and_growing_buffers(driver):
    s = run(driver, "mix")
    # zeroed / raw / zeroed(0 elements: no block, null slot) / grow / grow / grow beyond: fill only where asked, never on grow
    assert s["allocated"] == dict(rc=0, none_null=1, zero_flags=10000, c1=300, c2=7)
    consistent(s["before"])
    assert s["before"]["owner_live"] == 4 and s["before"]["owner_bytes"] == 10 * 4 + 5 * 8 + 300 * 8 + 7
    assert s["before"]["allocs"] == 5 and s["before"]["frees"] == 1          # the grown buffer's first block
    for step in ("after", "again"):
        consistent(s[step])
        assert s[step]["owner_live"] == 0 and s[step]["frees"] == s[step]["allocs"] == 5   # every block exactly once


def test_grow_keeps_the_pointer_within_capacity_and_frees_once_beyond(driver):
    s = run(driver, "grow")
    assert s["within"] == dict(rc=0, same=1, new_allocs=0, cap=64, frees=0)
    assert s["beyond"] == dict(rc=0, same=0, new_allocs=1, cap=65, old_freed=1, bytes=65 * 8)
    consistent(s["end"])
    assert s["end"]["owner_live"] == 1


def test_failed_grow_leaves_an_empty_slot_and_the_next_one_succeeds(driver):
    s = run(driver, "grow_fail")
    assert s["failed"]["rc"] != 0 and s["failed"]["null"] == 1 and s["failed"]["cap"] == 0 and s["failed"]["old_freed"] == 1
    consistent(s["failed_state"])
    assert s["failed_state"]["owner_live"] == 0
    assert s["retry"] == dict(rc=0, null=0, cap=20)
    consistent(s["end"])
    assert s["end"]["owner_live"] == 1 and s["end"]["owner_bytes"] == 20 * 8


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_group_resize_with_the_kth_allocation_failing(driver, k):
    s = run(driver, "group", k)
    for r in (0, 1):
        f = s["failed%d" % r]
        assert f["rc"] != 0 and f["dangling"] == 0 and f["held"] == k - 1        # valid and owned, or null
        st = s["failed_state%d" % r]
        consistent(st)
        assert st["owner_live"] == k - 1                                          # the live count = the successes
        consistent(s["freed%d" % r])
        assert s["freed%d" % r]["owner_live"] == 0 and s["freed%d" % r]["frees"] == s["freed%d" % r]["allocs"]
    assert s["retry"] == dict(rc=0, held=5, dangling=0)
    consistent(s["retry_state"])
    assert s["retry_state"]["owner_live"] == 5 and s["retry_state"]["owner_bytes"] == 40 * (4 + 42 * 8 + 1 + 2 * 8 + 8)


def test_release_of_a_null_slot_and_repeated_resize(driver):
    s = run(driver, "release")
    assert s["null_release"]["frees"] == 0 and s["null_release"]["owner_live"] == 0 and s["null_release"]["bad_frees"] == 0
    consistent(s["once"])
    assert s["thrice"] == dict(rc=0, held=5, dangling=0)
    consistent(s["thrice_state"])
    for key in ("owner_live", "owner_bytes"):
        assert s["thrice_state"][key] == s["once"][key]
    assert s["thrice_state"]["frees"] == 10
    # a fixed allocation into a slot that still holds a block gives the old block back first: nothing piles up
    assert s["refill"] == dict(rc=0, same=0, old_freed=1)
    consistent(s["refill_state"])
    assert s["refill_state"]["owner_live"] == s["once"]["owner_live"] and s["refill_state"]["frees"] == 11
