"""CPU-only: the host mirrors of the feature pool (xivo_amd/csrc/pool_mirror.h) - who is live, who is linked, and what a refused
xivo_hip_edit_batch leaves behind. tests/pool_mirror_driver.cpp is compiled with g++ -std=c++17 -Wall -Wextra against the header
alone, once plainly and once with -fsanitize=address,undefined; every scenario runs on both and prints "step key=value ..."
lines.

Shapes: 2 filters, pool_max 3, anchor_max 2, group slots 0..2. A state line holds every cell: e<b><i> the anchor of entry i of
filter b (-1: free), a<b><k> the link of its anchor k (-2: never created, -1: unlinked, else the slot). The scenarios act on
filter 1 and every assertion compares all cells, so an index that drops its filter term shows.

What the entry points do with the type (status codes) is in tests/test_feature_pool_gpu.py and test_pool_lifecycle_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/pool_mirror_driver.cpp"
    exe = str(tmp_path_factory.mktemp("pool_mirror") / "driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", *extra, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "pool_mirror_driver.cpp"), "-o", exe], check=True)
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


def cells(e0=(-1, -1, -1), e1=(-1, -1, -1), a0=(-2, -2), a1=(-2, -2)):
    d = {}
    for b, (e, a) in enumerate(((e0, a0), (e1, a1))):
        d.update({"e%d%d" % (b, i): v for i, v in enumerate(e)})
        d.update({"a%d%d" % (b, k): v for k, v in enumerate(a)})
    return d


# the pool the edit scenarios start from: filter 1 has both anchors created and entries 0 / 1 on anchors 0 / 1; filter 0 links its
# anchor 0 to slot 1 - the slot the scenarios use in filter 1
PREPARED = cells(e1=(0, 1, -1), a0=(1, -2), a1=(-1, -1))


def test_header_is_plain_cxx():
    """No HIP header, no header of the project: a host compiler alone takes it."""
    text = open(os.path.join(CSRC, "pool_mirror.h")).read().split("#pragma once")[1]
    assert "hip/" not in text and '#include "' not in text


def test_a_fresh_pool_is_empty_until_one_anchor_or_one_entry(driver):
    s = run(driver, "life")
    assert s["unconfigured"] == dict(empty=1, pm=0, am=0, exists=0, free=-1)
    assert s["fresh"] == cells() and s["fresh_q"] == dict(empty=1, pm=3, am=2)
    assert s["add_rule"]["empty"] == 0                       # after one anchor_created
    assert s["entry_only"] == dict(empty=0, anchor=1, other_filter=-1)
    assert s["released"] == dict(empty=1, pm=0, am=0)


def test_an_entry_needs_an_anchor_that_was_created(driver):
    """never created (-2): refused; created and unlinked (-1): fine; the same anchor of the other filter and the other anchor of
    the same filter are still never created"""
    s = run(driver, "life")
    assert s["add_rule"] == dict(never=0, unlinked=1, other_filter=0, other_anchor=0, empty=0)


def test_indices_out_of_range_read_as_free_and_never_created(driver):
    s = run(driver, "life")
    assert s["range"] == dict(e_hi=-1, e_lo=-1, b_hi=-1, a_hi=-2, a_lo=-2, linked=0, slot=0)


def test_a_linked_anchor_cannot_be_created_again(driver):
    s = run(driver, "edits")
    assert s["prepared"] == PREPARED
    assert s["recreate"] == dict(linked=1, unlinked=0)


def test_group_anchored_and_entry_admitted_rules(driver):
    """group anchored: accepted on an unlinked anchor though filter 0 links the same slot; refused on an anchor never created,
    on a linked one, and for a slot another anchor of the filter holds (another slot is fine). entry admitted: refused for a free
    entry and for one whose anchor is unlinked, accepted once an earlier op of the same Edit linked it - the other entry's anchor
    is still unlinked."""
    s = run(driver, "edits")
    assert s["anchor_rule"] == dict(ok=1, never=0, admit_free=0, admit_unlinked=0, again=0, slot_taken=0, other_slot=1,
                                    admit_linked=1, admit_other=0)
    assert s["anchored"] == cells(e1=(0, 1, -1), a0=(1, -2), a1=(1, -1))


def test_group_removed_unlinks_the_anchors_of_that_slot_and_no_other(driver):
    """filter 1: anchor 0 -> slot 1, anchor 1 -> slot 2; slot 1 removed. Filter 0 keeps its link to slot 1."""
    s = run(driver, "edits")
    assert s["removed"] == cells(e1=(0, 1, -1), a0=(1, -2), a1=(-1, 2))


def test_a_refused_edit_restores_every_cell_and_the_same_ops_commit(driver):
    """[anchor 0 -> slot 1, admit entry 0, remove group 1, admit entry 0 again]: the last op is refused (the entry is free by
    then) and the mirrors are what they were; without it the three ops stay."""
    s = run(driver, "transaction")
    assert s["before"] == PREPARED
    assert s["ops"] == dict(anchor=1, admit=1, bad=0)
    assert s["linked_admitted"] == cells(e1=(-1, 1, -1), a0=(1, -2), a1=(1, -1))
    assert s["removed"] == cells(e1=(-1, 1, -1), a0=(1, -2), a1=(-1, -1))
    assert s["rolled_back"] == PREPARED
    assert s["committed"] == cells(e1=(-1, 1, -1), a0=(1, -2), a1=(-1, -1))


def test_a_refused_edit_undoes_only_its_own_ops(driver):
    """an entry added after the committed call stays when the next call is refused"""
    s = run(driver, "transaction")
    assert s["second_inside"] == cells(e1=(-1, 1, -1), a0=(1, -2), a1=(-1, 2))
    assert s["second_rolled_back"] == cells(e1=(-1, 1, 1), a0=(1, -2), a1=(-1, -1))


def test_entries_dead_frees_what_the_step_found_dead_in_its_filters_only(driver):
    s = run(driver, "dead")
    assert s["one_filter"] == cells(e0=(0, -1, 0), e1=(0, 0, 0), a0=(-1, -2), a1=(-1, -2))     # B = 1: filter 1 untouched
    assert s["both"] == cells(e0=(0, -1, 0), e1=(-1, 0, -1), a0=(-1, -2), a1=(-1, -2))


def test_reread_clamps_as_the_device_books_mean(driver):
    """an entry's ref_sind outside [0, anchor_max) reads as free; an unused anchor as never created, whatever its slot; a used
    anchor with slot -1 as unlinked, with slot 2 as linked to 2. What the mirrors held before does not survive."""
    s = run(driver, "reread")
    assert s["reread"] == cells(e1=(1, -1, -1), a0=(-2, -2), a1=(-1, 2))
    assert s["unused_with_slot"] == cells(e1=(1, -1, -1), a0=(-2, -1), a1=(-2, 2))
