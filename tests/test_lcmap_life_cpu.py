"""CPU-only: loop closure inside the device life cycle (xivo_hip_lcmap_life_config), what needs no GPU of it.

The rules (xivo_amd/csrc/lcmap_life_device.h) under a host compiler: tests/lcmap_life_driver.cpp is a stand-alone program built
from the header alone - plain, and under AddressSanitizer and UBSan - that walks hand-made books as the begin and the query
kernel do and prints every add record and query with its list position. The lines are held against the host life cycle's own
code: the leaving features as SequenceRunner.frame collects them, through the runner's _lc_add and _lc_close on a backend that
writes the records down. Also here: SequenceConfig(lc_lifecycle=...), the header's declarations, the bindings.

What this does not cover: the kernels' own walks, the keys' way through the track block and the book, P and the map
(tests/test_lcmap_life_gpu.py)."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from xivo_amd import lib as L
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "lcmap_life_driver.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
NEW_CALLS = ("xivo_hip_lcmap_life_config", "xivo_hip_life_begin_keys", "xivo_hip_lcmap_add_resident", "xivo_hip_lcmap_close_resident",
             "xivo_hip_lcmap_life_get_keys", "xivo_hip_lcmap_life_get_track_keys")


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/lcmap_life_driver.cpp"
    exe = str(tmp_path_factory.mktemp("lcmap_life_" + request.param) / "driver")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, DRIVER, "-o", exe] + BUILDS[request.param], check=True)
    return exe


class _Writes:
    """a backend that writes down what the runner hands to the map"""

    def __init__(self):
        self.recs, self.queries = None, None

    def lcmap_add(self, recs):
        self.recs = recs

    def lcmap_close(self, queries):
        self.queries = queries
        return 0


def _host(books, F):
    """books: per filter F slots (feat_id, slot_track, u_is_nan, mask, key) -> what the host life cycle hands to the map: the add
    records (b, slot, key), the queries (b, slot, key) and feat_key after the begin stage. The leaving features are collected as
    SequenceRunner.frame collects them; _lc_add and _lc_close are the runner's own."""
    B = len(books)
    cfg = sequence.SequenceConfig(n_groups=4, n_features=F, loop_closure=True)
    r = sequence.SequenceRunner(_Writes(), cfg, B)
    leaving, xp, mask = [], np.full((B, F, 2), np.nan), np.zeros((B, F), dtype=np.uint8)
    for b, slots in enumerate(books):
        bk = r.books[b]
        for j, (fid, st, nan, m, key) in enumerate(slots):
            bk.feat_id[j], bk.feat_key[j], mask[b, j] = fid, key, m
            if fid >= 0:
                bk.feat_ref[j] = 0; bk.group_refs[0] = max(bk.group_refs[0], 0) + 1; bk.id2slot[fid] = j
        for j, (fid, st, nan, m, key) in enumerate(slots):
            if fid < 0:
                continue
            if st >= 0:                                   # (frame: `fid in pos` - the track's pixel, a NaN u included)
                xp[b, j] = (np.nan if nan else 100.0 + j, 50.0)
            else:
                leaving.append((b, j, bk.feat_key[j]))
                bk.drop_feature(j)
                bk.feat_key[j] = -1                       # (a freed slot reads -1: the device book's rule; the host's is never read)
    r._lc_add(leaving)
    r._lc_close(xp, mask)
    recs = [] if r.be.recs is None else [(int(x["b"]), int(x["feat"]), int(x["key"])) for x in r.be.recs]
    slot_of = {(b, round(float(x) - 100.0)): None for b in range(B) for x in xp[b, :, 0] if not np.isnan(x)}
    queries = [(int(q["b"]), int(round(q["xp"][0] - 100.0)), int(q["key"])) for q in r.be.queries]
    assert all((b, j) in slot_of for b, j, _ in queries) and all(q["group_sind"] == -1 for q in r.be.queries)
    return recs, queries, [list(r.books[b].feat_key) for b in range(B)]


def _device(exe, books, F, row):
    lines = ["%d %d %d" % (len(books), row, F)] + [" ".join("%d %d %d %d %d" % s for s in slots) for slots in books]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "S %d %d" % (L.lcmap_add_dtype.itemsize, L.lcmap_query_dtype.itemsize)
    assert out[-1] == "c 0 0 8 8"          # a count is trusted inside the row only
    recs, queries, keys, pos = [], [], [], []
    for b in range(len(books)):
        for kind, dst in (("r", recs), ("q", queries)):
            w = out[1 + 3 * b + (kind == "q")].split()
            assert w[0] == kind and len(w) == 2 + 3 * int(w[1])
            for i in range(int(w[1])):
                slot, key, p = (int(v) for v in w[2 + 3 * i:5 + 3 * i])
                dst.append((b, slot, key)); pos.append((kind, b, i, p))
        keys.append([int(v) for v in out[3 + 3 * b].split()[1:]])
    return recs, queries, keys, pos


FREE = (-1, -1, 0, 0, -1)


def _check(exe, books, F, row=None):
    row = F if row is None else row
    want = _host(books, F)
    recs, queries, keys, pos = _device(exe, books, F, row)
    assert (recs, queries, keys) == want
    # ascending slot order, and position = the filter's row + the rank in it: no position depends on another filter
    for lst in (recs, queries):
        assert lst == sorted(lst, key=lambda v: (v[0], v[1]))
    assert all(p == b * row + i for _, b, i, p in pos)
    return recs, queries


def test_an_empty_filter(driver):
    assert _check(driver, [[FREE] * 6], 6) == ([], [])


def test_every_slot_leaving(driver):
    recs, queries = _check(driver, [[(500 + j, -1, 0, 1, 70 + j) for j in range(6)]], 6)
    assert recs == [(0, j, 70 + j) for j in range(6)] and queries == []


def test_a_slot_with_key_minus_one_still_yields_its_record_and_its_query(driver):
    """the negative key is the map's to skip and count (lcmap_add_decide: skipped), not the list's to leave out"""
    recs, queries = _check(driver, [[(500, -1, 0, 1, -1), (501, 3, 0, 1, -1), (502, 0, 0, 1, 9)]], 3)
    assert recs == [(0, 0, -1)] and queries == [(0, 1, -1), (0, 2, 9)]


def test_a_rejected_slot_that_was_tracked_asks_nothing(driver):
    recs, queries = _check(driver, [[(500, 2, 0, 0, 5), (501, 1, 0, 1, 6), (502, 0, 0, 255, 7)]], 3)
    assert recs == [] and queries == [(0, 1, 6), (0, 2, 7)]       # (a mask byte is zero or not)


def test_a_tracked_slot_and_a_free_slot_side_by_side(driver):
    recs, queries = _check(driver, [[FREE, (500, 0, 0, 1, 5), FREE, (501, -1, 0, 1, 6), (-1, -1, 0, 1, 8), (502, 4, 1, 1, 7)]], 6)
    # a free slot whose mask byte is set asks nothing; nor does a track without a pixel (NaN u)
    assert recs == [(0, 3, 6)] and queries == [(0, 1, 5)]


def test_positions_across_three_filters_of_which_the_first_has_none(driver):
    books = [[FREE] * 5,
             [(500, -1, 0, 1, 1), (501, 0, 0, 1, 2), (502, -1, 0, 1, 3), FREE, (503, 1, 0, 1, 4)],
             [(600 + j, j if j % 2 else -1, 0, 1, 10 + j) for j in range(5)]]
    recs, queries = _check(driver, books, 5, row=7)               # (rows longer than the list in use: slot_ld > F)
    assert [r[0] for r in recs] == [1, 1, 2, 2, 2] and [q[0] for q in queries] == [1, 1, 2, 2]


def test_fuzz_equals_the_host_life_cycle(driver):
    rng = np.random.default_rng(7)
    for _ in range(40):
        F, B = int(rng.integers(1, 9)), int(rng.integers(1, 4))
        books = [[FREE if rng.uniform() < 0.3 else
                  (int(1000 * b + j), int(rng.integers(-1, 4)), int(rng.uniform() < 0.1), int(rng.uniform() < 0.7), int(rng.integers(-1, 6)))
                  for j in range(F)] for b in range(B)]
        _check(driver, books, F, row=F + int(rng.integers(0, 3)))


def test_header_stays_plain_cxx():
    text = open(os.path.join(CSRC, "lcmap_life_device.h")).read()
    for name in ("lclife_leaves", "lclife_tracked", "lclife_queries", "lclife_list_pos", "lclife_list_count", "lclife_no_key"):
        assert name in text
    body = text.split("#pragma once")[1]
    assert body.count("#include") == 1 and "hip/hip_runtime.h" in body.split("#else")[0]      # HIP's only, under __HIPCC__


# ---- SequenceConfig
def test_lc_lifecycle_device_accepted_and_refused():
    C = sequence.SequenceConfig
    assert C().lc_lifecycle == "host"
    ok = C(loop_closure=True, lc_lifecycle="device", lifecycle="device")
    r = sequence.SequenceRunner(types.SimpleNamespace(life_begin_keys=None, life_end=None), ok, 1)      # (never called below)
    assert r.device_lc and r.device_lifecycle
    sequence.check_lifecycle(C(loop_closure=True, lc_lifecycle="device", lifecycle="device", track_source="device", npts=500))
    refused = [dict(loop_closure=True, lc_lifecycle="device"),                                                   # neither device life cycle
               dict(loop_closure=True, lc_lifecycle="device", feature_init="subfilter"),
               dict(loop_closure=True, lc_lifecycle="device", lifecycle="device", feature_init="subfilter", pool_lifecycle="device"),   # both
               dict(lc_lifecycle="device", lifecycle="device"),                                                  # without loop_closure
               dict(loop_closure=True, lc_lifecycle="device", feature_init="subfilter", pool_lifecycle="device", use_oos=True),
               dict(loop_closure=True, lc_lifecycle="device", lifecycle="device", lc_max=L.LCMAP_MAX_MATCHES + 1),
               dict(loop_closure=True, lc_lifecycle="nowhere"),
               # the pool half is not there: the pool book carries no keys, so its refusal stays
               dict(loop_closure=True, lc_lifecycle="device", feature_init="subfilter", pool_lifecycle="device")]
    for kw in refused:
        with pytest.raises(ValueError):
            sequence.check_lifecycle(C(**kw))
    # every refusal of lc_lifecycle="host" stays
    for kw in (dict(lifecycle="device"), dict(feature_init="subfilter", pool_lifecycle="device")):
        with pytest.raises(ValueError, match="host life cycles only"):
            sequence.check_lifecycle(C(loop_closure=True, **kw))
    # keys are required with host tracks, and parallel to the ids
    with pytest.raises(ValueError, match="needs keys"):
        r.frame(None, [(np.zeros(0, dtype=np.int64), np.zeros((0, 3)))])
    with pytest.raises(ValueError, match="not parallel"):
        r.frame(None, [(np.array([10000]), np.zeros((1, 3)))], keys=[[]])


class _NoLog(sequence.HipBackend):
    """HipBackend's two refusals of the innovation log, without a context"""

    def __init__(self, innov_on, lc_on):
        self.innov_on, self.lc_on, self.oos_on = innov_on, lc_on, False
        self.cfg = sequence.SequenceConfig(loop_closure=True, lc_lifecycle="device", lifecycle="device")


def test_the_innovation_log_stays_refused():
    with pytest.raises(ValueError, match="innovation log"):
        _NoLog(True, False).enable_loop_closure()
    with pytest.raises(ValueError, match="loop_closure"):
        _NoLog(False, True).enable_innovation_log(8)


# ---- header and bindings
def test_new_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "xivo_hip.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"^int %s\(xivo_hip_ctx\* ctx, " % name, hdr, re.M), name
        assert name in L.ALL_SYMBOLS and name in L._SIGS
    assert len(L._SIGS["xivo_hip_life_begin_keys"]) == len(L._SIGS["xivo_hip_life_begin"]) + 1
    # the existing begin calls keep their signatures
    assert "int xivo_hip_life_begin(xivo_hip_ctx* ctx, int B, int F, const int* off, const long long* ids, const double* meas);" in hdr
    assert "int xivo_hip_pool_life_begin(" in hdr and "xivo_hip_pool_life_begin_keys" not in hdr      # (the pool half is not there)


def test_the_lists_hold_the_structs_of_the_host_calls(driver):
    """no new struct: the device's lists are xivo_lcmap_add_rec / xivo_lcmap_query, whose ctypes-side sizes equal the compiler's"""
    out = subprocess.run([driver], input="0 1 0\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "S %d %d" % (L.lcmap_add_dtype.itemsize, L.lcmap_query_dtype.itemsize) == "S 16 32"
