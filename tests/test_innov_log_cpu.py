"""Innovation log, what can be checked without a GPU: the per-row and per-filter arithmetic of xivo_amd/csrc/innov_device.h
under a host compiler (tests/innov_row_driver.cpp, compiled from the header alone; its sanitizer build runs as a program)
against the longdouble restatement of tests/innov_restate.py within the restatement's bounds; the binding (record size and
offsets, symbols, refusals without a context); and run_pcw with a backend that has no innovation log."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import innov_restate as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNOV_SYMBOLS = ("xivo_hip_innov_config", "xivo_hip_innov_record", "xivo_hip_innov_count", "xivo_hip_innov_reset",
                 "xivo_hip_innov_read", "xivo_hip_innov_stats")
W = 28


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tests/innov_row_driver.cpp"
    exe = str(tmp / name)
    # -ffp-contract=off: the products and sums as written, fused multiply-adds only where the header calls fma
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra"] + extra +
                   [os.path.join(ROOT, "tests", "innov_row_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("innov_row")
    return _build(tmp, "driver", []), _build(tmp, "driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _hex(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())


def _text(case):
    """one case in the driver's input format"""
    M, N, er = case["M"], case["N"], case["er"]
    parts = ["%d %d %d %d %d %d" % (M, N, er, case.get("lead_k", 0), case.get("status", 0), case.get("ldlt", 0)),
             " ".join(str(int(v)) for v in case["idx"].ravel()), _hex(case["val"])]
    if case.get("lead_k", 0):
        parts.append(_hex(case["lead"]))
    parts += [_hex(case["Hd"]), _hex(case["inn"]), _hex(case["R"]), _hex(case["dx"])]
    return "\n".join(parts) + "\n"


def _run(exe, cases):
    out = subprocess.run([exe], input="".join(_text(c) for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].startswith("layout ")
    recs = []
    for line in out[1:]:
        t = line.split()
        assert t[0] == "rec"
        recs.append(dict(nis=float.fromhex(t[1]), prefit=float.fromhex(t[2]), postfit=float.fromhex(t[3]),
                         inn_max=float.fromhex(t[4]), dx_max=float.fromhex(t[5]), dof=int(t[6]), rows=int(t[7]), flags=int(t[8])))
    assert len(recs) == len(cases)
    return out[0], recs


def _dense(case):
    """the rows of a case as the dense [M, N] matrix xivo_hip_get_H would return"""
    M, N, er = case["M"], case["N"], case["er"]
    H = np.zeros((M + 1, N))
    for p in range((er + 1) // 2):
        for t in range(W):
            for h in range(2):
                v = case["val"][p, t, h]
                if v != 0.0:
                    assert H[2 * p + h, case["idx"][p, t]] == 0.0      # a column is stored once per pair
                    H[2 * p + h, case["idx"][p, t]] = v
        for k in range(case.get("lead_k", 0)):
            for h in range(2):
                if case["lead"][2 * p + h, k] != 0.0:
                    assert H[2 * p + h, k] == 0.0
                    H[2 * p + h, k] = case["lead"][2 * p + h, k]
    H[er:M] = case["Hd"]
    return H[:M]


def _pairs_case(rng, N, used, scale=1.0, R=(1.0,), neutral=(), lead_k=0, dense_rows=0, **kw):
    """compressed pairs with used[p] slots in use (common slots first), optionally neutralised pairs, a lead block, dense
    rows behind them"""
    pairs = len(used)
    er, M = 2 * pairs, 2 * pairs + dense_rows
    idx = np.zeros((pairs, W), dtype=np.int64)
    val = np.zeros((pairs, W, 2))
    lo = lead_k                                                      # the compressed columns lie behind the lead block's
    for p, n in enumerate(used):
        cols = lo + rng.permutation(N - lo)[:n]
        slots = list(range(16))[:min(n, 16)] + list(range(16, 16 + max(0, n - 16)))
        idx[p, slots] = cols
        val[p, slots] = rng.normal(size=(n, 2)) * scale
    lead = rng.normal(size=(2 * pairs, lead_k)) * scale * (rng.uniform(size=(2 * pairs, lead_k)) < 0.5)
    inn = rng.normal(size=M) * scale
    Rv = np.resize(np.asarray(R, dtype=np.float64), M).copy()
    for p in neutral:                                                # what a gate leaves of a rejected pair
        val[p] = 0.0; inn[2 * p:2 * p + 2] = 0.0; Rv[2 * p:2 * p + 2] = 1.0
        if lead_k:
            lead[2 * p:2 * p + 2] = 0.0
    Hd = rng.normal(size=(dense_rows, N)) * scale * (rng.uniform(size=(dense_rows, N)) < 0.4)
    dx = rng.normal(size=N) / max(scale, 1e-300) * 1e-2 if scale >= 1 else rng.normal(size=N) * 1e-2
    c = dict(M=M, N=N, er=er, idx=idx, val=val, lead=lead, lead_k=lead_k, Hd=Hd, inn=inn, R=Rv, dx=dx)
    c.update(kw)
    return c


def _cases():
    rng = np.random.default_rng(11)
    out = []
    out.append(("slots_1_12_28_0", _pairs_case(rng, 59, [1, 12, 28, 0])))
    out.append(("neutralised_pair", _pairs_case(rng, 59, [18, 18, 18], neutral=[1])))
    out.append(("R_1_and_1e-12", _pairs_case(rng, 59, [21, 21], R=[1.0, 1e-12])))
    out.append(("scale_1e150", _pairs_case(rng, 64, [21, 12], scale=1e150, R=[1e300])))
    out.append(("scale_1e-150", _pairs_case(rng, 64, [21, 12], scale=1e-150, R=[1e-300])))
    den = _pairs_case(rng, 64, [21, 12], scale=1.0, R=[1.0])
    den["val"] *= 1e-310; den["inn"] *= 1e-310; den["R"][:] = 1.0    # subnormal rows: every product underflows to a subnormal or 0
    out.append(("denormal", den))
    out.append(("lead_block", _pairs_case(rng, 96, [18, 9, 0], lead_k=48)))
    out.append(("mixed_dense_rows", _pairs_case(rng, 59, [18, 18], dense_rows=5)))
    out.append(("all_dense_odd_M", dict(_pairs_case(rng, 37, [], dense_rows=7), er=0)))
    big = _pairs_case(rng, 64, [21] * 140, dense_rows=3)            # more rows than threads: two rows per thread
    out.append(("283_rows", big))
    out.append(("failed_update", _pairs_case(rng, 59, [18, 18], status=3)))
    out.append(("ldlt_update", _pairs_case(rng, 59, [18, 18], ldlt=1)))
    return out


def _slots(case):
    return case["N"] if case["er"] == 0 else max(W + case.get("lead_k", 0), case["N"] if case["er"] < case["M"] else 0)


def test_row_driver_agrees_with_the_restatement(exes):
    """every representation of the rows, the edge scales and the flags through the header's arithmetic, against the
    longdouble restatement on the dense form of the same rows; dof / rows / flags / the maxima exact"""
    names, cases = zip(*_cases())
    layout, recs = _run(exes[0], cases)
    worst = 0.0
    for name, case, rec in zip(names, cases, recs):
        ref = ir.restate(_dense(case), case["inn"], case["R"], case["dx"], case.get("status", 0), case.get("ldlt", 0), w=_slots(case))
        worst = max(worst, ir.check(rec, ref, name))
    print("innov row driver: worst error / bound %.3f" % worst)
    by = dict(zip(names, recs))
    assert by["slots_1_12_28_0"]["dof"] == 8 and by["slots_1_12_28_0"]["rows"] == 8           # the empty pair counts: its inn is not 0
    assert by["neutralised_pair"]["dof"] == 4 and by["neutralised_pair"]["rows"] == 6
    assert by["failed_update"]["flags"] == 1 and np.isnan(by["failed_update"]["nis"]) and by["failed_update"]["dof"] == 4
    assert by["ldlt_update"]["flags"] == 2 and np.isfinite(by["ldlt_update"]["nis"])
    assert by["283_rows"]["dof"] == 283
    assert by["denormal"]["prefit"] >= 0 and np.isfinite(by["denormal"]["nis"])


def test_empty_and_absent_rows_are_not_counted(exes):
    rng = np.random.default_rng(5)
    c = _pairs_case(rng, 59, [0, 0, 9])
    c["inn"][:4] = 0.0                                              # two absent features: empty rows, no innovation
    _, (rec,) = _run(exes[0], [c])
    assert rec["dof"] == 2 and rec["rows"] == 6
    ref = ir.restate(_dense(c), c["inn"], c["R"], c["dx"], w=W)
    ir.check(rec, ref, "absent")
    c["val"][:] = 0.0; c["inn"][:] = 0.0                            # nothing at all
    _, (rec,) = _run(exes[0], [c])
    assert rec["dof"] == 0 and rec["nis"] == 0.0 and rec["prefit"] == 0.0 and rec["inn_max"] == 0.0 and rec["dx_max"] > 0


def test_nan_in_dx_propagates_through_the_columns_in_use(exes):
    rng = np.random.default_rng(6)
    c = _pairs_case(rng, 59, [12, 12])
    used = int(c["idx"][0, 3])
    unused = next(n for n in range(59) if n not in set(c["idx"][c["val"].any(axis=2)].tolist()) and n != 0)
    a = dict(c, dx=c["dx"].copy()); a["dx"][used] = np.nan
    b = dict(c, dx=c["dx"].copy()); b["dx"][unused] = np.nan
    z = dict(c, dx=c["dx"].copy()); z["dx"][0] = np.nan             # column 0 is what the unused slots name
    col0_used = 0 in set(c["idx"][c["val"].any(axis=2)].tolist())
    _, (ra, rb, rz) = _run(exes[0], [a, b, z])
    assert np.isnan(ra["nis"]) and np.isnan(ra["postfit"]) and np.isfinite(ra["prefit"]) and np.isnan(ra["dx_max"])
    assert np.isfinite(rb["nis"]) and np.isnan(rb["dx_max"])        # a column no row uses: the sums do not see it
    assert col0_used or np.isfinite(rz["nis"])
    assert ra["flags"] == 0 and ra["dof"] == 4


def test_sanitizer_build_of_the_driver_runs_clean(exes):
    """address + undefined-behaviour sanitizers on the host build of the header's arithmetic, run as a program"""
    _, cases = zip(*_cases())
    text = "".join(_text(c) for c in cases)
    plain, san = (subprocess.run([e], input=text, capture_output=True, text=True, check=True) for e in exes)
    assert plain.stdout == san.stdout and san.stderr == ""           # (the printed hex floats: NaN compares as text)


def test_record_dtype_is_the_c_struct(exes):
    from xivo_amd import lib as L
    layout, _ = _run(exes[0], [])
    got = dict(kv.split("=") for kv in layout.split()[1:])
    assert int(got.pop("sizeof")) == L.innov_rec_dtype.itemsize == 64
    assert {k: int(v) for k, v in got.items()} == {k: L.innov_rec_dtype.fields[k][1] for k in L.innov_rec_dtype.names}
    assert L.innov_opts_dtype.itemsize == 4 and (L.INNOV_FAILED, L.INNOV_LDLT) == (1, 2)


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "xivo_amd", "csrc", "innov_device.h")).read().split("#pragma once")[1]
    assert text.count("hip/") == 1 and text.index("#if defined(__HIPCC__)") < text.index("hip/") < text.index("#else")
    assert "atomic" not in text


def test_library_exports_the_innovation_log(built):
    from xivo_amd import lib as L
    lib = L.load_library()
    for name in INNOV_SYMBOLS:
        assert name in L.ALL_SYMBOLS and hasattr(lib, name), name
    from xivo_amd.batch import load_host_library
    assert hasattr(load_host_library(), "xivo_batch_innov_log")


def test_calls_without_a_context_return_status_codes(built):
    """No context, so no device: every entry point has to refuse on its arguments alone."""
    from xivo_amd import lib as L
    lib = L.load_library()
    o = np.zeros(1, dtype=L.innov_opts_dtype); o["T_max"] = 4
    k = C.c_int(7)
    buf = np.zeros(64)
    assert lib.xivo_hip_innov_config(None, o.ctypes.data) == -1
    assert lib.xivo_hip_innov_record(None, 1, 0, C.byref(k)) == -1 and k.value == 7
    assert lib.xivo_hip_innov_count(None) == -1
    assert lib.xivo_hip_innov_reset(None) == -1
    assert lib.xivo_hip_innov_read(None, 0, 1, 0, 1, buf.ctypes.data, None) == -1
    assert lib.xivo_hip_innov_stats(None, 0, 1, 0, 1, buf.ctypes.data, None, None, None, None, None) == -1


def test_batch_cfg_size_is_unchanged(built):
    from xivo_amd import batch
    assert batch.load_host_library().xivo_batch_cfg_size() == batch.batch_cfg_dtype.itemsize


def test_run_pcw_with_a_backend_without_the_log():
    """the oracle backend has no enable_innovation_log: run_pcw(innovation_log=True) leaves the report keys out and does not
    raise, and the run is the run without the flag"""
    from seq_oracle import OracleBackend
    from xivo_amd import pcw, sequence
    assert not hasattr(OracleBackend, "enable_innovation_log")
    runs = {}
    for flag in (False, True):
        cfg = sequence.SequenceConfig()
        worlds = [pcw.RandomPCW(npts=300, seed=3)]
        sims = [pcw.TrajectorySim("lissajous", seed=103)]
        runs[flag] = sequence.run_pcw(OracleBackend, cfg, worlds, sims, total_time=0.2, innovation_log=flag)
    on, off = runs[True], runs[False]
    for k in ("nis_per_dof", "nis_per_dof_seq", "nis_used", "nis_records_left_out", "innovation"):
        assert k not in on and k not in off
    assert np.array_equal(on["Tsb"], off["Tsb"]) and np.array_equal(on["ts"], off["ts"])


def test_restatement_on_a_case_by_hand():
    H = np.array([[2.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    r = ir.restate(H, [3.0, 0.0, 1.0], [2.0, 1.0, 4.0], [0.5, 7.0])
    # row 0: r = 3 - 1 = 2; row 1 not counted; row 2 counted through its innovation, r = 1
    assert r["dof"] == 2 and float(r["nis"]) == 3 * 2 / 2 + 1 / 4 and float(r["prefit"]) == 9 / 2 + 1 / 4
    assert float(r["postfit"]) == 4 / 2 + 1 / 4 and r["inn_max"] == 3.0 and r["dx_max"] == 7.0 and r["flags"] == 0
    assert ir.chain(60) == 9 and ir.chain(257) == 10
