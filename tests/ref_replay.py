"""The compiled reference (oracle/_ref) for the tests that compare against it - live, or as stored calls.

oracle/_ref is built from the reference's own sources where they lie (oracle/ref/Makefile) and a clean checkout does not
have it. Where it is built, `reference()` hands the tests the library itself. Where it is not, it hands them a stand-in that
answers every call, in the order the test makes them, with what the library returned for that call on the same seeded
inputs - stored in tests/golden/ref_calls.npz by tests/golden/make_ref_calls.py, which runs the tests with XIVO_REF_RECORD
set. Every stored call carries a fingerprint of its inputs (size, sum, sum of magnitudes), checked on replay: inputs that
drifted fail the test rather than meet the outputs of other inputs. Arguments the library writes into are stored and
written back the same way.

Tests whose calls return large matrices that are not kept (several covariances of N = 150 .. 251 each: megabytes that no
compression removes, since what they hold is the reference's rounding) ask for reference(..., stored=False) and run where
oracle/_ref is built only; tests/test_oracle_pinned.py names, next to each, the golden-vector test that makes the same
comparison of the oracle with the reference where there is one."""
import atexit
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls.npz")
RECORD = os.environ.get("XIVO_REF_RECORD")      # recording run: where the calls go
FP_RTOL = 1e-9

_seq = {"test": None, "n": 0}
_rec = {"calls": {}, "attrs": {}}
_rec_arrays = {}
_replay = None


def _next_key():
    """<test module>::<test name>#<number of this call within the test> (the same from whichever directory pytest runs)"""
    path, _, name = os.environ.get("PYTEST_CURRENT_TEST", "").rsplit(" (", 1)[0].partition("::")
    test = os.path.basename(path) + "::" + name
    if test != _seq["test"]:
        _seq["test"], _seq["n"] = test, 0
    _seq["n"] += 1
    return "%s#%d" % (test, _seq["n"])


def _store(a):
    a = np.ascontiguousarray(a)
    k = "a" + hashlib.sha1(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()[:16]
    _rec_arrays[k] = a                           # (equal outputs of two builds are stored once)
    return k


def _mirror_xor(y):
    """(uint64 view of) a square matrix with its strict lower triangle XOR-ed with the mirrored upper one - its own inverse"""
    y = y.copy()
    il = np.tril_indices(y.shape[0], -1)
    y[il] ^= y.T[il]
    return y


def _enc_array(a, inputs):
    """A float64 array is stored as itself; or as the entries in which it differs from an input of the same shape (an
    integrator leaves most of P as it was: on replay those entries come from the input the test passes); or with its lower
    triangle XOR-ed with the mirrored upper one (a covariance that is symmetric to the last bits) - whichever compresses
    best. Exact either way."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64 or a.size < 64:
        return {"__a": _store(a)}
    bits = a.view(np.uint64)
    size = lambda *parts: sum(len(zlib.compress(q.tobytes(), 6)) for q in parts)
    options = [(size(bits), lambda: {"__bits": _store(bits)})]
    for i, b in enumerate(inputs):
        if b.shape == a.shape and b.dtype == a.dtype:
            same = bits == np.ascontiguousarray(b).view(np.uint64)
            mask = np.packbits(same.ravel())
            options.append((size(mask, bits[~same]),
                            lambda i=i, mask=mask, same=same: {"same_as_in": i, "mask": _store(mask), "__bits": _store(bits[~same])}))
    if a.ndim == 2 and a.shape[0] == a.shape[1]:
        y = _mirror_xor(bits)
        options.append((size(y), lambda: {"xor_mirror": True, "__bits": _store(y)}))
    return min(options, key=lambda o: o[0])[1]()


def _dec_array(obj, arrays, inputs):
    if "__a" in obj:
        return arrays[obj["__a"]].copy()
    y = arrays[obj["__bits"]].copy()
    if "same_as_in" in obj:
        base = np.ascontiguousarray(inputs[obj["same_as_in"]], dtype=np.float64).copy()
        same = np.unpackbits(arrays[obj["mask"]], count=base.size).astype(bool).reshape(base.shape)
        base.view(np.uint64)[~same] = y
        return base
    if obj.get("xor_mirror"):
        y = _mirror_xor(y)
    return y.view(np.float64)


def _enc(obj, inputs=()):
    if isinstance(obj, np.ndarray):
        return _enc_array(obj, inputs)
    if isinstance(obj, np.bool_):
        return bool(obj)
    if isinstance(obj, np.integer):
        return int(obj)
    if isinstance(obj, np.floating):
        return float(obj)
    if isinstance(obj, tuple):
        return {"__t": [_enc(v, inputs) for v in obj]}
    if isinstance(obj, list):
        return [_enc(v, inputs) for v in obj]
    if isinstance(obj, dict):
        return {"__d": {str(k): _enc(v, inputs) for k, v in obj.items()}}
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    raise TypeError(f"cannot store a {type(obj).__name__} returned by the reference")


def _dec(obj, arrays, inputs=()):
    if isinstance(obj, list):
        return [_dec(v, arrays, inputs) for v in obj]
    if isinstance(obj, dict):
        if "__a" in obj or "__bits" in obj:
            return _dec_array(obj, arrays, inputs)
        if "__t" in obj:
            return tuple(_dec(v, arrays, inputs) for v in obj["__t"])
        return {k: _dec(v, arrays, inputs) for k, v in obj["__d"].items()}
    return obj


def _fingerprint(args, kwargs):
    vals = []

    def walk(o):
        if isinstance(o, np.ndarray):
            if o.dtype.kind in "fiub":
                vals.append(o.astype(np.float64).ravel())
        elif isinstance(o, (int, float, np.number)):
            vals.append(np.array([float(o)]))
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for k in sorted(o, key=str):
                walk(o[k])
        elif hasattr(o, "__dict__"):
            for _, v in sorted(vars(o).items()):
                walk(v)

    walk(args)
    walk(kwargs)
    v = np.concatenate(vals) if vals else np.zeros(0)
    return [int(v.size), float(v.sum()), float(np.abs(v).sum())]


def _arrays_in(args, kwargs):
    return [(i, a) for i, a in enumerate(list(args) + [kwargs[k] for k in sorted(kwargs)]) if isinstance(a, np.ndarray)]


class _Recorder:
    """The live library; every call and attribute read is also stored (recording runs only)."""

    def __init__(self, name, live):
        self._name, self._live = name, live

    def __getattr__(self, attr):
        v = getattr(self._live, attr)
        if attr == "lib" or attr.startswith("_"):
            return v
        if not callable(v):
            _rec["attrs"][f"{self._name}.{attr}"] = _enc(v)
            return v

        def call(*args, **kwargs):
            fp = _fingerprint(args, kwargs)
            before = [(i, a.copy()) for i, a in _arrays_in(args, kwargs)]
            out = v(*args, **kwargs)
            after = dict(_arrays_in(args, kwargs))
            inputs = [a for _, a in before]
            written = {str(i): _enc(after[i], inputs) for i, a in before
                       if not np.array_equal(a, after[i], equal_nan=a.dtype.kind == "f")}
            _rec["calls"][_next_key()] = {"lib": self._name, "fn": attr, "fp": fp, "out": _enc(out, inputs), "written": written}
            return out
        return call


class _NoFunction:
    def __call__(self, *args, **kwargs):
        return None


class _NoLibrary:
    """Stands in for the ctypes handle on replay: configuration calls straight into the library do nothing (their effect is
    in the stored outputs)."""

    def __getattr__(self, name):
        return _NoFunction()


class _Replay:
    """Answers the calls of one test from tests/golden/ref_calls.npz."""

    def __init__(self, name):
        self._name = name
        self.lib = _NoLibrary()

    def __getattr__(self, attr):
        index, arrays = _load()
        key = f"{self._name}.{attr}"
        if key in index["attrs"]:
            return _dec(index["attrs"][key], arrays)

        def call(*args, **kwargs):
            k = _next_key()
            rec = index["calls"].get(k)
            assert rec is not None and (rec["lib"], rec["fn"]) == (self._name, attr), \
                f"{k}: no stored call {self._name}.{attr} (tests/golden/make_ref_calls.py regenerates ref_calls.npz)"
            n, s, a = _fingerprint(args, kwargs)
            n0, s0, a0 = rec["fp"]
            assert n == n0 and abs(a - a0) <= FP_RTOL * a0 and abs(s - s0) <= FP_RTOL * a0, \
                f"{k}: the inputs of {self._name}.{attr} are not the ones stored ({(n, s, a)} vs {(n0, s0, a0)})"
            arrs = _arrays_in(args, kwargs)
            inputs = [a.copy() for _, a in arrs]
            for i, w in rec["written"].items():
                np.copyto(dict(arrs)[int(i)], _dec(w, arrays, inputs))
            return _dec(rec["out"], arrays, inputs)
        return call


def _load():
    global _replay
    if _replay is None:
        with np.load(GOLDEN) as z:
            index, data = json.loads(bytes(z["index"]).decode()), z["data"]
        arrays = {k: np.frombuffer(data, dtype=dt, count=int(np.prod(shape)), offset=off).reshape(shape)
                  for k, (dt, shape, off) in index["arrays"].items()}
        _replay = (index, arrays)
    return _replay


def _save():
    """One compressed blob of every stored array (a member per array would cost more in headers than the small ones hold)"""
    keys = sorted(_rec_arrays)
    offs = np.cumsum([0] + [_rec_arrays[k].nbytes for k in keys])
    _rec["arrays"] = {k: [_rec_arrays[k].dtype.str, list(_rec_arrays[k].shape), int(o)] for k, o in zip(keys, offs)}
    data = np.frombuffer(b"".join(_rec_arrays[k].tobytes() for k in keys), dtype=np.uint8)
    index = np.frombuffer(json.dumps(_rec, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(RECORD, index=index, data=data)


if RECORD:
    atexit.register(_save)


def reference(name, loader, stored=True):
    """loader() - oracle/_ref's library - when it is built; else the stored calls of the library under `name`.
    stored=False: the test runs against the library only and skips where it is not built (its calls are not stored)."""
    try:
        live = loader()
    except (FileNotFoundError, OSError):
        if RECORD and stored:
            raise
        if not stored:
            pytest.skip("oracle/_ref not built (this test runs against the library only)")
        return _Replay(name)
    return _Recorder(name, live) if RECORD and stored else live
