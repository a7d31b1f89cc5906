"""CPU-only: the feature-pool entry points (include/xivo_hip.h xivo_hip_pool_*) are exported and bound, reject NULL /
out-of-range arguments with a status code without touching a device, and the reference cfg keys of the "subfilter" life
cycle reach SequenceConfig."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_SYMBOLS = ("xivo_hip_pool_config", "xivo_hip_pool_anchor", "xivo_hip_pool_add", "xivo_hip_pool_step", "xivo_hip_pool_get")


def test_pool_symbols_are_exported_and_bound(built):
    from xivo_amd.lib import ALL_SYMBOLS, lib_path, load_library
    lib = ctypes.CDLL(lib_path())
    for name in POOL_SYMBOLS:
        assert hasattr(lib, name) and name in ALL_SYMBOLS, name
    load_library()


def test_pool_record_layouts_and_edit_kinds():
    import numpy as np
    from xivo_amd import lib as L
    assert L.pool_new_dtype.itemsize == 64 and L.pool_new_dtype.fields["xp"][1] == 16
    # appended after XIVO_EDIT_SET_XP; the existing kinds keep their values
    assert (L.EDIT_SET_XP, L.EDIT_ADD_GROUP_ANCHOR, L.EDIT_ADMIT_POOL) == (7, 8, 9)
    hdr = open(os.path.join(ROOT, "include", "xivo_hip.h")).read()
    assert "XIVO_EDIT_ADD_GROUP_ANCHOR = 8" in hdr and "XIVO_EDIT_ADMIT_POOL = 9" in hdr
    assert "#define XIVO_POOL_MAX_ENTRIES %d" % L.POOL_MAX_ENTRIES in hdr
    assert np.dtype(L.subfilter_opts_dtype).itemsize == 48


def test_pool_entry_points_reject_bad_arguments_without_a_device(built):
    import numpy as np
    from xivo_amd import lib as L
    lib = L.load_library()
    o = np.zeros(1, dtype=L.subfilter_opts_dtype)
    p = o.ctypes.data_as(ctypes.c_void_p)
    assert lib.xivo_hip_pool_config(None, 16, 4, p, 10.0) == -1
    assert lib.xivo_hip_pool_anchor(None, 0, 1, p) == -1
    assert lib.xivo_hip_pool_add(None, 1, p) == -1
    assert lib.xivo_hip_pool_step(None, 1, p, 0, p, p, p) == -1
    assert lib.xivo_hip_pool_get(None, 0, 1, None, None, None) == -1
    assert lib.xivo_hip_pool_add(None, -1, None) == -1 and lib.xivo_hip_pool_step(None, 0, None, 0, None, None, None) == -1


def test_reference_cfg_keys_of_the_subfilter_life_cycle():
    from xivo_amd import pyxivo, sequence
    c = sequence.SequenceConfig()
    assert c.feature_init == "immediate"           # the default life cycle is unchanged
    cfg = {"initial_z": 0.25, "remove_outlier_counter": 7, "strict_criteria_timesteps": 3, "max_group_lifetime": 60,
           "max_subfilter_outlier": 0.02, "subfilter": {"visual_meas_std": 3.0, "ready_steps": 2, "MH_thresh": 8.991}}
    c = pyxivo.config_from_cfg(cfg)
    assert (c.initial_z, c.remove_outlier_counter, c.strict_criteria_timesteps, c.max_group_lifetime) == (0.25, 7.0, 3, 60)
    assert c.max_subfilter_outlier == 0.02
    assert c.subfilter == dict(visual_meas_std=3.0, MH_thresh=8.991, ready_steps=2)
    assert isinstance(c.subfilter["ready_steps"], int)
    assert sequence.SequenceConfig().subfilter == dict(visual_meas_std=3.5, MH_thresh=5.991, ready_steps=5)


def test_host_library_exports_the_subfilter_life_cycle(built):
    from xivo_amd import batch
    host = batch.load_host_library()
    for name in ("xivo_batch_enable_subfilter", "xivo_batch_pool_stats", "xivo_batch_subfilter_cfg_size"):
        assert hasattr(host, name), name
    # the numpy mirror of struct xivo_batch_subfilter_cfg has the size the C++ side compiled
    assert batch.batch_subfilter_cfg_dtype.itemsize == host.xivo_batch_subfilter_cfg_size() == 80
