"""Estimator::Propagate on the device - propagate_state_wave_kernel<4|7>, propagate_state_calib_kernel and the covariance tail -
against the 80-bit restatement of the reference (tests/propagate_restate.py) on the families and exact step cases of
tests/propagate_edge_cases.py. Every bound is computed on the spot as that module describes (4 x the fp64 oracle's own error
against the restatement, per batch and metric, floored at 4 * 2^-53); tests/test_propagate_accuracy_cpu.py holds them under the
suite's typed-in tolerances. Also here: the inputs both entry points refuse because their sub-step loop would not end, and a
mixed batch against its filters run alone."""
import numpy as np
import pytest

import propagate_edge_cases as pc
from scene_util import scene_arrays
from xivo_amd import synth
from xivo_amd.lib import Context, XivoHipError, calib_dtype, imu_dtype

pytestmark = pytest.mark.gpu
CAM = synth.PINHOLE
STATE_FIELDS = ("bg", "ba", "Rsg", "Rbc", "Tbc")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _imu_records(bt):
    imu = np.zeros((bt.B, bt.n), dtype=imu_dtype)
    imu["gyro"], imu["accel"], imu["slope_gyro"], imu["slope_accel"], imu["dt"] = (bt.imu[k] for k in ("gyro", "accel", "sg", "sa", "dt"))
    return imu


class Device:
    """a context holding a batch's filters; run() propagates them as the batch says (one call, or two at bt.split)"""

    def __init__(self, bt):
        self.bt = bt
        lay = bt.layout
        sc = synth.g_level(pc.NG, pc.NF, pc.NF, bt.B, seed=7, cam=CAM)
        self.poses, self.groups, self.feats, _ = scene_arrays(sc, CAM)
        for b, X in enumerate(bt.X0):
            p = self.poses[b]
            p["Rsb"] = X.Rsb.T.reshape(-1); p["Tsb"] = X.Tsb; p["Vsb"] = X.Vsb; p["bg"] = X.bg; p["ba"] = X.ba
            p["Rsg"] = X.Rsg.T.reshape(-1)
        self.imu = _imu_records(bt)
        self.ctx = Context(bt.N, 2 * pc.NF, bt.B)
        gb = 23 if lay is None else lay.group_begin
        self.ctx.set_layout(bt.N, gb, pc.NG, gb + 6 * pc.NG, pc.NF, CAM)
        if lay is not None:
            self.ctx.set_calib(lay.td, lay.Cg, lay.cam_begin, lay.cam_dim)
            self.calib = np.zeros(bt.B, dtype=calib_dtype)
            for b in range(bt.B):
                self.calib[b]["Cg"] = bt.Cg[b].T.reshape(-1); self.calib[b]["Ca"] = bt.Ca[b].T.reshape(-1)
                self.calib[b]["td"] = bt.td[b]; self.calib[b]["gyro"] = bt.imu["gyro"][b, 0]

    def __enter__(self):
        self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)

    def load(self):
        self.ctx.upload_P(self.bt.P0)
        if self.bt.name.startswith("asym"):
            # xivo_hip_upload_P keeps the lower triangle and mirrors it; xivo_hip_propagate_cov writes the P_mm it is handed as it
            # is (Phi = I leaves the cross blocks alone, exactly): the one way to hand the device an asymmetric motion block
            self.ctx.propagate_cov(np.tile(np.eye(23), (self.bt.B, 1, 1)), self.bt.P0[:, :23, :23])
            assert np.array_equal(self.ctx.download_P(), self.bt.P0)
        self.ctx.set_scene(self.poses, self.groups, self.feats)
        if self.bt.layout is not None:
            self.ctx.set_calib_state(self.calib)

    def propagate(self, imu, b0=0, stepsize=None, max_scale=None):
        bt = self.bt
        ms = bt.ctl if max_scale is None else max_scale
        ctl = None if ms is None else dict(tolerance=1e-3, attempts=12, min_scale_factor=0.125, max_scale_factor=ms)
        f = self.ctx.propagate if bt.layout is None else self.ctx.propagate_calib
        f(imu, bt.Qi, bt.Qm, bt.g, method=bt.method, stepsize=bt.stepsize if stepsize is None else stepsize, b0=b0, pd_control=ctl)

    def run(self):
        cuts = [0, self.bt.n] if self.bt.split is None else [0, self.bt.split, self.bt.n]
        for a, e in zip(cuts[:-1], cuts[1:]):
            self.propagate(self.imu[:, a:e])
        return self.read()

    def read(self):
        return self.ctx.download_P(), self.ctx.get_scene()[0]


def _check_batch(key, extra=None, coded=False):
    """run the batch, assert every filter's metrics within the bounds and what must not change bit for bit; -> (ev, P, poses)"""
    ev = pc.evaluated(key)
    bt = ev.bt
    with Device(bt) as dev:
        dev.load()
        P, poses = dev.run()
    worst = {}
    nm = bt.nm
    for b in range(bt.B):
        Rsb = poses[b]["Rsb"].reshape(3, 3).T
        if extra is not None:
            ev.check(b, P[b], Rsb, poses[b]["Tsb"], poses[b]["Vsb"], extra(ev, b))
        got = ev.check(b, P[b], Rsb, poses[b]["Tsb"], poses[b]["Vsb"], coded=coded) if extra is None or coded else {}
        for m, v in got.items():
            worst[m] = max(worst.get(m, 0.0), v)
        assert np.array_equal(P[b][nm:, nm:], bt.P0[b][nm:, nm:]), b         # outside the motion rows and columns
        for f in STATE_FIELDS:
            assert np.array_equal(poses[b][f], dev.poses[b][f]), (b, f)
    print("device worst %s: %s" % (key, " ".join("%s=%.1e/%.1e" % (m, worst[m], ev.bounds[m]) for m in worst)))
    return ev, P, poses


FAMILIES = [k for k in sorted(pc.BATCHES, key=str) if k[0] not in ("asym", "mixed")]


@pytest.mark.parametrize("key", FAMILIES, ids=str)
def test_propagate_against_the_80_bit_restatement(built, key):
    """one launch (two for the controlled chains) of the batch's filters: P by relative Frobenius error, in units of the prior's
    standard deviations and by its symmetry defect; Rsb, Tsb, Vsb and the orthogonality defect of Rsb; bg, ba, Rsg and every
    entry of P outside the motion rows and columns bit for bit"""
    ev, P, poses = _check_batch(key)
    bt = ev.bt
    if key[0] == "at_rest":          # Rsb accel_calib + Rsg g == 0 exactly: nothing to integrate
        for b in range(bt.B):
            assert not poses[b]["Vsb"].any() and np.array_equal(poses[b]["Tsb"], bt.X0[b].Tsb), b
    if key[0] == "no_rotation":      # w == 0 in every stage: exp is the identity, exactly
        for b, mag in bt.tags.items():
            if mag == 0.0:
                assert np.array_equal(poses[b]["Rsb"].reshape(3, 3).T, bt.X0[b].Rsb), b
    if key[0] == "long_chain":       # copies of one filter: one result
        for b in range(1, bt.B):
            assert np.array_equal(P[b], P[0]) and _same(poses[b], poses[0]), b


@pytest.mark.parametrize("rel", [0, 1e-9])
@pytest.mark.parametrize("method", pc.METHODS)
def test_propagate_asymmetric_prior(built, method, rel):
    """P_mm with an upper triangle a few ulps, or 1e-9, off the lower one, planted through xivo_hip_propagate_cov. The reference
    multiplies the P it was given, the device takes P0 F^T as (F P0)^T: the device is pinned to that form, as coded, at the plain
    bounds. At a few ulps - what propagation itself emits, through G Q G^T - it also stays within the bounds plus one additive
    term against the reference as it is: the restatement's own distance between the result on P and on its symmetrised copy.
    At 1e-9, which no route of the library emits, the as-coded form itself is up to 2.04 times that away from the reference
    (corr; tests/test_propagate_accuracy_cpu.py), a deliberate deviation, and only the pin is asserted."""
    _check_batch(("asym", method, rel), extra=pc.asym_extra if rel == 0 else None, coded=True)


@pytest.mark.parametrize("method", pc.METHODS)
def test_mixed_batch_equals_its_filters_run_alone(built, method):
    """fast-spin, no-rotation and nominal filters in one launch: each bit for bit what it is when launched alone (the halving
    loop of so3_exp_small has a trip count per lane of the pre-pass and per filter)"""
    ev, P, poses = _check_batch(("mixed", method))
    bt = ev.bt
    with Device(bt) as dev:
        for b in range(bt.B):
            dev.load()
            dev.propagate(dev.imu[b:b + 1], b0=b)
            P1, poses1 = dev.read()
            assert np.array_equal(P1[b], P[b]) and _same(poses1[b], poses[b]), (b, bt.tags[b])
            others = [o for o in range(bt.B) if o != b]
            assert np.array_equal(P1[others], bt.P0[others]) and _same(poses1[others], dev.poses[others]), b


def _refused(dev, imu, **kw):
    with pytest.raises(XivoHipError) as e:
        dev.propagate(imu, **kw)
    assert e.value.status == -1
    P, poses = dev.read()
    assert np.array_equal(P, dev.bt.P0) and _same(poses, dev.poses)


@pytest.mark.parametrize("key", [("controlled", 4.0), ("calib", "PrinceDormand", 24)], ids=str)
def test_inputs_whose_step_loop_would_not_end_are_refused(built, key):
    """xivo_hip_propagate and xivo_hip_propagate_calib return XIVO_HIP_ERR_INVALID before anything is uploaded or launched for a
    dt that is not finite, a stepsize that is NaN and, under control_stepsize, a max_scale_factor below 1 (or NaN): P and the
    poses bit for bit, and a valid call afterwards gives what it gives on a fresh context (the carried steps included)."""
    bt = pc.evaluated(key).bt
    with Device(bt) as dev:
        dev.load()
        fresh_P, fresh_poses = dev.run()
    with Device(bt) as dev:
        dev.load()
        for bad in (np.inf, np.nan):
            imu = dev.imu.copy()
            imu["dt"][bt.B - 1, bt.n - 1] = bad
            _refused(dev, imu)
        _refused(dev, dev.imu, stepsize=np.nan)
        for ms in (0.5, 1.0 - 2.0 ** -53, 0.0, np.nan):
            _refused(dev, dev.imu, max_scale=ms)
        P, poses = dev.run()
        assert np.array_equal(P, fresh_P) and _same(poses, fresh_poses)


def test_trajsim_frame_refuses_a_sample_time_that_is_not_finite(built):
    """xivo_hip_propagate_resident cannot read the records it is handed, so xivo_hip_trajsim_frame vouches for their dt: with a
    finite imu_dt of 1e305, t_1797 is finite and t_1798 = +inf, so dt_1798 = +inf passes a `dt > 0` test. The frame is refused
    before its kernel is enqueued (status -1) and the ground-truth log stays empty; nothing is launched by this test."""
    with Context(38, 6, 2) as ctx:
        ctx.trajsim_config(4, T_max=3, imu_dt=1e305)
        assert np.isfinite(1797.0 * 1e305) and np.isinf(1798.0 * 1e305) and 1795.0 * 1e305 - 1794.0 * 1e305 > 0
        for k0, n in ((1794, 4), (1797, 1), (2 ** 63, 4)):
            with pytest.raises(XivoHipError) as e:
                ctx.trajsim_frame(k0, n)
            assert e.value.status == -1 and ctx.trajsim_count() == 0

