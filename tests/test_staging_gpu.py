"""The producers of staged measurement rows in sequence, through the public API only: what one producer leaves must not leak
into what the next one stages. Every sequence ends in updates whose P+, dx are held against the extended-precision reference
of tests/precise_ref.py on the rows as staged (xivo_hip_get_H of an identically staged twin context, or the sequence's own
get_H where it has one), the gate masks against the oracle's gate on those rows, and get_H against the twin's; the twin's
in-state rows of a default context are themselves held against the oracle's stacking.

Run as a script (python tests/test_staging_gpu.py [sequence ...]) it prints one line per step - last_route, last_path, the
return code and SHA-256 of P, dx, status, mask, dist and H - so that two builds of the library can be compared line for line."""
import hashlib
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import precise_ref as pr
import xivo_oracle as orc
from helpers import rel_fro, TOL_DX
from scene_util import oracle_jacobians, spd
from xivo_amd import synth
from xivo_amd.lib import (Context, XivoHipError, lc_dtype, FLAG_DENSE_H, FLAG_SYMMETRIC_FORM, FLAG_STANDALONE_TAIL,
                          FLAG_THROUGHPUT_ROUTE)

pytestmark = pytest.mark.gpu
R, MH, MULT, MIN_INL, ROOS = 2.25, 5.991, 1.1, 5, 3.5 ** 2
GATE = (MH, MULT, MIN_INL)
FLAGSETS = {"default": 0, "dense_h": FLAG_DENSE_H, "symmetric": FLAG_SYMMETRIC_FORM, "tail": FLAG_STANDALONE_TAIL}


def _sha(a):
    return "-" if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


class Trace:
    """One line per step. The read-backs it makes (P, dx, status, get_gate) change nothing on the context."""

    def __init__(self, out=None):
        self.out = out

    def step(self, name, ctx, F, rows=None, rc=0):
        if self.out is None:
            return
        try:
            mask, dist = ctx.get_gate(F)
        except XivoHipError:
            mask = dist = None
        H = None if rows is None else np.concatenate([np.concatenate([r[0].ravel(), r[1], r[2]]) for r in rows])
        self.out.write("%s route=%s path=%d rc=%d P=%s dx=%s st=%s mask=%s dist=%s H=%s\n" % (
            name, ctx.last_route(), ctx.last_path(), rc, _sha(ctx.download_P()), _sha(ctx.get_err()),
            _sha(ctx.get_status(check=False)), _sha(mask), _sha(dist), _sha(H)))


def _verify(rows, P0, ctx, what, keep=None, posterior=False):
    """P+ and dx of the update just run against the 80-bit reference on `rows` (per filter H, inn, diagR) from the prior P0,
    within the 8 u (kappa + N) bound of precise_ref. posterior: P0 is itself the result of an update with the same rows. Then
    P0 H^T = (prior H^T) S^-1 R is what is left of a cancellation of size ||S|| / ||R|| in the sum over the state, which the
    bound - written for a prior - does not know (its kappa is that of the NEW S, ~1): dx is held to TOL_DX as the neighbouring
    tests hold it (P+ keeps the bound)."""
    assert (ctx.get_status() == 0).all() and not ctx.get_ldlt_used().any(), what
    Pn, dx = ctx.download_P(), ctx.get_err()
    for b, (H, inn, dR) in enumerate(rows):
        ref = pr.extended(H, P0[b], inn, dR, None if keep is None else np.repeat(keep[b], 2))
        pr.check(ref, Pn[b], None if posterior else dx[b], what=(what, b))
        if posterior:
            assert rel_fro(dx[b], ref.dx.astype(np.float64)) < TOL_DX, (what, b)


def _gate_ref(rows, P0, F):
    """Estimator::MHGating on stacked rows: d_f = inn_f^T (H_f P H_f^T + R_f)^-1 inn_f, then the oracle's relaxation"""
    masks = []
    for b, (H, inn, dR) in enumerate(rows):
        d = np.zeros(F)
        for f in range(F):
            Hf, rf = H[2 * f:2 * f + 2], inn[2 * f:2 * f + 2]
            d[f] = rf @ np.linalg.solve(Hf @ P0[b] @ Hf.T + np.diag(dR[2 * f:2 * f + 2]), rf)
        masks.append(orc.mh_gate(d, *GATE)[0])
    return np.array(masks)


def _same_rows(a, b, what):
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), what


# ------------------------------------------------------------------ hand-over sequences
def seq_handover(T, flags, kind, check):
    """hand-over (all filters fit / none fit / mixed batch) -> update -> get_H -> update again"""
    N, F, B = 96, 12, 4
    P, H, inn, dR = synth.s_level(N, F, B, seed=21, dense=(kind == "none"))
    if kind == "mixed":
        H[1] = synth.s_level(N, F, B, seed=22, dense=True)[1][1]
    rows = [(H[b], inn[b], dR[b]) for b in range(B)]
    with Context(N, 2 * F, B, flags=flags) as ctx:
        ctx.upload_P(P)
        ctx.set_measurements(H, inn, dR); T.step("hand_over", ctx, F)
        ctx.update_joseph(); T.step("update", ctx, F)
        if check:
            _verify(rows, P, ctx, "hand-over " + kind)
        P1 = ctx.download_P()
        got = [ctx.get_H(b) for b in range(B)]; T.step("get_H", ctx, F, got)
        if check:
            for b in range(B):
                assert np.array_equal(got[b][0], H[b]) and np.array_equal(got[b][1], inn[b]) and np.array_equal(got[b][2], dR[b])
        ctx.update_joseph(); T.step("update_again", ctx, F)
        if check:
            _verify(rows, P1, ctx, "hand-over, second update " + kind, posterior=True)


def seq_gated_dense(T, flags, check):
    """hand-over -> mh_gate_dense -> update_dense_gated, get_gate read in the packed layout after each"""
    N, F, B = 96, 12, 3
    P, H, inn, dR = synth.s_level(N, F, B, seed=23)
    inn[:, 4:8] *= 1e4
    rows = [(H[b], inn[b], dR[b]) for b in range(B)]
    with Context(N, 2 * F, B, flags=flags) as ctx:
        ctx.upload_P(P); ctx.set_measurements(H, inn, dR)
        mask, dist = ctx.mh_gate_dense(F, R, *GATE); T.step("mh_gate_dense", ctx, F)
        m2, d2 = ctx.get_gate(F)
        ctx.update_dense_gated(F, R, *GATE); T.step("update_dense_gated", ctx, F)
        m3, _ = ctx.get_gate(F)
        if check:
            assert np.array_equal(mask, m2) and np.array_equal(dist, d2)
            assert m3.all()      # (the stand-alone gate neutralised the rejected rows: the gate inside the update passes them)
            assert np.array_equal(mask, _gate_ref(rows, P, F)) and not mask[:, 2:4].any()
            _verify(rows, P, ctx, "gated dense", keep=mask)


# ------------------------------------------------------------------ feature-level sequences
def _scene(flags, calib, B=3, M_extra=0, ng=4, nf=10):
    if calib:
        import test_calib_gpu as cal
        _, lay, sc, poses, groups, feats, xp, cs, _, ctx = cal.setup("radtan", True, True, True, B=B, ng=6, nf=14, seed=8, M_extra=M_extra)
        if flags:
            ctx.set_flags(flags)
        F = 14
    else:
        import test_glevel_gpu as gl
        sc, lay, ctx, poses, groups, feats, xp = gl.make(ng, nf, nf, B, 12, synth.PINHOLE, flags=flags, M_max=2 * nf + M_extra)
        cs, F = None, nf
    feats["xp"][1, [0, 3]] += 55.0; xp[1, [0, 3]] += 55.0
    P = np.array([spd(lay.N, 140 + b) * 1e-4 for b in range(B)])
    ctx.upload_P(P); ctx.set_scene(poses, groups, feats)
    if calib:
        ctx.set_calib_state(cs)
    return ctx, P, dict(sc=sc, lay=lay, xp=xp), F


def _stacked(flags, calib, M_extra=0, oos=0, compress=False, ransac=False, T=None):
    """Jacobians -> mh_gate [-> one_point_ransac] -> stack [-> oos_project (-> compress_oos)] on a fresh context"""
    T = T or Trace()
    ctx, P, info, F = _scene(flags, calib, M_extra=M_extra)
    sc, lay = info["sc"], info["lay"]
    ctx.jacobians_instate()
    mask, _ = ctx.mh_gate(R, *GATE); T.step("mh_gate", ctx, F)
    assert not mask[1, [0, 3]].any()
    info["mask"] = mask
    if ransac:
        ctx.one_point_ransac(R, 2.0, 5.89, want=False); T.step("one_point_ransac", ctx, F)
    ctx.stack(R); T.step("stack", ctx, F)
    if oos:
        from test_update_accuracy_gpu import _oos_list
        lst = _oos_list(sc, lay, synth.PINHOLE, P.shape[0], oos, [4, 3], 5)
        nrows = ctx.oos_project(lst, ROOS); T.step("oos_project", ctx, F)
        assert (nrows > 0).all()
        if compress:
            crow = ctx.compress_oos(1.0); T.step("compress_oos", ctx, F)
            assert (crow < nrows).all()
    return ctx, P, F, info


def _oracle_stack(info, b, mask):
    """FilterUpdate's stacking of filter b as the oracle does it (FillJacobianBlock quirk included), rejected features neutral"""
    Js, inns, _ = oracle_jacobians(info["sc"], synth.PINHOLE, info["lay"], info["xp"], b)
    H, inn, dR = orc.stack_measurements(Js, inns, info["sc"]["ref"][b], info["sc"]["sind"][b], info["lay"], R, fix_group_block=False)
    return orc.neutralise_rows(H, inn, dR, np.repeat(mask[b], 2))


def _twin_rows(flags, calib, **k):
    """The rows an identically staged context reads back. The in-state rows of a default context are held against the oracle's
    stacking here, so that the reference rows of the update checks are not only this library's own word."""
    ctx, P, F, info = _stacked(flags, calib, **k)
    with ctx:
        rows = [ctx.get_H(b) for b in range(P.shape[0])]
    if not calib and not k.get("ransac"):
        for b, (H, inn, dR) in enumerate(rows):
            Ho, io, Ro = _oracle_stack(info, b, info["mask"])
            assert rel_fro(H[:2 * F], Ho) < 1e-12 and np.abs(inn[:2 * F] - io).max() < 1e-9 and np.array_equal(dR[:2 * F], Ro), b
    return rows


def seq_stack(T, flags, calib, check, M_extra=0, oos=0, compress=False, ransac=False, read_H=False, gated=False, again=False,
              path=None):
    """... -> stack [-> OOS rows] [-> get_H] -> update (or update_dense_gated) [-> a second OOS append and the resident list
    projected again after the next stacking]. path: the pipeline the route table must pick for the update (1 sparse: the OOS
    append was mixed and neither DENSE_H nor STANDALONE_TAIL is set; 0 dense: the append found no 16 spare rows, or a flag)"""
    kw = dict(M_extra=M_extra, oos=oos, compress=compress, ransac=ransac)
    rows = _twin_rows(flags, calib, **kw) if check else None
    ctx, P, F, _ = _stacked(flags, calib, T=T, **kw)
    B = P.shape[0]
    with ctx:
        if read_H:
            got = [ctx.get_H(b) for b in range(B)]; T.step("get_H", ctx, F, got)
            if check:
                _same_rows(got, rows, "get_H in sequence")
        if gated:
            ctx.update_dense_gated(F, R, *GATE); T.step("update_dense_gated", ctx, F)
            mask, _ = ctx.get_gate(F)
            if check:
                assert np.array_equal(mask, _gate_ref(rows, P, F))
                _verify(rows, P, ctx, "gated", keep=mask)
        else:
            ctx.update_joseph(); T.step("update", ctx, F)
            if check:
                assert path is None or ctx.last_path() == path, (ctx.last_route(), path)
                _verify(rows, P, ctx, "stacked rows")
        if again:      # a second append on the rows of the next frame goes dense; then the resident list once more, mixed again
            from test_update_accuracy_gpu import _oos_list
            ctx.jacobians_instate(); ctx.mh_gate(R, *GATE, want=False); ctx.stack(R); T.step("stack_2", ctx, F)
            n1 = ctx.oos_project((B, oos), ROOS); T.step("oos_project_resident", ctx, F)
            n2 = ctx.oos_project((B, oos), ROOS); T.step("oos_project_second_append", ctx, F)
            P1 = ctx.download_P()
            got = [ctx.get_H(b) for b in range(B)]; T.step("get_H_2", ctx, F, got)
            ctx.update_joseph(); T.step("update_2", ctx, F)
            if check:
                assert np.array_equal(n1, n2) and ctx.last_path() == 0
                _verify(got, P1, ctx, "two OOS blocks")


def seq_stack_gate_dense(T, flags, calib, check):
    """Jacobians -> mh_gate (passing everything; get_gate in the strided layout) -> stack -> mh_gate_dense (the stacking is
    re-stacked densely - a lead stacking demoted -, H^T rebuilt; get_gate in the packed layout) -> update_dense_gated"""
    lax = (1e12, MULT, MIN_INL)

    def stage(T):
        ctx, P, info, F = _scene(flags, calib)
        ctx.jacobians_instate()
        mask, dist = ctx.mh_gate(R, *lax); T.step("mh_gate", ctx, F)
        ms, ds = ctx.get_gate(F)
        assert mask.all() and np.array_equal(mask, ms) and np.array_equal(dist, ds)      # strided layout, read back packed
        ctx.stack(R); T.step("stack", ctx, F)
        return ctx, P, info, F
    rows = None
    if check:
        ctx, P, info, F = stage(Trace())
        with ctx:
            rows = [ctx.get_H(b) for b in range(P.shape[0])]
        if not calib:
            for b, (H, inn, dR) in enumerate(rows):
                Ho, io, Ro = _oracle_stack(info, b, np.ones((P.shape[0], F), bool))
                assert rel_fro(H, Ho) < 1e-12 and np.abs(inn - io).max() < 1e-9 and np.array_equal(dR, Ro), b
    ctx, P, _, F = stage(T)
    with ctx:
        mask, dist = ctx.mh_gate_dense(F, R, *GATE); T.step("mh_gate_dense", ctx, F)
        mg, dg = ctx.get_gate(F)
        ctx.update_dense_gated(F, R, *GATE); T.step("update_dense_gated", ctx, F)
        if check:
            assert np.array_equal(mask, mg) and np.array_equal(dist, dg)                 # packed layout
            assert np.array_equal(mask, _gate_ref(rows, P, F)) and not mask[1, [0, 3]].any()
            # (the route table: a lead stacking with a gate, or DENSE_H, takes the dense pipeline; plain stacked rows stay sparse)
            assert ctx.last_path() == (0 if calib or flags & FLAG_DENSE_H else 1), ctx.last_route()
            _verify(rows, P, ctx, "stack, dense-row gate, gated update", keep=mask)


def seq_close_loop(T, flags, check):
    """stack -> oos_project -> close_loop_stack -> update: the loop-closure rows replace everything staged before"""
    ctx, P, F, _ = _stacked(flags, False, T=T, M_extra=92, oos=12)
    B, n = P.shape[0], 4
    mt = np.zeros((B, n), dtype=lc_dtype)
    with ctx:
        feats = ctx.get_scene()[2]
        for b in range(B):
            for i in range(n):
                mt[b, i]["feat"], mt[b, i]["group_sind"], mt[b, i]["xp"] = i, feats["ref_sind"][b, i], feats["xp"][b, i] + 0.5
        ctx.close_loop_stack(mt, 1.5 ** 2); T.step("close_loop_stack", ctx, F)
        got = [ctx.get_H(b) for b in range(B)]; T.step("get_H", ctx, F, got)
        ctx.update_joseph(); T.step("update", ctx, F)
        if check:
            assert all(g[0].shape[0] == 2 * n for g in got)
            _verify(got, P, ctx, "loop closure after OOS rows")


def seq_dropin(T, flags, check, calib=False):
    """a batched (calibration) stacking + update, then the one-filter call on filter 1 of the same context, then the batched
    stacking + update again"""
    ctx, P, F, _ = _stacked(flags, calib, T=T)
    B, N = P.shape[0], P.shape[1]
    _, Hs, inns, dRs = synth.s_level(N, 8, 1, seed=31)
    with ctx:
        ctx.update_joseph(); T.step("update", ctx, F)
        Pio = np.asfortranarray(ctx.download_P()[1])
        P1 = Pio.copy()
        err, rc = ctx.update_joseph_host(Hs[0], inns[0], dRs[0], Pio, b=1); T.step("update_joseph_host", ctx, F, rc=rc)
        if check:
            ref = pr.extended(Hs[0], P1, inns[0], dRs[0])
            pr.check(ref, Pio, err, what="one-filter call after a stacking")
        P2 = ctx.download_P()
        ctx.jacobians_instate(); ctx.mh_gate(R, *GATE, want=False); ctx.stack(R); T.step("stack_2", ctx, F)
        ctx.update_joseph(); T.step("update_2", ctx, F)
        Pn, dx = ctx.download_P(), ctx.get_err()
        got = [ctx.get_H(b) for b in range(B)]; T.step("get_H", ctx, F, got)
        if check:
            for b in range(B):
                pr.check(pr.extended(*got[b][:1], P2[b], *got[b][1:]), Pn[b], dx[b], what=("stacking after the one-filter call", b))


SEQUENCES = {}
for _k in ("fit", "none", "mixed"):
    for _f in FLAGSETS:
        SEQUENCES["handover_%s-%s" % (_k, _f)] = (lambda T, c, f=FLAGSETS[_f], k=_k: seq_handover(T, f, k, c))
for _f in ("default", "dense_h"):
    SEQUENCES["gated_dense-%s" % _f] = (lambda T, c, f=FLAGSETS[_f]: seq_gated_dense(T, f, c))
for _f in FLAGSETS:
    SEQUENCES["stack-%s" % _f] = (lambda T, c, f=FLAGSETS[_f]: seq_stack(T, f, False, c))
    SEQUENCES["stack_oos-%s" % _f] = (lambda T, c, f=FLAGSETS[_f]: seq_stack(T, f, False, c, M_extra=92, oos=12,
                                                                            path=0 if f & (FLAG_DENSE_H | FLAG_STANDALONE_TAIL) else 1))
    SEQUENCES["calib_stack-%s" % _f] = (lambda T, c, f=FLAGSETS[_f]: seq_stack(T, f, True, c))
SEQUENCES.update({
    "stack_oos_compress": lambda T, c: seq_stack(T, 0, False, c, M_extra=92, oos=12, compress=True, path=1),
    "stack_oos_get_H": lambda T, c: seq_stack(T, 0, False, c, M_extra=92, oos=12, read_H=True, path=1),
    "stack_oos_compress_get_H": lambda T, c: seq_stack(T, 0, False, c, M_extra=92, oos=12, compress=True, read_H=True, path=1),
    "stack_oos_twice_and_resident": lambda T, c: seq_stack(T, 0, False, c, M_extra=140, oos=12, again=True),
    "stack_oos_no_spare_rows": lambda T, c: seq_stack(T, 0, False, c, M_extra=60, oos=12, path=0),
    "stack_oos_throughput": lambda T, c: seq_stack(T, FLAG_THROUGHPUT_ROUTE, False, c, M_extra=92, oos=12, path=1),
    "stack_gated": lambda T, c: seq_stack(T, 0, False, c, gated=True),
    "calib_stack_get_H": lambda T, c: seq_stack(T, 0, True, c, read_H=True),
    "calib_stack_gated": lambda T, c: seq_stack(T, 0, True, c, gated=True),
    "calib_oos": lambda T, c: seq_stack(T, 0, True, c, M_extra=92, oos=12),
    "ransac_stack": lambda T, c: seq_stack(T, 0, False, c, ransac=True),
    "calib_ransac_stack": lambda T, c: seq_stack(T, 0, True, c, ransac=True),
    "stack_gate_dense": lambda T, c: seq_stack_gate_dense(T, 0, False, c),
    "stack_gate_dense-dense_h": lambda T, c: seq_stack_gate_dense(T, FLAG_DENSE_H, False, c),
    "calib_stack_gate_dense": lambda T, c: seq_stack_gate_dense(T, 0, True, c),
    "close_loop": lambda T, c: seq_close_loop(T, 0, c),
    "dropin_and_batch": lambda T, c: seq_dropin(T, 0, c),
    "dropin_after_calib_stack": lambda T, c: seq_dropin(T, 0, c, calib=True),
})


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_sequence(built, monkeypatch, name, chunk):
    if chunk is None:
        monkeypatch.delenv("XIVO_HIP_CHUNK", raising=False)
    else:
        monkeypatch.setenv("XIVO_HIP_CHUNK", str(chunk))
    SEQUENCES[name](Trace(), True)


if __name__ == "__main__":
    for chunk in (None, "2"):
        os.environ.pop("XIVO_HIP_CHUNK", None)
        if chunk:
            os.environ["XIVO_HIP_CHUNK"] = chunk
        for name in (sys.argv[1:] or sorted(SEQUENCES)):
            sys.stdout.write("== %s chunk=%s\n" % (name, chunk))
            SEQUENCES[name](Trace(sys.stdout), False)
