"""The cases of tests/test_glevel_edges_gpu.py, checked where no GPU is: each case's shape is on the side of its limit that the
case claims - by xivo_hip_selftest_glevel_launch, which calls the function the launch itself calls, where the launch picks by
size, and by the kernel's loop bounds where one kernel crosses a pass - and together the cases reach every instantiation of
oos_compress_kernel, both block sizes of the gate in the default and the online-calibration build, both tail kernels, and
tails of none, one and several passes. Host code only."""
from collections import defaultdict

import test_glevel_edges_gpu as edges


def _passes(case):
    """passes of the loop the case's limit counts, from its shape (the kernels' loop bounds: csrc/glevel_kernels.hip, state_kernels.hip)"""
    name, kernel, limit, side, entry, sh = case[:6]
    up = lambda a, b: -(-a // b)
    if kernel in ("relax_threshold", "ransac_select_kernel"):
        return up(sh["F"], 64)                                  # one wave, 64 features a pass
    if kernel == "stack_kernel":
        return up(2 * sh["F"], 256)                             # 256 threads, M = 2F rows
    if kernel == "oos_kernel":
        return max(sh["k"])                                     # one lane per observation
    if kernel == "givens_kernel":
        return up(sh["nx"] if entry == "qr" else sh["nf"], 64)  # pivot columns in chunks of 64
    if kernel == "xivo_hip_create":
        return sh["F"]                                          # M_max = 2F: round16(2F) / 16 block rows of the factor
    if kernel == "absorb_error_kernel":
        return up(sh["N"], 256)                                 # 256 threads over the state width
    raise AssertionError(name)


def test_glevel_edge_cases_sit_where_they_claim(built):
    from xivo_amd.lib import load_library
    lib = load_library()
    groups = defaultdict(lambda: defaultdict(set))
    names = set()
    for case in edges.GLEVEL_EDGE_CASES:
        name, kernel, limit, side, entry, sh, hk, passes = case
        assert name not in names and side in ("in", "out", "refused"), name
        names.add(name)
        if hk is not None:
            kind, a, b, c, want, label = hk
            assert edges.hook(lib, kind, a, b, c) == (want, label), (name, edges.hook(lib, kind, a, b, c), (want, label))
        if passes is not None:
            assert _passes(case) == passes, (name, _passes(case), passes)
        groups[(kernel, limit)][side].add(passes if passes is not None else (want, label))
    for (kernel, limit), sides in groups.items():
        if limit == "filter b0 + blockIdx.x":
            continue                                            # (a batch offset, not a size: the case runs inside)
        outside = sides["out"] | sides["refused"]
        assert sides["in"] and outside, (kernel, limit, dict(sides))
        assert not sides["in"] & outside, (kernel, limit, dict(sides))
        if all(isinstance(v, int) for v in sides["in"] | outside):   # a loop pass: the last inside and the first outside
            assert max(sides["in"]) + 1 == min(outside), (kernel, limit, dict(sides))


def test_glevel_edge_cases_reach_every_instantiation(built):
    hooks = [c[6] for c in edges.GLEVEL_EDGE_CASES if c[6] is not None]
    oosc = {h[4] for h in hooks if h[0] == edges.OOSC}
    assert oosc == {0, 1, 2, -1}, oosc
    gate = {(h[3], h[4]) for h in hooks if h[0] == edges.GATE}
    assert gate >= {(0, 1024), (0, 256), (1, 512), (1, 256)}, gate
    tails = defaultdict(set)
    for h in hooks:
        if h[0] == edges.TAIL:
            tails[h[5]].add(min(h[4], 2))
    assert tails[edges.FIX23] == {0, 1, 2} and tails[edges.GEN] == {0, 1, 2} and tails[""] == {-1}, dict(tails)


def test_glevel_launch_hook_answers(built):
    """The hook on its own: gate block sizes by batch and LDS, the three compression instantiations and the declined shape,
    the tail kernels and their passes, the refusals."""
    from xivo_amd.lib import load_library
    lib = load_library()
    h = lambda kind, a, b, c=0: edges.hook(lib, kind, a, b, c)
    assert h(edges.GATE, 1, 1, 0) == (1024, "gate_sparse_kernel@1024")
    assert h(edges.GATE, 70, 192, 0) == (1024, "gate_sparse_kernel@1024")
    assert h(edges.GATE, 70, 224, 0) == (512, "gate_sparse_kernel@512")     # 16 waves of scratch no longer fit 64 KB
    assert h(edges.GATE, 16384, 80, 0) == (256, "gate_sparse_kernel@256")
    assert h(edges.GATE, 0, 10, 0)[0] < 0 and h(edges.GATE, 10, 0, 0)[0] < 0
    assert h(edges.OOSC, 9, 1) == (0, edges.OC[0]) and h(edges.OOSC, 20, 1) == (2, edges.OC[2])
    assert h(edges.OOSC, 10, 256) == (-1, "") and h(edges.OOSC, 0, 10)[0] < 0
    assert h(edges.TAIL, 23, 203) == (1, edges.FIX23) and h(edges.TAIL, 38, 276) == (1, edges.GEN)
    assert h(edges.TAIL, 0, 10) == (-1, "") and h(edges.TAIL, 24, 23) == (-1, "")
    assert h(3, 0, 0, 0)[0] < 0
