"""The cases of tests/test_pool_oos_edges_gpu.py - the pool's MSCKF path (pool_oos_collect_kernel, oos_gate_kernel; the device life
cycle's select / record kernels have their sequence in tests/test_pool_oos_sequence_wide_gpu.py) at its shape limits and the gate's
branches - with the scripted scenes and the references both the GPU test and its CPU check (tests/test_pool_oos_edges_cpu.py)
use. Nothing here needs a GPU.

A scene is one scripted frame in the style of tests/test_pool_oos_gpu.py: a synth.g_level scene of n_groups group slots, anchor
a of every filter at the pose of group slot a (0 and 1 linked, 2 and 3 frozen there), pool entries whose points are placed in
their anchor's camera, and per entry the group slots that observed it, oldest first (99: a slot outside the layout)."""
import numpy as np

import xivo_oracle as orc
from precise_ref import LD, _chol
from scene_util import spd
from xivo_amd import synth
from xivo_amd import lib as L

CAM = synth.PINHOLE
NF, AM, N_ANCHORS = 6, 6, 4
ROOS = 3.5 ** 2
MIN_DEPTH, MAX_DEPTH = 0.05, 10.0
NONE, USED, SHORT, SURPLUS = range(4)
BAD_SLOT = 99

# the limits the cases name, as literals: tests/test_pool_oos_edges_cpu.py holds them against the header and the kernels' text
LIMITS = {
    "lanes": 64,            # one wave per filter: for (e = lane; e < n; e += 64) in collect / select / record
    "pool_max": 512,        # XIVO_POOL_MAX_ENTRIES: sCase[]
    "oos_max": 64,          # one lane per list position: the cap of xivo_hip_pool_oos_config
    "max_obs": 16,          # XIVO_OOS_MAX_OBS
    "gate_rows": 29,        # 2 XIVO_OOS_MAX_OBS - 3: sS[29][30]
    "gate_cols": 102,       # 6 + 6 XIVO_OOS_MAX_OBS: sH[29][103], sCol[102]
    "gate_pass": 64,        # columns / elements a pass of the gate's lane-strided loops
}


def rows_of(oos_max, max_obs):
    """the fixed block of a frame (plife_oos_rows)"""
    return oos_max * (2 * max_obs - 3)


def m_max(oos_max, max_obs):
    """rows the context needs: the in-state rows and the 16-row-padded block (xivo_hip_pool_oos_project)"""
    return 2 * NF + ((rows_of(oos_max, max_obs) + 16 + 15) // 16) * 16


# name, kernel, limit (a key of LIMITS), side ("in": at or below the limit, "out": past it - a further pass of a loop -,
# "refused"), value the case puts against the limit, shape
POOL_OOS_EDGE_CASES = [
    ("collect_pool130", "pool_oos_collect_kernel", "lanes", "out", 130, dict(B=3, ng=4, pool_max=130, oos_max=4, max_obs=3, min_obs=2)),
    # (collect's lane-strided loop runs over the RECORDS it is handed, select's over the entries: entries past 64 and 128 with seven
    # records address the pool there, a second and a third pass need more than 64 and 128 records - collect_records130, collect_oos64)
    ("collect_records130", "pool_oos_collect_kernel", "lanes", "out", 130, dict(B=3, ng=4, pool_max=130, oos_max=4, max_obs=3, min_obs=2)),
    ("collect_poolcap", "pool_oos_collect_kernel", "pool_max", "in", 512, dict(B=2, ng=4, pool_max=512, oos_max=4, max_obs=3, min_obs=2)),
    ("collect_oos64", "pool_oos_collect_kernel", "oos_max", "in", 64, dict(B=3, ng=4, pool_max=130, oos_max=64, max_obs=2, min_obs=2)),
    ("collect_oos65", "xivo_hip_pool_oos_config", "oos_max", "refused", 65, dict(B=3, ng=4, pool_max=130, oos_max=65, max_obs=2, min_obs=2)),
    ("collect_invdepth", "pool_oos_collect_kernel", "lanes", "out", 130,
     dict(B=3, ng=4, pool_max=130, oos_max=4, max_obs=3, min_obs=2, invdepth=True)),
    ("collect_badslot", "pool_oos_collect_kernel", "lanes", "out", 130, dict(B=3, ng=4, pool_max=130, oos_max=4, max_obs=3, min_obs=3)),
    ("gate_obs16", "oos_gate_kernel", "gate_rows", "in", 29, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2)),
    ("gate_cols102", "oos_gate_kernel", "gate_cols", "in", 102, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("gate_cols60", "oos_gate_kernel", "gate_pass", "in", 60, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("gate_cols66", "oos_gate_kernel", "gate_pass", "out", 66, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("gate_cond", "oos_gate_kernel", "gate_rows", "in", 29, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("gate_dup", "oos_gate_kernel", "gate_pass", "in", 30, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2)),
    ("gate_threshold", "oos_gate_kernel", "gate_rows", "in", 29, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("gate_bad_pivot", "oos_gate_kernel", "gate_rows", "in", 29, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("two_frames", "oos_block_init_kernel", "gate_rows", "in", 29, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=16, min_obs=2, scene="gate_obs16")),
    ("refuse_rows1856", "xivo_hip_pool_oos_project", "max_obs", "in", 16, dict(B=3, ng=16, pool_max=8, oos_max=64, max_obs=16, min_obs=2)),
    ("refuse_obs17", "xivo_hip_pool_oos_config", "max_obs", "refused", 17, dict(B=3, ng=16, pool_max=8, oos_max=2, max_obs=17, min_obs=2)),
]
CASE = {c[0]: c for c in POOL_OOS_EDGE_CASES}


def shape(name):
    return CASE[name][5]


# ---- the scripted entries. (filter, entry): (anchor, observing group slots oldest first, late: added after the first step, so
# INITIALIZING at the frame, depth: a factor on the drawn depth of 2.5 .. 3.5 m, or ("z", depth) for that depth exactly)
def _e(anchor, groups, late=False, depth=1.0):
    return (anchor, list(groups), late, depth)


def _pool130(invdepth):
    # filter 0 keeps its one track; filter 1: used, short, used, INITIALIZING, out of depth, used, used - the eligible ones on
    # both sides of entries 64 and 128; filter 2: all seven eligible (one with a slot outside the layout that leaves it two
    # valid observations), so the last three are surplus
    z0, z1 = (("z", 2.0), ("z", 4.0)) if invdepth else (1.0, 1.0)
    ent = {(0, 70): _e(0, []),
           (1, 0): _e(0, [0, 1, 2], depth=z0), (1, 63): _e(2, [3]), (1, 64): _e(1, [2, 3]), (1, 65): _e(3, [0, 1], late=True),
           (1, 127): _e(0, [1, 3, 2], depth=8.0), (1, 128): _e(1, [3, 0]), (1, 129): _e(2, [0, 2, 3], depth=z1),
           (2, 0): _e(3, [1, 0]), (2, 63): _e(0, [1, BAD_SLOT, 0]), (2, 64): _e(1, [0, 1, 2]), (2, 65): _e(2, [2, 1]),
           (2, 127): _e(3, [3, 2, 1]), (2, 128): _e(0, [0, 3]), (2, 129): _e(1, [1, 2, 3])}
    return ent, [k for k in ent if k[0] > 0]


def _records130():
    # every entry of filters 1 and 2 is dropped: 130 records, three passes of the lanes. Filter 1: all eligible, the first four
    # used; filter 2: entries 1 .. 126 short, so the used ones come from the first and the third pass
    ent = {(0, 70): _e(0, [])}
    for e in range(130):
        ent[1, e] = _e(e % N_ANCHORS, [e % 4, (e + 1) % 4])
        ent[2, e] = _e((e + 1) % N_ANCHORS, [e % 4] if 1 <= e <= 126 else [(e + 2) % 4, e % 4, (e + 1) % 4])
    return ent, [k for k in ent if k[0] > 0]


def _poolcap():
    ent = {(0, 300): _e(1, []), (1, 0): _e(0, [0, 1, 2]), (1, 255): _e(1, [1, 3, 2], depth=8.0), (1, 256): _e(2, [3, 0]),
           (1, 511): _e(3, [2, 1, 0])}
    return ent, [k for k in ent if k[0] > 0]


def _oos64():
    # filter 0: one eligible entry; filter 1: 70 (64 used, 6 surplus); filter 2: exactly 64, behind the first pass of lanes
    ent = {(0, 129): _e(0, [1, 2])}
    for e in range(70):
        ent[1, e] = _e(e % N_ANCHORS, [e % 4, (e + 1 + e // 4 % 3) % 4])
    for e in range(66, 130):
        ent[2, e] = _e(e % N_ANCHORS, [(e + 2) % 4, e % 4])
    return ent, sorted(ent)


def _badslot():
    # min_obs = 3: a slot outside the layout takes (1, 65) and (2, 128) from 3 to 2 valid observations
    ent = {(0, 5): _e(0, []), (1, 64): _e(0, [0, 1, 2]), (1, 65): _e(1, [1, BAD_SLOT, 0]), (2, 128): _e(2, [BAD_SLOT, 2, 3]),
           (2, 129): _e(3, [3, 2, 1])}
    return ent, [k for k in ent if k[0] > 0]


def _perm(seed, k, ng=16):
    return [int(g) for g in np.random.default_rng(seed).permutation(ng)[:k]]


def _obs16():
    # filter 1: k = 16 (29 rows, 102 columns) and k = 11 (72 columns: past one pass of 64); filter 2: k = 9 and 10 (60 and 66
    # columns); (2, 6) keeps its track in the first frame and is the one feature of two_frames' second frame
    ent = {(0, 2): _e(0, []), (1, 0): _e(0, _perm(1, 16)), (1, 3): _e(3, _perm(2, 11)), (2, 1): _e(1, _perm(3, 9)),
           (2, 4): _e(2, _perm(4, 10)), (2, 6): _e(1, [4, 9])}
    return ent, [(1, 0), (1, 3), (2, 1), (2, 4)]


def _dup():
    # one group seen twice (three distinct groups keep Hf at rank 3), twice non-adjacent, and two pairs
    ent = {(0, 2): _e(0, []), (1, 0): _e(0, [2, 5, 2, 9]), (1, 3): _e(3, [7, 1, 12]), (2, 1): _e(1, [6, 6, 1, 3, 1]),
           (2, 4): _e(2, [15, 0, 8, 15])}
    return ent, [k for k in ent if k[0] > 0]


SCENES = {"collect_records130": _records130, "collect_pool130": lambda: _pool130(False), "collect_invdepth": lambda: _pool130(True), "collect_poolcap": _poolcap,
          "collect_oos64": _oos64, "collect_badslot": _badslot, "gate_obs16": _obs16, "gate_dup": _dup}
# used / short / surplus per filter, by hand: the CPU check derives the same from the script, the GPU test from the resident pool
COUNTERS = {"collect_records130": ([0, 4, 4], [0, 0, 126], [0, 126, 0]), "collect_pool130": ([0, 4, 4], [0, 1, 0], [0, 0, 3]), "collect_invdepth": ([0, 4, 4], [0, 1, 0], [0, 0, 3]),
            "collect_poolcap": ([0, 3], [0, 0], [0, 0]), "collect_oos64": ([1, 64, 64], [0, 0, 0], [0, 6, 0]),
            "collect_badslot": ([0, 1, 1], [0, 1, 1], [0, 0, 0]), "gate_obs16": ([0, 2, 2], [0, 0, 0], [0, 0, 0]),
            "gate_dup": ([0, 2, 2], [0, 0, 0], [0, 0, 0])}


def build(name, seed=5):
    """-> dict(sh, sc, lay, ent, dropped): ent[(b, e)] = dict(anchor, xp0, z0 (the first pixel and the depth pool_add takes), Xs,
    obs [(group slot, pixel)], late, exact (the depth is meant bit for bit))"""
    sh = shape(name)
    spec, dropped = SCENES[sh.get("scene", name)]()
    ng, B = sh["ng"], sh["B"]
    sc = synth.g_level(ng, NF, NF, B, seed=seed, cam=CAM)
    lay = orc.Layout(ng, NF, N=sc["N"])
    rng = np.random.default_rng(11)
    ent = {}
    for (b, e), (a, gs, late, depth) in spec.items():
        exact = isinstance(depth, tuple)
        z = depth[1] if exact else rng.uniform(2.5, 3.5) * depth
        xc = rng.uniform(-0.15, 0.15, 2)
        Xc = np.array([xc[0] * z, xc[1] * z, z])                               # in the anchor's camera
        Xs = sc["gR"][b, a] @ (sc["Rbc"][b] @ Xc + sc["Tbc"][b]) + sc["gT"][b, a]
        xp0 = orc.camera_project(CAM, xc)[0]
        obs = []
        for g in gs:
            gg = g if g < ng else 0
            _, _, inn = orc.oos_jacobian_internal(Xs, sc["gR"][b, gg], sc["gT"][b, gg], sc["Rbc"][b], sc["Tbc"][b], [0, 0], CAM, lay, gg)
            obs.append((g, -inn + rng.normal(0, 1.0, 2)))
        ent[b, e] = dict(anchor=a, xp0=xp0, z0=z, Xs=Xs, obs=obs, late=late, exact=exact)
    return dict(name=name, sh=sh, sc=sc, lay=lay, ent=ent, dropped=sorted(dropped))


def valid_obs(obs, ng, max_obs):
    return [(g, px) for g, px in obs[:max_obs] if 0 <= g < ng]


def decide(ready, depth_ok, k, min_obs, n_used, oos_max):
    """plife_oos_decide (xivo_amd/csrc/pool_lifecycle_device.h), restated"""
    if not ready:
        return NONE
    if k < min_obs:
        return SHORT
    if not depth_ok:
        return NONE
    return USED if n_used < oos_max else SURPLUS


def split(sh, dropped, facts):
    """the rule over a frame's dropped entries in the order of the hand-over, (b, entry) ascending; facts[(b, e)] = (ready, depth,
    valid observations) -> ({(b, e): decision}, used [B] lists of (b, e), counters [B][4])"""
    dec, used, cnt = {}, [[] for _ in range(sh["B"])], [[0] * 4 for _ in range(sh["B"])]
    for (b, e) in sorted(dropped):
        ready, z, k = facts[b, e]
        d = decide(ready, sh.get("min_depth", MIN_DEPTH) < z < sh.get("max_depth", MAX_DEPTH), k, sh["min_obs"], len(used[b]), sh["oos_max"])
        dec[b, e] = d
        cnt[b][d] += 1
        if d == USED:
            used[b].append((b, e))
    return dec, used, cnt


def cands(scene, dropped=None, moved=None):
    """the host's hand-over: the dropped entries, ordered by (b, entry), with their observations; moved: (b, e) whose first pixel
    is off by 200 px"""
    out = []
    for (b, e) in sorted(scene["dropped"] if dropped is None else dropped):
        r = np.zeros((), dtype=L.pool_oos_cand_dtype)
        obs = scene["ent"][b, e]["obs"]
        r["b"], r["entry"], r["n_obs"] = b, e, len(obs)
        for q, (g, px) in enumerate(obs):
            r["group_sind"][q] = g
            r["xp"][q] = px + (200.0 if (b, e) == moved and q == 0 else 0.0)
        out.append(r)
    return np.array(out, dtype=L.pool_oos_cand_dtype)


# ---- the gate's reference
EPS = 2.0 ** -52
BAD_PIVOT_C = 1.0   # gate_bad_pivot: P = -c I on the observing columns (the rows' entries are ~1e2: the first pivot is ~ -1e4)
CAP = 1e-9        # the relative bound of tests/test_pool_oos_gpu.py::test_gamma_equals_numpy: no case is held to a looser one


def gamma_extended(Ho, P, r, Roos=ROOS):
    """gamma = r^T S^-1 r, S = H_o P H_o^T + Roos I over ALL columns of the rows, in longdouble (precise_ref._chol and a forward
    substitution) -> (gamma, cond_2(S) from the longdouble S rounded to fp64, first pivot S[0, 0])"""
    Hl, Pl, rl = np.asarray(Ho).astype(LD), np.asarray(P).astype(LD), np.asarray(r).astype(LD)
    S = Hl @ Pl @ Hl.T + LD(Roos) * np.eye(len(rl), dtype=LD)
    if not S[0, 0] > 0:
        return None, None, S[0, 0]
    Lc = _chol(S)
    y = np.zeros_like(rl)
    for i in range(len(rl)):
        y[i] = (rl[i] - Lc[i, :i] @ y[:i]) / Lc[i, i]
    return y @ y, float(np.linalg.cond(S.astype(np.float64))), S[0, 0]


def gamma_numpy(Ho, P, r, Roos=ROOS):
    """the same formula in plain fp64 numpy"""
    S = Ho @ P @ Ho.T + Roos * np.eye(len(r))
    return float(r @ np.linalg.solve(S, r))


def gate_bound(Ho, P, r, nc, Roos=ROOS):
    """-> (gamma longdouble, e_np, cond(S), bound): e_np the relative error of fp64 numpy against longdouble, the device's bound
    max(16 e_np, nc eps cond(S)) - 16 for another summation order over dot products of up to 102 terms, the second term the
    standard forward bound of a Cholesky solve - capped at CAP"""
    g, cond, _ = gamma_extended(Ho, P, r, Roos)
    e_np = float(abs(LD(gamma_numpy(Ho, P, r, Roos)) - g) / g)
    return g, e_np, cond, min(max(16 * e_np, nc * EPS * cond), CAP)


COND_SCALE = 2.0 ** 24
COND_T = 4          # cond_exponent of the k = 16 feature (tests/test_pool_oos_edges_cpu.py): cond(S) = 1.5e6


def cond_units(lay, t):
    """D = 2^(-t (g % 4)) on the six columns of group slot g, 1 elsewhere"""
    D = np.ones(lay.N)
    for g in range(lay.n_groups):
        D[lay.group_begin + 6 * g:lay.group_begin + 6 * g + 6] = 2.0 ** (-t * (g % 4))
    return D


def cond_prior(P, lay, t, s=COND_SCALE):
    """gate_cond's prior: s D P D, every factor a power of two (exact). s alone makes H_o P H_o^T dominate Roos, but cond(S) then
    stops at cond(H_o P H_o^T), about 50 with the prior of these scenes; the groups' units D spread it"""
    D = cond_units(lay, t)
    return s * P * np.outer(D, D)


def cond_exponent(Ho, P, r, lay, target=1e6):
    """the smallest t with cond(S) >= target under cond_prior"""
    for t in range(1, 20):
        if gamma_extended(Ho, cond_prior(P, lay, t), r)[1] >= target:
            return t
    raise AssertionError("cond(S) stays below %g" % target)


def prior(scene):
    return np.array([spd(scene["lay"].N, 40 + b) * 1e-4 for b in range(scene["sh"]["B"])])


def oracle_block(scene, b, feats, groups_R=None, groups_T=None):
    """the oracle's OOS rows of the features feats = [(Xs, [(group, pixel)])] of filter b -> [(Hx', r')]"""
    sc = scene["sc"]
    gR = sc["gR"][b] if groups_R is None else groups_R
    gT = sc["gT"][b] if groups_T is None else groups_T
    return [orc.oos_jacobian(Xs, obs, gR, gT, sc["Rbc"][b], sc["Tbc"][b], CAM, scene["lay"])[:2] for Xs, obs in feats]
