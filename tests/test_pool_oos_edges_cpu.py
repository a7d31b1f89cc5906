"""The cases of tests/test_pool_oos_edges_gpu.py, checked where no GPU is: the limits the table names against the header and the
kernels' text, every scripted scene against the oracle alone (observations in front of their cameras, 2k - 3 rows per used
feature, the used / short / surplus / none split from a restatement of plife_oos_decide), and for every gate scene the fp64-numpy
gamma against the longdouble one. Host code only."""
import os
import re

import numpy as np
import pytest

import pool_oos_edge_cases as pc
import xivo_oracle as orc
from xivo_amd import lib as L
from xivo_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xivo_amd", "csrc")


def _text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _define(name):
    for f in sorted(os.listdir(os.path.join(ROOT, "include"))) if os.path.isdir(os.path.join(ROOT, "include")) else []:
        m = re.search(r"#define\s+%s\s+(\d+)" % name, _text("include", f))
        if m:
            return int(m.group(1))
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            m = re.search(r"#define\s+%s\s+(\d+)" % name, _text("xivo_amd", "csrc", f))
            if m:
                return int(m.group(1))
    raise AssertionError(name)


def test_limits_of_the_table_are_the_codes():
    lim = pc.LIMITS
    assert lim["max_obs"] == L.OOS_MAX_OBS == _define("XIVO_OOS_MAX_OBS")
    assert lim["pool_max"] == L.POOL_MAX_ENTRIES == _define("XIVO_POOL_MAX_ENTRIES")
    assert lim["gate_rows"] == 2 * L.OOS_MAX_OBS - 3 == 29 and lim["gate_cols"] == 6 + 6 * L.OOS_MAX_OBS == 102
    glevel, pool, capi = _text("xivo_amd", "csrc", "glevel_kernels.hip"), _text("xivo_amd", "csrc", "pool_oos_kernels.hip"), \
        _text("xivo_amd", "csrc", "capi_pool_oos.hip")
    assert re.search(r"OOS_G_R\s*=\s*2 \* XIVO_OOS_MAX_OBS - 3;", glevel) and re.search(r"OOS_G_C\s*=\s*6 \+ 6 \* XIVO_OOS_MAX_OBS;", glevel)
    gate = glevel.split("void oos_gate_kernel")[1].split("\n}\n")[0]
    assert "__launch_bounds__(%d)" % lim["gate_pass"] in glevel.split("void oos_gate_kernel")[0][-60:]
    assert gate.count("+= %d)" % lim["gate_pass"]) >= 5 and "rr = 2 * k - 3, nc = 6 + 6 * k" in gate
    # one wave per filter, one lane per list position, and the cap that follows from it
    assert "o->oos_max > %d) return XIVO_HIP_ERR_UNSUPPORTED" % lim["oos_max"] in capi
    assert pool.count("__launch_bounds__(%d)" % lim["lanes"]) == 3 and pool.count("sPick[%d]" % lim["oos_max"]) == 2
    assert pool.count("sCase[XIVO_POOL_MAX_ENTRIES]") == 2 and "e += %d)" % lim["lanes"] in pool and "i += %d)" % lim["lanes"] in pool
    # the row reservation
    assert "return oos_max * (2 * max_obs - 3);" in _text("xivo_amd", "csrc", "pool_lifecycle_device.h")
    for om, mo in ((2, 3), (4, 3), (64, 2), (2, 16), (64, 16)):
        c = sequence.SequenceConfig(use_oos=True, feature_init="subfilter", oos_max=om, oos_max_obs=mo, oos_min_observations=2)
        assert c.oos_rows() == pc.rows_of(om, mo) == om * (2 * mo - 3)
    assert pc.rows_of(64, 16) == 1856 and pc.rows_of(2, 16) == 58 and pc.rows_of(64, 2) == 64
    assert pc.m_max(2, 16) == 2 * pc.NF + 80 == 92 and pc.m_max(64, 2) == 92


def test_cases_sit_where_they_claim():
    names = set()
    sides = {}
    for name, kernel, limit, side, value, sh in pc.POOL_OOS_EDGE_CASES:
        assert name not in names and limit in pc.LIMITS and side in ("in", "out", "refused"), name
        names.add(name)
        lim = pc.LIMITS[limit]
        assert (value <= lim) == (side == "in"), name
        sides.setdefault(limit, set()).add(side)
        assert sh["B"] <= 3 and sh["pool_max"] <= L.POOL_MAX_ENTRIES and 2 <= sh["min_obs"], name
        # the value is the shape's
        k_all = [len(pc.valid_obs(d["obs"], sh["ng"], sh["max_obs"])) for d in pc.build(name)["ent"].values()] \
            if sh.get("scene", name) in pc.SCENES else []
        if limit in ("lanes", "pool_max"):
            assert value == sh["pool_max"], name
        elif limit == "oos_max":
            assert value == sh["oos_max"], name
        elif limit == "max_obs":
            assert value == sh["max_obs"], name
        elif limit == "gate_rows":
            assert value == max(2 * k - 3 for k in k_all), name
        elif limit == "gate_cols":
            assert value == max(6 + 6 * k for k in k_all), name
        elif limit == "gate_pass":
            assert value in [6 + 6 * k for k in k_all], name
    for limit in ("lanes", "oos_max", "max_obs", "gate_pass"):
        assert "in" in sides[limit] or limit == "lanes"
        assert sides[limit] & {"out", "refused"}, limit
    # the largest context of the file: N about 135, M <= 92
    assert max(pc.m_max(sh["oos_max"], sh["max_obs"]) for *_, sh in pc.POOL_OOS_EDGE_CASES if sh["oos_max"] * sh["max_obs"] < 1024
               and sh["oos_max"] <= 64 and sh["max_obs"] <= 16) <= 92
    assert pc.build("gate_obs16")["lay"].N == 23 + 6 * 16 + 3 * pc.NF == 137


def _facts(scene):
    sh = scene["sh"]
    return {k: (not d["late"], d["z0"], len(pc.valid_obs(d["obs"], sh["ng"], sh["max_obs"]))) for k, d in scene["ent"].items()}


@pytest.mark.parametrize("name", sorted(pc.SCENES))
def test_scripted_scenes_against_the_oracle(name):
    scene = pc.build(name)
    sh, sc, lay, ent = scene["sh"], scene["sc"], scene["lay"], scene["ent"]
    for (b, e), d in ent.items():
        assert 0 <= b < sh["B"] and 0 <= e < sh["pool_max"] and 0 <= d["anchor"] < pc.N_ANCHORS and len(d["obs"]) <= sh["max_obs"]
        for g, px in d["obs"]:
            gg = g if g < sh["ng"] else 0
            Xcn = sc["Rbc"][b].T @ (sc["gR"][b, gg].T @ (d["Xs"] - sc["gT"][b, gg]) - sc["Tbc"][b])
            assert Xcn[2] > 0.5 and np.abs(Xcn[:2] / Xcn[2]).max() < 1.0, (b, e, g)        # in front of the observing camera
        # the log-depth run cannot be decided by exp's rounding: the depth is 1e-6 relative away from the window
        if not d["exact"]:
            assert min(abs(d["z0"] / pc.MIN_DEPTH - 1), abs(d["z0"] / pc.MAX_DEPTH - 1)) > 1e-6
    dec, used, cnt = pc.split(sh, scene["dropped"], _facts(scene))
    want = pc.COUNTERS[name]
    assert [c[pc.USED] for c in cnt] == want[0] and [c[pc.SHORT] for c in cnt] == want[1] and [c[pc.SURPLUS] for c in cnt] == want[2]
    assert all(len(u) <= sh["oos_max"] for u in used)
    if name != "collect_oos64":
        assert not used[0]                                                              # filter 0 is an empty list
    for b in range(sh["B"]):
        for key in used[b]:
            obs = pc.valid_obs(ent[key]["obs"], sh["ng"], sh["max_obs"])
            (Hx, r), = pc.oracle_block(scene, b, [(ent[key]["Xs"], obs)])
            assert Hx.shape == (2 * len(obs) - 3, lay.N) and len(r) == 2 * len(obs) - 3, key     # Hf has rank 3
            assert len({g for g, _ in obs}) >= 2
        assert sum(2 * len(pc.valid_obs(ent[k]["obs"], sh["ng"], sh["max_obs"])) - 3 for k in used[b]) <= pc.rows_of(sh["oos_max"], sh["max_obs"])


def test_pool130_puts_eligible_entries_on_both_sides_of_64_and_128():
    for name in ("collect_pool130", "collect_invdepth"):
        scene = pc.build(name)
        dec, used, _ = pc.split(scene["sh"], scene["dropped"], _facts(scene))
        assert sorted({e for _, e in scene["dropped"]}) == [0, 63, 64, 65, 127, 128, 129]
        for b in (1, 2):
            es = [e for (bb, e), d in dec.items() if bb == b and d in (pc.USED, pc.SURPLUS)]
            assert min(es) < 64 and any(64 <= e < 128 for e in es) and max(es) >= 128, (name, b, es)
        assert {d for d in dec.values()} == {pc.NONE, pc.USED, pc.SHORT, pc.SURPLUS}
        assert any(scene["ent"][k]["late"] for k in dec) and any(scene["ent"][k]["z0"] > pc.MAX_DEPTH for k in dec)
    # the depth window on exact values, invdepth only: 1 / (1 / 2) = 2 and 1 / (1 / 4) = 4 exactly
    ent = pc.build("collect_invdepth")["ent"]
    assert (ent[1, 0]["exact"], ent[1, 0]["z0"], ent[1, 129]["exact"], ent[1, 129]["z0"]) == (True, 2.0, True, 4.0)
    assert 1.0 / (1.0 / 2.0) == 2.0 and 1.0 / (1.0 / 4.0) == 4.0
    assert all(2.0 < d["z0"] < 4.0 or d["z0"] > pc.MAX_DEPTH or d["exact"] for d in ent.values())


def _gate_features(scene):
    """per used feature of a gate scene: (b, key, H_o from the oracle on the scripted Xs, r, nc)"""
    sh, ent = scene["sh"], scene["ent"]
    _, used, _ = pc.split(sh, scene["dropped"], _facts(scene))
    for b in range(sh["B"]):
        for key in used[b]:
            obs = pc.valid_obs(ent[key]["obs"], sh["ng"], sh["max_obs"])
            (Hx, r), = pc.oracle_block(scene, b, [(ent[key]["Xs"], obs)])
            yield b, key, Hx, r, 6 + 6 * len(obs)


@pytest.mark.parametrize("name", ["gate_obs16", "gate_cond", "gate_dup"])
def test_gate_scenes_numpy_gamma_against_longdouble(name):
    scene = pc.build(name)
    P = pc.prior(scene)
    feats = list(_gate_features(scene))
    assert sorted((len(r), nc) for _, _, _, r, nc in feats) == \
        ([(3, 24), (5, 30), (5, 30), (7, 36)] if name == "gate_dup" else [(15, 60), (17, 66), (19, 72), (29, 102)])
    t = 0
    if name == "gate_cond":
        b, _, Hx, r, _ = max(feats, key=lambda f: len(f[3]))
        t = pc.cond_exponent(Hx, P[b], r, scene["lay"])
        assert t == pc.COND_T                                       # the exponent the GPU test uses
        P = np.array([pc.cond_prior(P[b], scene["lay"], t) for b in range(len(P))])
    for b, key, Hx, r, nc in feats:
        g, e_np, cond, bound = pc.gate_bound(Hx, P[b], r, nc)
        print("%s %s: rows %d columns %d units 2^-%d(g %% 4) cond(S) %.3e gamma %.6g e_np %.2e bound %.2e" % (name, key, len(r), nc, t, cond, float(g), e_np, bound))
        assert g > 0 and e_np <= nc * pc.EPS * cond and bound <= pc.CAP       # numpy meets the forward bound; nothing looser than 1e-9
        if name == "gate_cond" and len(r) == 29:
            assert 1e6 <= cond < 1e7
        # a duplicate group: the rows over all columns and over the 6 + 6k - 6 distinct ones are the same rows
        if name == "gate_dup":
            gs = [g_ for g_, _ in scene["ent"][key]["obs"]]
            assert len(set(gs)) < len(gs) or key == (1, 3)
            assert len(set(gs)) >= 3


def test_bad_pivot_prior_makes_the_first_pivot_negative():
    scene = pc.build("gate_obs16")
    for b, key, Hx, r, nc in _gate_features(scene):
        if key == (1, 0):
            cols = np.flatnonzero(np.abs(Hx).sum(axis=0) > 0)
            assert len(cols) == nc
            P = pc.prior(scene)[b].copy()
            P[np.ix_(cols, cols)] = -pc.BAD_PIVOT_C * np.eye(nc)
            assert pc.gamma_extended(Hx, P, r)[2] < -1.0 and (Hx @ P @ Hx.T)[0, 0] + pc.ROOS < -1.0


def test_restated_rule_is_the_hosts():
    """decide() against the decision SequenceRunner's double makes (tests/test_pool_oos_cpu.py restates it the same way) and the
    header's text"""
    text = _text("xivo_amd", "csrc", "pool_lifecycle_device.h").split("XIVO_LIFE_HD int plife_oos_decide")[1].split("}")[0]
    assert [ln.strip() for ln in text.splitlines()[1:5]] == [
        "if (!ready) return PLIFE_OOS_NONE;", "if (k < min_obs) return PLIFE_OOS_SHORT;", "if (!depth_ok) return PLIFE_OOS_NONE;",
        "return n_used < oos_max ? PLIFE_OOS_USED : PLIFE_OOS_SURPLUS;"]
    assert (pc.NONE, pc.USED, pc.SHORT, pc.SURPLUS) == (0, 1, 2, 3)
    assert pc.decide(False, True, 9, 2, 0, 1) == pc.NONE and pc.decide(True, False, 1, 2, 0, 1) == pc.SHORT
    assert pc.decide(True, False, 2, 2, 0, 1) == pc.NONE and pc.decide(True, True, 2, 2, 0, 1) == pc.USED
    assert pc.decide(True, True, 2, 2, 1, 1) == pc.SURPLUS
