"""The inputs of the point-covariance tests (tests/test_lcmap_cov_gpu.py), built once here so that
tests/test_lcmap_cov_cpu.py can check them on the oracle alone. Shapes and scenes are tests/lcmap_cases.py's."""
import numpy as np

import lcmap_cases as LC
import lcmap_cov_restate as CR
import lcmap_restate as R
from xivo_amd import synth

MOVED, MOVE_PX, S_POINT = 2, 8.0, 0.05


def sigma(m, s=S_POINT):
    """the covariance of stored point m: s^2 (A A^T / 3 + I / 2), A uniform in (-1, 1) - a few centimetres, not isotropic"""
    A = np.random.default_rng(100 + m).uniform(-1, 1, (3, 3))
    return s * s * (A @ A.T / 3 + 0.5 * np.eye(3))


def gate_case(cam=synth.EQUI):
    """LC.update_case with the pixel of filter 0's pair MOVED off by MOVE_PX in both components: outside the gate with exact
    points, inside with sigma(m). -> the case, with queries replaced and ms0: filter 0's matches for lcmap_restate.rows"""
    c = LC.update_case(cam)
    qs = []
    for i, (b, k, xp) in enumerate(c["queries"]):
        qs.append((b, k, xp + MOVE_PX if (b == 0 and i == MOVED) else xp))
    c["queries"] = qs
    c["ms0"] = [dict(Xs=c["Xs"][0, j], Rsb=c["Rsb_p"][0], Tsb=c["Tsb_p"][0], g_sind=-1, xp=qs[j][2]) for j in range(6)]
    return c


def rows0(c, cam=synth.EQUI):
    """filter 0's unwhitened rows (H, inn, dR) and its R_e per pair under sigma(m)"""
    sc = c["sc"]
    H, inn, dR = R.rows(c["ms0"], sc["Rbc"][0], sc["Tbc"][0], cam, LC.layout(), LC.LC_MAX, LC.RLC)
    Res = [CR.r_eff(H[2 * m:2 * m + 2], sigma(m), LC.RLC) for m in range(6)]
    return H, inn, dR, Res
