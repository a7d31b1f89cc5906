"""The scenes of the landmark-map tests (tests/test_lcmap_gpu.py), built once here so that tests/test_lcmap_cpu.py can check
their inputs on the oracle alone: B = 3 filters of 4 groups and 8 features (N = 71), every feature of a filter a world point
whose key is 100 b + j."""
import numpy as np

import xivo_oracle as orc
from xivo_amd import synth

CAMS = {"pinhole": synth.PINHOLE, "equi": synth.EQUI, "radtan": synth.RADTAN, "atan": synth.ATAN}
B, NG, NF = 3, 4, 8
MAP_MAX, LC_MAX, MIN_MATCHES = 8, 6, 5
RLC = 1.5 ** 2
CHI2 = 5.991464547107979


def layout():
    return orc.Layout(NG, NF)


def to_invdepth(x):
    y = np.array(x, dtype=np.float64, copy=True)
    y[..., 2] = np.exp(-y[..., 2])
    return y


def scene(cam, seed=11, invdepth=False):
    """-> (sc, x [B, NF, 3] in the build's parametrisation, Xs [B, NF, 3] the features' world points by the oracle)"""
    sc = synth.g_level(NG, NF, NF, B, seed=seed, cam=cam)
    x = to_invdepth(sc["x"]) if invdepth else sc["x"].copy()
    Xs = np.array([[orc.feature_xs(x[b, j], sc["gR"][b, sc["ref"][b, j]], sc["gT"][b, sc["ref"][b, j]], sc["Rbc"][b], sc["Tbc"][b], invdepth)
                    for j in range(NF)] for b in range(B)])
    return sc, x, Xs


def key(b, j):
    return 100 * b + j


def pixel(cam, Xs, Rsb, Tsb, Rbc, Tbc):
    """the pixel of world point Xs seen from the body pose (Rsb, Tsb)"""
    Xcn = Rbc.T @ (Rsb.T @ (Xs - Tsb) - Tbc)
    return orc.camera_project(cam, Xcn[:2] / Xcn[2])[0]


def covariance(seed):
    """a covariance whose pose block (columns 0..5, variance 1e-4) dominates: the loop closure corrects the pose"""
    N = layout().N
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, size=(N, N))
    d = np.full(N, 1e-8); d[:6] = 1e-4
    return np.diag(d) + 1e-9 * (A @ A.T / N)


def update_case(cam, seed=11):
    """GPU test 4: the body pose of every filter perturbed inside its covariance (0.7 sigma per component), the pixels those of
    the unperturbed pose. Filter 0 queries six of its points (closes), filter 1 four (short), filter 2 six keys that are in no
    map. -> dict(sc, x, Xs, P [B], dW, dT [B, 3], Rsb_p, Tsb_p: the perturbed poses, queries: [(b, key, xp)])"""
    sc, x, Xs = scene(cam, seed)
    rng = np.random.default_rng(seed + 1)
    P = np.array([covariance(seed + 10 + b) for b in range(B)])
    sig = np.sqrt(1e-4)
    dW = 0.7 * sig * rng.choice([-1.0, 1.0], size=(B, 3)); dT = 0.7 * sig * rng.choice([-1.0, 1.0], size=(B, 3))
    Rsb_p = np.array([sc["Rsb"][b] @ orc.so3_exp(dW[b]) for b in range(B)])
    Tsb_p = sc["Tsb"] + dT
    queries = []
    for b, n in enumerate((6, 4, 6)):
        for j in range(n):
            xp = pixel(cam, Xs[b, j], sc["Rsb"][b], sc["Tsb"][b], sc["Rbc"][b], sc["Tbc"][b])
            queries.append((b, key(b, j) if b < 2 else 9000 + j, xp))
    return dict(sc=sc, x=x, Xs=Xs, P=P, dW=dW, dT=dT, Rsb_p=Rsb_p, Tsb_p=Tsb_p, queries=queries)
