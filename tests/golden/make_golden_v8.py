#!/usr/bin/env python
"""Generates tests/golden/golden_v8.npz: the reference cameras' own Project(xc, &jac) (oracle/_ref/libxivo_ref_*.so,
Ref.camera_project) at the branch points of tests/geometry_edge_cases.py - the atan camera at R = 0, 1e-9,
1e-4 (1 -+ 1e-6) and 0.3, the equidistant camera on its axis (a NaN Jacobian: -y / 0) and next to it, radtan and pinhole at
the principal point, every model's control point. Per model the arrays <name>_xc [n, 2], <name>_xp [n, 2] and
<name>_jac [n, 2, 2]; data only.

The reference binding has no UnProject: un-projection is pinned by restatement only (tests/geometry_edge_cases.py
against the g++ build of xivo_amd/csrc/camera_device.h).
Run in the authoring container only:  python tests/golden/make_golden_v8.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


if __name__ == "__main__":
    import geometry_edge_cases as ge
    import ref_binding
    ref = ref_binding.load()
    out = {}
    for name, cam in ge.CAMS.items():
        pts = np.array(ge.PROJECT_POINTS[name], dtype=np.float64)
        res = [ref.camera_project(cam, p) for p in pts]
        out[name + "_xc"] = pts
        out[name + "_xp"] = np.array([r[0] for r in res])
        out[name + "_jac"] = np.array([r[1] for r in res])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "golden_v8.npz"), **out)
    print("wrote golden_v8.npz with", len(out), "arrays")
