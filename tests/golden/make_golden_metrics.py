"""Generates tests/golden/metrics_v1.npz: what the reference's ComputeATE / ComputeRPE (src/metrics.cpp, over
TrajectoryAlignment of src/geometry.cpp) return for generated trajectories - DATA only, inputs and recorded results.

    python tests/golden/make_golden_metrics.py [--ref /root/reference]

How: the two reference files are compiled WHERE THEY LIE, in a temporary directory outside the repository, together with a
small driver written here (DRIVER below: it reads poses from a binary file and prints the numbers the two functions return)
against the reference's Eigen, Sophus and jsoncpp headers, oracle/ref/shim for glog and a three-line stand-in for the one
OpenCV header its utility header names (only in templates that are not instantiated). Nothing of the reference is copied.

Compiler: clang++ -O0, and that is not a free choice. The refinement loop of TrajectoryAlignment binds an Eigen product of
two temporaries to `auto` (src/geometry.cpp:135) and reads it after they are gone - undefined behaviour. Built with g++
(-O0 ... -O3, the reference's own -O3 included) or clang++ -O3 the program ends in a segmentation fault or std::bad_alloc
on every case; a host AddressSanitizer build of this stand-alone program names that line (stack-use-after-scope). At
clang++ -O0 the temporaries' stack slots are still intact when they are read, and the result is checked by what it is: a
minimiser that agrees with the closed-form optimum to the gap recorded below.

Cases: 10 generated (nt in {20, 200}, noise 1e-3 ... 1e-1, uniform stamps of 40 ms, the same stamps for estimate and ground
truth); a case is kept when the reference's five Gauss-Newton steps converged, which is read off its own result:
ate_reference / ate_closed_form - 1 < 1e-6. 10 of 10 were kept when this file was last run.

Two things the reference does that the fixture records instead of hiding:
  * ComputeATE walks the ground truth with next(it_gt) < gt.end(): of nt associated poses it scores the first nt - 1
    (`n_ate`).
  * ComputeRPE advances it_est BEFORE it forms `desire`: pose i is paired with the pose nearest ts[i + 1] + dt, with uniform
    frames lag = 1 + round(dt / period) (`lag`), over all nt poses.
Recorded next to the results: the largest relative gap ate_reference / ate_restatement - 1 (`ate_gap`) and the largest
|R_ref - R_restatement| entry (`R_gap`) over the kept cases - the measured distance between the reference's iteration and
the closed-form optimum that the tests' two-sided tolerance is made of - and the RPE's relative difference (`rpe_gap`)."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_restate as sr  # noqa: E402

PERIOD_NS = 40_000_000
RES = 0.005

DRIVER = r"""
// reads: n, dt, res, then n estimated and n true poses (ts ns, R column-major, T); prints ate, rpe_pos, rpe_rot, gYX
#include <cstdio>
#include <vector>
#include "metrics.h"
using namespace xivo;
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long n; double dt, res;
  if (fread(&n, 8, 1, f) != 1 || fread(&dt, 8, 1, f) != 1 || fread(&res, 8, 1, f) != 1) return 2;
  std::vector<msg::Pose> traj[2];   // est, gt
  for (int k = 0; k < 2; ++k)
    for (long long i = 0; i < n; ++i) {
      long long ts; double v[12];
      if (fread(&ts, 8, 1, f) != 1 || fread(v, 8, 12, f) != 12) return 2;
      Mat3 R; Vec3 T;
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R(r, c) = v[r + 3 * c]; T(r) = v[9 + r]; }
      traj[k].emplace_back(timestamp_t(ts), SE3(SO3(R), T));
    }
  fclose(f);
  auto [ate, g] = ComputeATE(traj[0], traj[1], res);
  auto [rp, rr] = ComputeRPE(traj[0], traj[1], dt, res);
  Mat3 R = g.so3().matrix(); Vec3 T = g.translation();
  printf("%.17g %.17g %.17g", ate, rp, rr);
  for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) printf(" %.17g", R(r, c));
  for (int r = 0; r < 3; ++r) printf(" %.17g", T(r));
  printf("\n");
  return 0;
}
"""
CV_STANDIN = "#pragma once\nnamespace cv { struct Mat { int rows = 0, cols = 0; template <class T> T at(int, int) const { return T(); } }; }\n"


def build_driver(ref, tmp, cxx):
    os.makedirs(os.path.join(tmp, "stub", "opencv2", "core"))
    with open(os.path.join(tmp, "stub", "opencv2", "core", "core.hpp"), "w") as f:
        f.write(CV_STANDIN)
    with open(os.path.join(tmp, "driver.cpp"), "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "ref_metrics")
    inc = [os.path.join(tmp, "stub"), os.path.join(ROOT, "oracle", "ref", "shim"), os.path.join(ref, "src"),
           os.path.join(ref, "common"), os.path.join(ref, "thirdparty", "eigen"), os.path.join(ref, "thirdparty", "sophus"),
           os.path.join(ref, "thirdparty", "jsoncpp", "include")]
    cmd = [cxx, "-std=c++17", "-O0", "-Wno-c++11-narrowing", "-Wno-missing-template-arg-list-after-template-kw", "-DNDEBUG",
           "-DEIGEN_INITIALIZE_MATRICES_BY_ZERO", "-DSOPHUS_USE_BASIC_LOGGING", "-w"]
    cmd += ["-I" + i for i in inc]
    cmd += [os.path.join(tmp, "driver.cpp"), os.path.join(ref, "src", "metrics.cpp"), os.path.join(ref, "src", "geometry.cpp"),
            "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_reference(exe, tmp, est_R, est_T, gt_R, gt_T, dt):
    nt = est_T.shape[0]
    path = os.path.join(tmp, "case.bin")
    with open(path, "wb") as f:
        f.write(np.int64(nt).tobytes() + np.float64(dt).tobytes() + np.float64(RES).tobytes())
        for R, T in ((est_R, est_T), (gt_R, gt_T)):
            for i in range(nt):
                f.write(np.int64(i * PERIOD_NS).tobytes() + np.ascontiguousarray(R[i].T).tobytes() + T[i].tobytes())
    v = np.array(subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split(), dtype=np.float64)
    return dict(ate=v[0], rpe_pos=v[1], rpe_rot=v[2], R=v[3:12].reshape(3, 3).T.copy(), T=v[12:15].copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("XIVO_REF", "/root/reference"))
    ap.add_argument("--cxx", default=shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++")
    ap.add_argument("--out", default=os.path.join(HERE, "metrics_v1.npz"))
    a = ap.parse_args()
    rng = np.random.default_rng(20241)
    specs = [(20, 1e-3, 5), (20, 1e-2, 5), (20, 3e-2, 3), (20, 1e-1, 5), (200, 1e-3, 25), (200, 3e-3, 25), (200, 1e-2, 25),
             (200, 3e-2, 10), (200, 1e-1, 25), (200, 1e-2, 1)]          # nt, noise, dt in frames
    NT = 200
    keep = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp, a.cxx)
        for nt, noise, k in specs:
            gt_R, gt_T = sr.smooth_trajectory(rng, nt, offset=10.0, size=2.0)
            g_R, g_T = sr.rot(rng.normal(size=3)), rng.normal(size=3) * 3
            est_R, est_T = sr.moved(rng, gt_R, gt_T, g_R, g_T, noise)
            dt = k * PERIOD_NS * 1e-9
            ref = run_reference(exe, tmp, est_R, est_T, gt_R, gt_T, dt)
            lag = 1 + k
            mine = sr.score(est_R[:nt - 1], est_T[:nt - 1], gt_R[:nt - 1], gt_T[:nt - 1], align=True)
            rpe = sr.score(est_R, est_T, gt_R, gt_T, align=False, rpe_lag=lag)
            gap = float(ref["ate"] / float(mine["ate"]) - 1)
            Rgap = float(np.abs(ref["R"] - mine["R"]).max())
            rgap = max(abs(ref["rpe_pos"] / float(rpe["rpe_pos"]) - 1), abs(ref["rpe_rot"] / float(rpe["rpe_rot"]) - 1))
            ok = gap < 1e-6
            print("nt %3d noise %.0e lag %2d: ate ref %.12e restatement %.12e gap %.3e |dR| %.3e rpe gap %.3e pairs %d %s"
                  % (nt, noise, lag, ref["ate"], float(mine["ate"]), gap, Rgap, rgap, rpe["n_pairs"], "kept" if ok else "DROPPED"))
            if ok:
                keep.append(dict(nt=nt, noise=noise, lag=lag, dt=dt, est_R=est_R, est_T=est_T, gt_R=gt_R, gt_T=gt_T, ref=ref,
                                 gap=gap, Rgap=Rgap, rgap=rgap))
    n = len(keep)
    assert n >= 6, n
    pad = lambda key, tail: np.array([np.concatenate([c[key], np.zeros((NT - c["nt"],) + tail)]) for c in keep])
    np.savez_compressed(
        a.out, nt=np.array([c["nt"] for c in keep]), n_ate=np.array([c["nt"] - 1 for c in keep]),
        lag=np.array([c["lag"] for c in keep]), dt=np.array([c["dt"] for c in keep]), noise=np.array([c["noise"] for c in keep]),
        period_ns=np.int64(PERIOD_NS), res=np.float64(RES),
        est_R=pad("est_R", (3, 3)), est_T=pad("est_T", (3,)), gt_R=pad("gt_R", (3, 3)), gt_T=pad("gt_T", (3,)),
        ref_ate=np.array([c["ref"]["ate"] for c in keep]), ref_R=np.array([c["ref"]["R"] for c in keep]),
        ref_T=np.array([c["ref"]["T"] for c in keep]), ref_rpe_pos=np.array([c["ref"]["rpe_pos"] for c in keep]),
        ref_rpe_rot=np.array([c["ref"]["rpe_rot"] for c in keep]),
        ate_gap=np.float64(max(abs(c["gap"]) for c in keep)), R_gap=np.float64(max(c["Rgap"] for c in keep)),
        rpe_gap=np.float64(max(c["rgap"] for c in keep)))
    print("kept %d of %d; ate_gap %.3e R_gap %.3e rpe_gap %.3e -> %s" % (n, len(specs), max(abs(c["gap"]) for c in keep),
                                                                        max(c["Rgap"] for c in keep), max(c["rgap"] for c in keep), a.out))


if __name__ == "__main__":
    main()
