// Innovation log (innov_kernels.hip): the per-row and per-filter arithmetic of the normalised innovation squared, as plain fp64
// C++ for host and device. A host compiler takes the header alone: tests/innov_row_driver.cpp (tests/test_innov_log_cpu.py)
// runs it - with the lanes of a wave and the threads of a workgroup as arrays - without a GPU.
//
// After dx = K inn the three sums need no factor of S: with r = inn - H dx (the post-fit residual), inn - H dx = R S^-1 inn, so
//   nis     = inn^T S^-1 inn = sum_i inn_i r_i / R_i
//   prefit  = sum_i inn_i^2 / R_i
//   postfit = sum_i r_i^2 / R_i
// PRICE of the factor-free form: nis is what is left of prefit after a cancellation, so the rounding of r (a few u |H||dx|
// per row) is amplified by prefit / nis ~ |S| / R: about 1e-9 relative at a ratio of 1e7, 2e-6 at 1e11 (DESIGN.md,
// "Innovation log"). prefit is in the record so that a caller can see the ratio.
//
// ORDER of every addition (a function of M, N and the representation of the rows only):
//   row of a compressed pair   lane t < 28 holds slot t's product (+ the lead column t's, t < 48, as one fma on top of it),
//                              then the butterfly of innov_wave_sum over the 64 lanes: 6 additions deep (+ 1 with a lead block)
//   dense row                  one thread, columns 0 .. N-1 in ascending order, one fma each
//   rows -> filter             thread t of 256 adds rows t, t + 256, ... in ascending order; then the tree of innov_tree over the
//                              256 partial sums: 8 additions deep
// A structurally zero entry (value 0) adds nothing and is not multiplied: a NaN in dx reaches nis only through a column the
// row uses.
#pragma once
#include <math.h>

#include "../../include/xivo_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_INNOV_HD __host__ __device__ __forceinline__
#else
#define XIVO_INNOV_HD inline
#endif

namespace xivo_hip {

constexpr int kInnovThreads = 256;   // threads of the record kernel's workgroup = leaves of innov_tree
constexpr int kInnovWave = 64;

struct InnovAcc { double nis, prefit, postfit, inn_max, dx_max; int dof; };

XIVO_INNOV_HD InnovAcc innov_zero() { return InnovAcc{0.0, 0.0, 0.0, 0.0, 0.0, 0}; }
// the larger of two magnitudes; a NaN wins whatever the order of the operands
XIVO_INNOV_HD double innov_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// one stored entry of a row times its column of dx, as the first term of a lane (compressed slot) ...
XIVO_INNOV_HD double innov_term(double v, double dx) { return v != 0.0 ? v * dx : 0.0; }
// ... and on top of what the lane / thread already holds (lead column, dense column)
XIVO_INNOV_HD double innov_term_add(double acc, double v, double dx) { return v != 0.0 ? fma(v, dx, acc) : acc; }

// row i of a filter enters its thread's partial sums: hdx = (H dx)_i, nz = the row has a non-zero H entry. Counted rows only
// (nz or inn != 0): neutralised pairs (values 0, inn 0, diagR 1) and absent features drop out here.
XIVO_INNOV_HD void innov_add_row(InnovAcc& a, double inn, double R, double hdx, bool nz) {
  if (!nz && inn == 0.0) return;
  const double r = inn - hdx;
  a.nis += inn * r / R;
  a.prefit += inn * inn / R;
  a.postfit += r * r / R;
  a.inn_max = innov_max(a.inn_max, fabs(inn));
  a.dof += 1;
}
XIVO_INNOV_HD void innov_add_dx(InnovAcc& a, double dx) { a.dx_max = innov_max(a.dx_max, fabs(dx)); }

// a <- a (+) b: one node of the tree
XIVO_INNOV_HD void innov_combine(InnovAcc& a, const InnovAcc& b) {
  a.nis += b.nis; a.prefit += b.prefit; a.postfit += b.postfit;
  a.inn_max = innov_max(a.inn_max, b.inn_max); a.dx_max = innov_max(a.dx_max, b.dx_max); a.dof += b.dof;
}

// the filter's record from the root of the tree. status != 0: the update kept the prior and dx = 0 - the sums say nothing
XIVO_INNOV_HD xivo_innov_rec innov_finish(const InnovAcc& a, int rows, int status, int ldlt_used) {
  xivo_innov_rec r;
  const bool failed = status != 0;
  r.nis = failed ? (double)NAN : a.nis; r.prefit = failed ? (double)NAN : a.prefit; r.postfit = failed ? (double)NAN : a.postfit;
  r.inn_max = a.inn_max; r.dx_max = a.dx_max; r.dof = a.dof; r.rows = rows;
  r.flags = (failed ? XIVO_INNOV_FAILED : 0) | (ldlt_used ? XIVO_INNOV_LDLT : 0); r.reserved = 0; r.reserved2 = 0.0;
  return r;
}
// whether a record enters xivo_hip_innov_stats
XIVO_INNOV_HD bool innov_in_stats(const xivo_innov_rec& r) { return r.flags == 0 && fabs(r.nis) < INFINITY; }

#if !defined(__HIP_DEVICE_COMPILE__)
// the wave's cross-lane sum as the kernel's xor butterfly forms it (offsets 32, 16, ..., 1): every lane ends with the same value
inline double innov_wave_sum(const double lane[kInnovWave]) {
  double v[kInnovWave], w[kInnovWave];
  for (int i = 0; i < kInnovWave; ++i) v[i] = lane[i];
  for (int off = kInnovWave / 2; off > 0; off >>= 1) {
    for (int i = 0; i < kInnovWave; ++i) w[i] = v[i] + v[i ^ off];
    for (int i = 0; i < kInnovWave; ++i) v[i] = w[i];
  }
  return v[0];
}
// the workgroup's tree over the 256 partial results: part[t] (+)= part[t + h], h = 128, 64, ..., 1
inline InnovAcc innov_tree(InnovAcc part[kInnovThreads]) {
  for (int h = kInnovThreads / 2; h > 0; h >>= 1)
    for (int t = 0; t < h; ++t) innov_combine(part[t], part[t + h]);
  return part[0];
}
#endif

}  // namespace xivo_hip
