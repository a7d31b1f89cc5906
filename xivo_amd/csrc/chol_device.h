// The 16 x 16 diagonal-block factor-and-invert step shared by every kernel that factors S: the Cholesky kernels of
// chol_f64.hip (chol_f64_kernel, chol_reg_f64_kernel, chol_reg_la_f64_kernel) and the one-kernel update (fused_update.hip).
// They all use this one routine (there is no second form and no build switch that selects one) with the same operand order
// around it, so that they all produce the SAME bits. A non-positive pivot is recorded, not replaced: the factor of a flagged
// filter may hold NaNs, and its caller discards it (status, ldlt_fallback.hip).
#pragma once
#include "mfma_util.h"

#ifndef XIVO_CHAIN_STAMP
#define XIVO_CHAIN_STAMP(slot) do {} while (0)   // (trace builds of the one-kernel update: shader-clock stamp per pivot)
#endif

namespace xivo_hip {

namespace {

// one cubic step on v_rsq_f64's 2^-24 estimate: e = 1 - p rd^2 ~ 1e-7, rd (1 + e/2 + 3 e^2 / 8) leaves e^3 ~ 1e-22 - a shorter dependent
// chain (mul, fma, fma, fma) than two Newton steps (mul, fma, mul, mul, fma, mul)
__device__ __forceinline__ double cubic_rsqrt(double p) {
#pragma clang fp contract(off)
  const double rd = __builtin_amdgcn_rsq(p);
  const double e = __builtin_fma(-(p * rd), rd, 1.0);
  const double t = __builtin_fma(0.375, e, 0.5);
  return __builtin_fma(rd * e, t, rd);
}

// Factor AND invert one 16x16 diagonal block, held by one wave in the C/D layout of v_mfma_f64_16x16x4_f64:
// x[r] of lane (li, lg) is X[li][lg + 4 r] on entry (X symmetric up to rounding; only X[i][c], i >= c, is consumed). On return
// x[r] = L[li][lg + 4 r] (for lg + 4 r <= li, zero above) and y[r] = inv(L)[lg + 4 r][li].
// Four steps of four columns (round 6; the sixteen-pivot forms it replaced paid one matrix-pipe round trip per pivot). Per step:
//   1. the 4 x 4 diagonal sub-block D (ten elements of register x[q], lanes (c + a) + 16 b) is read into scalar registers;
//   2. every lane factors it with plain VALU arithmetic on those uniform values (four v_rsq_f64 chains, no cross-lane
//      traffic), and lane group lg solves L44 y = e_lg for column lg of M = inv(L44) (ten operations with per-lane constants e,
//      the same for every lane) and picks y[li & 3];
//   3. the two panel products run on v_mfma_f64_4x4x4_4b_f64 (four passes instead of sixteen: operands A lane 16 k + 4 blk + i,
//      B lane 16 k + 4 blk + j, result lane 16 i + 4 blk + j - scripts/mfma44_layout.hip - i.e. M[li & 3][lg] against the lane's
//      own x[q] gives L[li][c + lg] in place, and against y[q] the four new rows of inv(L));
//   4. the trailing update X -= Lp Lp^T (and Y -= Lp Ytop) is ONE rank-four MFMA each, operands again the lane's own registers.
// The chain is issue-bound (~170 instructions per step at 4 - 8 cycles each; v_rsq_f64's refinement is only an eighth of it).
// A non-positive pivot is only recorded (first one wins, bad = 1 + its row); the arithmetic runs on (NaNs at worst: the caller
// discards the factor of such a filter).
__device__ __forceinline__ void factor_invert_diag(d4& x, d4& y, int& bad, const int row0, const int li, const int lg) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = (lg + 4 * r == li) ? 1.0 : 0.0;
  const double e0 = lg == 0 ? 1.0 : 0.0, e1 = lg == 1 ? 1.0 : 0.0, e2 = lg == 2 ? 1.0 : 0.0, e3 = lg == 3 ? 1.0 : 0.0;
  const int n = li & 3;
  static_for<4>([&](auto qc) {
    constexpr int q = decltype(qc)::value, c = 4 * q;
    XIVO_CHAIN_STAMP(row0 == 0 ? 16 + 4 * q : 99);
    // D[a][b] = X[c + a][c + b]: register q of lane li = c + b, lg = a
    const double d00 = readlane_d(x[q], c + 0), d10 = readlane_d(x[q], c + 16), d20 = readlane_d(x[q], c + 32), d30 = readlane_d(x[q], c + 48);
    const double d11 = readlane_d(x[q], c + 1 + 16), d21 = readlane_d(x[q], c + 1 + 32), d31 = readlane_d(x[q], c + 1 + 48);
    const double d22 = readlane_d(x[q], c + 2 + 32), d32 = readlane_d(x[q], c + 2 + 48), d33 = readlane_d(x[q], c + 3 + 48);
    const double p0 = d00;
    const double r0 = cubic_rsqrt(p0);
    const double l10 = d10 * r0, l20 = d20 * r0, l30 = d30 * r0;
    const double p1 = __builtin_fma(-l10, l10, d11);
    const double t21 = __builtin_fma(-l20, l10, d21), t31 = __builtin_fma(-l30, l10, d31);
    const double t22 = __builtin_fma(-l20, l20, d22), t32 = __builtin_fma(-l30, l20, d32), t33 = __builtin_fma(-l30, l30, d33);
    const double r1 = cubic_rsqrt(p1);
    const double y0 = e0 * r0;
    const double l21 = t21 * r1, l31 = t31 * r1;
    const double p2 = __builtin_fma(-l21, l21, t22);
    const double u32 = __builtin_fma(-l31, l21, t32), u33 = __builtin_fma(-l31, l31, t33);
    const double r2 = cubic_rsqrt(p2);
    const double y1 = __builtin_fma(-l10, y0, e1) * r1;
    const double a2 = __builtin_fma(-l21, y1, __builtin_fma(-l20, y0, e2));
    const double a3 = __builtin_fma(-l31, y1, __builtin_fma(-l30, y0, e3));
    const double l32 = u32 * r2;
    const double p3 = __builtin_fma(-l32, l32, u33);
    const double r3 = cubic_rsqrt(p3);
    const double y2 = a2 * r2;
    const double b3 = __builtin_fma(-l32, y2, a3);
    const double pre = n == 0 ? y0 : (n == 1 ? y1 : y2);
    const double mt = n == 3 ? b3 * r3 : pre;             // M[li & 3][lg] (0 above the diagonal: e is)
    const bool ok = (p0 > 0.0) && (p1 > 0.0) && (p2 > 0.0) && (p3 > 0.0);
    if (!ok && !bad) bad = 1 + row0 + c + (!(p0 > 0.0) ? 0 : !(p1 > 0.0) ? 1 : !(p2 > 0.0) ? 2 : 3);
    const double pan0 = __builtin_amdgcn_mfma_f64_4x4x4f64(mt, x[q], 0.0, 0, 0, 0);
    const double ytp0 = __builtin_amdgcn_mfma_f64_4x4x4f64(mt, y[q], 0.0, 0, 0, 0);
    const double lp = (li >= c + lg) ? pan0 : 0.0;
    x[q] = lp;
    y[q] = ytp0;
    if constexpr (q < 3) {
      const double lb = (li > c + 3) ? lp : 0.0;   // rows below the sub-block
      const double al = -lb;
      x = mfma(al, lb, x);
      y = mfma(al, ytp0, y);
    }
  });
}

}  // namespace

}  // namespace xivo_hip
