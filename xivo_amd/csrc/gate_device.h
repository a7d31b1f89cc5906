// Estimator::MHGating, src/update.cpp:60-96, stated once for the five kernels that run it: gate_sparse_kernel,
// gate_dense_kernel, gate_ell_kernel (gate_kernels.hip), section 3 of fused_update_f64_kernel (fused_update.hip) and the GATE
// prologue of chol_reg_la_f64_kernel (chol_f64.hip). How a copy obtains the three sums of J P J^T - the 21 / 43-column walks,
// the dense-row sums, the diagonal blocks of an S already formed - is its own; everything behind them is here. (Two stated
// exceptions in the fused kernel, which is at its register limits: it lets every wave relax the threshold, and it keeps the
// lines of gate_reject_pair / gate_zero_rows written out - DESIGN.md section 5.)
#pragma once
#include "common.h"
#include "../../include/xivo_hip.h"

namespace xivo_hip {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// d = res^T (S.llt().solve(res)) for 2x2 S given by its lower triangle
// (src/update.cpp:65-69; Eigen LLT reads the lower triangle)
__device__ __forceinline__ double mh_dist_2x2(double s00, double s10, double s11, double r0, double r1) {
  const double l00 = sqrt(s00);
  const double l10 = s10 / l00;
  const double l11 = sqrt(s11 - l10 * l10);
  const double y0 = r0 / l00;
  const double y1 = (r1 - l10 * y0) / l11;
  const double x1 = y1 / l11;
  const double x0 = (y0 - l10 * x1) / l00;
  return r0 * x0 + r1 * x1;
}

// the distance of one feature from the lower triangle of J P J^T: S_f = J P J^T + R I2 (src/update.cpp:62-64)
__device__ __forceinline__ double gate_dist(double jpj00, double jpj10, double jpj11, double R, double r0, double r1) {
  return mh_dist_2x2(jpj00 + R, jpj10, jpj11 + R, r0, r1);
}
// ... from a diagonal block of S = H P H^T + diag(diagR) (d00, s10, d11) and the pair's diagR: (d - diagR) + R, s10 as it is
__device__ __forceinline__ double gate_dist_S(double d00, double s10, double d11, double dr0, double dr1, double R, double r0,
                                              double r1) {
  return gate_dist(d00 - dr0, s10, d11 - dr1, R, r0, r1);
}

// threshold relaxation loop of src/update.cpp:73-96, run by one wave over the
// F distances in LDS. Returns the threshold that was in force when the loop
// exited (inlier <=> dist < thresh).
// `present` = number of real entries among the F (absent ones carry +inf and can never become inliers).
__device__ inline double relax_threshold(const double* sdist, int F, const GateParams& p, int lane, int present = -1) {
  if (present < 0) present = F;
  if (p.min_inliers <= 0) return -1.0;  // loop body never runs: no inliers (update.cpp:73)
  double thresh = p.thresh;
  for (int it = 0; it < 4096; ++it) {
    int cnt = 0;
    for (int f0 = 0; f0 < F; f0 += 64) {
      const int f = f0 + lane;
      const bool in = (f < F) && (sdist[f] < thresh);
      cnt += __popcll(__ballot(in));
    }
    if (cnt >= p.min_inliers || cnt >= present) return thresh;
    thresh *= p.mult;
  }
  return thresh;
}

// the hand-off of the threshold: behind a barrier (every distance is in sdist[0, F)) wave 0 forms it (`relax`, a callable
// returning the wave-uniform threshold), lane 0 publishes it in sdist[F], and behind a second barrier everybody reads it
template <class Relax>
__device__ __forceinline__ double gate_threshold(double* sdist, int F, int wave, int lane, Relax relax) {
  __syncthreads();
  if (wave == 0) {
    const double th = relax();
    if (lane == 0) sdist[F] = th;
  }
  __syncthreads();
  return sdist[F];
}

// the verdict: inlier <=> dist < thresh (src/update.cpp:78)
__device__ __forceinline__ bool gate_inlier(const double* sdist, int f, double th) { return sdist[f] < th; }
// ... of entry f with its stores, mask[e] and dist[e]. `shown` = 0: dist shows 0 instead of the distance (an absent entry,
// whose distance is +inf, and every entry of a filter that does not gate)
__device__ __forceinline__ bool gate_verdict(const double* sdist, int f, double th, unsigned char* mask, double* dist, long e,
                                             bool shown = true) {
  const bool in = gate_inlier(sdist, f, th);
  mask[e] = in ? 1 : 0;
  dist[e] = shown ? sdist[f] : 0.0;
  return in;
}

// a rejected pair f made neutral - algebraically "row not stacked": innovation 0, measurement variance 1 ...
__device__ __forceinline__ void gate_reject_pair(double* inn, double* diagR, int f) {
  inn[2 * f] = 0.0; inn[2 * f + 1] = 0.0;
  diagR[2 * f] = 1.0; diagR[2 * f + 1] = 1.0;
}
// ... and, where the copy keeps the compressed form, the pair's nval values val[0, nval) 0
__device__ __forceinline__ void gate_reject_pair(double* inn, double* diagR, int f, double* val, int nval) {
  gate_reject_pair(inn, diagR, f);
  for (int t = 0; t < nval; ++t) val[t] = 0.0;
}
// ... and its columns 2f, 2f + 1 of AT [Np x Mp, leading dimension ldat] zeroed by the nt threads of the workgroup
__device__ __forceinline__ void gate_zero_rows(double* AT, int ldat, int f, int Np, int tid, int nt) {
  for (int n = tid; n < Np; n += nt) { AT[n + (long)(2 * f) * ldat] = 0.0; AT[n + (long)(2 * f + 1) * ldat] = 0.0; }
}
// ... with the rows 2f, 2f + 1 of the matrix A [Mp x Np, lda] it is the transpose of
__device__ __forceinline__ void gate_zero_rows(double* A, int lda, double* AT, int ldat, int f, int Np, int tid, int nt) {
  for (int n = tid; n < Np; n += nt) {
    A[2 * f + (long)n * lda] = 0.0; A[2 * f + 1 + (long)n * lda] = 0.0;
    AT[n + (long)(2 * f) * ldat] = 0.0; AT[n + (long)(2 * f + 1) * ldat] = 0.0;
  }
}

// entries present in a filter (sind >= 0), counted by the nt threads of the workgroup through *s_present in LDS;
// Estimator::OutlierRejection gates only when there are more than min_required_inliers_ of them (src/manager.cpp:635).
// s_slot (LDS, [2 F], or null): every entry's sind, ref_sind parked on the way. Ends in a barrier.
__device__ __forceinline__ int gate_count_present(const xivo_feat_in* feats, int F, int* s_present, int* s_slot, int tid, int nt) {
  if (tid == 0) *s_present = 0;
  __syncthreads();
  int cnt = 0;
  for (int f = tid; f < F; f += nt) {
    const int si = feats[f].sind;
    if (s_slot) { s_slot[2 * f] = si; s_slot[2 * f + 1] = feats[f].ref_sind; }
    cnt += si >= 0 ? 1 : 0;
  }
  if (cnt) atomicAdd(s_present, cnt);
  __syncthreads();
  return *s_present;
}

}  // namespace xivo_hip
