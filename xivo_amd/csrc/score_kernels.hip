// Trajectory score (xivo_hip_traj_score, capi_score.hip): per filter of a slice of the trajectory log the least-squares rigid
// alignment of ground truth onto the logged positions, the aligned and unaligned ATE and the RPE at a frame lag
// (src/metrics.cpp of the reference; the alignment is the closed form, score_device.h). Plain fp64 C++; no atomics.
//
// One wave-sized workgroup per filter, the lanes stride over the frames of the slice: lane l adds frames l, l + 64, ... in that
// order, then a fixed-shape tree over the 64 partial sums - the additions and their order depend on (t0, nt) alone, not on
// b0, nb, the grid or the other filters. Three passes over the frames (centroids, centred cross-covariance, residuals), then
// the pairs of the RPE. The log is frame-major [T_max][batch_max]: the records one wave reads are batch_max x 176 bytes
// apart, so nothing coalesces - a lane's 96 useful bytes (Rsb, Tsb) lie in one or two 128-byte lines of its own.
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"
#include "geometry_device.h"
#include "score_device.h"

namespace xivo_hip {

namespace {

constexpr int SCORE_LANES = 64;
static_assert(sizeof(xivo_traj_score) == 19 * sizeof(double) + 4 * sizeof(int), "xivo_traj_score: 19 doubles and 4 ints, no padding");

// v[k] <- the sum over the 64 lanes of v[k], k < K, in every lane: 32 + 16 + ... + 1 pairwise additions through LDS
template <int K> __device__ __forceinline__ void wave_sum(double (&v)[K], double* lds /* [K][64] */) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) lds[k * SCORE_LANES + tid] = v[k];
  __syncthreads();
  for (int h = SCORE_LANES / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < K; ++k) lds[k * SCORE_LANES + tid] += lds[k * SCORE_LANES + tid + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = lds[k * SCORE_LANES];
  __syncthreads();                             // the next call writes lds again
}

struct FramePose { double R[9], T[3]; bool ok; };

__device__ __forceinline__ FramePose load12(const double* p) {
  FramePose f;
  f.ok = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { f.R[i] = p[i]; f.ok = f.ok && fabs(f.R[i]) < INFINITY; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { f.T[i] = p[9 + i]; f.ok = f.ok && fabs(f.T[i]) < INFINITY; }
  return f;
}

// g1^-1 g2 of two poses (R column-major): R1^T R2, R1^T (T2 - T1)
__device__ __forceinline__ void relative_pose(const FramePose& g1, const FramePose& g2, M3& R, V3& p) {
  const M3 R1t = m3_t(m3_from_colmajor(g1.R));
  R = m3_mul(R1t, m3_from_colmajor(g2.R));
  p = m3_mulv(R1t, V3{{g2.T[0] - g1.T[0], g2.T[1] - g1.T[1], g2.T[2] - g1.T[2]}});
}

__global__ __launch_bounds__(SCORE_LANES) void traj_score_kernel(TrajScoreArgs a) {
  __shared__ double lds[9 * SCORE_LANES];
  const int b = blockIdx.x, tid = threadIdx.x;
  // estimate (the record starts with Rsb, Tsb) and truth of frame t of the slice
  auto est_at = [&](long t) { return load12(reinterpret_cast<const double*>(a.rec + ((a.t0 + t) * a.Bmax + a.b0 + b))); };
  auto gt_at = [&](long t) { return load12(a.gt + (t * a.nb + b) * 12); };

  // pass 1: centroids of the used frames
  double s1[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long t = tid; t < a.nt; t += SCORE_LANES) {
    const FramePose y = est_at(t), x = gt_at(t);
    if (!(y.ok && x.ok)) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i) { s1[i] += x.T[i]; s1[3 + i] += y.T[i]; }
    s1[6] += 1.0;
  }
  wave_sum(s1, lds);
  const int n_used = (int)s1[6];
  double xb[3] = {0, 0, 0}, yb[3] = {0, 0, 0};
  if (n_used > 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { xb[i] = s1[i] / s1[6]; yb[i] = s1[3 + i] / s1[6]; }
  }

  // pass 2: H = sum (y - ybar)(x - xbar)^T
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long t = tid; t < a.nt; t += SCORE_LANES) {
    const FramePose y = est_at(t), x = gt_at(t);
    if (!(y.ok && x.ok)) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) h[3 * i + j] += (y.T[i] - yb[i]) * (x.T[j] - xb[j]);
  }
  wave_sum(h, lds);
  double H[3][3], R[3][3], sv[3], T[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = h[3 * i + j];
  int flags = score_kabsch(H, R, sv);          // every lane the same arithmetic on the same H
  if (n_used < 3) flags |= XIVO_TRAJ_SCORE_UNDETERMINED;
  if (!a.align || n_used == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = a.align ? yb[i] - (R[i][0] * xb[0] + R[i][1] * xb[1] + R[i][2] * xb[2]) : 0.0;

  // pass 3: the residuals themselves, y - (R x + T) written about the centroids (T = ybar - R xbar), and y - x
  double s3[2] = {0, 0};
  for (long t = tid; t < a.nt; t += SCORE_LANES) {
    const FramePose y = est_at(t), x = gt_at(t);
    if (!(y.ok && x.ok)) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double xc0 = x.T[0] - xb[0], xc1 = x.T[1] - xb[1], xc2 = x.T[2] - xb[2];
      const double r = a.align ? (y.T[i] - yb[i]) - (R[i][0] * xc0 + R[i][1] * xc1 + R[i][2] * xc2) : y.T[i] - x.T[i];
      const double w = y.T[i] - x.T[i];
      s3[0] += r * r; s3[1] += w * w;
    }
  }
  wave_sum(s3, lds);

  // RPE: pairs (t, t + lag) inside the slice with both frames used
  double s4[3] = {0, 0, 0};
  if (a.rpe_lag > 0) {
    for (long t = tid; t < (long)a.nt - a.rpe_lag; t += SCORE_LANES) {
      const FramePose y1 = est_at(t), x1 = gt_at(t), y2 = est_at(t + a.rpe_lag), x2 = gt_at(t + a.rpe_lag);
      if (!(y1.ok && x1.ok && y2.ok && x2.ok)) continue;
      M3 RX, RY; V3 pX, pY;
      relative_pose(x1, x2, RX, pX);
      relative_pose(y1, y2, RY, pY);
      const M3 RXt = m3_t(RX);
      const V3 w = so3_log_dev(m3_mul(RXt, RY));
      const V3 p = m3_mulv(RXt, V3{{pY.v[0] - pX.v[0], pY.v[1] - pX.v[1], pY.v[2] - pX.v[2]}});
      s4[0] += p.v[0] * p.v[0] + p.v[1] * p.v[1] + p.v[2] * p.v[2];
      s4[1] += w.v[0] * w.v[0] + w.v[1] * w.v[1] + w.v[2] * w.v[2];
      s4[2] += 1.0;
    }
    wave_sum(s4, lds);
  }

  if (tid != 0) return;
  xivo_traj_score o;
  const int n_pairs = (int)s4[2];
  o.ate = n_used > 0 ? sqrt(s3[0] / s1[6]) : -1.0;
  o.ate_raw = n_used > 0 ? sqrt(s3[1] / s1[6]) : -1.0;
  o.rpe_pos = n_pairs > 0 ? sqrt(s4[0] / s4[2]) : -1.0;
  o.rpe_rot = n_pairs > 0 ? sqrt(s4[1] / s4[2]) : -1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.R[i + 3 * j] = R[i][j];
    o.T[i] = T[i];
    o.sv[i] = n_used > 0 ? sv[i] : 0.0;
  }
  o.n_used = n_used; o.n_pairs = n_pairs; o.flags = flags; o.reserved = 0;
  a.out[b] = o;
}

}  // namespace

int launch_traj_score(const TrajScoreArgs& a, hipStream_t s) {
  if (a.nb <= 0) return 0;
  // one wave per filter: a launch holds fewer than 2^32 threads
  if (a.nt < 0 || a.rpe_lag < 0 || (long)a.nb * SCORE_LANES > 0xffffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(traj_score_kernel, dim3((unsigned)a.nb), dim3(SCORE_LANES), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace xivo_hip
