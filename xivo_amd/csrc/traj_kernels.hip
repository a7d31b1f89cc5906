// Trajectory log (xivo_hip_traj_*, capi_traj.hip): the per-frame record of every filter's motion state and marginal covariance,
// and the consistency score of the logged poses against ground truth (pose error in the filter's own error coordinates, NEES,
// ensemble mean per frame). Plain fp64 C++; no atomics - the ensemble mean is a fixed-shape tree, so it is reproducible.
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"
#include "geometry_device.h"

namespace xivo_hip {

namespace {

constexpr int TRAJ_REC_WORDS = (int)(sizeof(xivo_traj_rec) / sizeof(double));   // 21 state doubles + the status word
static_assert(sizeof(xivo_traj_rec) == 22 * sizeof(double), "xivo_traj_rec is 22 eight-byte words");
static_assert(offsetof(xivo_pose_in, Vsb) == 24 * sizeof(double) && offsetof(xivo_traj_rec, Vsb) == 12 * sizeof(double),
              "the record is the pose's words 0..11 (Rsb, Tsb) and 24..32 (Vsb, bg, ba)");

// packed lower triangle, row by row: (i, j), i >= j, at i (i + 1) / 2 + j
__device__ __forceinline__ int tri_index(int i, int j) { return i * (i + 1) / 2 + j; }
__device__ __forceinline__ int tri_row(int k) {   // the row i with i (i + 1) / 2 <= k < (i + 1) (i + 2) / 2
  int i = (int)((sqrtf(8.0f * (float)k + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > k) --i;
  while ((i + 1) * (i + 2) / 2 <= k) ++i;
  return i;
}

// One wave-sized workgroup per filter. The lanes stride over the record's 22 words and then the packed covariance entries:
// consecutive lanes write consecutive words of the log; the reads of P are a gather through its padded leading dimension.
__global__ __launch_bounds__(64) void traj_record_kernel(TrajRecordArgs a) {
  __shared__ int cols[XIVO_TRAJ_MAX_COLS];
  const int filt = blockIdx.x, tid = threadIdx.x;
  if (tid < a.n_cols) cols[tid] = a.cols[tid];
  __syncthreads();
  const double* pose = reinterpret_cast<const double*>(a.poses + filt);
  double* rec = reinterpret_cast<double*>(a.rec + filt);
  const double* P = a.P + (long)filt * a.strideP;
  double* cov = a.cov + (long)filt * a.pack;
  for (int k = tid; k < TRAJ_REC_WORDS + a.pack; k += 64) {
    if (k < 12) rec[k] = pose[k];                            // Rsb, Tsb
    else if (k < TRAJ_REC_WORDS - 1) rec[k] = pose[k + 12];  // Vsb, bg, ba (behind Rbc, Tbc in xivo_pose_in)
    else if (k == TRAJ_REC_WORDS - 1) {
      int2 w; w.x = a.status[filt]; w.y = 0;
      *reinterpret_cast<int2*>(rec + k) = w;
    } else {
      const int e = k - TRAJ_REC_WORDS, i = tri_row(e), j = e - i * (i + 1) / 2;
      const int ci = cols[i], cj = cols[j];
      const int r = ci > cj ? ci : cj, c = ci > cj ? cj : ci;
      cov[e] = P[r + (long)c * a.ldp];
    }
  }
}

// One thread per (frame, filter) entry of the slice: e = (log(R_est^T R_gt), T_gt - T_est), Sigma = L L^T in registers,
// nees = |L^-1 e|^2 (NaN when the un-pivoted factorisation meets a pivot that is not positive).
__global__ __launch_bounds__(256) void traj_nees_kernel(TrajNeesArgs a) {
  const long n = (long)a.nt * a.nb;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int t = (int)(id / a.nb), b = (int)(id % a.nb);
  const long at = (long)(a.t0 + t) * a.Bmax + a.b0 + b;
  const xivo_traj_rec& X = a.rec[at];
  const double* cov = a.cov + at * a.pack;
  const double* g = a.gt + id * 12;
  const V3 w = so3_log_dev(m3_mul(m3_t(m3_from_colmajor(X.Rsb)), m3_from_colmajor(g)));
  double e[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) { e[i] = w.v[i]; e[3 + i] = g[9 + i] - X.Tsb[i]; }
  double L[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const int pi = a.pos6[i], pj = a.pos6[j];
      L[i][j] = cov[pi > pj ? tri_index(pi, pj) : tri_index(pj, pi)];
    }
  bool ok = true;
  double nees = 0.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {                       // column Cholesky with the forward substitution of e folded in
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && d > 0.0 && d < INFINITY;               // (a NaN pivot fails the first comparison)
    const double l = sqrt(d);
    L[j][j] = l;
    double y = e[j];
#pragma unroll
    for (int k = 0; k < j; ++k) y -= L[j][k] * e[k];
    y /= l;
    e[j] = y;                                         // e becomes y = L^-1 e as the columns complete
    nees += y * y;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  if (a.err6) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.err6[id * 6 + i] = w.v[i]; a.err6[id * 6 + 3 + i] = g[9 + i] - X.Tsb[i]; }
  }
  a.nees[id] = ok ? nees : NAN;
}

// The mean of the finite values of every frame, v [nt][per] -> anees [nt], n_used [nt] (the trajectory log's [nb] NEES, the
// landmark log's [nb][n_out]). One workgroup per frame: every thread adds the finite entries tid, tid + 256, ... in that order,
// then a fixed-shape tree over the 256 partial sums - the same additions in the same order whatever the machine does.
__global__ __launch_bounds__(256) void frame_anees_kernel(const double* nees, long per, double* anees, int* n_used) {
  __shared__ double ssum[256];
  __shared__ int scnt[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* v = nees + (long)t * per;
  double s = 0.0;
  int c = 0;
  for (long i = tid; i < per; i += 256) {
    const double x = v[i];
    if (fabs(x) < INFINITY) { s += x; ++c; }
  }
  ssum[tid] = s; scnt[tid] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { ssum[tid] += ssum[tid + h]; scnt[tid] += scnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    anees[t] = scnt[0] > 0 ? ssum[0] / (double)scnt[0] : NAN;
    n_used[t] = scnt[0];
  }
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_traj_record(const TrajRecordArgs& a, int batch, hipStream_t s) {
  if (batch <= 0) return 0;
  hipLaunchKernelGGL(traj_record_kernel, dim3(batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}

int launch_traj_nees(const TrajNeesArgs& a, hipStream_t s) {
  const long n = (long)a.nt * a.nb;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(traj_nees_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return (int)hipErrorLaunchFailure;
  return launch_frame_anees(a.nees, a.nb, a.nt, a.anees, a.n_used, s);
}

int launch_frame_anees(const double* nees, long per, int nt, double* anees, int* n_used, hipStream_t s) {
  if (nt <= 0 || per <= 0) return 0;
  hipLaunchKernelGGL(frame_anees_kernel, dim3(nt), dim3(256), 0, s, nees, per, anees, n_used);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
