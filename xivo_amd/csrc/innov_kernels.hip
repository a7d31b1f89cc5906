// Innovation log (xivo_hip_innov_*, capi_innov.hip): the per-frame record of every filter's normalised innovation squared from
// the staged rows and the resident dx, and the ensemble / per-filter sums of the logged records. The arithmetic and the order
// of its additions are innov_device.h's; this file maps them onto a workgroup. Plain fp64, no atomics: every sum is a
// fixed-shape reduction, so a record and a statistic are reproducible bit for bit.
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"
#include "ell.h"
#include "innov_device.h"

namespace xivo_hip {

namespace {

static_assert(sizeof(xivo_innov_rec) == 64, "xivo_innov_rec is eight eight-byte words");
static_assert(ELL_W <= kInnovWave, "one lane per slot of a row pair");

// the tree of innov_tree over the workgroup's partial results (every thread calls it)
__device__ __forceinline__ void tree_reduce(InnovAcc* part, int tid) {
  __syncthreads();
  for (int h = kInnovThreads / 2; h > 0; h >>= 1) {
    if (tid < h) innov_combine(part[tid], part[tid + h]);
    __syncthreads();
  }
}

__device__ __forceinline__ double wave_sum(double v) {   // innov_wave_sum: xor butterfly, offsets 32 .. 1
#pragma unroll
  for (int off = kInnovWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kInnovWave);
  return v;
}

// One workgroup of four waves per filter. dx is staged in LDS once; phase 1 leaves (H dx)_i and "row i has a non-zero entry"
// in LDS - a wave per compressed row pair (lane t reads slot t: the pair's 28 indices and 28 value pairs arrive as two
// coalesced requests; lane t < lead_k reads the lead block's column t), a thread per dense row (consecutive threads read
// consecutive rows of a column: coalesced along the column-major rows); phase 2 adds the rows in the fixed order of
// innov_device.h and the first eight lanes store the record's eight words as one 64-byte request.
__global__ __launch_bounds__(kInnovThreads) void innov_record_kernel(InnovRecordArgs a) {
  extern __shared__ double smem[];
  __shared__ InnovAcc part[kInnovThreads];
  __shared__ xivo_innov_rec out;
  const int filt = blockIdx.x, tid = threadIdx.x, lane = tid & (kInnovWave - 1), wave = tid / kInnovWave;
  const int N = a.N, M = a.M, Me = (M + 1) & ~1;
  double* dx = smem;
  double* hdx = dx + N;
  int* nzr = reinterpret_cast<int*>(hdx + Me);
  const double* err = a.err + (long)filt * a.strideErr;
  InnovAcc acc = innov_zero();
  for (int k = tid; k < N; k += kInnovThreads) { const double d = err[k]; dx[k] = d; innov_add_dx(acc, d); }
  __syncthreads();

  const bool dense = a.dense_all || a.over[filt] != 0;
  const int er = dense ? 0 : a.ell_rows;              // rows [0, er) are compressed, rows [er, M) dense
  const int* idx = a.ell_idx + (long)filt * a.stride_idx;
  const double2* val = reinterpret_cast<const double2*>(a.ell_val + (long)filt * a.stride_val);
  const double* lead = a.lead ? a.lead + (long)filt * a.strideLead : nullptr;
  for (int p = wave; p < (er + 1) / 2; p += kInnovThreads / kInnovWave) {
    double h0 = 0.0, h1 = 0.0;
    int z = 0;
    if (lane < ELL_W) {
      const int n = idx[(long)p * ELL_W + lane];
      const double2 v = val[(long)p * ELL_W + lane];
      const double d = dx[n];
      h0 = innov_term(v.x, d); h1 = innov_term(v.y, d);
      z = (v.x != 0.0 ? 1 : 0) | (v.y != 0.0 ? 2 : 0);
    }
    if (lead && lane < a.lead_k) {
      const double l0 = lead[2 * p + (long)lane * a.ldlead], l1 = lead[2 * p + 1 + (long)lane * a.ldlead];
      const double d = dx[lane];
      h0 = innov_term_add(h0, l0, d); h1 = innov_term_add(h1, l1, d);
      z |= (l0 != 0.0 ? 1 : 0) | (l1 != 0.0 ? 2 : 0);
    }
    h0 = wave_sum(h0); h1 = wave_sum(h1);
    const bool nz0 = __ballot(z & 1) != 0, nz1 = __ballot(z & 2) != 0;
    if (lane == 0) { hdx[2 * p] = h0; hdx[2 * p + 1] = h1; nzr[2 * p] = nz0; nzr[2 * p + 1] = nz1; }
  }
  const double* H = a.H + (long)filt * a.strideH;
  for (int i = er + tid; i < M; i += kInnovThreads) {
    double h = 0.0;
    int z = 0;
    for (int n = 0; n < N; ++n) {
      const double v = H[i + (long)n * a.ldh];
      h = innov_term_add(h, v, dx[n]);
      z |= v != 0.0 ? 1 : 0;
    }
    hdx[i] = h; nzr[i] = z;
  }
  __syncthreads();

  const double* inn = a.inn + (long)filt * a.strideInn;
  const double* dR = a.diagR + (long)filt * a.strideR;
  for (int i = tid; i < M; i += kInnovThreads) innov_add_row(acc, inn[i], dR[i], hdx[i], nzr[i] != 0);
  part[tid] = acc;
  tree_reduce(part, tid);
  if (tid == 0) out = innov_finish(part[0], M, a.status[filt], a.ldlt_used[filt]);
  __syncthreads();
  if (tid < 8) reinterpret_cast<double*>(a.rec + filt)[tid] = reinterpret_cast<const double*>(&out)[tid];
}

// One workgroup per group (a frame: its filters; a filter: its frames): thread t adds elements t, t + 256, ... in ascending
// order, then the same tree.
__global__ __launch_bounds__(kInnovThreads) void innov_stats_kernel(InnovStatsArgs a) {
  __shared__ double ssum[kInnovThreads];
  __shared__ long long sdof[kInnovThreads];
  __shared__ int scnt[kInnovThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const xivo_innov_rec* rec = a.rec + a.base + (long)g * a.g_stride;
  double s = 0.0;
  long long d = 0;
  int c = 0;
  for (int e = tid; e < a.n_elems; e += kInnovThreads) {
    const xivo_innov_rec r = rec[(long)e * a.e_stride];
    if (innov_in_stats(r)) { s += r.nis; d += r.dof; ++c; }
  }
  ssum[tid] = s; sdof[tid] = d; scnt[tid] = c;
  __syncthreads();
  for (int h = kInnovThreads / 2; h > 0; h >>= 1) {
    if (tid < h) { ssum[tid] += ssum[tid + h]; sdof[tid] += sdof[tid + h]; scnt[tid] += scnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) { a.nis[g] = ssum[0]; a.dof[g] = sdof[0]; a.used[g] = scnt[0]; }
}

}  // namespace

// dx, (H dx) and the row flags of one filter in LDS next to the tree's 256 partial results
size_t innov_record_lds(int M, int N) { const size_t Me = ((size_t)M + 1) & ~(size_t)1; return ((size_t)N + Me) * sizeof(double) + Me * sizeof(int); }

int launch_innov_record(const InnovRecordArgs& a, int batch, hipStream_t s) {
  if (batch <= 0) return 0;
  const size_t lds = innov_record_lds(a.M, a.N);
  if (lds > 48 * 1024) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(innov_record_kernel, dim3(batch), dim3(kInnovThreads), lds, s, a);
  return (int)hipGetLastError();
}

int launch_innov_stats(const InnovStatsArgs& a, hipStream_t s) {
  if (a.n_groups <= 0) return 0;
  hipLaunchKernelGGL(innov_stats_kernel, dim3(a.n_groups), dim3(kInnovThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace xivo_hip
