// Resident-state plumbing of the EKF (gfx950): layout moves of P and of the measurement buffers, edits of P and of
// the resident scene, AbsorbError, and the fp64 MFMA issue-rate probe.
//
//  unpack_P_kernel      host-layout P -> padded device P (lower triangle authoritative, p_unpack_device.h)
//  pack_P_kernel        padded device P -> host layout
//  unpack_meas_kernel   raw H -> padded H / H^T
//  transpose_H_kernel   H^T from the dense H (staged_rows.h: ht_alive)
//  p_* kernels          host edits of P_; p_copy_rc: Estimator::AddGroupToState   src/estimator.cpp:808-816
//  set_pixels_kernel    the tracker's pixels into the resident features (xivo_hip_set_pixels)
//  edit_batch_kernel    Estimator::{Add,Remove}{Group,Feature}{To,From}State on P_ and the scene
//                                                          src/estimator.cpp:739-846
//  absorb_error_kernel  Estimator::AbsorbError             src/estimator.cpp:875-921
//  mfma_peak_kernel     fp64 MFMA issue-rate probe (no reference counterpart)
// (paths relative to the reference tree). Byte movers and one-workgroup-per-filter edits, no MFMA outside the probe.
#include "edit_device.h"
#include "ekf_kernels.h"
#include "geometry_device.h"
#include "p_unpack_device.h"

namespace xivo_hip {

namespace {

// ---------------------------------------------------------------- pack/unpack
// (lower triangle of the host matrix authoritative: p_unpack_device.h)
__global__ __launch_bounds__(256) void unpack_P_kernel(const double* __restrict__ raw, double* __restrict__ P, int N, int Np,
                                                      int ldp, long strideP) {
  __shared__ double tile[kPUnpackTile][kPUnpackTile + 1];
  const int f = blockIdx.y;
  p_unpack_tile_pair(raw + (long)f * N * N, N, N, P + (long)f * strideP, ldp, Np, blockIdx.x, tile);
}

__global__ void pack_P_kernel(const double* __restrict__ P, double* __restrict__ raw, int N, int ldp,
                              long strideP) {
  const int f = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)N * N) return;
  const int i = (int)(e % N), j = (int)(e / N);
  raw[(long)f * N * N + e] = P[(long)f * strideP + i + (long)j * ldp];
}

// dense padded H / H^T of the filters that do NOT fit the row-pair compressed form (only_if[f] != 0; null: all)
__global__ void unpack_meas_kernel(const double* __restrict__ rawH, long strideRaw, int ldraw,
                                   const int* __restrict__ only_if, MeasBuffers mb, int M, int Mp, int N, int Np) {
  const int f = blockIdx.y;
  if (only_if && !only_if[f]) return;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long tot = (long)Mp * Np;
  if (e < tot) {
    {  // H: m fastest
      const int m = (int)(e % Mp), n = (int)(e / Mp);
      double v = 0.0;
      if (m < M && n < N) v = rawH[(long)f * strideRaw + m + (long)n * ldraw];
      mb.H[(long)f * mb.strideH + m + (long)n * mb.ldh] = v;
    }
    {  // H^T: n fastest
      const int n = (int)(e % Np), m = (int)(e / Np);
      double v = 0.0;
      if (m < M && n < N) v = rawH[(long)f * strideRaw + m + (long)n * ldraw];
      mb.HT[(long)f * mb.strideHT + n + (long)m * mb.ldht] = v;
    }
  }
}

// ---------------------------------------------------------------- P edits
__global__ void p_zero_rc_kernel(double* P, int ldp, int Np, int off, int len) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Np) return;
  for (int r = 0; r < len; ++r) {
    P[(off + r) + (long)t * ldp] = 0.0;
    P[t + (long)(off + r) * ldp] = 0.0;
  }
}
// rows first, then columns - the order of Estimator::AddGroupToState
// (src/estimator.cpp:808-816); phase selects which.
__global__ void p_copy_rc_kernel(double* P, int ldp, int Np, int dst, int src, int len, int phase) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Np) return;
  for (int r = 0; r < len; ++r) {
    if (phase == 0) P[(dst + r) + (long)t * ldp] = P[(src + r) + (long)t * ldp];
    else P[t + (long)(dst + r) * ldp] = P[t + (long)(src + r) * ldp];
  }
}
__global__ void p_diag_kernel(const double* P, int ldp, int N, double* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < N) out[t] = P[t + (long)t * ldp];
}

// ---------------------------------------------------------------- batched resident edits (xivo_hip_edit_batch)
// (every edit is a function of edit_device.h, shared with the device life cycles)
// xivo_hip_set_pixels: one thread per (filter, list entry)
__global__ void set_pixels_kernel(xivo_feat_in* feats, int Fmax, int F, const double* xp, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double u = xp[2 * t], v = xp[2 * t + 1];
  if (u != u || v != v) return;   // NaN: not tracked in this frame
  xivo_feat_in& f = feats[(long)(t / F) * Fmax + (t % F)];
  f.xp[0] = u; f.xp[1] = v;
}
// One workgroup per filter that has ops; its ops run in array order.
__global__ __launch_bounds__(256) void edit_batch_kernel(EditArgs a) {
  const int w = blockIdx.x, tid = threadIdx.x;
  const int filt = a.wg_filter[w];
  double* P = a.P + (long)filt * a.strideP;
  xivo_feat_in* feats = a.feats + (long)filt * a.Fmax;
  xivo_group_in* groups = a.groups + (long)filt * a.lay.n_groups;
  const xivo_pose_in& X = a.poses[filt];
  for (int o = a.wg_begin[w]; o < a.wg_begin[w + 1]; ++o) {
    const xivo_edit_op& op = a.ops[o];
    switch (op.kind) {
      case XIVO_EDIT_P_ZERO_RC: edit_zero_rc(P, a.ldp, a.Np, op.i0, op.i1, tid); break;
      case XIVO_EDIT_P_COPY_RC: edit_copy_rc(P, a.ldp, a.Np, op.i0, op.i1, op.i2, tid); break;
      case XIVO_EDIT_P_SET_BLOCK3: edit_set_block3(P, a.ldp, op.i0, tid < 9 ? op.v[tid] : 0.0, tid); break;
      case XIVO_EDIT_ADD_GROUP: edit_add_group(P, a.ldp, a.Np, a.lay, groups, X.Rsb, X.Tsb, op.i0, tid); break;
      case XIVO_EDIT_REMOVE_GROUP:
        edit_remove_group(P, a.ldp, a.Np, a.lay, groups, a.anchors + (long)filt * a.anchor_max, a.anchor_max, op.i0, tid);
        break;
      case XIVO_EDIT_ADD_FEATURE:
        edit_add_feature(P, a.ldp, a.Np, a.lay, feats[op.i0], op.v, op.v + 3, op.i1, op.i2, tid < 9 ? op.v[5 + tid] : 0.0, tid);
        break;
      case XIVO_EDIT_REMOVE_FEATURE: edit_remove_feature(P, a.ldp, a.Np, a.lay, feats, op.i0, tid); break;
      case XIVO_EDIT_SET_XP:
        if (tid < 2) feats[op.i0].xp[tid] = op.v[tid];
        __syncthreads();
        break;
      case XIVO_EDIT_ADD_GROUP_ANCHOR:
        edit_add_group_anchor(P, a.ldp, a.Np, a.lay, groups, a.anchors[(long)filt * a.anchor_max + op.i1], op.i0, tid);
        break;
      case XIVO_EDIT_ADMIT_POOL:   // (the host checked that the entry's anchor is linked)
        edit_admit_pool(P, a.ldp, a.Np, a.lay, feats, a.pool[(long)filt * a.pool_max + op.i2], a.anchors + (long)filt * a.anchor_max,
                        op.i0, op.i1, tid);
        break;
      default: break;
    }
  }
}

// ---------------------------------------------------------------- AbsorbError
__device__ __forceinline__ void rot_retract(double* Rcm, double wx, double wy, double wz) {   // R <- R exp(w), column-major storage
  const M3 R = m3_mul(m3_from_colmajor(Rcm), so3_exp_dev(wx, wy, wz));
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rcm[i + 3 * j] = R.m[i][j];
}
// The periodic re-normalisation of State::operator+= (src/core.h:154-162, every kEnforceSO3Freq = 50 absorbs):
// Sophus SO3::normalize() on Rsb / Rbc (unit quaternion; here: matrix -> quaternion -> normalise -> matrix, which
// also re-orthonormalises the stored matrix) and Rsg <- exp(log(Rsg) with its z component zeroed).
__device__ __forceinline__ void quat_to_colmajor(const double q[4], double* Rcm) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  Rcm[0] = 1.0 - 2.0 * (y * y + z * z); Rcm[3] = 2.0 * (x * y - w * z);       Rcm[6] = 2.0 * (x * z + w * y);
  Rcm[1] = 2.0 * (x * y + w * z);       Rcm[4] = 1.0 - 2.0 * (x * x + z * z); Rcm[7] = 2.0 * (y * z - w * x);
  Rcm[2] = 2.0 * (x * z - w * y);       Rcm[5] = 2.0 * (y * z + w * x);       Rcm[8] = 1.0 - 2.0 * (x * x + y * y);
}
__device__ __forceinline__ void rot_normalize(double* Rcm) {
  double q[4];
  rot_to_quat(m3_from_colmajor(Rcm), q);
  quat_to_colmajor(q, Rcm);
}
__device__ __forceinline__ void rot_zero_log_z(double* Rcm) {   // Sophus SO3::log on the unit quaternion, z <- 0, exp
  const V3 w = so3_log_dev(m3_from_colmajor(Rcm));
  const M3 R = so3_exp_dev(w.v[0], w.v[1], 0.0);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rcm[i + 3 * j] = R.m[i][j];
}

// One workgroup per filter; thread 0 retracts the motion state, threads 1.. the group slots and features.
__global__ __launch_bounds__(256) void absorb_error_kernel(AbsorbArgs a) {
  const int filt = blockIdx.x, tid = threadIdx.x;
  double* err = a.err + (long)filt * a.strideErr;
  if (a.status && a.status[filt]) {                      // S was not positive definite: K / dx of that filter are meaningless
    for (int n = tid; n < a.lay.N; n += 256) err[n] = 0.0;
    return;
  }
  if (tid == 0) {                                        // State::operator+= (core.h:135-165)
    xivo_pose_in& X = a.poses[filt];
    rot_retract(X.Rsb, err[0], err[1], err[2]);
    rot_retract(X.Rbc, err[15], err[16], err[17]);
    rot_retract(X.Rsg, err[21], err[22], 0.0);
    for (int i = 0; i < 3; ++i) {
      X.Tsb[i] += err[3 + i]; X.Vsb[i] += err[6 + i]; X.bg[i] += err[9 + i]; X.ba[i] += err[12 + i]; X.Tbc[i] += err[18 + i];
    }
    if (a.calib) {                                       // online-calibration builds
      xivo_calib_in& cb = a.calib[filt];
      if (a.cl.td >= 0) cb.td += err[a.cl.td];           // core.h:150-152
      if (a.cl.Cg >= 0) {                                // estimator.cpp:879-884 -> IMUState::operator+= (imu.cpp:7-21): Ca's upper
        int k = a.cl.Cg + 9;                             // triangle row by row, then Cg row by row (both stored column-major)
        for (int i = 0; i < 3; ++i)
          for (int j = i; j < 3; ++j) cb.Ca[i + 3 * j] += err[k++];
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) cb.Cg[i + 3 * j] += err[a.cl.Cg + 3 * i + j];
      }
      for (int k = 0; k < a.cl.cam_dim && k < 9; ++k) cb.intr[k] += err[a.cl.cam_begin + k];   // estimator.cpp:886-890
    }
    if (a.counter && ++a.counter[filt] % 50 == 0) {      // kEnforceSO3Freq (core.h:111,154-162)
      rot_normalize(X.Rsb);
      rot_normalize(X.Rbc);
      rot_zero_log_z(X.Rsg);
    }
  }
  const unsigned long long gmask = a.group_mask ? a.group_mask[filt] : ~0ull;   // instate_groups_ (estimator.cpp:897)
  for (int g = tid; g < a.lay.n_groups; g += 256) {      // SO3xR3::operator+= (group.h:25-29); empty slots have dx = 0
    if (g < 64 && !((gmask >> g) & 1ull)) continue;
    xivo_group_in& G = a.groups[(long)filt * a.lay.n_groups + g];
    const int off = a.lay.group_begin + 6 * g;
    rot_retract(G.Rsb, err[off], err[off + 1], err[off + 2]);
    for (int i = 0; i < 3; ++i) G.Tsb[i] += err[off + 3 + i];
  }
  for (int f = tid; f < (a.mask ? a.F : 0); f += 256) {  // Feature::UpdateState for in_current_ekf_update_ (estimator.cpp:906-912)
    if (!a.mask[(long)filt * a.Fmax + f]) continue;
    xivo_feat_in& ft = a.feats[(long)filt * a.Fmax + f];
    if (ft.sind < 0) continue;
    const int off = a.lay.feature_begin + 3 * ft.sind;
    for (int i = 0; i < 3; ++i) ft.x[i] += err[off + i];
  }
  __syncthreads();
  for (int n = tid; n < a.lay.N; n += 256) err[n] = 0.0;  // err_.setZero() (estimator.cpp:920)
}

// ---------------------------------------------------------------- fp64 MFMA issue-rate probe
// Every wave issues `iters` x 8 independent v_mfma_f64_16x16x4_f64; wave 0 of
// block 0 also reports the shader-clock cycles it spent (s_memtime), so the
// host can separate "cycles per MFMA" from "sustained clock".
__global__ __launch_bounds__(256) void mfma_peak_kernel(double* sink, int iters) {
  d4 acc[8];
  const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  const long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    // accumulators pinned to VGPRs: left to itself the compiler parks the accumulators of a small kernel like this one in
    // AGPRs, and v_mfma_f64_16x16x4_f64 with an AGPR destination issues at 50 TFLOP/s instead of 77 on this part
    // (scripts/mfma_agpr_probe.hip) - rounds 1 and 2 took that for the instruction's ceiling. The update kernels keep
    // their accumulators in VGPRs (checked in the ISA), so 77 TFLOP/s = 98 % of the datasheet is the ceiling that applies.
    for (int i = 0; i < 8; ++i) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  const long long t1 = clock64();
  if (blockIdx.x == 0 && threadIdx.x == 0) sink[1] = (double)(t1 - t0);
  if (s == 12345.678) sink[0] = s;
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_unpack_P(const double* raw, double* P, int N, int Np, int ldp, long strideP, int batch,
                    hipStream_t s) {
  dim3 grid((unsigned)p_unpack_pairs(Np), batch);
  hipLaunchKernelGGL(unpack_P_kernel, grid, dim3(256), 0, s, raw, P, N, Np, ldp, strideP);
  CHECK_LAUNCH();
}
int launch_pack_P(const double* P, double* raw, int N, int ldp, long strideP, int batch, hipStream_t s) {
  dim3 grid((unsigned)(((long)N * N + 255) / 256), batch);
  hipLaunchKernelGGL(pack_P_kernel, grid, dim3(256), 0, s, P, raw, N, ldp, strideP);
  CHECK_LAUNCH();
}
int launch_unpack_meas(const double* rawH, long strideRaw, int ldraw, const int* only_if, MeasBuffers mb, int M,
                       int Mp, int N, int Np, int batch, hipStream_t s) {
  dim3 grid((unsigned)(((long)Mp * Np + 255) / 256), batch);
  hipLaunchKernelGGL(unpack_meas_kernel, grid, dim3(256), 0, s, rawH, strideRaw, ldraw, only_if, mb, M, Mp, N, Np);
  CHECK_LAUNCH();
}
// H^T [Np x Mp, ldht] from the dense H [Mp x Np, ldh] of every filter: the transposed copy is optional for the G-level
// producers (staged_rows.h: ht_alive) and rebuilt here when a consumer turns up after all. 32 x 32 tiles through LDS so that
// both sides move 256-byte runs.
__global__ __launch_bounds__(256) void transpose_H_kernel(const double* __restrict__ Hall, long strideH, int ldh,
                                                         double* __restrict__ HTall, long strideHT, int ldht, int Mp, int Np) {
  __shared__ double t[32][33];
  const double* H = Hall + (long)blockIdx.z * strideH;
  double* HT = HTall + (long)blockIdx.z * strideHT;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8)
    t[j][tx] = (m0 + tx < Mp && n0 + j < Np) ? H[(m0 + tx) + (long)(n0 + j) * ldh] : 0.0;
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (n0 + tx < Np && m0 + j < Mp) HT[(n0 + tx) + (long)(m0 + j) * ldht] = t[tx][j];
}
int launch_transpose_H(const double* H, long strideH, int ldh, double* HT, long strideHT, int ldht, int Mp, int Np, int batch,
                       hipStream_t s) {
  if (batch <= 0) return 0;
  hipLaunchKernelGGL(transpose_H_kernel, dim3((Mp + 31) / 32, (Np + 31) / 32, batch), dim3(256), 0, s, H, strideH, ldh, HT, strideHT, ldht, Mp, Np);
  CHECK_LAUNCH();
}
int launch_p_zero_rc(double* P, int ldp, int Np, int off, int len, hipStream_t s) {
  hipLaunchKernelGGL(p_zero_rc_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, P, ldp, Np, off, len);
  CHECK_LAUNCH();
}
int launch_p_copy_rc(double* P, int ldp, int Np, int dst, int src, int len, hipStream_t s) {
  hipLaunchKernelGGL(p_copy_rc_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, P, ldp, Np, dst, src, len, 0);
  hipLaunchKernelGGL(p_copy_rc_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, P, ldp, Np, dst, src, len, 1);
  CHECK_LAUNCH();
}
int launch_p_diag(const double* P, int ldp, int N, double* out, hipStream_t s) {
  hipLaunchKernelGGL(p_diag_kernel, dim3((N + 255) / 256), dim3(256), 0, s, P, ldp, N, out);
  CHECK_LAUNCH();
}
int launch_set_pixels(xivo_feat_in* feats, int Fmax, int F, const double* xp, int nb, hipStream_t s) {
  const int n = nb * F;
  hipLaunchKernelGGL(set_pixels_kernel, dim3((n + 255) / 256), dim3(256), 0, s, feats, Fmax, F, xp, n);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_edit_batch(const EditArgs& a, int n_wg, hipStream_t s) {
  hipLaunchKernelGGL(edit_batch_kernel, dim3(n_wg), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_absorb_error(const AbsorbArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(absorb_error_kernel, dim3(a.batch), dim3(256), 0, s, a);
  CHECK_LAUNCH();
}
int launch_mfma_peak(double* sink, int iters, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, s, sink, iters);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
