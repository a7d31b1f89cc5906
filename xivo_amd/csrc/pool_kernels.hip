// Depth sub-filter and the out-of-state feature pool of the EKF (gfx950), driven by capi_glevel.hip (xivo_hip_subfilter,
// xivo_hip_pool_*).
//
//  subfilter_kernel     Feature::SubfilterUpdate + Criteria::Candidate(Strict) + Feature::score
//                                                          src/feature.cpp:246-297,133-142, src/options.cpp:10-33
//  pool_anchor_kernel   Group::Create(X_.Rsb, X_.Tsb)      src/group.cpp:17-24, src/manager.cpp:121
//  pool_add_kernel      Feature::Initialize                src/feature.cpp:144-160
//  pool_step_kernel     the out-of-state branch of ProcessTracks + the candidate order
//                                                          src/manager.cpp:171-250
// (paths relative to the reference tree). One thread per feature; one workgroup per filter for the pool step.
#include "ekf_kernels.h"
#include "camera_device.h"
#include "geometry_device.h"

namespace xivo_hip {

namespace {

// ---------------------------------------------------------------- depth sub-filter
// Feature::SubfilterUpdate of one feature against the sensor pose and its anchor's pose, then Criteria::Candidate(Strict) and
// Feature::score. Every product below is 3x3 / 2x3 / 2x2 and is written in the reference's association order
// (feature.cpp:246-297). Shared by subfilter_kernel and pool_step_kernel, which must agree bit for bit.
__device__ __forceinline__ void subfilter_step(xivo_subfilter_feat& f, const xivo_pose_in& pose, const xivo_group_in& grp,
                                               const xivo_cam& cam, const xivo_subfilter_opts& o, int invdepth) {
  const M3 Rsb = m3_from_colmajor(pose.Rsb), Rbc = m3_from_colmajor(pose.Rbc), Rsbr = m3_from_colmajor(grp.Rsb);
  const V3 Tsb{{pose.Tsb[0], pose.Tsb[1], pose.Tsb[2]}}, Tbc{{pose.Tbc[0], pose.Tbc[1], pose.Tbc[2]}};
  const V3 Tsbr{{grp.Tsb[0], grp.Tsb[1], grp.Tsb[2]}};
  const int init_counter = f.init_counter + 1;                                   // :256
  // Xc(&dXc_dx) (:258; feature.cpp:98-105)
  M3 dXc_dx;
  const V3 Xc = feature_unproject(f.x, invdepth, dXc_dx);
  // gtot = (gsb * gbc)^-1 * ref.gsb * gbc   (:260)
  const M3 Rsc = m3_mul(Rsb, Rbc), Rrc = m3_mul(Rsbr, Rbc);
  V3 Tsc = m3_mulv(Rsb, Tbc), Trc = m3_mulv(Rsbr, Tbc);
  V3 dT;
#pragma unroll
  for (int i = 0; i < 3; ++i) { Tsc.v[i] += Tsb.v[i]; Trc.v[i] += Tsbr.v[i]; dT.v[i] = Trc.v[i] - Tsc.v[i]; }
  const M3 Rsc_t = m3_t(Rsc);
  const M3 Rtot = m3_mul(Rsc_t, Rrc);
  const V3 Ttot = m3_mulv(Rsc_t, dT);
  V3 Xcn = m3_mulv(Rtot, Xc);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xcn.v[i] += Ttot.v[i];                              // :261
  double xp[2], dxp_dXcn[2][3];
  project_pixel(cam, Xcn, xp, dxp_dXcn);                                          // :263-267 (dxp_dxcn * dxcn_dXcn)
  double tmp[2][3], H[2][3];
  m23_mul(dxp_dXcn, Rtot, tmp);
  m23_mul(tmp, dXc_dx, H);                                                        // :269
  const double inn0 = f.xp[0] - xp[0], inn1 = f.xp[1] - xp[1];
  M3 P = m3_from_colmajor(f.P);
  // S = H P H^T + Rtri I  (:272-275)
  double HPm[2][3];
  m23_mul(H, P, HPm);
  double S[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) S[i][j] = HPm[i][0] * H[j][0] + HPm[i][1] * H[j][1] + HPm[i][2] * H[j][2];
  S[0][0] += o.Rtri; S[1][1] += o.Rtri;
  // ratio = inn . S^-1 inn / MH_thresh  (:277; 2x2 LDL^T without the pivot search, same value to rounding)
  double outlier = f.outlier_counter;
  {
    const double l10 = S[1][0] / S[0][0], d1 = S[1][1] - l10 * S[0][1];
    const double y1 = inn1 - l10 * inn0;
    const double s1 = y1 / d1, s0 = (inn0 - S[0][1] * s1) / S[0][0];
    const double ratio = (inn0 * s0 + inn1 * s1) / o.MH_thresh;
    if (ratio > 1) {                                                              // :279-285
      S[0][0] += o.Rtri * (ratio - 1); S[1][1] += o.Rtri * (ratio - 1);
      outlier += sqrt(ratio);
    } else {
      outlier = 0.0;
    }
  }
  // K = P H^T S^-1 (:287; Eigen's 2x2 inverse = adjugate / determinant)
  const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0], idet = 1.0 / det;
  const double Si[2][2] = {{S[1][1] * idet, -S[0][1] * idet}, {-S[1][0] * idet, S[0][0] * idet}};
  double PHt[3][2], K[3][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) PHt[i][j] = P.m[i][0] * H[j][0] + P.m[i][1] * H[j][1] + P.m[i][2] * H[j][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) K[i][j] = PHt[i][0] * Si[0][j] + PHt[i][1] * Si[1][j];
  double xn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) xn[i] = f.x[i] + (K[i][0] * inn0 + K[i][1] * inn1);   // :289
  M3 A;                                                                           // I - K H (:290)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A.m[i][j] = (i == j ? 1.0 : 0.0) - (K[i][0] * H[0][j] + K[i][1] * H[1][j]);
  const M3 AP = m3_mul(A, P);
  M3 Pn;                                                                          // :291
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Pn.m[i][j] = (AP.m[i][0] * A.m[j][0] + AP.m[i][1] * A.m[j][1] + AP.m[i][2] * A.m[j][2]) +
                   ((K[i][0] * o.Rtri) * K[j][0] + (K[i][1] * o.Rtri) * K[j][1]);
  const int status = init_counter > o.ready_steps ? XIVO_FEAT_READY : XIVO_FEAT_INITIALIZING;   // :293-297
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f.x[i] = xn[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) f.P[i + 3 * j] = Pn.m[i][j];
  }
  f.outlier_counter = outlier; f.init_counter = init_counter; f.status = status;
  // Criteria::Candidate / CandidateStrict (options.cpp:10-33), Feature::score (feature.cpp:133-142)
  const double zed = feature_depth(xn[2], invdepth);                              // Feature::z (feature.cpp:120-126)
  const bool ok = outlier < o.max_subfilter_outlier && zed > o.min_depth && zed < o.max_depth;
  f.candidate = (ok ? 1 : 0) | ((ok && status == XIVO_FEAT_READY) ? 2 : 0);
  f.score = -Pn.m[2][2];
}
// One thread per (filter, feature)
__global__ void subfilter_kernel(xivo_subfilter_feat* feats, int n, const xivo_pose_in* poses,
                                 const xivo_group_in* groups, int n_groups, xivo_cam cam_ctx, xivo_subfilter_opts o,
                                 int batch, const xivo_calib_in* calib, int cam_dim, int invdepth) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch * n) return;
  const int filt = t / n;
  const xivo_cam cam = filter_cam(cam_ctx, calib, cam_dim, filt);
  xivo_subfilter_feat& f = feats[t];
  subfilter_step(f, poses[filt], groups[(long)filt * n_groups + f.ref_sind], cam, o, invdepth);
}

// ---------------------------------------------------------------- out-of-state feature pool (xivo_hip_pool_*)
// Group::Create(X_.Rsb, X_.Tsb): one thread per filter
__global__ void pool_anchor_kernel(PoolAnchor* anchors, int anchor_max, const xivo_pose_in* poses, const int* slot, int nb) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb || slot[b] < 0) return;
  PoolAnchor& A = anchors[(long)b * anchor_max + slot[b]];
#pragma unroll
  for (int i = 0; i < 9; ++i) A.g.Rsb[i] = poses[b].Rsb[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) A.g.Tsb[i] = poses[b].Tsb[i];
  A.slot = -1;
}
// Feature::Initialize (feature.cpp:144-160): one thread per new track
__global__ void pool_add_kernel(xivo_subfilter_feat* pool, int pool_max, const xivo_pool_new* recs, int n, xivo_cam cam_ctx,
                                const xivo_calib_in* calib, int cam_dim, int invdepth) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const xivo_pool_new& r = recs[t];
  const xivo_cam cam = filter_cam(cam_ctx, calib, cam_dim, r.b);
  xivo_subfilter_feat& f = pool[(long)r.b * pool_max + r.entry];
  double xc[2];
  camera_unproject(cam, r.xp[0], r.xp[1], xc);
  f.x[0] = xc[0]; f.x[1] = xc[1];
  f.x[2] = invdepth ? 1.0 / r.z0 : log(r.z0);
#pragma unroll
  for (int i = 0; i < 9; ++i) f.P[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) f.P[4 * i] = r.std_xyz[i] * r.std_xyz[i];   // P_ = diag(std); P_ *= P_
  f.xp[0] = r.xp[0]; f.xp[1] = r.xp[1];
  f.outlier_counter = 0.0; f.score = 0.0;
  f.ref_sind = r.anchor; f.status = XIVO_FEAT_INITIALIZING; f.init_counter = 0; f.candidate = 0;
}
// The out-of-state branch of ProcessTracks (manager.cpp:171-250) and the candidate order, one workgroup per filter: its threads
// take the entries (one thread per entry for pool_max <= 256), then sort the keys (rank, P(2,2), entry) in LDS by a bitonic
// network over the next power of two >= pool_max. rank 2 = passing and READY, 1 = passing and INITIALIZING, 0 = not passing
// (sorted last); best first = higher rank, then smaller P(2,2) (larger Feature::score), then the lower entry - the order
// std::stable_sort gives xivo_hip_candidate_order.
__device__ __forceinline__ bool pool_before(int ra, double pa, int ia, int rb, double pb, int ib) {
  return ra > rb || (ra == rb && (pa < pb || (pa == pb && ia < ib)));
}
__global__ __launch_bounds__(256) void pool_step_kernel(PoolStepArgs a) {
  __shared__ double key_p[XIVO_POOL_MAX_ENTRIES];
  __shared__ int key_r[XIVO_POOL_MAX_ENTRIES], key_i[XIVO_POOL_MAX_ENTRIES];
  __shared__ int n_pass;
  const int filt = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, pm = a.pool_max;
  int p2 = 1;
  while (p2 < pm) p2 <<= 1;
  if (tid == 0) n_pass = 0;
  __syncthreads();
  const xivo_cam cam = filter_cam(a.cam, a.calib, a.cam_dim, filt);
  const xivo_pose_in& pose = a.poses[filt];
  const int want = a.strict ? 2 : 1;
  for (int e = tid; e < p2; e += nt) {
    int rank = 0;
    double p22 = 0.0;
    if (e < pm) {
      const long ent = (long)filt * pm + e;
      xivo_subfilter_feat& f = a.pool[ent];
      unsigned char live = 0;
      if (f.ref_sind >= 0) {
        const double u = a.xp[2 * ent], v = a.xp[2 * ent + 1];
        if (u != u || v != v) {
          f.ref_sind = -1;                                  // dropped by the tracker while out of state
        } else {
          f.xp[0] = u; f.xp[1] = v;
          const PoolAnchor& A = a.anchors[(long)filt * a.anchor_max + f.ref_sind];
          subfilter_step(f, pose, A.slot >= 0 ? a.groups[(long)filt * a.n_groups + A.slot] : A.g, cam, a.o, a.invdepth);
          if (f.outlier_counter > a.remove_outlier) {
            f.ref_sind = -1;                                // manager.cpp:236-240
          } else {
            live = 1;
            if (f.candidate & want) {
              rank = f.status == XIVO_FEAT_READY ? 2 : 1;
              p22 = f.P[8];
              atomicAdd(&n_pass, 1);
            }
          }
        }
      }
      a.live[ent] = live;
    }
    key_r[e] = rank; key_p[e] = p22; key_i[e] = e;
  }
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (p2 >> 1); t += nt) {
        const int i = 2 * j * (t / j) + (t % j), l = i + j;
        const bool up = (i & k) == 0;   // this half of the bitonic sequence is sorted best first
        if (pool_before(key_r[l], key_p[l], key_i[l], key_r[i], key_p[i], key_i[i]) == up) {
          const int r = key_r[i], ix = key_i[i];
          const double p = key_p[i];
          key_r[i] = key_r[l]; key_p[i] = key_p[l]; key_i[i] = key_i[l];
          key_r[l] = r; key_p[l] = p; key_i[l] = ix;
        }
      }
      __syncthreads();
    }
  const int n = n_pass;
  for (int e = tid; e < pm; e += nt) a.order[(long)filt * pm + e] = e < n ? key_i[e] : -1;
  if (tid == 0) a.n[filt] = n;
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_subfilter(xivo_subfilter_feat* feats, int n, const xivo_pose_in* poses, const xivo_group_in* groups,
                     int n_groups, xivo_cam cam, xivo_subfilter_opts o, int batch, hipStream_t s, const xivo_calib_in* calib,
                     int cam_dim, int invdepth) {
  const int tot = batch * n;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(subfilter_kernel, dim3((tot + 127) / 128), dim3(128), 0, s, feats, n, poses, groups, n_groups, cam,
                     o, batch, calib, cam_dim, invdepth);
  CHECK_LAUNCH();
}
int launch_pool_anchor(PoolAnchor* anchors, int anchor_max, const xivo_pose_in* poses, const int* slot, int nb, hipStream_t s) {
  if (nb <= 0) return 0;
  hipLaunchKernelGGL(pool_anchor_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, anchors, anchor_max, poses, slot, nb);
  CHECK_LAUNCH();
}
int launch_pool_add(xivo_subfilter_feat* pool, int pool_max, const xivo_pool_new* recs, int n, xivo_cam cam,
                    const xivo_calib_in* calib, int cam_dim, int invdepth, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(pool_add_kernel, dim3((n + 127) / 128), dim3(128), 0, s, pool, pool_max, recs, n, cam, calib, cam_dim,
                     invdepth);
  CHECK_LAUNCH();
}
// threads per workgroup: one per entry up to 256, at least one wave
int pool_step_threads(int pool_max) {
  const int t = (pool_max + 63) / 64 * 64;
  return t < 64 ? 64 : (t > 256 ? 256 : t);
}
int launch_pool_step(const PoolStepArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  if (a.pool_max < 1 || a.pool_max > XIVO_POOL_MAX_ENTRIES) return 1;
  hipLaunchKernelGGL(pool_step_kernel, dim3(a.batch), dim3(pool_step_threads(a.pool_max)), 0, s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
