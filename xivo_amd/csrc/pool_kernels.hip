// Depth sub-filter and the out-of-state feature pool of the EKF (gfx950), driven by capi_glevel.hip (xivo_hip_subfilter,
// xivo_hip_pool_*).
//
//  subfilter_kernel     Feature::SubfilterUpdate + Criteria::Candidate(Strict) + Feature::score
//                                                          src/feature.cpp:246-297,133-142, src/options.cpp:10-33
//  pool_anchor_kernel   Group::Create(X_.Rsb, X_.Tsb)      src/group.cpp:17-24, src/manager.cpp:121
//  pool_add_kernel      Feature::Initialize                src/feature.cpp:144-160
//  pool_tri_kernel      Feature::Triangulate at an entry's first step (triangulate_pre_subfilter), before pool_step_kernel
//                                                          src/manager.cpp:227-231, src/feature.cpp:686-751
//  pool_step_kernel     the out-of-state branch of ProcessTracks + the candidate order
//                                                          src/manager.cpp:171-250
//  triangulate_kernel   the triangulators of src/helpers.cpp:103-371 on host-array problems (xivo_hip_triangulate)
//  adapt_depth_kernel   Estimator::AdaptInitialDepth       src/manager.cpp:255-278
// (paths relative to the reference tree). One thread per feature; one workgroup per filter for the pool step.
#include "ekf_kernels.h"
#include "camera_device.h"
#include "geometry_device.h"
#include "pool_device.h"
#include "triangulate_device.h"

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
  pool_create_anchor(anchors[(long)b * anchor_max + slot[b]], poses[b]);
}
// Feature::Initialize (feature.cpp:144-160): one thread per new track; init_z (non-null: XIVO_POOL_ADD_ADAPTIVE_Z): z0 is the
// filter's resident init_z (AdaptInitialDepth's init_z_)
__global__ void pool_add_kernel(xivo_subfilter_feat* pool, int pool_max, const xivo_pool_new* recs, int n, xivo_cam cam_ctx,
                                const xivo_calib_in* calib, int cam_dim, int invdepth, const double* init_z) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const xivo_pool_new& r = recs[t];
  const xivo_cam cam = filter_cam(cam_ctx, calib, cam_dim, r.b);
  pool_init_entry(pool[(long)r.b * pool_max + r.entry], cam, r.xp, init_z ? init_z[r.b] : r.z0, r.std_xyz, r.anchor, invdepth);
}
// The out-of-state branch of ProcessTracks (manager.cpp:171-250) and the candidate order, one workgroup per filter: its threads
// take the entries (one thread per entry for pool_max <= 256), then sort the keys (rank, P(2,2), entry) in LDS by a bitonic
// network over the next power of two >= pool_max. rank 2 = passing and READY, 1 = passing and INITIALIZING, 0 = not passing
// (sorted last); best first = higher rank, then smaller P(2,2) (larger Feature::score), then the lower entry - the order
// std::stable_sort gives xivo_hip_candidate_order.
__device__ __forceinline__ bool pool_before(int ra, double pa, int ia, int rb, double pb, int ib) {
  return ra > rb || (ra == rb && (pa < pb || (pa == pb && ia < ib)));
}
// g12 = (anchor gsb * gbc)^-1 (gsb * gbc) of Feature::Triangulate (feature.cpp:692): R12 = Ra^T Rc, t12 = Ra^T (Tc - Ta) with
// Rc = Rsb Rbc, Tc = Rsb Tbc + Tsb and the same for the anchor. No contraction and every sum left to right, so a caller can
// restate these values bit for bit in plain fp64 (xivo_hip_triangulate then reproduces the pool's triangulation exactly).
__device__ __forceinline__ void pool_g12(const xivo_pose_in& pose, const xivo_group_in& anc, double R12[9], double t12[3]) {
#pragma clang fp contract(off)
  const double* Rsb = pose.Rsb; const double* Rbc = pose.Rbc; const double* Ra0 = anc.Rsb;   // column-major
  double Rc[9], Ra[9], Tc[3], Ta[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      Rc[i + 3 * j] = (Rsb[i] * Rbc[3 * j] + Rsb[i + 3] * Rbc[1 + 3 * j]) + Rsb[i + 6] * Rbc[2 + 3 * j];
      Ra[i + 3 * j] = (Ra0[i] * Rbc[3 * j] + Ra0[i + 3] * Rbc[1 + 3 * j]) + Ra0[i + 6] * Rbc[2 + 3 * j];
    }
    Tc[i] = ((Rsb[i] * pose.Tbc[0] + Rsb[i + 3] * pose.Tbc[1]) + Rsb[i + 6] * pose.Tbc[2]) + pose.Tsb[i];
    Ta[i] = ((Ra0[i] * pose.Tbc[0] + Ra0[i + 3] * pose.Tbc[1]) + Ra0[i + 6] * pose.Tbc[2]) + anc.Tsb[i];
  }
  const double d[3] = {Tc[0] - Ta[0], Tc[1] - Ta[1], Tc[2] - Ta[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      R12[i + 3 * j] = (Ra[3 * i] * Rc[3 * j] + Ra[1 + 3 * i] * Rc[1 + 3 * j]) + Ra[2 + 3 * i] * Rc[2 + 3 * j];
    t12[i] = (Ra[3 * i] * d[0] + Ra[1 + 3 * i] * d[1]) + Ra[2 + 3 * i] * d[2];
  }
}
// triangulate_pre_subfilter (manager.cpp:227-231) for the entries of one pool step, launched just before pool_step_kernel
// when the option is on: one thread per entry; a live entry with a pixel this frame and init_counter == 0 (f->size() == 2:
// x[0:2] is still UnProject(front()), only the sub-filter step writes x after pool_add_kernel and it increments
// init_counter) is triangulated from its anchor pose and the frame's pose. pool_step_kernel then stores the pixel and takes
// the sub-filter step from the x written here - the order of ProcessTracks.
__global__ void pool_tri_kernel(PoolStepArgs a) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)a.batch * a.pool_max) return;
  const int filt = (int)(t / a.pool_max);
  xivo_subfilter_feat& f = a.pool[t];
  if (f.ref_sind < 0 || f.init_counter != 0) return;
  const double u = a.xp[2 * t], v = a.xp[2 * t + 1];
  if (u != u || v != v) return;                             // dropped this frame: pool_step_kernel frees it
  const xivo_cam cam = filter_cam(a.cam, a.calib, a.cam_dim, filt);
  const PoolAnchor& A = a.anchors[(long)filt * a.anchor_max + f.ref_sind];
  const xivo_group_in& G = A.slot >= 0 ? a.groups[(long)filt * a.n_groups + A.slot] : A.g;
  double R12[9], t12[3], xc2[2], X[3];
  pool_g12(a.poses[filt], G, R12, t12);
  camera_unproject(cam, u, v, xc2);
  const double xc1[2] = {f.x[0], f.x[1]};
  const bool ret = tri::triangulate_one(R12, t12, xc1, xc2, a.tri.method, (float)a.tri.max_theta_thresh,
                                        (float)a.tri.beta_thresh, X);
  if (!tri::triangulation_good(ret, X, a.tri)) {
    atomicAdd(&a.tri_bad[filt], 1);
    return;
  }
  const double z = X[2];
  f.x[0] = X[0] / z; f.x[1] = X[1] / z;
  f.x[2] = a.invdepth ? 1.0 / z : log(z);
  atomicAdd(&a.tri_good[filt], 1);
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

// xivo_hip_triangulate: one thread per problem
__global__ void triangulate_kernel(const xivo_tri_in* in, xivo_tri_out* out, int n, xivo_triangulate_opts o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const xivo_tri_in& p = in[t];
  double X[3];
  const bool ret = tri::triangulate_one(p.R12, p.t12, p.xc1, p.xc2, o.method, (float)o.max_theta_thresh, (float)o.beta_thresh, X);
  xivo_tri_out& r = out[t];
  r.X[0] = X[0]; r.X[1] = X[1]; r.X[2] = X[2];
  r.ret = ret ? 1 : 0;
  r.good = tri::triangulation_good(ret, X, o) ? 1 : 0;
}

// AdaptInitialDepth (manager.cpp:255-278), one workgroup per filter: the depths of the in-state features [0, F) of the
// resident list and of the live READY pool entries with init_counter > min_lifetime go to LDS; the value of rank n / 2 is the
// one with exactly n / 2 smaller values before it in (value, index) order - one thread per candidate counts them.
__global__ __launch_bounds__(256) void adapt_depth_kernel(AdaptDepthArgs a) {
  extern __shared__ double dep[];
  __shared__ int n_dep;
  __shared__ double med;
  __shared__ int found;
  const int filt = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) { n_dep = 0; found = 0; }
  __syncthreads();
  // (a non-finite depth is left out: the rank count below needs a strict total order)
  for (int j = tid; j < a.F; j += nt) {
    const xivo_feat_in& f = a.feats[(long)filt * a.Fmax + j];
    const double z = feature_depth(f.x[2], a.invdepth);
    if (f.sind >= 0 && isfinite(z)) dep[atomicAdd(&n_dep, 1)] = z;
  }
  for (int e = tid; e < a.pool_max; e += nt) {
    const xivo_subfilter_feat& f = a.pool[(long)filt * a.pool_max + e];
    const double z = feature_depth(f.x[2], a.invdepth);
    if (f.ref_sind >= 0 && f.status == XIVO_FEAT_READY && f.init_counter > a.min_lifetime && isfinite(z))
      dep[atomicAdd(&n_dep, 1)] = z;
  }
  __syncthreads();
  const int n = n_dep, k = n >> 1;
  for (int i = tid; i < n; i += nt) {
    const double di = dep[i];
    int below = 0;
    for (int j = 0; j < n; ++j) {
      const double dj = dep[j];
      below += (dj < di || (dj == di && j < i)) ? 1 : 0;
    }
    if (below == k) { med = di; found = 1; }   // exactly one i has rank k
  }
  __syncthreads();
  if (tid == 0) {
    double z = a.init_z[filt];
    if (found && med >= a.min_z && med <= a.max_z) {   // !(m < min_z || m > max_z)
      z = (1.0 - a.beta) * z + a.beta * med;
      a.init_z[filt] = z;
    }
    if (a.init_z_out) a.init_z_out[filt] = z;
  }
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
                    const xivo_calib_in* calib, int cam_dim, int invdepth, hipStream_t s, const double* init_z) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(pool_add_kernel, dim3((n + 127) / 128), dim3(128), 0, s, pool, pool_max, recs, n, cam, calib, cam_dim,
                     invdepth, init_z);
  CHECK_LAUNCH();
}
int launch_triangulate(const xivo_tri_in* in, xivo_tri_out* out, int n, const xivo_triangulate_opts& o, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(triangulate_kernel, dim3((n + 127) / 128), dim3(128), 0, s, in, out, n, o);
  CHECK_LAUNCH();
}
// LDS bytes of adapt_depth_kernel's depth list: one double per resident feature and pool entry
size_t adapt_depth_lds(int F, int pool_max) { return (size_t)(F + pool_max) * sizeof(double); }
int launch_adapt_depth(const AdaptDepthArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  const size_t lds = adapt_depth_lds(a.F, a.pool_max);
  if (lds > 60 * 1024) return 1;
  hipLaunchKernelGGL(adapt_depth_kernel, dim3(a.batch), dim3(256), lds, s, a);
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
  if (a.tri.method != XIVO_TRI_OFF) {
    const long ne = (long)a.batch * a.pool_max;
    hipLaunchKernelGGL(pool_tri_kernel, dim3((unsigned)((ne + 127) / 128)), dim3(128), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(pool_step_kernel, dim3(a.batch), dim3(pool_step_threads(a.pool_max)), 0, s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
