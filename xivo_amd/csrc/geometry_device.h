// Device helpers of the per-feature 3x3 chains, shared by glevel_kernels.hip, pool_kernels.hip, state_kernels.hip and
// propagate_kernels.hip: 3x3 / 2x3 products, SO3::hat, pixel projection, the per-filter camera of the online-calibration
// builds and Feature::Xc / Feature::z; SO3 exp / log (state_kernels.hip: AbsorbError, traj_kernels.hip: the pose error); the
// loop-closure world point and row pair (glevel_kernels.hip, lcmap_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "camera_device.h"
#include "../../include/xivo_hip.h"

namespace xivo_hip {

// ---------------------------------------------------------------- 3x3 helpers (row-major m[i][j])
struct M3 { double m[3][3]; };
struct V3 { double v[3]; };

__device__ __forceinline__ M3 m3_from_colmajor(const double* p) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = p[i + 3 * j];
  return r;
}
__device__ __forceinline__ M3 m3_t(const M3& a) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[j][i];
  return r;
}
__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return r;
}
__device__ __forceinline__ M3 m3_neg(const M3& a) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = -a.m[i][j];
  return r;
}
__device__ __forceinline__ M3 m3_add(const M3& a, const M3& b) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][j] + b.m[i][j];
  return r;
}
__device__ __forceinline__ V3 m3_mulv(const M3& a, const V3& x) {
  V3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i) r.v[i] = a.m[i][0] * x.v[0] + a.m[i][1] * x.v[1] + a.m[i][2] * x.v[2];
  return r;
}
// SO3::hat (sophus/so3.hpp): [0 -z y; z 0 -x; -y x 0]
__device__ __forceinline__ M3 hat(const V3& w) {
  M3 r;
  r.m[0][0] = 0; r.m[0][1] = -w.v[2]; r.m[0][2] = w.v[1];
  r.m[1][0] = w.v[2]; r.m[1][1] = 0; r.m[1][2] = -w.v[0];
  r.m[2][0] = -w.v[1]; r.m[2][1] = w.v[0]; r.m[2][2] = 0;
  return r;
}
// ---------------------------------------------------------------- SO3 exp / log
// SO3::exp (Rodrigues), as SO3_from_rotvec (src/helpers.cpp:374-378)
__device__ __forceinline__ M3 so3_exp_dev(double wx, double wy, double wz) {
  const double th = sqrt(wx * wx + wy * wy + wz * wz);
  const V3 w{{wx, wy, wz}};
  const M3 W = hat(w), W2 = m3_mul(W, W);
  const double a = th < 1e-10 ? 1.0 : sin(th) / th, b = th < 1e-10 ? 0.5 : (1.0 - cos(th)) / (th * th);
  M3 R;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R.m[i][j] = (i == j ? 1.0 : 0.0) + a * W.m[i][j] + b * W2.m[i][j];
  return R;
}
// rotation matrix -> unit quaternion
__device__ __forceinline__ void rot_to_quat(const M3& R, double q[4]) {   // (w, x, y, z), Shepperd's branch on the largest diagonal term
  const double t = R.m[0][0] + R.m[1][1] + R.m[2][2];
  if (t > 0.0) {
    const double s = sqrt(t + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (R.m[2][1] - R.m[1][2]) / s; q[2] = (R.m[0][2] - R.m[2][0]) / s; q[3] = (R.m[1][0] - R.m[0][1]) / s;
  } else if (R.m[0][0] > R.m[1][1] && R.m[0][0] > R.m[2][2]) {
    const double s = sqrt(1.0 + R.m[0][0] - R.m[1][1] - R.m[2][2]) * 2.0;
    q[0] = (R.m[2][1] - R.m[1][2]) / s; q[1] = 0.25 * s; q[2] = (R.m[0][1] + R.m[1][0]) / s; q[3] = (R.m[0][2] + R.m[2][0]) / s;
  } else if (R.m[1][1] > R.m[2][2]) {
    const double s = sqrt(1.0 + R.m[1][1] - R.m[0][0] - R.m[2][2]) * 2.0;
    q[0] = (R.m[0][2] - R.m[2][0]) / s; q[1] = (R.m[0][1] + R.m[1][0]) / s; q[2] = 0.25 * s; q[3] = (R.m[1][2] + R.m[2][1]) / s;
  } else {
    const double s = sqrt(1.0 + R.m[2][2] - R.m[0][0] - R.m[1][1]) * 2.0;
    q[0] = (R.m[1][0] - R.m[0][1]) / s; q[1] = (R.m[0][2] + R.m[2][0]) / s; q[2] = (R.m[1][2] + R.m[2][1]) / s; q[3] = 0.25 * s;
  }
  const double n = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] *= n; q[1] *= n; q[2] *= n; q[3] *= n;
}
// Sophus SO3::log on the unit quaternion of R: the rotation vector w with exp(w) = R
__device__ __forceinline__ V3 so3_log_dev(const M3& R) {
  double q[4];
  rot_to_quat(R, q);
  const double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3], w = q[0];
  double k;
  if (n2 < 1e-20) k = 2.0 / w - 2.0 / 3.0 * n2 / (w * w * w);
  else {
    const double n = sqrt(n2);
    k = fabs(w) < 1e-10 ? (w > 0.0 ? 3.141592653589793 / n : -3.141592653589793 / n) : 2.0 * atan(n / w) / n;
  }
  return V3{{k * q[1], k * q[2], k * q[3]}};
}

// 2x3 = (2x3) * (3x3)
__device__ __forceinline__ void m23_mul(const double a[2][3], const M3& b, double out[2][3]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[i][j] = a[i][0] * b.m[0][j] + a[i][1] * b.m[1][j] + a[i][2] * b.m[2][j];
}

// project(Xcn) with Jacobian (common/project.h:11-24) then Camera::Project;
// returns dxp_dXcn = dxp_dxcn * dxcn_dXcn (feature.cpp:611-620, oos.cpp:66-70)
__device__ __forceinline__ void project_pixel(const xivo_cam& cam, const V3& Xcn, double xp[2],
                                              double dxp_dXcn[2][3]) {
  const double X = Xcn.v[0], Y = Xcn.v[1], Z = Xcn.v[2];
  const double xcn0 = X / Z, xcn1 = Y / Z;
  const double d[2][3] = {{1 / Z, 0, -X / (Z * Z)}, {0, 1 / Z, -Y / (Z * Z)}};
  double Jc[2][2];
  camera_project(cam, xcn0, xcn1, xp, Jc);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) dxp_dXcn[i][j] = Jc[i][0] * d[0][j] + Jc[i][1] * d[1][j];
}

// Online camera calibration (USE_ONLINE_CAMERA_CALIB): the intrinsics are state, one set per filter, resident in
// xivo_calib_in::intr (fx fy cx cy d[0..4] - the order of the state slots); the context's xivo_cam names the model
__device__ __forceinline__ xivo_cam filter_cam(const xivo_cam& cam, const xivo_calib_in* calib, int cam_dim, int filt) {
  xivo_cam c = cam;
  if (calib && cam_dim > 0) {
    const double* p = calib[filt].intr;
    c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3];
#pragma unroll
    for (int k = 0; k < 5; ++k) c.d[k] = p[4 + k];
  }
  return c;
}

// Feature::Xc (feature.cpp:98-105): Xc and dXc/dx from the feature's local state x = (X/Z, Y/Z, log Z) through
// unproject_logz (project.h:79-95) or, in the USE_INVDEPTH build (XIVO_HIP_FLAG_INVDEPTH), x = (X/Z, Y/Z, 1/Z) through
// unproject_invz = project_invz (project.h:31-56). Feature::z (feature.cpp:120-126) for the depth tests.
__device__ __forceinline__ V3 feature_unproject(const double* x, int invdepth, M3& dXc_dx) {
  V3 Xc;
  if (invdepth) {
    const double r = x[2];
    Xc.v[0] = x[0] / r; Xc.v[1] = x[1] / r; Xc.v[2] = 1.0 / r;
    dXc_dx.m[0][0] = 1 / r; dXc_dx.m[0][1] = 0; dXc_dx.m[0][2] = -x[0] / (r * r);
    dXc_dx.m[1][0] = 0; dXc_dx.m[1][1] = 1 / r; dXc_dx.m[1][2] = -x[1] / (r * r);
    dXc_dx.m[2][0] = 0; dXc_dx.m[2][1] = 0; dXc_dx.m[2][2] = -1 / (r * r);
  } else {
    const double z = exp(x[2]);
    Xc.v[0] = x[0] * z; Xc.v[1] = x[1] * z; Xc.v[2] = z;
    dXc_dx.m[0][0] = z; dXc_dx.m[0][1] = 0; dXc_dx.m[0][2] = x[0] * z;
    dXc_dx.m[1][0] = 0; dXc_dx.m[1][1] = z; dXc_dx.m[1][2] = x[1] * z;
    dXc_dx.m[2][0] = 0; dXc_dx.m[2][1] = 0; dXc_dx.m[2][2] = z;
  }
  return Xc;
}
__device__ __forceinline__ double feature_depth(double x2, int invdepth) { return invdepth ? 1.0 / x2 : exp(x2); }

// ---------------------------------------------------------------- loop closure (Feature::ComputeLCJacobian, oos.cpp:92-145)
// Xs(gbc) = ref_->gsb() * gbc * Xc (feature.cpp:107-118) of in-state feature ft anchored in group gref: what lc_rows_kernel
// re-observes and what the landmark map stores (lcmap_add_kernel) - one evaluation order for both
__device__ __forceinline__ V3 lc_world_point(const xivo_pose_in& pose, const xivo_feat_in& ft, const xivo_group_in& gref, int invdepth) {
  const M3 Rbc = m3_from_colmajor(pose.Rbc), Rsbr = m3_from_colmajor(gref.Rsb);
  M3 dXc_dx;
  const V3 Xc = feature_unproject(ft.x, invdepth, dXc_dx);
  V3 Xbr = m3_mulv(Rbc, Xc);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xbr.v[i] += pose.Tbc[i];
  V3 Xs = m3_mulv(Rsbr, Xbr);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xs.v[i] += gref.Tsb[i];
  return Xs;
}
// The row pair r0, r0 + 1 of a zeroed H for world point Xs re-observed at pixel obs_xp from the pose (gRsb, gTsb) whose six
// error-state columns (W, T) start at goff - a group slot, or the body pose itself at 0: the two share the retraction -:
// d xp / d (W, T, Wbc, Tbc) [+ the intrinsics block of :141-144 when cam_dim > 0], inn = obs_xp - xp, diagR = Rlc. No block for
// the point: as coded. The one place this arithmetic lives (lc_rows_kernel, lcmap_close_kernel).
__device__ __forceinline__ void lc_row_pair(const V3& Xs, const double* gRsb, const double* gTsb, int goff, const xivo_pose_in& pose,
                                            const xivo_cam& cam, int cam_begin, int cam_dim, const double* obs_xp, double Rlc,
                                            double* H, int ldh, int r0, double* inn, double* dR) {
  const M3 Rbc = m3_from_colmajor(pose.Rbc), Rsb = m3_from_colmajor(gRsb);
  const M3 Rsb_t = m3_t(Rsb), Rbc_t = m3_t(Rbc);
  V3 d;
#pragma unroll
  for (int i = 0; i < 3; ++i) d.v[i] = Xs.v[i] - gTsb[i];
  const V3 Xb = m3_mulv(Rsb_t, d);                              // :107
#pragma unroll
  for (int i = 0; i < 3; ++i) d.v[i] = Xb.v[i] - pose.Tbc[i];
  const V3 Xcn = m3_mulv(Rbc_t, d);                             // :113
  double xp[2], dxp_dXcn[2][3];
  project_pixel(cam, Xcn, xp, dxp_dXcn);                        // :123-133
  const M3 dXcn_dTsb = m3_mul(Rbc_t, m3_neg(Rsb_t));            // :120  dXcn_dXb * dXb_dTsb
  const M3 dXcn_dWsb = m3_mul(Rbc_t, hat(Xb));                  // :121  dXcn_dXb * dXb_dWsb
  double blk[2][3];
  auto put = [&](int col) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) H[r0 + i + (long)(col + j) * ldh] = blk[i][j];
  };
  m23_mul(dxp_dXcn, dXcn_dWsb, blk); put(goff);                 // :136
  m23_mul(dxp_dXcn, dXcn_dTsb, blk); put(goff + 3);             // :137
  m23_mul(dxp_dXcn, hat(Xcn), blk); put(15);                    // :138  Index::Wbc
  m23_mul(dxp_dXcn, m3_neg(Rbc_t), blk); put(18);               // :139  Index::Tbc
  if (cam_dim > 0) {                                            // :141-144
    double xq[2], Jq[2][2], jacc[2][9];
    camera_project_jacc(cam, Xcn.v[0] / Xcn.v[2], Xcn.v[1] / Xcn.v[2], xq, Jq, jacc);
#pragma unroll
    for (int j = 0; j < 9; ++j)                                 // (unrolled and predicated: jacc stays in registers)
      if (j < cam_dim) { H[r0 + (long)(cam_begin + j) * ldh] = jacc[0][j]; H[r0 + 1 + (long)(cam_begin + j) * ldh] = jacc[1][j]; }
  }
  inn[r0] = obs_xp[0] - xp[0]; inn[r0 + 1] = obs_xp[1] - xp[1];   // :146
  dR[r0] = Rlc; dR[r0 + 1] = Rlc;                                 // update.cpp:193
}

}  // namespace xivo_hip
