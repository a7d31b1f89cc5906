// Device helpers of the per-feature 3x3 chains, shared by glevel_kernels.hip, pool_kernels.hip, state_kernels.hip and
// propagate_kernels.hip: 3x3 / 2x3 products, SO3::hat, pixel projection, the per-filter camera of the online-calibration
// builds and Feature::Xc / Feature::z; SO3 exp / log (state_kernels.hip: AbsorbError, traj_kernels.hip: the pose error).
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

}  // namespace xivo_hip
