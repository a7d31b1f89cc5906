// What enters the out-of-state feature pool, as device functions that pool_anchor_kernel / pool_add_kernel (pool_kernels.hip)
// and the device pool life cycle (pool_lifecycle_kernels.hip) share, so that a new anchor and a new entry come out bit for bit
// the same whoever decided on them.
#pragma once
#include "camera_device.h"
#include "ekf_kernels.h"

namespace xivo_hip {

// Group::Create(X_.Rsb, X_.Tsb) (src/group.cpp:17-24, src/manager.cpp:121): the anchor takes the pose, unlinked. One thread.
__device__ __forceinline__ void pool_create_anchor(PoolAnchor& A, const xivo_pose_in& pose) {
#pragma unroll
  for (int i = 0; i < 9; ++i) A.g.Rsb[i] = pose.Rsb[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) A.g.Tsb[i] = pose.Tsb[i];
  A.slot = -1;
}

// Feature::Initialize (src/feature.cpp:144-160) of one new track into entry f: x = (UnProject(xp), log z0 or 1 / z0),
// P = diag(std_xyz)^2, anchored at `anchor`. One thread.
__device__ __forceinline__ void pool_init_entry(xivo_subfilter_feat& f, const xivo_cam& cam, const double* xp, double z0,
                                                const double* std_xyz, int anchor, int invdepth) {
  double xc[2];
  camera_unproject(cam, xp[0], xp[1], xc);
  f.x[0] = xc[0]; f.x[1] = xc[1];
  f.x[2] = invdepth ? 1.0 / z0 : log(z0);
#pragma unroll
  for (int i = 0; i < 9; ++i) f.P[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) f.P[4 * i] = std_xyz[i] * std_xyz[i];   // P_ = diag(std); P_ *= P_
  f.xp[0] = xp[0]; f.xp[1] = xp[1];
  f.outlier_counter = 0.0; f.score = 0.0;
  f.ref_sind = anchor; f.status = XIVO_FEAT_INITIALIZING; f.init_counter = 0; f.candidate = 0;
}

}  // namespace xivo_hip
