// Row / column edits of one filter's padded P by its own workgroup of 256 threads: the building blocks of
// Estimator::{Add,Remove}{Group,Feature}{To,From}State (src/estimator.cpp:739-846) that edit_batch_kernel (state_kernels.hip)
// and the device life cycles (lifecycle_kernels.hip, pool_lifecycle_kernels.hip) share. Every call ends on a workgroup barrier, so calls may follow each
// other directly; all 256 threads must make the call.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"

namespace xivo_hip {

__device__ __forceinline__ void edit_zero_rc(double* P, int ldp, int Np, int off, int len, int tid) {
  for (int t = tid; t < Np; t += 256)
    for (int r = 0; r < len; ++r) {
      P[(off + r) + (long)t * ldp] = 0.0;
      P[t + (long)(off + r) * ldp] = 0.0;
    }
  __syncthreads();
}
// rows, then columns (which re-read the rows just written): the order of src/estimator.cpp:808-816
__device__ __forceinline__ void edit_copy_rc(double* P, int ldp, int Np, int dst, int src, int len, int tid) {
  for (int t = tid; t < Np; t += 256)
    for (int r = 0; r < len; ++r) P[(dst + r) + (long)t * ldp] = P[(src + r) + (long)t * ldp];
  __syncthreads();
  for (int t = tid; t < Np; t += 256)
    for (int r = 0; r < len; ++r) P[t + (long)(dst + r) * ldp] = P[t + (long)(src + r) * ldp];
  __syncthreads();
}
// XIVO_EDIT_P_SET_BLOCK3: the 3 x 3 block at (off, off); thread t < 9 brings element t (column-major) as v
__device__ __forceinline__ void edit_set_block3(double* P, int ldp, int off, double v, int tid) {
  if (tid < 9) P[(off + tid % 3) + (long)(off + tid / 3) * ldp] = v;
  __syncthreads();
}

// ---- the edits of the scene and the pool that go with them (the cases of edit_batch_kernel of the same names); `anchors` /
// `pool` / `groups` / `feats` are the filter's own rows
// XIVO_EDIT_REMOVE_FEATURE of list position j: Estimator::RemoveFeatureFromState (src/estimator.cpp:762-783); an entry that is
// not in the state is left alone
__device__ __forceinline__ void edit_remove_feature(double* P, int ldp, int Np, const xivo_layout& lay, xivo_feat_in* feats, int j,
                                                    int tid) {
  const int sind = feats[j].sind;
  __syncthreads();
  if (sind >= 0) {
    if (sind < lay.n_features) edit_zero_rc(P, ldp, Np, lay.feature_begin + 3 * sind, 3, tid);
    if (tid == 0) feats[j].sind = -1;
    __syncthreads();
  }
}
// XIVO_EDIT_REMOVE_GROUP: an anchor linked to the slot keeps the group's last pose and becomes unlinked (no pool: anchor_max = 0,
// `anchors` is not read)
__device__ __forceinline__ void edit_remove_group(double* P, int ldp, int Np, const xivo_layout& lay, const xivo_group_in* groups,
                                                  PoolAnchor* anchors, int anchor_max, int g, int tid) {
  for (int t = tid; t < anchor_max; t += 256) {
    PoolAnchor& A = anchors[t];
    if (A.slot == g) { A.g = groups[g]; A.slot = -1; }
  }
  edit_zero_rc(P, ldp, Np, lay.group_begin + 6 * g, 6, tid);
}
// XIVO_EDIT_ADD_GROUP: Estimator::AddGroupToState (src/estimator.cpp:801-816) into slot g with the pose (Rsb, Tsb)
__device__ __forceinline__ void edit_add_group(double* P, int ldp, int Np, const xivo_layout& lay, xivo_group_in* groups,
                                               const double* Rsb, const double* Tsb, int g, int tid) {
  if (tid < 9) groups[g].Rsb[tid] = Rsb[tid];
  else if (tid < 12) groups[g].Tsb[tid - 9] = Tsb[tid - 9];
  const int off = lay.group_begin + 6 * g;
  edit_copy_rc(P, ldp, Np, off, 0, 3, tid);       // Index::Wsb
  edit_copy_rc(P, ldp, Np, off + 3, 3, 3, tid);   // Index::Tsb
}
// XIVO_EDIT_ADD_GROUP_ANCHOR: XIVO_EDIT_ADD_GROUP of anchor A's group into slot g, with the anchor's pose
__device__ __forceinline__ void edit_add_group_anchor(double* P, int ldp, int Np, const xivo_layout& lay, xivo_group_in* groups,
                                                      PoolAnchor& A, int g, int tid) {
  edit_add_group(P, ldp, Np, lay, groups, A.g.Rsb, A.g.Tsb, g, tid);
  if (tid == 0) A.slot = g;
  __syncthreads();
}
// XIVO_EDIT_ADD_FEATURE: AddFeatureToState (src/estimator.cpp:820-846) + FillCovarianceBlock (src/feature.cpp:753-760). List
// entry f takes (x, xp), feature slot sind and reference group ref - x, xp and ref are thread 0's, the others' are not read -;
// thread t < 9 brings element t of the slot's block of P as pv
__device__ __forceinline__ void edit_add_feature(double* P, int ldp, int Np, const xivo_layout& lay, xivo_feat_in& f, const double* x,
                                                 const double* xp, int sind, int ref, double pv, int tid) {
  if (tid == 0) {
    f.x[0] = x[0]; f.x[1] = x[1]; f.x[2] = x[2];
    f.xp[0] = xp[0]; f.xp[1] = xp[1];
    f.sind = sind; f.ref_sind = ref;
  }
  const int off = lay.feature_begin + 3 * sind;
  edit_zero_rc(P, ldp, Np, off, 3, tid);
  edit_set_block3(P, ldp, off, pv, tid);
}
// XIVO_EDIT_ADMIT_POOL: XIVO_EDIT_ADD_FEATURE with (x, xp, P) taken from pool entry e, whose anchor is linked and which becomes
// free; list position j, feature slot sind
__device__ __forceinline__ void edit_admit_pool(double* P, int ldp, int Np, const xivo_layout& lay, xivo_feat_in* feats,
                                                xivo_subfilter_feat& e, const PoolAnchor* anchors, int j, int sind, int tid) {
  const double pv = tid < 9 ? e.P[tid] : 0.0;
  int slot = -1;
  if (tid == 0) { slot = anchors[e.ref_sind].slot; e.ref_sind = -1; }   // (nobody else reads the entry's anchor)
  edit_add_feature(P, ldp, Np, lay, feats[j], e.x, e.xp, sind, slot, pv, tid);
}

}  // namespace xivo_hip
