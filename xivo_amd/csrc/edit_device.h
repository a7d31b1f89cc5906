// Row / column edits of one filter's padded P by its own workgroup of 256 threads: the building blocks of
// Estimator::{Add,Remove}{Group,Feature}{To,From}State (src/estimator.cpp:739-846) that edit_batch_kernel (state_kernels.hip)
// and the device life cycle (lifecycle_kernels.hip) share. Every call ends on a workgroup barrier, so calls may follow each
// other directly; all 256 threads must make the call.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace xivo_hip
