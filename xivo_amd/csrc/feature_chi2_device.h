// The compact 2 x 21 Jacobian of an in-state feature on the device: where its columns sit in the error state (jcol: stack_kernel,
// glevel_kernels.hip, and the gate) and the feature's distance from them by one wave (feature_chi2_lds: gate_sparse_kernel,
// gate_kernels.hip, and the rescue of OnePointRANSAC, ransac_rescue_kernel, glevel_kernels.hip).
#pragma once
#include "gate_device.h"

namespace xivo_hip {

// column of the error state that compact-J column c (0..20) maps to (stack_kernel walks the same map)
__device__ __forceinline__ int jcol(const xivo_layout& lay, const xivo_feat_in& ft, int c) {
  const int b = c / 3, o = c % 3;
  switch (b) {
    case 0: return 0 + o;    // Index::Wsb  (core.h:41)
    case 1: return 3 + o;    // Index::Tsb
    case 2: return 15 + o;   // Index::Wbc
    case 3: return 18 + o;   // Index::Tbc
    case 4: return lay.group_begin + 6 * ft.ref_sind + o;
    case 5: return lay.group_begin + 6 * ft.ref_sind + 3 + o;
    default: return lay.feature_begin + 3 * ft.sind + o;
  }
}

// res^T (J P J^T + R I2)^-1 res of one feature by one wave64 (src/update.cpp:60-70, :352-356; gate_sparse_kernel and the
// rescue of OnePointRANSAC, ransac_rescue_kernel): the 21 x 21 sub-block of
// P the full row J touches, lane (a, c) forming (P J^T)(a, c) in ascending b, reduced across lanes, 2x2 LLT. The value is
// valid in every lane. The gathers of P are issued as seven wave-wide loads: the wave parks the sub-block (element
// e = a + 21 b in lane e mod 64) and the two rows of J in its own LDS scratch and reads its operands from there. (The first
// version had every lane (a, c) gather its 21 elements itself - 42 gather instructions per feature, half of them duplicates
// between the c = 0 and c = 1 lanes - and the gate kernel was bound by the number of 8-byte gathers a CU's address unit
// retires, not by memory latency: 0.40 -> 0.28 ms per 4096 filters x 60 features, same bits.) scratch: 441 + 42 doubles.
__device__ __forceinline__ double feature_chi2_lds(const double* P, int ldp, const xivo_layout& lay, const xivo_feat_in& ft,
                                                   const double* J, const double* inn, double R, int lane, double* scratch) {
  double* sP = scratch;          // [a + 21 b]
  double* sJ = scratch + 441;    // [c * 21 + b]
  double pv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int e = lane + 64 * k;
    const int ea = e < 441 ? e % 21 : 0, eb = e < 441 ? e / 21 : 0;
    pv[k] = P[jcol(lay, ft, ea) + (long)jcol(lay, ft, eb) * ldp];
  }
  const double jmine = lane < 42 ? J[lane] : 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int e = lane + 64 * k;
    if (e < 441) sP[e] = pv[k];
  }
  if (lane < 42) sJ[lane] = jmine;
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are done (one wave, no barrier needed)
  __builtin_amdgcn_wave_barrier();
  double v = 0.0;
  const int ra = lane % 21, rc = lane / 21;
  if (lane < 42) {
#pragma unroll
    for (int b = 0; b < 21; ++b) v = fma(sP[ra + 21 * b], sJ[rc * 21 + b], v);
  }
  const double j0 = lane < 42 ? sJ[ra] : 0.0, j1 = lane < 42 ? sJ[21 + ra] : 0.0;
  __builtin_amdgcn_wave_barrier();      // (the next feature's writes stay behind these reads: program order within the wave)
  const double s00 = (lane < 21) ? j0 * v : 0.0;
  const double s10 = (lane < 21) ? j1 * v : 0.0;
  const double s11 = (lane >= 21 && lane < 42) ? j1 * v : 0.0;
  return gate_dist(wave_sum(s00), wave_sum(s10), wave_sum(s11), R, inn[0], inn[1]);
}

}  // namespace xivo_hip
