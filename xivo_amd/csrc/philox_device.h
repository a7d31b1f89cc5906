// The counter-based noise generator the device simulators share (pcw_device.h: pixel noise; trajsim_device.h: IMU noise), as
// plain functions. Host and device; no project header is included.
//
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), multipliers 0xD2511F53 /
//   0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped before every round but the first
//   the four output words w0 .. w3 give two uniforms in (0, 1) of 52 bits each:
//     u1 = (((uint64)w0 << 20 | w1 >> 12) + 0.5) 2^-52        u2 = (((uint64)w2 << 20 | w3 >> 12) + 0.5) 2^-52
//   (w0 / w2 are the high 32 bits, the top 20 bits of w1 / w3 the low ones; u >= 2^-53, so |normal| <= sqrt(106 ln 2) < 8.6)
//   one Box-Muller pair, contraction off: r = sqrt(-2 ln u1), a = 6.283185307179586 u2, (n0, n1) = (r cos a, r sin a)
// What goes into the key and the counter is the caller's rule. Two callers that use the same key and counters draw the same
// words: streams that must be independent need different keys (seeds).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_PHILOX_HD __host__ __device__ __forceinline__
#else
#define XIVO_PHILOX_HD inline
#endif

namespace xivo_hip {

XIVO_PHILOX_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// 52 bits -> (0, 1): every value and the + 0.5 are exact in a double
XIVO_PHILOX_HD double philox_uniform(uint32_t hi, uint32_t lo) {
  return ((double)(((uint64_t)hi << 20) | (uint64_t)(lo >> 12)) + 0.5) * 2.220446049250313e-16;   // 2^-52
}
// the pair of unit normals of four words
XIVO_PHILOX_HD void philox_box_muller(const uint32_t w[4], double* n0, double* n1) {
#pragma clang fp contract(off)
  const double u1 = philox_uniform(w[0], w[1]), u2 = philox_uniform(w[2], w[3]);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
  *n0 = r * cos(a); *n1 = r * sin(a);
}

}  // namespace xivo_hip
