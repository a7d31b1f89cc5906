// The point-cloud world's track producer as plain functions over ONE point of ONE world: projection through the frame's
// ground-truth camera pose, the visibility test, the pixel noise and who gets which track id. Host and device: the kernel of
// pcw_kernels.hip calls these functions, and a host compiler takes the header alone (tests/pcw_driver.cpp runs whole frames
// through them without a GPU). No project header is included but philox_device.h, the generator, and camera_device.h, the
// estimator's camera models, which are as self-contained (camera_device.h includes the public header only).
//
// Every rule restates BatchPCW.generate / RandomPCW.generate_measurements (xivo_amd/pcw.py), which follow the reference's
// scripts/point_cloud_world.py:44-131: a point in front of the camera whose pixel lies inside the image (borders included) is
// visible; a visible point without a track id takes the next one, in ascending point order; a point that is not visible loses
// its id, so a point that comes back is a new track.
//
// Arithmetic, in this evaluation order and with contraction off (no product is fused with a sum):
//   d    = Xs - Tsc
//   Xc_i = (R[0][i] d0 + R[1][i] d1) + R[2][i] d2         R = Rsc row-major: Xc = Rsc^T d
//   front = Xc_2 > 0 ; z = front ? Xc_2 : 1
//   u = fx Xc_0 / z + cx ; v = fy Xc_1 / z + cy           (fx Xc_0) / z: the product first
//   vis = front && u >= 0 && v >= 0 && u <= imw && v <= imh
// Through one of the estimator's camera models (xivo_hip_pcw_camera; c: the xivo_cam, the image is c.cols x c.rows), d, Xc,
// front and z as above, then
//   x = Xc_0 / z ; y = Xc_1 / z ; radius = hypot(x, y)
//   XIVO_CAM_PINHOLE: u = fx Xc_0 / z + cx ; v = fy Xc_1 / z + cy      the statements above, bit for bit
//   otherwise:        (u, v) = camera_project(c, x, y)                  camera_device.h, where each model is stated once
//   vis = front && radius <= max_radius && u >= 0 && v >= 0 && u <= cols && v <= rows
// max_radius guards against the fold-back of a polynomial distortion far off axis (+inf: no guard). camera_project's own
// statements are compiled as the rest of the tree compiles them (the device build may fuse a product with a sum there).
//
// Noise - part of the interface: a host arm that wants the device's stream (pcw.philox_normal) restates exactly this. The
// generator is counter based, so the noise of a point depends on (seed, frame, filter, point) alone, not on the launch shape
// and not on who is visible:
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), multipliers 0xD2511F53 /
//   0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped before every round but the first
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (point, filter, frame & 0xffffffff, frame >> 32)
//   the four output words w0 .. w3 give two uniforms in (0, 1) of 52 bits each:
//     u1 = (((uint64)w0 << 20 | w1 >> 12) + 0.5) 2^-52        u2 = (((uint64)w2 << 20 | w3 >> 12) + 0.5) 2^-52
//   (w0 / w2 are the high 32 bits, the top 20 bits of w1 / w3 the low ones; u >= 2^-53, so |normal| <= sqrt(106 ln 2) < 8.6)
//   one Box-Muller pair: r = sqrt(-2 ln u1), a = 6.283185307179586 u2, (noise_u, noise_v) = (r cos a, r sin a)
//   the track's pixel is (u + noise_px_std noise_u, v + noise_px_std noise_v).
#pragma once

#include <math.h>
#include <stdint.h>

#include "philox_device.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_PCW_HD __host__ __device__ __forceinline__
#else
#define XIVO_PCW_HD inline
#endif

#include "camera_device.h"

namespace xivo_hip {

struct PcwCam { double fx, fy, cx, cy, imw, imh; };

// ---- projection and visibility
// X [3]: the world point; g [12]: Rsc row-major, then Tsc. uvz = (u, v, Xc_2) without noise; returns vis
XIVO_PCW_HD bool pcw_project(const double* X, const double* g, const PcwCam& k, double* uvz) {
#pragma clang fp contract(off)
  const double d0 = X[0] - g[9], d1 = X[1] - g[10], d2 = X[2] - g[11];
  const double xc0 = (g[0] * d0 + g[3] * d1) + g[6] * d2;
  const double xc1 = (g[1] * d0 + g[4] * d1) + g[7] * d2;
  const double xc2 = (g[2] * d0 + g[5] * d1) + g[8] * d2;
  const bool front = xc2 > 0.0;
  const double z = front ? xc2 : 1.0;
  const double u = k.fx * xc0 / z + k.cx;
  const double v = k.fy * xc1 / z + k.cy;
  uvz[0] = u; uvz[1] = v; uvz[2] = xc2;
  return front && u >= 0.0 && v >= 0.0 && u <= k.imw && v <= k.imh;
}

// the same through camera model c.model; a point whose normalised radius exceeds max_radius is not visible
XIVO_PCW_HD bool pcw_project(const double* X, const double* g, const xivo_cam& c, double max_radius, double* uvz) {
#pragma clang fp contract(off)
  const double d0 = X[0] - g[9], d1 = X[1] - g[10], d2 = X[2] - g[11];
  const double xc0 = (g[0] * d0 + g[3] * d1) + g[6] * d2;
  const double xc1 = (g[1] * d0 + g[4] * d1) + g[7] * d2;
  const double xc2 = (g[2] * d0 + g[5] * d1) + g[8] * d2;
  const bool front = xc2 > 0.0;
  const double z = front ? xc2 : 1.0;
  const double x = xc0 / z, y = xc1 / z;
  const double radius = hypot(x, y);
  double xp[2];
  if (c.model == XIVO_CAM_PINHOLE) {
    xp[0] = c.fx * xc0 / z + c.cx;
    xp[1] = c.fy * xc1 / z + c.cy;
  } else {
    double J[2][2];   // (not read: the compiler drops what only it needs)
    camera_project(c, x, y, xp, J);
  }
  uvz[0] = xp[0]; uvz[1] = xp[1]; uvz[2] = xc2;
  return front && radius <= max_radius && xp[0] >= 0.0 && xp[1] >= 0.0 && xp[0] <= (double)c.cols && xp[1] <= (double)c.rows;
}

// ---- track ids
// a visible point that holds no id yet starts a track
XIVO_PCW_HD bool pcw_is_new(bool vis, long long id) { return vis && id < 0; }
// the id the point holds after the frame; rank_new: the new points of its world before it, in point order
XIVO_PCW_HD long long pcw_id_after(bool vis, long long id, long long next_id, int rank_new) {
  return !vis ? -1 : (id < 0 ? next_id + rank_new : id);
}

// ---- noise (the generator itself: philox_device.h, shared with the trajectory producer)
XIVO_PCW_HD void pcw_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) { philox4x32_10(ctr, key, out); }
// the generator's words of one point
XIVO_PCW_HD void pcw_noise_words(unsigned long long seed, unsigned long long frame, int b, int p, uint32_t w[4]) {
  const uint32_t ctr[4] = {(uint32_t)p, (uint32_t)b, (uint32_t)(frame & 0xffffffffull), (uint32_t)(frame >> 32)};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, w);
}
// 52 bits -> (0, 1): every value and the + 0.5 are exact in a double
XIVO_PCW_HD double pcw_uniform(uint32_t hi, uint32_t lo) { return philox_uniform(hi, lo); }
// a pair of unit normals for point p of filter b in that frame
XIVO_PCW_HD void pcw_normal_pair(unsigned long long seed, unsigned long long frame, int b, int p, double* nu, double* nv) {
  uint32_t w[4];
  pcw_noise_words(seed, frame, b, p, w);
  philox_box_muller(w, nu, nv);
}
// the pixel a track reports
XIVO_PCW_HD double pcw_noisy(double u, double noise_px_std, double n) {
#pragma clang fp contract(off)
  return u + noise_px_std * n;
}

}  // namespace xivo_hip
