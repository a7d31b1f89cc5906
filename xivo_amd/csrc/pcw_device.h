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
//
// Track faults (xivo_hip_pcw_fault_config; opt-in) - part of the interface as the noise is: pcw.fault_draw and
// BatchPCW.generate(faults=...) restate exactly this. Random track loss, gross outliers (one frame, or sticky: a bias the track
// keeps until it ends) and heavy-tailed noise, from two more draws of the same generator under the pixel noise's key:
//   draw A: counter = (point | 0x80000000, filter, frame & 0xffffffff, frame >> 32)
//   draw B: counter = (point | 0x40000000, filter, frame & 0xffffffff, frame >> 32)
// The pixel noise has word 0 = point < 2048 (XIVO_LIFE_MAX_TRACKS bounds a world) and the trajectory producer word 0 in
// {0, 1, 2}: draw A, draw B and those two never share a counter, so under any key the streams are disjoint (the pixel noise
// and the IMU noise still need different seeds, as before). "filter" is b, or b % stream_mod after
// xivo_hip_pcw_stream_share(stream_mod) - in the pixel noise's counter too: filters w, w + W, w + 2 W, ... then draw the same
// words. The trajectory producer's stream is not touched by it.
//   draw A  e = uniform(w0, w1) selects the event against t1 = p_drop, t2 = t1 + p_outlier, t3 = t2 + p_tail, summed on the
//           host in this order and handed over as they are (all <= 1):
//             e < t1: drop ; t1 <= e < t2: outlier ; t2 <= e < t3: tail ; otherwise nominal
//           bit 0 of w2 is the sign of the outlier offset's u component, bit 1 that of v (set: negative)
//   draw B  (read on an outlier event only) m_u = uniform(w0, w1), m_v = uniform(w2, w3);
//           off_u = +-(outlier_min_px + (outlier_max_px - outlier_min_px) m_u), off_v likewise with m_v, contraction off.
//           No trigonometry and no logarithm: host and device agree to the last bit.
// Per point and frame, in this order:
//   1. vis: the geometric visibility above
//   2. if vis, draw A
//   3. vis_eff = vis && !drop. Ids, ranks, the count, next_id and the keys follow vis_eff where they followed vis: a dropped
//      point loses its id and returns as a new track, exactly as a point that left the image
//   4. the offset. sticky = 0: off on an outlier event, else 0. sticky = 1: a resident bias [2] per point holds it - an outlier
//      event overwrites it, it is added on every later frame of the same track, and it is zeroed when vis_eff is false
//   5. pixel = pcw_noisy(u + offset_u, noise_px_std * (tail ? tail_scale : 1), noise_u): the sum u + offset first, the product
//      std * scale formed once; v likewise
//   6. the track's flag byte: bit 0 an outlier event this frame, bit 1 a tail event, bit 2 a non-zero bias carried over from an
//      earlier frame and added unchanged (an outlier event that overwrites a carried bias sets bit 0 alone)
// The score (pcw_fault_cell): a track is faulty when flag & 5; with the update's inlier mask entry of the feature that follows
// the track, rejected = !mask, the four cells are outlier_rejected, outlier_kept, nominal_rejected, nominal_kept.
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

// ---- track faults (the rules: the header's opening comment)
// t1 <= t2 <= t3 <= 1: the event thresholds as the host summed them; sticky in {0, 1}
struct PcwFault { double t1, t2, t3, outlier_min_px, outlier_max_px, tail_scale; int sticky; };
enum PcwEvent { PCW_EV_NOMINAL = 0, PCW_EV_DROP = 1, PCW_EV_OUTLIER = 2, PCW_EV_TAIL = 3 };
enum PcwFlag { PCW_FLAG_OUTLIER = 1, PCW_FLAG_TAIL = 2, PCW_FLAG_BIASED = 4, PCW_FLAG_FAULTY = PCW_FLAG_OUTLIER | PCW_FLAG_BIASED };
constexpr uint32_t kPcwDrawA = 0x80000000u, kPcwDrawB = 0x40000000u;
// the filter word of the pixel-noise and fault counters (stream_mod 0: every filter its own stream)
XIVO_PCW_HD int pcw_stream_filter(int b, int stream_mod) { return stream_mod > 0 ? b % stream_mod : b; }
// the words of draw A / draw B (draw = kPcwDrawA / kPcwDrawB) of one point; b: the filter word
XIVO_PCW_HD void pcw_fault_words(unsigned long long seed, unsigned long long frame, int b, int p, uint32_t draw, uint32_t w[4]) {
  const uint32_t ctr[4] = {(uint32_t)p | draw, (uint32_t)b, (uint32_t)(frame & 0xffffffffull), (uint32_t)(frame >> 32)};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, w);
}
XIVO_PCW_HD int pcw_fault_event(const PcwFault& f, double e) {
  return e < f.t1 ? PCW_EV_DROP : (e < f.t2 ? PCW_EV_OUTLIER : (e < f.t3 ? PCW_EV_TAIL : PCW_EV_NOMINAL));
}
// the outlier offset of draw A's sign bits (wa) and draw B's two uniforms (wb)
XIVO_PCW_HD void pcw_fault_offset(const PcwFault& f, const uint32_t wa[4], const uint32_t wb[4], double off[2]) {
#pragma clang fp contract(off)
  const double m_u = philox_uniform(wb[0], wb[1]), m_v = philox_uniform(wb[2], wb[3]);
  const double span = f.outlier_max_px - f.outlier_min_px;
  const double a_u = f.outlier_min_px + span * m_u, a_v = f.outlier_min_px + span * m_v;
  off[0] = (wa[2] & 1u) ? -a_u : a_u;
  off[1] = (wa[2] & 2u) ? -a_v : a_v;
}
// Steps 2 - 4 and 6 of one point in one frame. vis: the geometric visibility; b: the filter word; bias [2]: the point's resident
// bias, read and written when f.sticky (else not touched; may be null). -> vis_eff; *event the draw's event (nominal when not
// visible); for a track (vis_eff) off [2] the offset to add, *scale the factor of noise_px_std and *flag its flag byte
XIVO_PCW_HD bool pcw_fault_point(const PcwFault& f, unsigned long long seed, unsigned long long frame, int b, int p, bool vis,
                                 double* bias, double off[2], double* scale, unsigned char* flag, int* event) {
  uint32_t wa[4] = {0u, 0u, 0u, 0u};
  int ev = PCW_EV_NOMINAL;
  if (vis && f.t3 > 0.0) {   // (t3 = 0: every event is nominal whatever the draw says)
    pcw_fault_words(seed, frame, b, p, kPcwDrawA, wa);
    ev = pcw_fault_event(f, philox_uniform(wa[0], wa[1]));
  }
  *event = ev;
  off[0] = 0.0; off[1] = 0.0; *scale = 1.0; *flag = 0;
  const bool vis_eff = vis && ev != PCW_EV_DROP;
  if (!vis_eff) {
    if (f.sticky) { bias[0] = 0.0; bias[1] = 0.0; }
    return false;
  }
  unsigned char fl = 0;
  if (ev == PCW_EV_OUTLIER) {
    uint32_t wb[4];
    pcw_fault_words(seed, frame, b, p, kPcwDrawB, wb);
    pcw_fault_offset(f, wa, wb, off);
    fl |= PCW_FLAG_OUTLIER;
    if (f.sticky) { bias[0] = off[0]; bias[1] = off[1]; }
  } else if (f.sticky) {
    off[0] = bias[0]; off[1] = bias[1];
    if (off[0] != 0.0 || off[1] != 0.0) fl |= PCW_FLAG_BIASED;
  }
  if (ev == PCW_EV_TAIL) { fl |= PCW_FLAG_TAIL; *scale = f.tail_scale; }
  *flag = fl;
  return true;
}
// step 5: the pixel a faulty track reports; std_eff = noise_px_std * scale, formed once by the caller (pcw_fault_std)
XIVO_PCW_HD double pcw_fault_std(double noise_px_std, double scale) {
#pragma clang fp contract(off)
  return noise_px_std * scale;
}
XIVO_PCW_HD double pcw_fault_pixel(double u, double offset, double std_eff, double n) {
#pragma clang fp contract(off)
  const double s = u + offset;
  return pcw_noisy(s, std_eff, n);
}

// ---- the score of the gate's decisions against the labels
enum PcwCell { PCW_CELL_OUTLIER_REJECTED = 0, PCW_CELL_OUTLIER_KEPT = 1, PCW_CELL_NOMINAL_REJECTED = 2, PCW_CELL_NOMINAL_KEPT = 3 };
// mask: the update's inlier mask entry of the feature (0: rejected); flag: the flag byte of the track it followed
XIVO_PCW_HD int pcw_fault_cell(unsigned char mask, unsigned char flag) {
  const bool faulty = (flag & PCW_FLAG_FAULTY) != 0, rejected = mask == 0;
  return faulty ? (rejected ? PCW_CELL_OUTLIER_REJECTED : PCW_CELL_OUTLIER_KEPT)
                : (rejected ? PCW_CELL_NOMINAL_REJECTED : PCW_CELL_NOMINAL_KEPT);
}

}  // namespace xivo_hip
