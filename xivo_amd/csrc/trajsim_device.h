// The trajectory simulator as plain functions over ONE IMU sample of ONE filter: the closed-form curve, the orientation profile,
// the IMU model with its noise, the feeder's record of a sample and the ground-truth body and camera pose. Host and device: the
// kernel of trajsim_kernels.hip calls these functions, and a host compiler takes the header alone (tests/trajsim_driver.cpp).
// No project header is included but philox_device.h, the generator.
//
// Every rule restates BatchTrajectorySim (xivo_amd/pcw.py) and ImuFeeder.imu (xivo_amd/sequence.py) for camera stamps that
// coincide with IMU stamps. Arithmetic in this evaluation order, contraction off (no product is fused with a sum); products
// and sums associate left to right where no parentheses are written:
//
// Times     t_k = (double)k imu_dt, k a 64-bit sample index;  dt_k = t_k - t_{k-1}  (the difference of the two products, which
//           is what a feeder that is handed t_k computes - not imu_dt)
// Profile   (shared by all filters) a_i = rot_w_i t;  w_i = rot_amp sin a_i;  wd_i = (rot_amp rot_w_i) cos a_i
//           th = sqrt((w0 w0 + w1 w1) + w2 w2);  W = hat w;  W2 = W W with its zero terms dropped:
//             W2 = [-(w1 w1 + w2 w2), w0 w1, w0 w2;  w0 w1, -(w0 w0 + w2 w2), w1 w2;  w0 w2, w1 w2, -(w0 w0 + w1 w1)]
//           R_ij  = (I_ij + a W_ij) + b W2_ij       th < 1e-9: a = 1, b = 0.5;   else a = sin th / th, b = (1 - cos th) / (th th)
//           Jr_ij = (I_ij - c W_ij) + e_ij          th < 1e-6: c = 0.5, e_ij = W2_ij / 6;
//                                                   else c = (1 - cos th) / (th th), e_ij = ((th - sin th) / (th th th)) W2_ij
// Curve     s = rate t;  c2 = cos(2 s), s2 = sin(2 s), c3 = cos(3 s), s3 = sin(3 s), s7 = sin(7 s)
//           Lissajous p = (4 c3, 0.1 s7, 4 s2)              acc = (-36 c3, -4.9 s7, -16 s2)
//           trefoil   p = ((4 + c3) c2, (4 + c3) s2, s3)    acc = (12 s2 s3 - 9 c2 c3 - 4 c2 (c3 + 4),
//                                                                  -4 s2 (c3 + 4) - 12 c2 s3 - 9 c3 s2,  -9 s3)
//           p0 = p at s = rate 0
// IMU       d_j = (rate rate) acc_j - grav_s_j;  accel_i = (R_0i d_0 + R_1i d_1) + R_2i d_2  [+ noise_accel n_a_i]
//           gyro_i = (Jr_i0 wd_0 + Jr_i1 wd_1) + Jr_i2 wd_2  [+ noise_gyro n_g_i]
// Noise     part of the interface (pcw.trajsim_normals restates it). The generator and the words-to-normals rule are
//           philox_device.h's; key = (seed & 0xffffffff, seed >> 32), counter = (pair j, filter b, k & 0xffffffff, k >> 32);
//           pair 0 = (n_a_0, n_a_1), pair 1 = (n_a_2, n_g_0), pair 2 = (n_g_1, n_g_2). A sample's noise depends on (seed, k, b)
//           only. A component whose standard deviation is 0 adds nothing, and a pair neither of whose components is used is
//           not drawn. The pixel noise of pcw_device.h uses the same generator with counter = (point, filter, frame): given the
//           same seed, the IMU stream of (j, b, k) IS the pixel stream of point j, filter b, frame k. Use different seeds.
// Record    of sample k >= 1 (ImuFeeder.imu): gyro, accel = the measurement at k - 1; slope = (m_k - m_{k-1}) / dt_k; dt = dt_k
// Truth     at t_k: Rsb = R, Tsb_i = p_i - p0_i; camera (sequence.camera_poses): Rsc_ij = (R_i0 Rbc_0j + R_i1 Rbc_1j) + R_i2 Rbc_2j,
//           Tsc_i = ((R_i0 Tbc_0 + R_i1 Tbc_1) + R_i2 Tbc_2) + Tsb_i; gsc [12] = Rsc row-major, then Tsc; the body pose gt [12] =
//           Rsb column-major, then Tsb (what xivo_hip_traj_score takes)
#pragma once

#include <math.h>
#include <stdint.h>

#include "philox_device.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_TRAJSIM_HD __host__ __device__ __forceinline__
#else
#define XIVO_TRAJSIM_HD inline
#endif

namespace xivo_hip {

// what all filters share (xivo_trajsim_opts without the sizes)
struct TrajsimModel {
  double imu_dt, rot_amp, rot_w[3], noise_accel, noise_gyro, grav_s[3], Rbc[9], Tbc[3];   // Rbc row-major
  unsigned long long seed;
};
// the feeder's record; the layout of xivo_imu_in (include/xivo_hip.h), which this header does not include
struct TrajsimRecord { double gyro[3], accel[3], slope_gyro[3], slope_accel[3], dt; };

XIVO_TRAJSIM_HD double trajsim_time(unsigned long long k, double imu_dt) {
#pragma clang fp contract(off)
  return (double)k * imu_dt;
}
// k >= 1
XIVO_TRAJSIM_HD double trajsim_dt(unsigned long long k, double imu_dt) {
#pragma clang fp contract(off)
  return trajsim_time(k, imu_dt) - trajsim_time(k - 1, imu_dt);
}

// R [9] and Jr [9] row-major, wd [3]
XIVO_TRAJSIM_HD void trajsim_profile(const TrajsimModel& m, double t, double* R, double* Jr, double* wd) {
#pragma clang fp contract(off)
  double w[3];
  for (int i = 0; i < 3; ++i) {
    const double a = m.rot_w[i] * t;
    w[i] = m.rot_amp * sin(a);
    wd[i] = m.rot_amp * m.rot_w[i] * cos(a);
  }
  const double xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2], xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
  const double th = sqrt(xx + yy + zz);
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  const double W2[9] = {-(yy + zz), xy, xz, xy, -(xx + zz), yz, xz, yz, -(xx + yy)};
  double a = 1.0, b = 0.5;
  if (!(th < 1e-9)) { a = sin(th) / th; b = (1.0 - cos(th)) / (th * th); }
  const bool small = th < 1e-6;
  const double c = small ? 0.5 : (1.0 - cos(th)) / (th * th);
  const double e = small ? 0.0 : (th - sin(th)) / (th * th * th);
  for (int i = 0; i < 9; ++i) {
    const double eye = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    R[i] = eye + a * W[i] + b * W2[i];
    Jr[i] = eye - c * W[i] + (small ? W2[i] / 6.0 : e * W2[i]);
  }
}

// position and second derivative with respect to s of curve `motion` (0 Lissajous, 1 trefoil)
XIVO_TRAJSIM_HD void trajsim_curve(int motion, double s, double* p, double* acc) {
#pragma clang fp contract(off)
  const double c3 = cos(3 * s), s2 = sin(2 * s);
  if (motion == 0) {
    const double s7 = sin(7 * s);
    p[0] = 4 * c3; p[1] = 0.1 * s7; p[2] = 4 * s2;
    acc[0] = -36 * c3; acc[1] = -4.9 * s7; acc[2] = -16 * s2;
  } else {
    const double c2 = cos(2 * s), s3 = sin(3 * s);
    p[0] = (4 + c3) * c2; p[1] = (4 + c3) * s2; p[2] = s3;
    acc[0] = 12 * s2 * s3 - 9 * c2 * c3 - 4 * c2 * (c3 + 4);
    acc[1] = -4 * s2 * (c3 + 4) - 12 * c2 * s3 - 9 * c3 * s2;
    acc[2] = -9 * s3;
  }
}

// the generator's words of pair j of sample k of filter b
XIVO_TRAJSIM_HD void trajsim_noise_words(unsigned long long seed, unsigned long long k, int b, int j, uint32_t w[4]) {
  const uint32_t ctr[4] = {(uint32_t)j, (uint32_t)b, (uint32_t)(k & 0xffffffffull), (uint32_t)(k >> 32)};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, w);
}
// the six unit normals (n_a [3], n_g [3]) of sample k of filter b; a pair that is not wanted is not drawn and reads 0
XIVO_TRAJSIM_HD void trajsim_normals(unsigned long long seed, unsigned long long k, int b, bool want_a, bool want_g, double* n6) {
  const bool want[3] = {want_a, want_a || want_g, want_g};
  for (int j = 0; j < 3; ++j) {
    n6[2 * j] = 0.0; n6[2 * j + 1] = 0.0;
    if (want[j]) {
      uint32_t w[4];
      trajsim_noise_words(seed, k, b, j, w);
      philox_box_muller(w, &n6[2 * j], &n6[2 * j + 1]);
    }
  }
}

// what the IMU of filter b (curve `motion`, rate `rate`) reports at sample k
XIVO_TRAJSIM_HD void trajsim_meas(const TrajsimModel& m, int motion, double rate, int b, unsigned long long k, double* accel,
                                  double* gyro) {
#pragma clang fp contract(off)
  const double t = trajsim_time(k, m.imu_dt);
  double R[9], Jr[9], wd[3], p[3], acc[3], d[3];
  trajsim_profile(m, t, R, Jr, wd);
  trajsim_curve(motion, rate * t, p, acc);
  const double r2 = rate * rate;
  for (int j = 0; j < 3; ++j) d[j] = r2 * acc[j] - m.grav_s[j];
  for (int i = 0; i < 3; ++i) {
    accel[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
    gyro[i] = Jr[3 * i] * wd[0] + Jr[3 * i + 1] * wd[1] + Jr[3 * i + 2] * wd[2];
  }
  const bool want_a = m.noise_accel != 0.0, want_g = m.noise_gyro != 0.0;
  if (want_a || want_g) {
    double n6[6];
    trajsim_normals(m.seed, k, b, want_a, want_g, n6);
    for (int i = 0; i < 3; ++i) {
      if (want_a) accel[i] = accel[i] + m.noise_accel * n6[i];
      if (want_g) gyro[i] = gyro[i] + m.noise_gyro * n6[3 + i];
    }
  }
}

// the feeder's record of sample k >= 1
XIVO_TRAJSIM_HD void trajsim_record(const TrajsimModel& m, int motion, double rate, int b, unsigned long long k, TrajsimRecord* r) {
#pragma clang fp contract(off)
  double a0[3], g0[3], a1[3], g1[3];
  trajsim_meas(m, motion, rate, b, k - 1, a0, g0);
  trajsim_meas(m, motion, rate, b, k, a1, g1);
  const double dt = trajsim_dt(k, m.imu_dt);
  for (int i = 0; i < 3; ++i) {
    r->gyro[i] = g0[i]; r->accel[i] = a0[i];
    r->slope_gyro[i] = (g1[i] - g0[i]) / dt;
    r->slope_accel[i] = (a1[i] - a0[i]) / dt;
  }
  r->dt = dt;
}

// ground truth at t_k: gt [12] the body pose (Rsb column-major, Tsb), gsc [12] the camera pose (Rsc row-major, Tsc)
XIVO_TRAJSIM_HD void trajsim_truth(const TrajsimModel& m, int motion, double rate, unsigned long long k, double* gt, double* gsc) {
#pragma clang fp contract(off)
  const double t = trajsim_time(k, m.imu_dt);
  double R[9], Jr[9], wd[3], p[3], p0[3], acc[3], T[3];
  trajsim_profile(m, t, R, Jr, wd);
  trajsim_curve(motion, rate * t, p, acc);
  trajsim_curve(motion, rate * 0.0, p0, acc);
  for (int i = 0; i < 3; ++i) T[i] = p[i] - p0[i];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      gt[3 * j + i] = R[3 * i + j];
      gsc[3 * i + j] = R[3 * i] * m.Rbc[j] + R[3 * i + 1] * m.Rbc[3 + j] + R[3 * i + 2] * m.Rbc[6 + j];
    }
    gt[9 + i] = T[i];
    gsc[9 + i] = R[3 * i] * m.Tbc[0] + R[3 * i + 1] * m.Tbc[1] + R[3 * i + 2] * m.Tbc[2] + T[i];
  }
}

}  // namespace xivo_hip
