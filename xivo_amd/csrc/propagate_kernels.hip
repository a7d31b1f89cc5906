// Propagation kernels of the EKF (gfx950), driven by capi_propagate.hip: the state + covariance stages of
// Estimator::Propagate and the covariance tail.
//
//  propagate_state_wave_kernel<4|7>   Estimator::Propagate: RK4Step / PrinceDormandStep, ComposeMotion,
//                                     ComputeMotionJacobianAt   src/rk4.cpp:35-103, src/princedormand.cpp:26-221,
//                                                               src/estimator.cpp:598-704
//  propagate_state_calib_kernel<4|7>  the same in the online-calibration builds   src/core.h:49-75,
//                                                               src/estimator.cpp:603-636, :674-684
//  propagate_cov_kernel               covariance cross-block tail               src/rk4.cpp:92-102
//  propagate_cov_fixed_kernel<23>     the same for the default motion size 23
// (paths relative to the reference tree).
#include <cstdio>

#include "ekf_kernels.h"
#include "geometry_device.h"

namespace xivo_hip {

namespace {

// ---------------------------------------------------------------- propagation tail
// P_mm <- Pmm_new ; P_ms <- Phi P_ms ; P_sm <- P_sm Phi^T (rk4.cpp:92-102). One
// workgroup per filter, Phi in LDS; thread j owns structure column / row j.
__global__ __launch_bounds__(256) void propagate_cov_kernel(double* Pall, long strideP, int ldp, int N, int nm,
                                                            const double* Phi_all, const double* Pmm_all,
                                                            int b0) {
  const int filt = b0 + blockIdx.x, tid = threadIdx.x;
  double* P = Pall + (long)filt * strideP;
  const double* Phi = Phi_all + (long)blockIdx.x * nm * nm;
  const double* Pmm = Pmm_all + (long)blockIdx.x * nm * nm;
  extern __shared__ double sPhi[];  // nm*nm, column-major
  for (int e = tid; e < nm * nm; e += 256) sPhi[e] = Phi[e];
  __syncthreads();
  constexpr int MAXM = 40;
  for (int j = nm + tid; j < N; j += 256) {
    double col[MAXM], row[MAXM];
    for (int k = 0; k < nm; ++k) { col[k] = P[k + (long)j * ldp]; row[k] = P[j + (long)k * ldp]; }
    for (int i = 0; i < nm; ++i) {
      double s = 0.0, t = 0.0;
      for (int k = 0; k < nm; ++k) {
        s = fma(sPhi[i + k * nm], col[k], s);   // (Phi P_ms)(i, j)
        t = fma(row[k], sPhi[i + k * nm], t);   // (P_sm Phi^T)(j, i)
      }
      P[i + (long)j * ldp] = s;
      P[j + (long)i * ldp] = t;
    }
  }
  for (int e = tid; e < nm * nm; e += 256) P[(e % nm) + (long)(e / nm) * ldp] = Pmm[e];
}

// Compile-time motion size (the default build's 23): col / row stay in registers (with a run-time nm the two
// arrays are indexed dynamically and live in scratch). One workgroup per filter, one thread per state column j >= NM.
// The row block P_ms (NM x (N - NM): NM contiguous doubles per column, columns ldp apart) goes through LDS so that
// HBM sees each 8 NM-byte run once, in lane order, on the way in and on the way out; the column block P_sm is
// coalesced as it lies. Phi sits in LDS with an even leading dimension so that one 16-byte broadcast read feeds two
// output rows (4 FMAs). Bound: HBM - 4 x 8 NM (N - NM) bytes per filter.
template <int NM>
__global__ __launch_bounds__(256) void propagate_cov_fixed_kernel(double* Pall, long strideP, int ldp, int N,
                                                                  const double* Phi_all, const double* Pmm_all, int b0) {
  constexpr int LP = NM + 1;        // even: rows (i, i + 1), i even, of one Phi column are 16-byte aligned
  static_assert(LP % 2 == 0, "NM must be odd");
  const int filt = b0 + blockIdx.x, tid = threadIdx.x;
  double* P = Pall + (long)filt * strideP;
  const double* Phi = Phi_all + (long)blockIdx.x * NM * NM;
  const double* Pmm = Pmm_all + (long)blockIdx.x * NM * NM;
  __shared__ __attribute__((aligned(16))) double sPhi[LP * NM];   // column-major, row NM = 0
  __shared__ double sBlk[NM * 256];                                // [k + NM * (j - j0)]
  for (int e = tid; e < NM * NM; e += 256) sPhi[(e % NM) + LP * (e / NM)] = Phi[e];
  if (tid < NM) sPhi[NM + LP * tid] = 0.0;
  for (int j0 = NM; j0 < N; j0 += 256) {
    const int nc = N - j0 < 256 ? N - j0 : 256;
    __syncthreads();                                // sPhi ready / previous chunk written back
    {
      int k = tid % NM, jj = tid / NM;              // element e = tid + 256 m  <->  (k, jj)
      for (int e = tid; e < NM * nc; e += 256) {
        sBlk[e] = P[k + (long)(j0 + jj) * ldp];
        k += 256 % NM; jj += 256 / NM;
        if (k >= NM) { k -= NM; ++jj; }
      }
    }
    __syncthreads();
    if (tid < nc) {
      const int j = j0 + tid;
      double col[NM], row[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) { col[k] = sBlk[k + NM * tid]; row[k] = P[j + (long)k * ldp]; }
#pragma unroll
      for (int i = 0; i < NM; i += 2) {
        double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int k = 0; k < NM; ++k) {
          const double2 ph = *reinterpret_cast<const double2*>(&sPhi[i + LP * k]);
          s0 = fma(ph.x, col[k], s0);   // (Phi P_ms)(i, j)
          t0 = fma(row[k], ph.x, t0);   // (P_sm Phi^T)(j, i)
          s1 = fma(ph.y, col[k], s1);
          t1 = fma(row[k], ph.y, t1);
        }
        sBlk[i + NM * tid] = s0;
        P[j + (long)i * ldp] = t0;
        if (i + 1 < NM) {
          sBlk[i + 1 + NM * tid] = s1;
          P[j + (long)(i + 1) * ldp] = t1;
        }
      }
    }
    __syncthreads();
    {
      int k = tid % NM, jj = tid / NM;
      for (int e = tid; e < NM * nc; e += 256) {
        P[k + (long)(j0 + jj) * ldp] = sBlk[e];
        k += 256 % NM; jj += 256 / NM;
        if (k >= NM) { k -= NM; ++jj; }
      }
    }
  }
  for (int e = tid; e < NM * NM; e += 256) P[(e % NM) + (long)(e / NM) * ldp] = Pmm[e];
}

// ---------------------------------------------------------------- propagation: state + covariance stages
// Runge-Kutta tableaus as the reference codes them: RK4Step (rk4.cpp:35-103; the 4th stage re-uses the half-step
// IMU sample, :77) and PrinceDormandStep (princedormand.cpp:85-221, weights :195-200). RkConst<NS> is the one
// definition of the coefficients: the wave kernel reads them as compile-time constants, and kTableau, which both
// kernels index at run time, is built from them.
template <int NS> struct RkConst;
template <> struct RkConst<4> {
  static constexpr double a[4][3] = {{0, 0, 0}, {0.5, 0, 0}, {0, 0.5, 0}, {0, 0, 1.0}};
  static constexpr double c_step[4] = {0.0, 0.5, 0.5, 1.0};
  static constexpr double c_imu[4] = {0.0, 0.5, 0.5, 0.5};
  static constexpr double b[4] = {1 / 6.0, 2 / 6.0, 2 / 6.0, 1 / 6.0};
};
template <> struct RkConst<7> {
  static constexpr double a[7][6] = {{0},
                                     {2 / 9.0},
                                     {1 / 12.0, 3 / 12.0},
                                     {55 / 324.0, -75 / 324.0, 200 / 324.0},
                                     {83 / 330.0, -195 / 330.0, 305 / 330.0, 27 / 330.0},
                                     {-19 / 28.0, 63 / 28.0, 4 / 28.0, -108 / 28.0, 88 / 28.0},
                                     {38 / 400.0, 0.0, 240 / 400.0, -243 / 400.0, 330 / 400.0, 35 / 400.0}};
  static constexpr double c_step[7] = {0.0, 2 / 9.0, 3 / 9.0, 5 / 9.0, 6 / 9.0, 1.0, 1.0};
  static constexpr double c_imu[7] = {0.0, 2 / 9.0, 3 / 9.0, 5 / 9.0, 6 / 9.0, 1.0, 1.0};
  static constexpr double b[7] = {0.0862, 0.0, 0.6660, -0.7857, 0.9570, 0.0965, -0.0200};
};
struct RkTableau { int ns; double a[7][6]; double c_step[7]; double c_imu[7]; double b[7]; };
template <int NS>
constexpr RkTableau tableau_of() {
  RkTableau t{};
  t.ns = NS;
  for (int i = 0; i < NS; ++i) {
    for (int j = 0; j + 1 < NS; ++j) t.a[i][j] = RkConst<NS>::a[i][j];
    t.c_step[i] = RkConst<NS>::c_step[i];
    t.c_imu[i] = RkConst<NS>::c_imu[i];
    t.b[i] = RkConst<NS>::b[i];
  }
  return t;
}
__constant__ RkTableau kTableau[2] = {tableau_of<4>(), tableau_of<7>()};

// exp(hat(w)) for the per-stage rotation increments (|w| = |gyro| * step, a few mrad): sin(t)/t and (1 - cos t)/t^2 as
// even Taylor series in t^2 - for |w| <= 0.25 the truncation is < 1e-20, below the rounding of the sin / cos route -
// which removes sqrt, sin, cos and two divisions (and their registers) from the chain every stage waits for. A larger
// increment (a single 0.1 s step of a fast spin) is halved until it is small and the result squared back:
// exp(w) = exp(w / 2^n)^(2^n), each squaring costing one rounding of a rotation matrix.
__device__ __forceinline__ M3 so3_exp_small(double wx, double wy, double wz) {
  double t2 = wx * wx + wy * wy + wz * wz;
  int halvings = 0;                         // scaling and squaring for the (unusual) large increment
  while (t2 > 0.0625 && halvings < 64) { wx *= 0.5; wy *= 0.5; wz *= 0.5; t2 *= 0.25; ++halvings; }
  const double a = fma(t2, fma(t2, fma(t2, fma(t2, fma(t2, fma(t2, 1.0 / 6227020800.0, -1.0 / 39916800.0), 1.0 / 362880.0),
                                                 -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0), 1.0);
  const double b = fma(t2, fma(t2, fma(t2, fma(t2, fma(t2, fma(t2, 1.0 / 87178291200.0, -1.0 / 479001600.0), 1.0 / 3628800.0),
                                                 -1.0 / 40320.0), 1.0 / 720.0), -1.0 / 24.0), 0.5);
  const V3 w{{wx, wy, wz}};
  const M3 W = hat(w), W2 = m3_mul(W, W);
  M3 R;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R.m[i][j] = (i == j ? 1.0 : 0.0) + a * W.m[i][j] + b * W2.m[i][j];
  for (; halvings > 0; --halvings) R = m3_mul(R, R);
  return R;
}

struct MotionRegs { M3 Rsb; V3 Tsb, Vsb, bg, ba; };   // Rsg is a constant of Propagate: its product Rsg g is passed separately

// ComposeMotion, estimator.cpp:598-613 (default build: Cg = Ca = I)
__device__ __forceinline__ void compose_motion_dev(MotionRegs& X, const V3& V, const V3& gyro, const V3& accel, double dt,
                                                   const V3& Rg) {
  V3 gc, ac;
#pragma unroll
  for (int i = 0; i < 3; ++i) { gc.v[i] = gyro.v[i] - X.bg.v[i]; ac.v[i] = accel.v[i] - X.ba.v[i]; }
  const V3 Ra = m3_mulv(X.Rsb, ac);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    X.Tsb.v[i] += V.v[i] * dt;                                   // :608
    X.Vsb.v[i] += (Ra.v[i] + Rg.v[i]) * dt;                      // :609
  }
  X.Rsb = m3_mul(X.Rsb, so3_exp_small(gc.v[0] * dt, gc.v[1] * dt, gc.v[2] * dt));   // :610
}

// Structure the propagation kernels exploit (the online-calibration kernel below: one workgroup of 256 threads per filter; the default
// build: one wave per filter, further down - same arithmetic per element):
//  * The nominal state of stage st - ComposeMotion of the sub-step's start state with the interpolated IMU sample
//    (rk4.cpp:49-88) - feeds the covariance stages only through Rsb(st), the bias-corrected gyro / accel and the stage
//    velocity K_st, and none of these depends on another stage (only Tsb does, through the a_ij-weighted velocities,
//    and Tsb enters no Jacobian). So the serial chain of ns ComposeMotion + ComputeMotionJacobianAt evaluations
//    (estimator.cpp:598-704) collapses to a pre-pass in which wave w evaluates stages w, w + 4 and publishes the
//    Jacobian blocks (36 numbers) and K_st in LDS, followed by one ComposeMotion for the sub-step itself.
//  * F = dX'/dX (23 x 23) has non-zero rows only for Wsb, Tsb, Vsb and at most 8 non-zeros in a row - dW/dW,
//    dW/dbg = -I, dT/dV = I, dV/dW, dV/dba = -Rsb, dV/dWsg - and G (23 x 12) is four 3 x 3 blocks (-I, -Rsb, I, I).
//    Neither is materialised: F M, M F^T and G Q G^T are formed from register copies of the 36 numbers with the
//    structural zeros skipped (exact: the skipped terms are 0 * x, the surviving ones are summed in the same
//    ascending-k order as the dense product).
//  * NS (stages) is a template parameter: the tableau-weighted sums are unrolled, all LDS loads of a sum are in
//    flight together, and coefficients of stages not yet computed are the tableau's zeros times finite stale values.
// The 23 x 23 matrices live in LDS (column-major, ld 23); FK keeps its 9 non-zero rows only ([i + 9 j]).

// ---------------------------------------------------------------- propagation, online-calibration builds
// The reference's USE_ONLINE_TEMPORAL_CALIB / USE_ONLINE_IMU_CALIB builds (src/core.h:49-75) carry td, Cg (9) and Ca (6) in the
// motion block: kMotionSize = 24 / 38 / 39, ComposeMotion uses imu_.Cg() / imu_.Ca() (estimator.cpp:603-604) and
// ComputeMotionJacobianAt adds dWsb/dCg (:626-631, :674-679) and dVsb/dCa (:633-636, :680-684). The rows of F that are not
// identically zero are still the nine of Wsb / Tsb / Vsb, so the products keep the shape of the default-build kernel above -
// F P0 is 9 x nm, P0 F^T is nm x 9, FK_q has nine rows, G Q G^T the same 12 x 12 support - but the nine rows are held DENSE
// (nm columns each, structural zeros multiplied through: 0 * x adds +0.0 in the same ascending-k sums) and nm is a run-time
// value. One workgroup of 256 threads per filter, everything in LDS (153 KB for nm = 39 with the seven Dormand-Prince
// stages: one workgroup per CU). Not a tuned kernel: these builds are off the metric path.
__device__ __forceinline__ void compose_motion_calib_dev(MotionRegs& X, const V3& V, const V3& gyro, const V3& accel, double dt,
                                                         const V3& Rg, const M3& Cg, const M3& Ca) {
  const V3 cg = m3_mulv(Cg, gyro), ca = m3_mulv(Ca, accel);
  V3 gc, ac;
#pragma unroll
  for (int i = 0; i < 3; ++i) { gc.v[i] = cg.v[i] - X.bg.v[i]; ac.v[i] = ca.v[i] - X.ba.v[i]; }   // :603-604
  const V3 Ra = m3_mulv(X.Rsb, ac);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    X.Tsb.v[i] += V.v[i] * dt;                                   // :608
    X.Vsb.v[i] += (Ra.v[i] + Rg.v[i]) * dt;                      // :609
  }
  X.Rsb = m3_mul(X.Rsb, so3_exp_small(gc.v[0] * dt, gc.v[1] * dt, gc.v[2] * dt));   // :610
}

template <int NS>
__global__ __launch_bounds__(256) void propagate_state_calib_kernel(PropStateArgs a) {
  constexpr int NT = 256, FR = 9, JS = 60;   // JS: doubles per stage of published Jacobian blocks
  const int nm = a.nm, NN = nm * nm, NF = FR * nm, iCg = a.iCg, iCa = iCg >= 0 ? iCg + 9 : -1;
  extern __shared__ double sm[];
  const int lane = threadIdx.x, filt = blockIdx.x;
  const RkTableau& tab = kTableau[NS == 4 ? 0 : 1];
  double* Pmm = sm;              // P_mm at the start of the sub-step
  double* P0 = Pmm + NN;
  double* PKs = P0 + NN;         // [NS][nm x nm]
  double* PhiA = PKs + NS * NN;  // rows < 9 of the accumulated transition ([i + 9 j]; the other rows stay identity rows)
  double* PhiB = PhiA + NF;
  double* S1 = PhiB + NF;        // [9 x nm] sum a_q FK_q, later rows < 9 of I + FK h
  double* F9 = S1 + NF;          // [9 x nm] the non-zero rows of F of the current stage, dense
  double* FPs = F9 + NF;         // [9 x nm]  F P0
  double* PFs = FPs + NF;        // [nm x 9]  P0 F^T ([i + nm j])
  double* FKs = PFs + NF;        // [NS][9 x nm]
  double* GQG = FKs + NS * NF;   // [12 x 12] support of G Q G^T: rows / cols (Wsb, Vsb, bg, ba)
  double* Q = GQG + 144;
  double* GQc = Q + 144;         // [12 x 12] the non-zero rows of G Q
  double* nom = GQc + 144;       // Rsb[9] row-major, Tsb, Vsb, bg, ba, Rsg g (3 each: 9..23), gyro, accel, slope_gyro, slope_accel
                                 // (24..35), Cg[9], Ca[9] row-major (36..53)
  double* sKs = nom + 64;        // [NS][3] stage velocities
  double* Jms = sKs + 24;        // [NS][JS]: dW/dW, dV/dW, -Rsb, dV/dWsg (3 x 3 row-major each), raw gyro (3), dV/dCa (3 x 6)

  const double* Pg = a.P + (long)filt * a.strideP;
  for (int e = lane; e < NN; e += NT) Pmm[e] = Pg[(e % nm) + (long)(e / nm) * a.ldp];
  for (int e = lane; e < NF; e += NT) PhiA[e] = (e % FR) == (e / FR) ? 1.0 : 0.0;
  for (int e = lane; e < NS * NF; e += NT) FKs[e] = 0.0;        // finite values under the tableau's zero coefficients
  for (int e = lane; e < NS * NN; e += NT) PKs[e] = 0.0;
  double* Phi = PhiA;
  double* PhiN = PhiB;
  for (int e = lane; e < 144; e += NT) {
    const double q = a.Qimu[filt * a.strideQimu + e];
    Q[e] = q;
    const int r = e % 12;     // rows of G Q that do not depend on the state: Wsb = -Q[0:3,:], bg = Q[6:9,:], ba = Q[9:12,:]
    if (r < 3) GQc[e] = -q;
    else if (r >= 6) GQc[e] = q;
  }
  xivo_pose_in& pose = a.poses[filt];
  const V3 gv{{a.g[0], a.g[1], a.g[2]}};
  if (lane == 0) {
    const V3 Rg0 = m3_mulv(m3_from_colmajor(pose.Rsg), gv);
    const xivo_calib_in& cb = a.calib[filt];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        nom[3 * i + j] = pose.Rsb[i + 3 * j];
        nom[36 + 3 * i + j] = iCg >= 0 ? cb.Cg[i + 3 * j] : (i == j ? 1.0 : 0.0);
        nom[45 + 3 * i + j] = iCg >= 0 ? cb.Ca[i + 3 * j] : (i == j ? 1.0 : 0.0);
      }
      nom[9 + i] = pose.Tsb[i]; nom[12 + i] = pose.Vsb[i]; nom[15 + i] = pose.bg[i]; nom[18 + i] = pose.ba[i];
      nom[21 + i] = Rg0.v[i];
    }
  }
  auto load_nominal = [&](MotionRegs& X, V3& Rg, M3& Cg, M3& Ca) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { X.Rsb.m[i][j] = nom[3 * i + j]; Cg.m[i][j] = nom[36 + 3 * i + j]; Ca.m[i][j] = nom[45 + 3 * i + j]; }
      X.Tsb.v[i] = nom[9 + i]; X.Vsb.v[i] = nom[12 + i]; X.bg.v[i] = nom[15 + i]; X.ba.v[i] = nom[18 + i];
      Rg.v[i] = nom[21 + i];
    }
  };
  __syncthreads();

  const xivo_imu_in* imu_f = a.imu + (long)filt * a.n_imu;
  // step-size-controlled Dormand-Prince (princedormand.cpp:26-60, as in propagate_state_wave_kernel): every thread carries the step
  const bool ctl = NS == 7 && a.pd_h != nullptr;
  double hs = ctl ? a.pd_h[filt] : 0.0;
  for (int smp = 0; smp < a.n_imu; ++smp) {
    if (lane < 3) {
      nom[24 + lane] = imu_f[smp].gyro[lane]; nom[27 + lane] = imu_f[smp].accel[lane];
      nom[30 + lane] = imu_f[smp].slope_gyro[lane]; nom[33 + lane] = imu_f[smp].slope_accel[lane];
    }
    const double dt = imu_f[smp].dt;
    if (ctl) {
      if (hs < 1e-6) hs = a.stepsize;        // :30-32
      hs = fmin(hs, dt);                     // :34
    }
    __syncthreads();
    double total = 0.0;
    while (total < dt || (!ctl && a.stepsize < 0)) {     // rk4.cpp:13-32, princedormand.cpp:62-81
      double h = a.stepsize;
      if (ctl) h = hs;
      else if (a.stepsize < 0) h = dt;
      else if (total + h > dt) h = dt - total;
      else if (total + h + 0.5 * h > dt) h = 0.5 * h;

      // -- nominal pre-pass: thread st evaluates stage st (ComposeMotion + ComputeMotionJacobianAt, estimator.cpp:598-704)
      if (lane < NS) {
        const int st = lane;
        MotionRegs X0; V3 Rg; M3 Cg, Ca;
        load_nominal(X0, Rg, Cg, Ca);
        const double ti = tab.c_imu[st] * h;
        V3 gi, ai;
#pragma unroll
        for (int i = 0; i < 3; ++i) { gi.v[i] = nom[24 + i] + nom[30 + i] * ti; ai.v[i] = nom[27 + i] + nom[33 + i] * ti; }
        if (st > 0) {
          const V3 V0{{0, 0, 0}};   // the a_ij-weighted velocities only move Tsb, which no Jacobian reads
          compose_motion_calib_dev(X0, V0, gi, ai, tab.c_step[st] * h, Rg, Cg, Ca);
        }
        const V3 cg = m3_mulv(Cg, gi), ca = m3_mulv(Ca, ai);
        V3 gc, ac;
#pragma unroll
        for (int i = 0; i < 3; ++i) { gc.v[i] = cg.v[i] - X0.bg.v[i]; ac.v[i] = ca.v[i] - X0.ba.v[i]; }
        const M3 w_dW_dW = m3_neg(hat(gc));
        const M3 w_dV_dW = m3_neg(m3_mul(X0.Rsb, hat(ac)));
        const M3 w_dV_dWsg = m3_neg(m3_mul(X0.Rsb, hat(gv)));
        const M3 w_nR = m3_neg(X0.Rsb);
        double* Jm = Jms + st * JS;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          sKs[3 * st + i] = X0.Vsb.v[i];
          Jm[36 + i] = gi.v[i];                                  // :626-631: the RAW gyro sample fills dWsb/dCg
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            Jm[3 * i + j] = w_dW_dW.m[i][j]; Jm[9 + 3 * i + j] = w_dV_dW.m[i][j];
            Jm[18 + 3 * i + j] = w_nR.m[i][j]; Jm[27 + 3 * i + j] = w_dV_dWsg.m[i][j];
          }
        }
        // :633-636 dV_dCa = dAB_dA<3,3>(accel) dAB_dB<3,3>(Rsb) dA_dAu<3>() with the index conventions of common/rodrigues.h
        // (:143-165 row index p N + n against :208-227 row index p N + n of a COLUMN-major vec): what survives is
        // dV_dCa(n, u(m, n)) = (Rsb^T accel)(m) for m <= n, u = the upper-triangle counter of dA_dAu (row by row)
        V3 w;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) v = fma(ai.v[k], X0.Rsb.m[k][m], v);
          w.v[m] = v;
        }
#pragma unroll
        for (int e = 0; e < 18; ++e) Jm[39 + e] = 0.0;
        {
          int u = 0;
#pragma unroll
          for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int n = m; n < 3; ++n) { Jm[39 + 6 * n + u] = w.v[m]; ++u; }
        }
      }
      __syncthreads();
      // the sub-step of the nominal state itself
      if (lane == 0) {
        MotionRegs X; V3 Rg; M3 Cg, Ca;
        load_nominal(X, Rg, Cg, Ca);
        V3 ge, ae, Kt{{0, 0, 0}};
#pragma unroll
        for (int i = 0; i < 3; ++i) { ge.v[i] = nom[24 + i] + nom[30 + i] * h; ae.v[i] = nom[27 + i] + nom[33 + i] * h; }
#pragma unroll
        for (int q = 0; q < NS; ++q)
#pragma unroll
          for (int i = 0; i < 3; ++i) Kt.v[i] += tab.b[q] * sKs[3 * q + i];
        compose_motion_calib_dev(X, Kt, ge, ae, h, Rg, Cg, Ca);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) nom[3 * i + j] = X.Rsb.m[i][j];
          nom[9 + i] = X.Tsb.v[i]; nom[12 + i] = X.Vsb.v[i];
          nom[24 + i] = ge.v[i]; nom[27 + i] = ae.v[i];   // rk4.cpp:27-28: the next sub-step starts from the interpolated sample
        }
      }
      auto phase_a = [&](int st) {   // P0 = Pmm + (sum a_q PK_q) h, S = sum a_q FK_q, this stage's F rows and G Q rows
        const double* Jm = Jms + st * JS;
        for (int e = lane; e < NN; e += NT) {
          double sp = 0.0;
#pragma unroll
          for (int q = 0; q < NS - 1; ++q) sp += tab.a[st][q] * PKs[q * NN + e];
          P0[e] = Pmm[e] + sp * h;
        }
        for (int e = lane; e < NF; e += NT) {
          double sf = 0.0;
#pragma unroll
          for (int q = 0; q < NS - 1; ++q) sf += tab.a[st][q] * FKs[q * NF + e];
          S1[e] = sf;
          const int i = e % FR, j = e / FR;
          double f = 0.0;
          if (i < 3) {                                            // Wsb rows
            if (j < 3) f = Jm[3 * i + j];
            else if (j == 9 + i) f = -1.0;
            else if (iCg >= 0 && j >= iCg + 3 * i && j < iCg + 3 * i + 3) f = Jm[36 + (j - iCg - 3 * i)];
          } else if (i < 6) {                                     // Tsb rows
            if (j == 3 + i) f = 1.0;
          } else {                                                // Vsb rows
            const int r = i - 6;
            if (j < 3) f = Jm[9 + 3 * r + j];
            else if (j >= 12 && j < 15) f = Jm[18 + 3 * r + (j - 12)];
            else if (j == 21 || j == 22) f = Jm[27 + 3 * r + (j - 21)];
            else if (iCa >= 0 && j >= iCa && j < iCa + 6) f = Jm[39 + 6 * r + (j - iCa)];
          }
          F9[e] = f;
        }
        if (lane >= 224 && lane < 236) {                          // (G Q)[Vsb_i, l] = sum_k -Rsb[i][k] Q[3 + k, l]
          const int l = lane - 224;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) v = fma(Jm[18 + 3 * i + k], Q[(3 + k) + 12 * l], v);
            GQc[(3 + i) + 12 * l] = v;
          }
        }
      };
      phase_a(0);
      __syncthreads();
      for (int st = 0; st < NS; ++st) {
        const double* Jm = Jms + st * JS;
        // -- phase B: F P0, FK_st = F + F S h, P0 F^T, G Q G^T
        for (int e = lane; e < NF; e += NT) {
          const int i = e % FR, j = e / FR;
          double fp = 0.0, fs = 0.0;
          for (int k = 0; k < nm; ++k) fp = fma(F9[i + FR * k], P0[k + nm * j], fp);
#pragma unroll
          for (int k = 0; k < FR; ++k) fs = fma(F9[i + FR * k], S1[k + FR * j], fs);   // rows >= 9 of S are zero
          FPs[e] = fp;
          FKs[st * NF + e] = F9[e] + fs * h;
        }
        for (int e = lane; e < NF; e += NT) {
          const int i = e % nm, j = e / nm;                       // (P0 F^T)[i, j < 9]
          double pf = 0.0;
          for (int k = 0; k < nm; ++k) pf = fma(P0[i + nm * k], F9[j + FR * k], pf);
          PFs[e] = pf;
        }
        if (lane < 144) {
          const int r = lane % 12, cidx = lane / 12;
          double v;
          if (cidx < 3) v = fma(GQc[r + 12 * cidx], -1.0, 0.0);
          else if (cidx < 6) {
            v = fma(GQc[r + 12 * 3], Jm[18 + 3 * (cidx - 3) + 0], 0.0);
            v = fma(GQc[r + 12 * 4], Jm[18 + 3 * (cidx - 3) + 1], v);
            v = fma(GQc[r + 12 * 5], Jm[18 + 3 * (cidx - 3) + 2], v);
          } else v = GQc[r + 12 * cidx];
          GQG[r + 12 * cidx] = v;
        }
        __syncthreads();
        // -- phase C: PK_st = F P0 + P0 F^T + G Q G^T, then phase A of the next stage
        for (int e = lane; e < NN; e += NT) {
          const int i = e % nm, j = e / nm;
          const int ci = i < 3 ? i : ((i >= 6 && i < 15) ? i - 3 : -1), cj = j < 3 ? j : ((j >= 6 && j < 15) ? j - 3 : -1);
          const double fp = i < FR ? FPs[i + FR * j] : 0.0, pf = j < FR ? PFs[i + nm * j] : 0.0;
          const double gq = (ci >= 0 && cj >= 0) ? GQG[ci + 12 * cj] : 0.0;
          PKs[st * NN + e] = (fp + pf) + gq;
        }
        __syncthreads();
        if (st + 1 < NS) { phase_a(st + 1); __syncthreads(); }
      }
      // combine the stages
      for (int e = lane; e < NN; e += NT) {
        double pk = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) pk += tab.b[q] * PKs[q * NN + e];
        Pmm[e] += pk * h;                              // rk4.cpp:92-93
      }
      for (int e = lane; e < NF; e += NT) {
        double fk = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) fk += tab.b[q] * FKs[q * NF + e];
        S1[e] = ((e % FR) == (e / FR) ? 1.0 : 0.0) + fk * h;    // rows < 9 of Phi_step = I + FK h
      }
      __syncthreads();
      for (int e = lane; e < NF; e += NT) {            // Phi <- Phi_step Phi (rows >= 9 of both are identity rows)
        const int i = e % FR, j = e / FR;
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < FR; ++k) v = fma(S1[i + FR * k], Phi[k + FR * j], v);
        if (j >= FR) v = fma(S1[i + FR * j], 1.0, v);
        PhiN[e] = v;
      }
      { double* t = Phi; Phi = PhiN; PhiN = t; }
      __syncthreads();
      total += h;
      if (ctl) {
        const double err = 0.0;                // PrinceDormandStep returns 0 (:216-220)
        double scale;
        if (err == 0.0) scale = a.pd_max_scale;                                                     // :42-43
        else scale = fmin(fmax(0.8 * sqrt(sqrt(a.pd_tol * h / err)), a.pd_min_scale), a.pd_max_scale);   // :45-47
        hs = h * scale;                                                                             // :51
        if (total < dt) {                                                                           // :52-58
          if (total + hs > dt) hs = dt - total;
          else if (total + hs + 0.5 * hs > dt) hs = 0.5 * hs;
        }
        // the next step starts from gyro0 + slope * total_step (:38-39)
        if (lane < 3) {
          nom[24 + lane] = imu_f[smp].gyro[lane] + imu_f[smp].slope_gyro[lane] * total;
          nom[27 + lane] = imu_f[smp].accel[lane] + imu_f[smp].slope_accel[lane] * total;
        }
        __syncthreads();
      } else if (a.stepsize < 0) break;
    }
    for (int e = lane; e < NN; e += NT) Pmm[e] += a.Qmodel[filt * a.strideQmodel + e];   // estimator.cpp:590, per Propagate
    __syncthreads();
  }
  for (int e = lane; e < NN; e += NT) {
    const int i = e % nm, j = e / nm;
    a.Pmm_out[(long)filt * NN + e] = Pmm[e];
    a.Phi_out[(long)filt * NN + e] = i < FR ? Phi[i + FR * j] : (i == j ? 1.0 : 0.0);
  }
  if (ctl && lane == 0) a.pd_h[filt] = hs;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pose.Tsb[i] = nom[9 + i]; pose.Vsb[i] = nom[12 + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) pose.Rsb[i + 3 * j] = nom[3 * i + j];
    }
  }
}

// ---------------------------------------------------------------- propagation, one wave per filter
// The workgroup kernel above spends its time in barriers between phases that keep a few dozen lanes busy. Here ONE
// wave owns a filter: nothing waits on another wave, the phases follow each other in program order, and what only
// ever belongs to one lane leaves the LDS:
//  * element e = lane + 64 m (m < 9) of every 23 x 23 matrix is handled by the same lane in the tableau sums, the
//    stage combination and the + Qmodel step, so P_mm and the stage derivatives PK_q live in registers (the stage
//    loop is unrolled: PK_q is a named register set and the tableau a compile-time constant whose zeros cost nothing);
//  * LDS (28 KB RK4 / 34 KB Dormand-Prince: 5 / 4 filters per CU) keeps what crosses lanes: P0, the F products,
//    the FK_q, the transition;
//  * the nominal pre-pass is vectorised over the stages: lane q < NS composes stage q, lane NS the sub-step itself
//    (the same ComposeMotion code with its own sample time, step and velocity; a stage of step 0 composes with the
//    identity, exactly), each lane forming the tableau-weighted velocity from the stage velocities it recomputes.
// Arithmetic per element is that of the workgroup kernel (same ascending-k / ascending-q sums).
template <int NS>
__global__ __launch_bounds__(64) void propagate_state_wave_kernel(PropStateArgs a) {
  constexpr int NM = 23, NN = NM * NM, FR = 9, NF = FR * NM, EL = 9, FL = 4;   // EL / FL: elements of a 23 x 23 / 9 x 23 matrix per lane
  using TB = RkConst<NS>;
  extern __shared__ double sm[];
  const int lane = threadIdx.x, filt = blockIdx.x;
  const RkTableau& tab = kTableau[NS == 4 ? 0 : 1];
  double* P0 = sm;
  double* S1 = P0 + NN;        // 23 x 23 scratch whose rows >= 9 stay zero: sum a_q FK_q, later I + FK h
  double* FPs = S1 + NN;       // [9 x 23]  F P0   ([i + 9 j])
  double* GQG = FPs + NF;      // [12 x 12] support of G Q G^T
  double* Q = GQG + 144;
  double* GQc = Q + 144;       // [12 x 12] the non-zero rows of G Q
  double* zero = GQc + 144;    // one 0.0 + pad
  double* nom = zero + 2;      // nominal state + IMU sample (layout of the workgroup kernel)
  double* Jms = nom + 36;      // [NS][4][3 x 3]
  double* F9 = Jms + NS * 36;  // [9 x 23] dense non-zero rows of F of the current stage
  double* FKs = F9 + NF;       // [NS][9 x 23]
  double* PhiA = FKs + NS * NF;

  const double* Pg = a.P + (long)filt * a.strideP;
  // Lanes past the end of a matrix repeat its last element (clamped index): no predicates in the loops, the copies
  // hold identical values and only the owner stores at the end.
  double Pmm[EL], PK[NS][EL];
  int off[EL];                 // the three terms of PK(e) as packed 8-bit offsets into FPs / FPs (transposed entry) / GQG (255: absent)
#pragma unroll
  for (int m = 0; m < EL; ++m) {
    const int e = min(lane + 64 * m, NN - 1), i = e % NM, j = e / NM;
    const int ci = i < 3 ? i : ((i >= 6 && i < 15) ? i - 3 : -1), cj = j < 3 ? j : ((j >= 6 && j < 15) ? j - 3 : -1);
    Pmm[m] = Pg[i + (long)j * a.ldp];
    off[m] = (i < FR ? i + FR * j : 255) | ((j < FR ? j + FR * i : 255) << 8) | (((ci >= 0 && cj >= 0) ? ci + 12 * cj : 255) << 16);   // F P0, (F P0)^T, G Q G^T
    S1[e] = 0.0;
#pragma unroll
    for (int q = 0; q < NS; ++q) PK[q][m] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < FL; ++u) {
    const int f = min(lane + 64 * u, NF - 1);
    const int i = f % FR, j = f / FR;
    PhiA[f] = i == j ? 1.0 : 0.0;
    F9[f] = (i < 3 && j == 9 + i) ? -1.0 : ((i >= 3 && i < 6 && j == 3 + i) ? 1.0 : 0.0);   // dWsb/dbg = -I, dTsb/dVsb = I
#pragma unroll
    for (int q = 0; q < NS; ++q) FKs[q * NF + f] = 0.0;
  }
  if (lane == 0) zero[0] = 0.0;
  for (int e = lane; e < 144; e += 64) {
    const double q = a.Qimu[filt * a.strideQimu + e];
    Q[e] = q;
    const int r = e % 12;      // rows of G Q that do not depend on the state: Wsb rows = -Q[0:3,:], bg / ba rows = Q[6:12,:]
    if (r < 3) GQc[e] = -q;
    else if (r >= 6) GQc[e] = q;
  }
  double* Phi = PhiA;
  xivo_pose_in& pose = a.poses[filt];
  const V3 gv{{a.g[0], a.g[1], a.g[2]}};
  if (lane == 0) {
    const V3 Rg0 = m3_mulv(m3_from_colmajor(pose.Rsg), gv);   // Rsg g (estimator.cpp:609)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) nom[3 * i + j] = pose.Rsb[i + 3 * j];
      nom[9 + i] = pose.Tsb[i]; nom[12 + i] = pose.Vsb[i]; nom[15 + i] = pose.bg[i]; nom[18 + i] = pose.ba[i];
      nom[21 + i] = Rg0.v[i];
    }
  }
  __syncthreads();   // (one wave: orders the LDS traffic, no waiting)

  const xivo_imu_in* imu_f = a.imu + (long)filt * a.n_imu;
  const int c3 = lane < 3 ? lane : 0;
  double n_g = imu_f[0].gyro[c3], n_a = imu_f[0].accel[c3], n_sg = imu_f[0].slope_gyro[c3], n_sa = imu_f[0].slope_accel[c3];
  double n_dt = imu_f[0].dt;
  // step-size-controlled Dormand-Prince (princedormand.cpp:26-60): the step the last sample - or the last call - left behind
  const bool ctl = NS == 7 && a.pd_h != nullptr;
  double hs = ctl ? a.pd_h[filt] : 0.0;
  for (int smp = 0; smp < a.n_imu; ++smp) {
    if (lane < 3) { nom[24 + lane] = n_g; nom[27 + lane] = n_a; nom[30 + lane] = n_sg; nom[33 + lane] = n_sa; }
    const double dt = n_dt;
    const double cur_g = n_g, cur_a = n_a, cur_sg = n_sg, cur_sa = n_sa;     // (lanes 0-2: this sample as it arrived)
    if (ctl) {
      if (hs < 1e-6) hs = a.stepsize;        // :30-32
      hs = fmin(hs, dt);                     // :34
    }
    if (smp + 1 < a.n_imu) {
      const xivo_imu_in& nx = imu_f[smp + 1];
      n_g = nx.gyro[c3]; n_a = nx.accel[c3]; n_sg = nx.slope_gyro[c3]; n_sa = nx.slope_accel[c3]; n_dt = nx.dt;
    }
    __syncthreads();
    double total = 0.0;
    // fixed sub-stepping with the half-step tail trick (rk4.cpp:13-32, princedormand.cpp:62-81)
    while (total < dt || (!ctl && a.stepsize < 0)) {
      double h = a.stepsize;
      if (ctl) h = hs;
      else if (a.stepsize < 0) h = dt;
      else if (total + h > dt) h = dt - total;
      else if (total + h + 0.5 * h > dt) h = 0.5 * h;

      {  // -- nominal pre-pass: lane q < NS = stage q, lane NS = the sub-step itself
        MotionRegs X0; V3 Rg;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) X0.Rsb.m[i][j] = nom[3 * i + j];
          X0.Tsb.v[i] = nom[9 + i]; X0.Vsb.v[i] = nom[12 + i]; X0.bg.v[i] = nom[15 + i]; X0.ba.v[i] = nom[18 + i];
          Rg.v[i] = nom[21 + i];
        }
        V3 g0, a0, sg, sa;
#pragma unroll
        for (int i = 0; i < 3; ++i) { g0.v[i] = nom[24 + i]; a0.v[i] = nom[27 + i]; sg.v[i] = nom[30 + i]; sa.v[i] = nom[33 + i]; }
        // the tableau-weighted velocity: K_q = Vsb of stage q's ComposeMotion (estimator.cpp:609)
        V3 Kt{{0, 0, 0}};
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const double tq = TB::c_imu[q] * h, dq = TB::c_step[q] * h;
          V3 ac;
#pragma unroll
          for (int i = 0; i < 3; ++i) ac.v[i] = (a0.v[i] + sa.v[i] * tq) - X0.ba.v[i];
          const V3 Ra = m3_mulv(X0.Rsb, ac);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            double kq = X0.Vsb.v[i];
            if (q > 0) kq += (Ra.v[i] + Rg.v[i]) * dq;
            Kt.v[i] += TB::b[q] * kq;
          }
        }
        const bool is_step = lane == NS;
        const int st = lane < NS ? lane : 0;
        const double ti = is_step ? h : tab.c_imu[st] * h;
        const double ds = is_step ? h : tab.c_step[st] * h;
        V3 gi, ai, V;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          gi.v[i] = g0.v[i] + sg.v[i] * ti; ai.v[i] = a0.v[i] + sa.v[i] * ti;
          V.v[i] = is_step ? Kt.v[i] : 0.0;   // the a_ij-weighted velocities of a stage only move Tsb, which no Jacobian reads
        }
        compose_motion_dev(X0, V, gi, ai, ds, Rg);
        // ComputeMotionJacobianAt (estimator.cpp:615-704): the blocks of F and G
        V3 gc, ac;
#pragma unroll
        for (int i = 0; i < 3; ++i) { gc.v[i] = gi.v[i] - X0.bg.v[i]; ac.v[i] = ai.v[i] - X0.ba.v[i]; }
        const M3 w_dW_dW = m3_neg(hat(gc));
        const M3 w_dV_dW = m3_neg(m3_mul(X0.Rsb, hat(ac)));
        const M3 w_dV_dWsg = m3_neg(m3_mul(X0.Rsb, hat(gv)));
        const M3 w_nR = m3_neg(X0.Rsb);
        if (lane < NS) {
          double* Jm = Jms + st * 36;
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              Jm[3 * i + j] = w_dW_dW.m[i][j]; Jm[9 + 3 * i + j] = w_dV_dW.m[i][j];
              Jm[18 + 3 * i + j] = w_nR.m[i][j]; Jm[27 + 3 * i + j] = w_dV_dWsg.m[i][j];
            }
        } else if (is_step) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) nom[3 * i + j] = X0.Rsb.m[i][j];
            nom[9 + i] = X0.Tsb.v[i]; nom[12 + i] = X0.Vsb.v[i];
            nom[24 + i] = gi.v[i]; nom[27 + i] = ai.v[i];   // rk4.cpp:27-28: the next sub-step starts from the interpolated sample
          }
        }
      }
      __syncthreads();

#pragma unroll
      for (int st = 0; st < NS; ++st) {
        const double* Jm = Jms + st * 36;
        // -- phase A: P0 = Pmm + (sum_q a_q PK_q) h, S = sum_q a_q FK_q (rows < 9), the stage's entries of F, Vsb rows of G Q
#pragma unroll
        for (int m = 0; m < EL; ++m) {
          const int e = min(lane + 64 * m, NN - 1);
          double sp = 0.0;
#pragma unroll
          // (explicit fma in the sums over P, here and in the stage combination: left to contraction, the compiler fused some
          //  of a lane's nine unrolled element instances and not others, and the two triangles of P_mm - which are different
          //  instances - rounded differently, while phase B takes P0 as symmetric. The FK sums next to them may stay as they
          //  are: no element of F is taken for another)
          for (int q = 0; q < st; ++q)
            if (TB::a[st][q] != 0.0) sp = fma(TB::a[st][q], PK[q][m], sp);
          P0[e] = fma(sp, h, Pmm[m]);
        }
#pragma unroll
        for (int u = 0; u < FL; ++u) {
          const int f = min(lane + 64 * u, NF - 1);
          double sf = 0.0;
#pragma unroll
          for (int q = 0; q < st; ++q)
            if (TB::a[st][q] != 0.0) sf += TB::a[st][q] * FKs[q * NF + f];
          S1[(f % FR) + NM * (f / FR)] = sf;
        }
        if (lane < 33) {                                            // the stage's 33 state-dependent entries of F
          const int l = lane, blk = l < 27 ? l / 9 : 3, m = l - 9 * blk;
          const int i = blk < 3 ? m / 3 : m / 2, j = blk < 3 ? m % 3 : m % 2;
          const int row = blk == 0 ? i : 6 + i, col = blk < 2 ? j : (blk == 2 ? 12 + j : 21 + j);
          F9[row + FR * col] = Jm[9 * blk + 3 * i + j];
        } else if (lane < 45) {                                     // (G Q)[Vsb_i, l] = sum_k -Rsb[i][k] Q[3 + k, l]
          const int l = lane - 33;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) v = fma(Jm[18 + 3 * i + k], Q[(3 + k) + 12 * l], v);
            GQc[(3 + i) + 12 * l] = v;
          }
        }
        __syncthreads();

        // -- phase B: the structured products (the published 3 x 3 blocks once into registers)
        M3 dW_dW, dV_dW, nR, dV_dWsg;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            dW_dW.m[i][j] = Jm[3 * i + j]; dV_dW.m[i][j] = Jm[9 + 3 * i + j];
            nR.m[i][j] = Jm[18 + 3 * i + j]; dV_dWsg.m[i][j] = Jm[27 + 3 * i + j];
          }
        {
          // lanes 0..22: column j of F P0, lanes 32..54: column j of F S and from it FK of the stage
          const bool fk_task = lane >= 32;
          const int j = fk_task ? lane - 32 : lane;
          if (j < NM) {
            const double* M = (fk_task ? S1 : P0) + NM * j;
            double o[9];
            const double m0 = M[0], m1 = M[1], m2 = M[2], m12 = M[12], m13 = M[13], m14 = M[14], m21 = M[21], m22 = M[22];
#pragma unroll
            for (int i = 0; i < 3; ++i) {                           // Wsb rows: k = 0..2 (dW/dW), k = 9 + i (-1)
              double v = fma(dW_dW.m[i][0], m0, 0.0);
              v = fma(dW_dW.m[i][1], m1, v);
              v = fma(dW_dW.m[i][2], m2, v);
              o[i] = fma(-1.0, M[9 + i], v);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) o[3 + i] = fma(1.0, M[6 + i], 0.0);   // Tsb rows: k = 6 + i (1)
#pragma unroll
            for (int i = 0; i < 3; ++i) {                           // Vsb rows: k = 0..2, 12..14, 21..22
              double v = fma(dV_dW.m[i][0], m0, 0.0);
              v = fma(dV_dW.m[i][1], m1, v);
              v = fma(dV_dW.m[i][2], m2, v);
              v = fma(nR.m[i][0], m12, v);
              v = fma(nR.m[i][1], m13, v);
              v = fma(nR.m[i][2], m14, v);
              v = fma(dV_dWsg.m[i][0], m21, v);
              o[6 + i] = fma(dV_dWsg.m[i][1], m22, v);
            }
            if (fk_task) {                                          // FK_st = F + F S h
#pragma unroll
              for (int i = 0; i < FR; ++i) FKs[st * NF + i + FR * j] = F9[i + FR * j] + o[i] * h;
            } else {
#pragma unroll
              for (int i = 0; i < FR; ++i) FPs[i + FR * j] = o[i];
            }
          }
        }
        // (P0 F^T is not formed: P0 is symmetric - P_mm and every stage derivative are, bit for bit but for the
        //  rounding-level asymmetry of G Q G^T - so (P0 F^T)[i][j] = (F P0)[j][i], the same products summed in the same order)
        if (lane >= 32 && lane < 44) {                              // (G Q G^T)[r, :] on the 12 x 12 support
          const int r = lane - 32;
          const double g3 = GQc[r + 12 * 3], g4 = GQc[r + 12 * 4], g5 = GQc[r + 12 * 5];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            GQG[r + 12 * j] = fma(GQc[r + 12 * j], -1.0, 0.0);     // Wsb columns: G[Wsb_j, j] = -1
            double v = fma(g3, nR.m[j][0], 0.0);                    // Vsb columns: G[Vsb_j, 3..5] = -Rsb[j][:]
            v = fma(g4, nR.m[j][1], v);
            GQG[r + 12 * (3 + j)] = fma(g5, nR.m[j][2], v);
            GQG[r + 12 * (6 + j)] = GQc[r + 12 * (6 + j)];          // bg, ba columns: +1
            GQG[r + 12 * (9 + j)] = GQc[r + 12 * (9 + j)];
          }
        }
        __syncthreads();

        // -- phase C: PK_st = F P0 + P0 F^T + G Q G^T
#pragma unroll
        for (int m = 0; m < EL; ++m) {
          const int o1 = off[m] & 255, o2 = (off[m] >> 8) & 255, o3 = (off[m] >> 16) & 255;
          const double t1 = o1 == 255 ? 0.0 : FPs[o1], t2 = o2 == 255 ? 0.0 : FPs[o2], t3 = o3 == 255 ? 0.0 : GQG[o3];
          PK[st][m] = (t1 + t2) + t3;
        }
        // (phase A of the next stage writes P0 / S1 / F9 / GQc, which phase B above has finished reading; FPs / PFs / GQG are
        //  rewritten by the next phase B only, after the reads just issued - program order within the one wave)
      }
      // combine the stages
#pragma unroll
      for (int m = 0; m < EL; ++m) {
        double pk = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q)
          if (TB::b[q] != 0.0) pk = fma(TB::b[q], PK[q][m], pk);
        Pmm[m] = fma(pk, h, Pmm[m]);                   // rk4.cpp:92-93
      }
#pragma unroll
      for (int u = 0; u < FL; ++u) {
        const int f = min(lane + 64 * u, NF - 1);
        const int i = f % FR, j = f / FR;
        double fk = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q)
          if (TB::b[q] != 0.0) fk += TB::b[q] * FKs[q * NF + f];
        S1[i + NM * j] = (i == j ? 1.0 : 0.0) + fk * h;     // rows < 9 of Phi_step = I + FK h
      }
      __syncthreads();
      {                                                // Phi <- Phi_step Phi (rows >= 9 of both are identity rows), in place:
        double pv[FL];                                 // every lane has read its column before any lane writes
#pragma unroll
        for (int u = 0; u < FL; ++u) {
          const int f = min(lane + 64 * u, NF - 1);
          const int i = f % FR, j = f / FR;
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < FR; ++k) v = fma(S1[i + NM * k], Phi[k + FR * j], v);
          const double tail = fma(S1[i + NM * j], 1.0, v);
          pv[u] = j >= FR ? tail : v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < FL; ++u) Phi[min(lane + 64 * u, NF - 1)] = pv[u];
      }
      __syncthreads();
      total += h;
      if (ctl) {
        const double err = 0.0;                // PrinceDormandStep returns 0: its error estimate is commented out (:216-220)
        double scale;
        if (err == 0.0) scale = a.pd_max_scale;                                                     // :42-43
        else scale = fmin(fmax(0.8 * sqrt(sqrt(a.pd_tol * h / err)), a.pd_min_scale), a.pd_max_scale);   // :45-47
        hs = h * scale;                                                                             // :51
        if (total < dt) {                                                                           // :52-58
          if (total + hs > dt) hs = dt - total;
          else if (total + hs + 0.5 * hs > dt) hs = 0.5 * hs;
        }
        // the next step starts from gyro0 + slope * total_step (:38-39), not from the running sum of the fixed-step branch
        if (lane < 3) { nom[24 + lane] = cur_g + cur_sg * total; nom[27 + lane] = cur_a + cur_sa * total; }
        __syncthreads();
      } else if (a.stepsize < 0) break;
    }
#pragma unroll
    for (int m = 0; m < EL; ++m) Pmm[m] += a.Qmodel[filt * a.strideQmodel + min(lane + 64 * m, NN - 1)];   // P_mm += Qmodel (estimator.cpp:590), per Propagate
  }
  __syncthreads();
  if (ctl && lane == 0) a.pd_h[filt] = hs;
#pragma unroll
  for (int m = 0; m < EL; ++m) {
    const int e = lane + 64 * m;
    if (e < NN) a.Pmm_out[(long)filt * NN + e] = Pmm[m];
  }
  for (int e = lane; e < NN; e += 64) {
    const int i = e % NM, j = e / NM;
    a.Phi_out[(long)filt * NN + e] = i < FR ? Phi[i + FR * j] : (i == j ? 1.0 : 0.0);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pose.Tsb[i] = nom[9 + i]; pose.Vsb[i] = nom[12 + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) pose.Rsb[i + 3 * j] = nom[3 * i + j];
    }
  }
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int propagate_cov_pick(int nm, int N, char* label, size_t n) {
  if (nm <= 0 || nm > 40 || N < nm) { if (label && n) label[0] = 0; return -1; }
  if (label && n) snprintf(label, n, "%s", nm == 23 ? "propagate_cov_fixed_kernel<23>" : "propagate_cov_kernel");
  return (N - nm + 255) / 256;                         // both kernels: one thread per tail column, 256 columns a pass
}
int launch_propagate_cov(double* P, long strideP, int ldp, int N, int Np, int nm, const double* Phi,
                         const double* Pmm, int b0, int nb, hipStream_t s) {
  (void)Np;
  if (propagate_cov_pick(nm, N, nullptr, 0) < 0) return (int)hipErrorInvalidValue;
  if (nm == 23) {
    hipLaunchKernelGGL(propagate_cov_fixed_kernel<23>, dim3(nb), dim3(256), 0, s, P, strideP, ldp, N, Phi, Pmm, b0);
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(propagate_cov_kernel, dim3(nb), dim3(256), nm * nm * sizeof(double), s, P, strideP, ldp, N,
                     nm, Phi, Pmm, b0);
  CHECK_LAUNCH();
}
template <int NS>
static int launch_propagate_state_wave(const PropStateArgs& a, hipStream_t s) {
  // LDS: P0, S1, F P0 / P0 F^T scratch, Q / GQ / GQG^T supports, nominal state, F9, two transition buffers, per stage 36
  // Jacobian entries + FK: RK4 28 KB (5 filters per CU), Dormand-Prince 34 KB (4)
  const size_t lds = (size_t)(2 * 529 + 3 * 207 + 3 * 144 + 2 + 36 + NS * (36 + 207)) * sizeof(double);
  hipLaunchKernelGGL(propagate_state_wave_kernel<NS>, dim3(a.batch), dim3(64), lds, s, a);
  CHECK_LAUNCH();
}
size_t propagate_calib_lds(int nm, int ns) {
  const size_t NN = (size_t)nm * nm, NF = 9 * (size_t)nm;
  return ((2 + ns) * NN + (6 + ns) * NF + 432 + 64 + 24 + (size_t)ns * 60) * sizeof(double);
}
template <int NS>
static int launch_propagate_state_calib_ns(const PropStateArgs& a, hipStream_t s) {
  const size_t lds = propagate_calib_lds(a.nm, NS);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&propagate_state_calib_kernel<NS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  hipLaunchKernelGGL(propagate_state_calib_kernel<NS>, dim3(a.batch), dim3(256), lds, s, a);
  return (int)hipGetLastError();
}
int launch_propagate_state_calib(const PropStateArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  if (a.nm < 23 || a.nm > 40 || !a.calib) return (int)hipErrorInvalidValue;
  return a.method ? launch_propagate_state_calib_ns<7>(a, s) : launch_propagate_state_calib_ns<4>(a, s);
}

int launch_propagate_state(const PropStateArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  return a.method ? launch_propagate_state_wave<7>(a, s) : launch_propagate_state_wave<4>(a, s);
}

}  // namespace xivo_hip
