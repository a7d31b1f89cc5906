// Feature-level kernels of the EKF update (gfx950), driven by capi_glevel.hip: Jacobians, stacking, OOS and
// loop-closure rows, OOS compression, Givens / QR and OnePointRANSAC. (The MH gates: gate_kernels.hip.)
//
//  jac_instate_kernel   Feature::ComputeJacobian           src/feature.cpp:542-656
//  stack_kernel         FilterUpdate stacking + Feature::FillJacobianBlock
//                                                          src/update.cpp:129-138, src/feature.cpp:658-684
//  oos_kernel           ComputeOOSJacobian(+Internal) + SlowGivens
//                                                          src/oos.cpp:8-89, src/helpers.cpp:13-23
//  lc_rows_kernel       Feature::ComputeLCJacobian as Estimator::CloseLoopInternal stacks it
//                                                          src/oos.cpp:92-145, src/update.cpp:183-196
//  oos_compress_kernel<RW, CPL>  xivo::QR measurement compression
//                                                          src/estimator.h:399-402, src/helpers.cpp:77-101
//  givens_kernel        xivo::Givens / xivo::QR            src/helpers.cpp:27-101
//  ransac_select_kernel Estimator::OnePointRANSAC: low-innovation set   src/update.cpp:238-265
//  ransac_zero_kernel   the same: P rows / columns zeroed               src/update.cpp:299-316
//  ransac_rescue_kernel, ransac_rescue_dist_kernel  the same: rescue    src/update.cpp:343-369
// (paths relative to the reference tree). Tiny per-feature 3x3 chains: one thread / one wave64 per feature, wave
// reductions for the chi-square gating, no MFMA.
#include <cstdio>

#include "ekf_kernels.h"
#include "camera_device.h"
#include "feature_chi2_device.h"
#include "geometry_device.h"

namespace xivo_hip {

namespace {

// ---------------------------------------------------------------- in-state Jacobian
// One thread per (filter, feature). Output J is 2 x 21 row-major with block
// order [Wsb Tsb Wbc Tbc Wsbr Tsbr x] (the 7 structural non-zero blocks of
// Feature::J_, feature.cpp:623-645).
__global__ void jac_instate_kernel(SceneBuffers sb, xivo_layout lay, xivo_cam cam_ctx, int batch) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch * sb.F) return;
  const int filt = t / sb.F, f = t % sb.F;
  const xivo_cam cam = filter_cam(cam_ctx, sb.calib, sb.cl.cam_dim, filt);
  const xivo_pose_in& pose = sb.poses[filt];
  const xivo_feat_in& ft = sb.feats[(long)filt * sb.Fmax + f];
  if (ft.sind < 0) {   // absent entry (ragged batches): no Jacobian, no innovation
    double* J0 = sb.J + ((long)filt * sb.Fmax + f) * 42;
    for (int i = 0; i < 42; ++i) J0[i] = 0.0;
    sb.finn[((long)filt * sb.Fmax + f) * 2] = 0.0;
    sb.finn[((long)filt * sb.Fmax + f) * 2 + 1] = 0.0;
    if (sb.Jc) { double* Jc0 = sb.Jc + ((long)filt * sb.Fmax + f) * 44; for (int i = 0; i < 44; ++i) Jc0[i] = 0.0; }
    return;
  }
  const xivo_group_in& grp = sb.groups[(long)filt * lay.n_groups + ft.ref_sind];

  const M3 Rsb = m3_from_colmajor(pose.Rsb), Rbc = m3_from_colmajor(pose.Rbc);
  const M3 Rsb_t = m3_t(Rsb), Rbc_t = m3_t(Rbc);
  const M3 Rsbr = m3_from_colmajor(grp.Rsb);
  const V3 Tsb{{pose.Tsb[0], pose.Tsb[1], pose.Tsb[2]}}, Tbc{{pose.Tbc[0], pose.Tbc[1], pose.Tbc[2]}};
  const V3 Tsbr{{grp.Tsb[0], grp.Tsb[1], grp.Tsb[2]}};

  // Xc = this->Xc(&dXc_dx) (feature.cpp:98-105, :555)
  M3 dXc_dx;
  const V3 Xc = feature_unproject(ft.x, sb.invdepth, dXc_dx);

  // feature.cpp:556-560
  V3 Xbr = m3_mulv(Rbc, Xc);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xbr.v[i] += Tbc.v[i];
  V3 Xs = m3_mulv(Rsbr, Xbr);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xs.v[i] += Tsbr.v[i];
  V3 dXs;
#pragma unroll
  for (int i = 0; i < 3; ++i) dXs.v[i] = Xs.v[i] - Tsb.v[i];
  const V3 Xb = m3_mulv(Rsb_t, dXs);
  V3 dXb;
#pragma unroll
  for (int i = 0; i < 3; ++i) dXb.v[i] = Xb.v[i] - Tbc.v[i];
  const V3 Xcn = m3_mulv(Rbc_t, dXb);

  // feature.cpp:563-590 (products associated left to right as Eigen does)
  const M3 dXbr_dWbc = m3_mul(m3_neg(Rbc), hat(Xc));
  const M3 dXs_dWsbr = m3_mul(m3_neg(Rsbr), hat(Xbr));
  const M3 dXb_dWsb = hat(Xb);
  const M3 dXcn_dXs = m3_mul(Rbc_t, Rsb_t);                 // dXcn_dXb * dXb_dXs
  const M3 dXcn_dXbr = m3_mul(dXcn_dXs, Rsbr);              // ... * dXs_dXbr
  const M3 dXcn_dTbc = m3_add(m3_neg(Rbc_t), dXcn_dXbr);    // :579-580 (dXbr_dTbc = I)
  const M3 dXcn_dWbc = m3_add(hat(Xcn), m3_mul(dXcn_dXbr, dXbr_dWbc));  // :581-582
  const M3 dXcn_dTsb = m3_mul(Rbc_t, m3_neg(Rsb_t));        // :585
  const M3 dXcn_dWsb = m3_mul(Rbc_t, dXb_dWsb);             // :586
  const M3 dXcn_dTsbr = dXcn_dXs;                           // :587 (dXs_dTsbr = I)
  const M3 dXcn_dWsbr = m3_mul(dXcn_dXs, dXs_dWsbr);        // :588
  const M3 dXcn_dx = m3_mul(m3_mul(dXcn_dXbr, Rbc), dXc_dx);  // :590

  double xp[2], dxp_dXcn[2][3];
  project_pixel(cam, Xcn, xp, dxp_dXcn);

  if (sb.Jc) {   // online-calibration builds: the td / Cg / bg / intrinsics blocks (feature.cpp:592-609, :611-618, :632-651)
    double* Jc = sb.Jc + ((long)filt * sb.Fmax + f) * 44;
    for (int i = 0; i < 44; ++i) Jc[i] = 0.0;
    if (sb.cl.td >= 0) {
      const xivo_calib_in& cb = sb.calib[filt];
      const M3 Cg = m3_from_colmajor(cb.Cg);
      const V3 gyro{{cb.gyro[0], cb.gyro[1], cb.gyro[2]}};
      V3 gyro_calib = m3_mulv(Cg, gyro);                                   // :593  Cg * gyro - bg
#pragma unroll
      for (int i = 0; i < 3; ++i) gyro_calib.v[i] -= pose.bg[i];
      const V3 Vsb{{pose.Vsb[0], pose.Vsb[1], pose.Vsb[2]}};
      // dXcn_dtd = -Rbc_t * (hat(gyro_calib) * Rsb_t * (Xs - Tsb) + Rsb_t * Vsb)          :594-595
      const V3 u1 = m3_mulv(m3_mul(hat(gyro_calib), Rsb_t), dXs);
      const V3 u2 = m3_mulv(Rsb_t, Vsb);
      V3 u;
#pragma unroll
      for (int i = 0; i < 3; ++i) u.v[i] = u1.v[i] + u2.v[i];
      const V3 dXcn_dtd = m3_mulv(m3_neg(Rbc_t), u);
      // dXcn_dW = dAB_dB<3,1>(Rbc_t * hat(Rsb_t * (Xs - Tsb)) * td) = that 3 x 3 matrix     :598-599
      M3 dXcn_dW = m3_mul(Rbc_t, hat(m3_mulv(Rsb_t, dXs)));
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dXcn_dW.m[i][j] *= cb.td;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        Jc[i * 22 + 0] = dxp_dXcn[i][0] * dXcn_dtd.v[0] + dxp_dXcn[i][1] * dXcn_dtd.v[1] + dxp_dXcn[i][2] * dXcn_dtd.v[2];   // :632
        double jw[3];                                                      // dxp_dXcn * dXcn_dW
#pragma unroll
        for (int j = 0; j < 3; ++j) jw[j] = dxp_dXcn[i][0] * dXcn_dW.m[0][j] + dxp_dXcn[i][1] * dXcn_dW.m[1][j] + dxp_dXcn[i][2] * dXcn_dW.m[2][j];
        // dXcn_dCg = dXcn_dW * dW_dCg, dW_dCg row k = gyro at columns 3k..3k+2 (:601-605): column 3k + j = dXcn_dW[:, k] * gyro[j]
        if (sb.cl.Cg >= 0)
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              double acc = 0.0;                                            // (the product as Eigen forms it: dxp_dXcn * (dXcn_dW * dW_dCg))
#pragma unroll
              for (int q = 0; q < 3; ++q) acc += dxp_dXcn[i][q] * (dXcn_dW.m[q][k] * gyro.v[j]);
              Jc[i * 22 + 1 + 3 * k + j] = acc;
            }
#pragma unroll
        for (int j = 0; j < 3; ++j) Jc[i * 22 + 10 + j] = -jw[j];          // dXcn_dbg = -dXcn_dW (:607, :636)
      }
    }
    if (sb.cl.cam_dim > 0) {                                               // :611-618, :647-651
      double xq[2], Jq[2][2], jacc[2][9];
      const double xcn0 = Xcn.v[0] / Xcn.v[2], xcn1 = Xcn.v[1] / Xcn.v[2];
      camera_project_jacc(cam, xcn0, xcn1, xq, Jq, jacc);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < sb.cl.cam_dim && j < 9; ++j) Jc[i * 22 + 13 + j] = jacc[i][j];
    }
  }

  double blk[7][2][3];
  m23_mul(dxp_dXcn, dXcn_dWsb, blk[0]);
  m23_mul(dxp_dXcn, dXcn_dTsb, blk[1]);
  m23_mul(dxp_dXcn, dXcn_dWbc, blk[2]);
  m23_mul(dxp_dXcn, dXcn_dTbc, blk[3]);
  m23_mul(dxp_dXcn, dXcn_dWsbr, blk[4]);
  m23_mul(dxp_dXcn, dXcn_dTsbr, blk[5]);
  m23_mul(dxp_dXcn, dXcn_dx, blk[6]);

  double* J = sb.J + ((long)filt * sb.Fmax + f) * 42;
#pragma unroll
  for (int b = 0; b < 7; ++b)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) J[i * 21 + 3 * b + j] = blk[b][i][j];
  double* inn = sb.finn + ((long)filt * sb.Fmax + f) * 2;
  inn[0] = ft.xp[0] - xp[0];   // feature.cpp:654-655
  inn[1] = ft.xp[1] - xp[1];
}

// Stack H (and H^T), inn, diagR for one filter: rows 2f, 2f+1 belong to feature
// f; a rejected feature keeps its two rows but they are neutral (H row = 0,
// inn = 0, diagR = 1), which is algebraically the reference's "row not stacked".
__global__ __launch_bounds__(256) void stack_kernel(StackArgs a) {
  const int filt = blockIdx.x, tid = threadIdx.x;
  const SceneBuffers& sb = a.sb;
  double* H = a.mb.H + (long)filt * a.mb.strideH;
  double* HT = a.mb.HT + (long)filt * a.mb.strideHT;
  // H_.setZero(total_size, N) (update.cpp:130)
  if (a.write_dense) {
    // (a.mb.HT == nullptr: the consumer never reads the transposed copy - the re-associated dense pipeline)
    if (a.mb.ldh == a.Mp && a.mb.ldht == a.Np) {
      // both copies are contiguous Mp x Np blocks (multiples of 16 doubles): one flat pass of 16-byte stores each
      d2* h2 = reinterpret_cast<d2*>(H);
      d2* t2 = reinterpret_cast<d2*>(HT);
      const long n2 = (long)a.Mp * a.Np / 2;
      if (a.mb.HT) for (long e = tid; e < n2; e += 256) { h2[e] = d2{0.0, 0.0}; t2[e] = d2{0.0, 0.0}; }
      else for (long e = tid; e < n2; e += 256) h2[e] = d2{0.0, 0.0};
    } else {
      for (int n = 0; n < a.Np; ++n)
        for (int m = tid; m < a.Mp; m += 256) H[m + (long)n * a.mb.ldh] = 0.0;
      if (a.mb.HT)
        for (int m = 0; m < a.Mp; ++m)
          for (int n = tid; n < a.Np; n += 256) HT[n + (long)m * a.mb.ldht] = 0.0;
    }
  }
  double* inn = a.mb.inn + (long)filt * a.mb.strideInn;
  double* dR = a.mb.diagR + (long)filt * a.mb.strideR;
  for (int m = tid; m < a.Mp; m += 256) { inn[m] = 0.0; dR[m] = 1.0; }
  __syncthreads();
  const double R = a.tune_R ? a.tune_R[filt] : a.R;   // (tuning table: the filter's own)
  for (int f = tid; f < sb.F; f += 256) {
    if (!sb.mask[(long)filt * sb.Fmax + f]) continue;
    const xivo_feat_in& ft = sb.feats[(long)filt * sb.Fmax + f];
    const double* J = sb.J + ((long)filt * sb.Fmax + f) * 42;
    const double* fi = sb.finn + ((long)filt * sb.Fmax + f) * 2;
    for (int b = 0; b < 7; ++b) {
      // Feature::FillJacobianBlock: the group-rotation block is overwritten by the
      // group-translation block and goff+3.. stays zero (feature.cpp:675-676)
      int src = b;
      if (!a.fix_group_block) {
        if (b == 4) src = 5;
        else if (b == 5) continue;
      }
      for (int o = 0; o < 3; ++o) {
        const int col = jcol(a.lay, ft, 3 * b + o);
        for (int i = 0; i < 2; ++i) {
          const double v = J[i * 21 + 3 * src + o];
          if (!a.write_dense) continue;
          H[(2 * f + i) + (long)col * a.mb.ldh] = v;
          if (a.mb.HT) HT[col + (long)(2 * f + i) * a.mb.ldht] = v;
        }
      }
    }
    if (sb.Jc && a.write_dense) {   // online-calibration builds: Feature::FillJacobianBlock :664-670, :679-683
      const double* Jc = sb.Jc + ((long)filt * sb.Fmax + f) * 44;
      auto put = [&](int col, int i, double v) {
        H[(2 * f + i) + (long)col * a.mb.ldh] = v;
        if (a.mb.HT) HT[col + (long)(2 * f + i) * a.mb.ldht] = v;
      };
      for (int i = 0; i < 2; ++i) {
        if (sb.cl.td >= 0) {
          put(sb.cl.td, i, Jc[i * 22]);
          if (sb.cl.Cg >= 0) for (int j = 0; j < 9; ++j) put(sb.cl.Cg + j, i, Jc[i * 22 + 1 + j]);
          for (int j = 0; j < 3; ++j) put(9 + j, i, Jc[i * 22 + 10 + j]);          // Index::bg
        }
        for (int j = 0; j < sb.cl.cam_dim && j < 9; ++j) put(sb.cl.cam_begin + j, i, Jc[i * 22 + 13 + j]);
      }
    }
    inn[2 * f] = fi[0]; inn[2 * f + 1] = fi[1];      // update.cpp:136
    dR[2 * f] = R; dR[2 * f + 1] = R;                // update.cpp:137
  }
  if (tid == 0 && a.rows_instate) a.rows_instate[filt] = 2 * sb.F;
  if (!a.emit_ell) return;
  // row-pair compressed form: the 12 sensor pose / extrinsics columns are the common slots, the
  // group and feature blocks the private ones (ell.h)
  int* eidx = a.ell.idx + (long)filt * a.ell.stride_idx();
  double* eval = a.ell.val + (long)filt * a.ell.stride_val();
  // (calibration blocks: dense rows - or, with a.lead, the "leading dense block" next to compressed rows)
  if (tid == 0) { a.ell.nc[filt] = 12; a.ell.over[filt] = (sb.Jc && !a.lead) ? 1 : 0; a.ell.pw[filt] = a.fix_group_block ? 9 : 6; }
  if (sb.Jc && a.lead) {
    // Online-calibration builds on the sparse pipeline: the td / Cg / bg / intrinsics blocks of FillJacobianBlock
    // (feature.cpp:664-670, :679-683) are columns EVERY row pair shares - more of them than the compressed form has common
    // slots - and all lie in the leading lead_k state columns: they go into a dense [Mp x lead_k] block of their own (zero
    // wherever the compressed rows hold the column: Wsb, Tsb, Wbc, Tbc), which the update multiplies by two skinny GEMMs
    double* L = a.lead + (long)filt * a.strideLead;
    for (int e = tid; e < a.Mp * a.lead_k; e += 256) {
      const int m = e % a.Mp, k = e / a.Mp, f = m >> 1, i = m & 1;
      double v = 0.0;
      if (f < sb.F && sb.mask[(long)filt * sb.Fmax + f]) {
        const double* Jc = sb.Jc + ((long)filt * sb.Fmax + f) * 44 + i * 22;
        if (sb.cl.td >= 0) {
          if (k == sb.cl.td) v = Jc[0];
          else if (sb.cl.Cg >= 0 && k >= sb.cl.Cg && k < sb.cl.Cg + 9) v = Jc[1 + k - sb.cl.Cg];
          else if (k >= 9 && k < 12) v = Jc[10 + k - 9];
        }
        if (k >= sb.cl.cam_begin && k < sb.cl.cam_begin + sb.cl.cam_dim) v = Jc[13 + k - sb.cl.cam_begin];
      }
      L[m + (long)k * a.Mp] = v;
    }
  }
  // one thread per (pair, slot): consecutive threads write consecutive 16-byte value slots / 4-byte index slots (a thread
  // per pair wrote 84 scalars 448 bytes apart from its neighbour's: 0.32 ms per 4096 filters, bound by the store count)
  const d2 zero2 = d2{0.0, 0.0};
  for (int e = tid; e < (a.Mp / 2) * ELL_W; e += 256) {
    const int p = e / ELL_W, t = e % ELL_W;
    const bool on = p < sb.F && sb.mask[(long)filt * sb.Fmax + p];
    const xivo_feat_in& ft = sb.feats[(long)filt * sb.Fmax + (p < sb.F ? p : 0)];
    const double* J = sb.J + ((long)filt * sb.Fmax + (p < sb.F ? p : 0)) * 42;
    int idx = 0, c = -1;        // c: compact-J column whose two values fill the slot
    if (t < 12) { idx = jcol(a.lay, ft, t); if (on) c = t; }
    else if (t >= ELL_CW && on) {
      const int k = t - ELL_CW;
      if (a.fix_group_block) { if (k < 9) { idx = jcol(a.lay, ft, 12 + k); c = 12 + k; } }
      // Feature::FillJacobianBlock as coded: the group-rotation block is overwritten by the group-translation block
      // (feature.cpp:675-676): columns of block 4 carry the values of block 5, block 5 contributes no slots
      else if (k < 3) { idx = jcol(a.lay, ft, 12 + k); c = 15 + k; }
      else if (k < 6) { idx = jcol(a.lay, ft, 15 + k); c = 15 + k; }
    }
    eidx[e] = idx;
    reinterpret_cast<d2*>(eval)[e] = c >= 0 ? d2{J[c], J[21 + c]} : zero2;
  }
}

// ---------------------------------------------------------------- OOS / MSCKF rows
// One wave64 per (filter, OOS feature). Lane 0 runs Eigen's FullPivLU on the
// 3 x 2k matrix Hf^T exactly as FullPivLU::computeInPlace / kernel() do
// (thirdparty/eigen/Eigen/src/LU/FullPivLU.h:490-580, 619-699) so that the
// null-space basis A - which is NOT orthonormal - matches SlowGivens
// (helpers.cpp:13-23) and not merely its span; lanes then form A^T Hx, A^T r.
constexpr int OOS_R = 2 * XIVO_OOS_MAX_OBS;  // max rows 2k

__global__ __launch_bounds__(64) void oos_kernel(OosArgs a) {
  const int filt = blockIdx.y, o = blockIdx.x, lane = threadIdx.x;
  const xivo_oos_in& ft = a.feats[(long)filt * a.n_oos + o];
  const xivo_pose_in& pose = a.poses[filt];
  const int k = ft.n_obs, R2 = 2 * k;
  __shared__ double sHf[OOS_R][3];
  __shared__ double sHx[OOS_R][12];   // per row: [Wg(3) Tg(3) Wbc(3) Tbc(3)]
  __shared__ double sInn[OOS_R];
  __shared__ double sA[OOS_R][OOS_R]; // kernel basis, 2k x dimker
  __shared__ int sQ[OOS_R];
  __shared__ int sRank;
  __shared__ int sRow0;

  // row offset of this feature = row0 + sum_{o' < o} (2 k_o' - 3): the reservation assumes rank(Hf) = 3. The kernel of
  // Hf^T has 2k - rank >= 2k - 3 vectors, so every reserved row is written; at rank < 3 (all observing groups at one pose)
  // only the first 2k - 3 columns of Eigen's basis fit and the last 3 - rank are dropped (include/xivo_hip.h,
  // xivo_hip_oos_project; tests/test_geometry_edges_gpu.py)
  if (lane == 0) {
    int r = a.row0;
    for (int q = 0; q < o; ++q) {
      const int kq = a.feats[(long)filt * a.n_oos + q].n_obs;
      r += kq >= 2 ? (a.whole ? a.whole - 3 : 2 * kq - 3) : 0;
    }
    sRow0 = r;
    if (o == a.n_oos - 1 && a.rows_out) a.rows_out[filt] = r + (k >= 2 ? (a.whole ? a.whole - 3 : 2 * k - 3) : 0) - a.row0;
  }
  // per-observation Jacobians (oos.cpp:39-89), one lane per observation
  if (lane < k) {
    const xivo_group_in& g = a.groups[(long)filt * a.lay.n_groups + ft.group_sind[lane]];
    const M3 Rsb = m3_from_colmajor(g.Rsb), Rbc = m3_from_colmajor(pose.Rbc);
    const M3 Rsb_t = m3_t(Rsb), Rbc_t = m3_t(Rbc);
    V3 d;
#pragma unroll
    for (int i = 0; i < 3; ++i) d.v[i] = ft.Xs[i] - g.Tsb[i];
    const V3 Xb = m3_mulv(Rsb_t, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) d.v[i] = Xb.v[i] - pose.Tbc[i];
    const V3 Xcn = m3_mulv(Rbc_t, d);
    double xp[2], dxp_dXcn[2][3];
    project_pixel(filter_cam(a.cam, a.calib, a.cam_dim, filt), Xcn, xp, dxp_dXcn);
    double t1[2][3], out[2][3];
    m23_mul(dxp_dXcn, Rbc_t, t1);                 // dxp_dXcn * dXcn_dXb
    m23_mul(t1, Rsb_t, out);                      // * dXb_dXs -> Hf        (oos.cpp:74-75)
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) sHf[2 * lane + i][j] = out[i][j];
    m23_mul(t1, hat(Xb), out);                    // * dXb_dWsb -> goff     (oos.cpp:78-79)
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) sHx[2 * lane + i][j] = out[i][j];
    m23_mul(t1, m3_neg(Rsb_t), out);              // * dXb_dTsb -> goff + 3 (oos.cpp:80-81)
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) sHx[2 * lane + i][3 + j] = out[i][j];
    m23_mul(dxp_dXcn, hat(Xcn), out);             // dXcn_dWbc              (oos.cpp:82-83)
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) sHx[2 * lane + i][6 + j] = out[i][j];
    m23_mul(dxp_dXcn, m3_neg(Rbc_t), out);        // dXcn_dTbc              (oos.cpp:84-85)
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 3; ++j) sHx[2 * lane + i][9 + j] = out[i][j];
    sInn[2 * lane] = ft.xp[lane][0] - xp[0];      // oos.cpp:72
    sInn[2 * lane + 1] = ft.xp[lane][1] - xp[1];
  }
  __syncthreads();

  // FullPivLU of Hf^T (3 x 2k) and its kernel (Eigen FullPivLU.h:446-534, 619-699; helpers.cpp:15-16), one lane per
  // column of Hf^T with the column's three entries in registers: the pivot search is a wave arg-max that keeps the
  // FIRST maximum of Eigen's column-major scan (smaller column, then smaller row), row swaps are register selects,
  // column swaps and the broadcasts of the pivot column are lane shuffles. Every arithmetic operation is the one the
  // serial algorithm performs on that element, so the basis equals Eigen's to rounding.
  {
    const int cols = R2;
    const bool incol = lane < cols;
    double c0 = incol ? sHf[lane][0] : 0.0, c1 = incol ? sHf[lane][1] : 0.0, c2 = incol ? sHf[lane][2] : 0.0;
    int q = lane;                     // m_q: position -> original column, built from the column transpositions
    int nonzero = 3;
    double maxpivot = 0.0;
    int colsT0 = 0, colsT1 = 1, colsT2 = 2;
    bool live = true;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
      if (!live) continue;
      // biggest |.| of the bottom-right corner: per lane over rows kk..2 (first maximum), then over lanes j >= kk
      double best = -1.0; int bi = kk;
      if (incol && lane >= kk) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (i < kk) continue;
          const double sv = fabs(i == 0 ? c0 : (i == 1 ? c1 : c2));
          if (sv > best) { best = sv; bi = i; }
        }
      }
      int bj = lane;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o);
        if (ob > best || (ob == best && oj < bj)) { best = ob; bi = oi; bj = oj; }
      }
      const double big = best; const int br = bi, bc = bj;     // wave-uniform
      if (big == 0.0) { nonzero = kk; live = false; continue; }   // the rest of the corner is exactly zero (FullPivLU.h:486-494)
      if (big > maxpivot) maxpivot = big;
      if (kk == 0) colsT0 = bc; else if (kk == 1) colsT1 = bc; else colsT2 = bc;
      // rows kk <-> br in every column
      if (br != kk) {
        double& a_ = kk == 0 ? c0 : (kk == 1 ? c1 : c2);
        if (br == 1) { const double t = a_; a_ = c1; c1 = t; }
        else if (br == 2) { const double t = a_; a_ = c2; c2 = t; }
      }
      // columns kk <-> bc
      if (bc != kk) {
        const int src = lane == kk ? bc : (lane == bc ? kk : lane);
        c0 = __shfl(c0, src); c1 = __shfl(c1, src); c2 = __shfl(c2, src);
        q = __shfl(q, src);
      }
      // multipliers in column kk, then the rank-1 update of the corner
      const double pk0 = __shfl(c0, kk), pk1 = __shfl(c1, kk), pk2 = __shfl(c2, kk);    // column kk as it is now
      const double piv = kk == 0 ? pk0 : (kk == 1 ? pk1 : pk2);
      double l1 = 0.0, l2 = 0.0;        // multipliers of rows 1, 2 (those below kk)
      if (kk == 0) { l1 = pk1 / piv; l2 = pk2 / piv; if (lane == 0) { c1 = l1; c2 = l2; } }
      else if (kk == 1) { l2 = pk2 / piv; if (lane == 1) c2 = l2; }
      if (lane > kk) {
        const double top = kk == 0 ? c0 : (kk == 1 ? c1 : c2);     // sLU[kk][j]
        if (kk == 0) { c1 -= l1 * top; c2 -= l2 * top; }
        else if (kk == 1) { c2 -= l2 * top; }
      }
    }
    (void)colsT0; (void)colsT1; (void)colsT2;
    if (incol) sQ[lane] = q;
    // rank with Eigen's default threshold eps * diagonalSize (FullPivLU.h threshold())
    const double thr = maxpivot * (2.220446049250313e-16 * 3);
    const double d0 = __shfl(c0, 0), d1 = __shfl(c1, 1), d2 = __shfl(c2, 2);
    int piv[3]; int np = 0;
    if (0 < nonzero && fabs(d0) > thr) piv[np++] = 0;
    if (1 < nonzero && fabs(d1) > thr) piv[np++] = 1;
    if (2 < nonzero && fabs(d2) > thr) piv[np++] = 2;
    const int rank = np, dimker = cols - rank;
    const int p0 = rank > 0 ? piv[0] : 0, p1 = rank > 1 ? piv[1] : 0, p2 = rank > 2 ? piv[2] : 0;
    if (lane == 0) sRank = rank;
    // trapezoid m (rank x cols): row i = row piv[i] of the LU with its strictly lower part zeroed (FullPivLU.h:660-672)
    auto rowsel = [&](int r) -> double { return r == 0 ? c0 : (r == 1 ? c1 : c2); };
    double m0 = rank > 0 ? rowsel(p0) : 0.0;
    double m1 = rank > 1 ? (lane < 1 ? 0.0 : rowsel(p1)) : 0.0;
    double m2 = rank > 2 ? (lane < 2 ? 0.0 : rowsel(p2)) : 0.0;
    auto swap_cols = [&](int ca, int cb) {
      if (ca == cb) return;
      const int src = lane == ca ? cb : (lane == cb ? ca : lane);
      m0 = __shfl(m0, src); m1 = __shfl(m1, src); m2 = __shfl(m2, src);
    };
    if (rank > 0) swap_cols(0, p0);
    if (rank > 1) swap_cols(1, p1);
    if (rank > 2) swap_cols(2, p2);
    // upper-triangular solve m[:, :rank] X = m[:, rank:], one lane per right-hand side
    const double u00 = __shfl(m0, 0), u01 = __shfl(m0, 1), u02 = __shfl(m0, 2), u11 = __shfl(m1, 1), u12 = __shfl(m1, 2), u22 = __shfl(m2, 2);
    if (lane >= rank && incol) {
      if (rank == 3) { m2 = m2 / u22; m1 = (m1 - u12 * m2) / u11; m0 = ((m0 - u01 * m1) - u02 * m2) / u00; }
      else if (rank == 2) { m1 = m1 / u11; m0 = (m0 - u01 * m1) / u00; }
      else if (rank == 1) { m0 = m0 / u00; }
    }
    if (rank > 2) swap_cols(2, p2);
    if (rank > 1) swap_cols(1, p1);
    if (rank > 0) swap_cols(0, p0);
    __syncthreads();                              // sQ complete
    // dst.row(q[i]) = -m.row(i).tail(dimker), rows q[rank..] zero, then the identity block (FullPivLU.h:690-697)
    if (incol && lane >= rank) {
      const int c = lane - rank;
      for (int j = 0; j < cols; ++j) sA[j][c] = 0.0;
      if (rank > 0) sA[sQ[0]][c] = -m0;
      if (rank > 1) sA[sQ[1]][c] = -m1;
      if (rank > 2) sA[sQ[2]][c] = -m2;
      sA[sQ[lane]][c] = 1.0;
    }
    (void)dimker;
  }
  __syncthreads();

  // Hx <- A^T Hx, inn <- A^T inn (helpers.cpp:20, oos.cpp:29); lane r owns output row r
  const int dimker = R2 - sRank;
  const int nrows_res = k >= 2 ? 2 * k - 3 : 0;  // rows reserved for this feature
  if (lane < nrows_res) {
    const int row = sRow0 + lane;
    double* H = a.mb.H + (long)filt * a.mb.strideH;
    double* HT = a.mb.HT + (long)filt * a.mb.strideHT;
    double* inn = a.mb.inn + (long)filt * a.mb.strideInn;
    double* dR = a.mb.diagR + (long)filt * a.mb.strideR;
    if (lane < dimker && row < a.Mp) {
      double rr = 0.0;
      for (int j = 0; j < R2; ++j) rr += sA[j][lane] * sInn[j];
      // the rows arrive zero-filled (stack). The camera-extrinsics columns collect a term from every observation: summed
      // in registers, stored once. A group block belongs to one observation - a plain store - unless the feature was
      // seen twice from the same group; only then the read-modify-write that a general accumulation needs.
      bool dup = false;
      for (int o1 = 0; o1 < k; ++o1)
        for (int o2 = o1 + 1; o2 < k; ++o2) dup = dup || ft.group_sind[o1] == ft.group_sind[o2];
      double ex[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int ob = 0; ob < k; ++ob) {
        const int goff = a.lay.group_begin + 6 * ft.group_sind[ob];
        const double a0 = sA[2 * ob][lane], a1 = sA[2 * ob + 1][lane];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double v = a0 * sHx[2 * ob][c] + a1 * sHx[2 * ob + 1][c];
          const int col = goff + c;
          if (dup) v += H[row + (long)col * a.mb.ldh];
          H[row + (long)col * a.mb.ldh] = v;
          if (a.mb.HT) HT[col + (long)row * a.mb.ldht] = v;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) ex[c] += a0 * sHx[2 * ob][6 + c] + a1 * sHx[2 * ob + 1][6 + c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int col = 15 + c;                       // Index::Wbc (15..17), Index::Tbc (18..20)
        H[row + (long)col * a.mb.ldh] = ex[c];
        if (a.mb.HT) HT[col + (long)row * a.mb.ldht] = ex[c];
      }
      inn[row] = rr;
      dR[row] = a.Roos;
    }
  }
  // src/oos.cpp:28 as coded hands SlowGivens the whole 2 kMaxGroup-row buffers: the rows behind the 2 k filled ones are zero
  // columns of Hf^T - never a pivot, never moved by a column transposition of the three pivot steps - so FullPivLU::kernel
  // appends one unit vector per such row behind the 2 k - 3 basis vectors above (checked against the oracle's
  // restatement on the padded buffers, tests/test_oos_gpu.py): zero rows of H, inn = 0, diagR = Roos
  if (a.whole && k >= 2) {
    double* inn = a.mb.inn + (long)filt * a.mb.strideInn;
    double* dR = a.mb.diagR + (long)filt * a.mb.strideR;
    for (int r = nrows_res + lane; r < a.whole - 3; r += 64) {
      const int row = sRow0 + r;
      if (row < a.Mp) { inn[row] = 0.0; dR[row] = a.Roos; }
    }
  }
}

// The fixed OOS block of the pool's MSCKF update before oos_kernel fills it: inn = 0, diagR = Roos over rows [row0, row0 + rows)
// of every filter (H arrives zero over the columns OOS rows ever touch: xivo_hip_pool_oos_project clears them)
__global__ void oos_block_init_kernel(MeasBuffers mb, int row0, int rows, double Roos, int batch) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)batch * rows) return;
  const int filt = (int)(t / rows), r = row0 + (int)(t % rows);
  mb.inn[(long)filt * mb.strideInn + r] = 0.0;
  mb.diagR[(long)filt * mb.strideR + r] = Roos;
}

// Chi-square gate of one OOS feature's projected rows, one wave64 per (filter, list position): gamma = r^T S_o^-1 r with
// S_o = H_o P H_o^T + Roos I over the feature's rr = 2k - 3 rows. H_o is non-zero only under Wbc / Tbc (15..20) and the k
// observing groups' 6-column blocks: those nc = 6 + 6k columns of the rows and that nc x nc sub-block of P are all that is read.
//   T = H_o P_sub   lane c owns column c of T: it walks column cols[c] of P once (nc loads) against the LDS copy of H_o
//   S = T H_o^T     lower triangle, one element per lane and pass, in LDS (at most 29 x 29)
//   Cholesky        right-looking in LDS by the one wave, then the forward solve on lane 0 (rr <= 29)
// A feature seen twice from one group has that block's columns once (the later copy is skipped).
// One workgroup is one wave and the 54 KB of LDS leave one of them per SIMD: fine for batch x oos_max small blocks of a few
// microseconds; the forward solve runs on lane 0 (at most 29 steps) and the S pass leaves lanes idle when rr^2 is no multiple of 64.
constexpr int OOS_G_R = 2 * XIVO_OOS_MAX_OBS - 3;    // 29 rows
constexpr int OOS_G_C = 6 + 6 * XIVO_OOS_MAX_OBS;    // 102 columns

__global__ __launch_bounds__(64) void oos_gate_kernel(OosGateArgs a) {
  const int filt = blockIdx.y, o = blockIdx.x, lane = threadIdx.x;
  const xivo_oos_in& ft = a.feats[(long)filt * a.n_oos + o];
  const int k = ft.n_obs;
  double* gamma_out = a.gamma + (long)filt * a.n_oos + o;
  if (k < 2 || k > XIVO_OOS_MAX_OBS) { if (lane == 0) *gamma_out = 0.0; return; }   // (block-uniform)
  __shared__ double sH[OOS_G_R][OOS_G_C + 1];
  __shared__ double sT[OOS_G_R][OOS_G_C + 1];
  __shared__ double sS[OOS_G_R][OOS_G_R + 1];
  __shared__ double sr[OOS_G_R];
  __shared__ int sCol[OOS_G_C];
  __shared__ int sBad;
  __shared__ double sGamma;
  const int rr = 2 * k - 3, nc = 6 + 6 * k;
  int row0 = a.row0;                                   // as oos_kernel places the features: behind those before it
  for (int q = 0; q < o; ++q) {
    const int kq = a.feats[(long)filt * a.n_oos + q].n_obs;
    row0 += kq >= 2 ? 2 * kq - 3 : 0;
  }
  if (row0 + rr > a.Mp) { if (lane == 0) *gamma_out = 0.0; return; }
  double* H = a.H + (long)filt * a.strideH;
  double* inn = a.inn + (long)filt * a.strideInn;
  const double* P = a.P + (long)filt * a.strideP;
  for (int c = lane; c < nc; c += 64) {
    int col;
    if (c < 6) col = 15 + c;
    else {
      const int ob = (c - 6) / 6, g = ft.group_sind[ob];
      col = a.lay.group_begin + 6 * g + (c - 6) % 6;
      if (g < 0 || g >= a.lay.n_groups) col = -1;
      for (int q = 0; q < ob; ++q) if (ft.group_sind[q] == g) col = -1;
    }
    sCol[c] = col;
  }
  if (lane == 0) sBad = 0;
  if (lane < rr) sr[lane] = inn[row0 + lane];
  __syncthreads();
  for (int e = lane; e < rr * nc; e += 64) {
    const int i = e % rr, c = e / rr;                  // (consecutive lanes read consecutive rows of a column)
    sH[i][c] = sCol[c] >= 0 ? H[row0 + i + (long)sCol[c] * a.ldh] : 0.0;
  }
  __syncthreads();
  for (int c = lane; c < nc; c += 64) {
    double acc[OOS_G_R];
#pragma unroll
    for (int i = 0; i < OOS_G_R; ++i) acc[i] = 0.0;
    if (sCol[c] >= 0) {
      const double* Pc = P + (long)sCol[c] * a.ldp;
      for (int d = 0; d < nc; ++d) {
        if (sCol[d] < 0) continue;
        const double p = Pc[sCol[d]];
#pragma unroll
        for (int i = 0; i < OOS_G_R; ++i) if (i < rr) acc[i] += sH[i][d] * p;
      }
    }
#pragma unroll
    for (int i = 0; i < OOS_G_R; ++i) if (i < rr) sT[i][c] = acc[i];
  }
  __syncthreads();
  for (int e = lane; e < rr * rr; e += 64) {
    const int i = e / rr, j = e % rr;
    if (j > i) continue;
    double s = 0.0;
    for (int c = 0; c < nc; ++c) s += sT[i][c] * sH[j][c];
    sS[i][j] = s + (i == j ? a.Roos : 0.0);
  }
  __syncthreads();
  for (int j = 0; j < rr; ++j) {
    const double d = sS[j][j];                         // (every lane reads the same pivot)
    if (!(d > 0.0)) { if (lane == 0) sBad = 1; break; }
    const double l = sqrt(d);
    __syncthreads();
    if (lane == 0) sS[j][j] = l;
    for (int i = j + 1 + lane; i < rr; i += 64) sS[i][j] /= l;
    __syncthreads();
    const int m = rr - j - 1;
    for (int e = lane; e < m * m; e += 64) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) sS[i][c] -= sS[i][j] * sS[c][j];
    }
    __syncthreads();
  }
  __syncthreads();
  const bool bad = sBad != 0;
  if (lane == 0) {                                     // y = L^-1 r in place, gamma = y^T y (rr <= 29 steps)
    double g = -1.0;
    if (!bad) {
      g = 0.0;
      for (int i = 0; i < rr; ++i) {
        double v = sr[i];
        for (int c = 0; c < i; ++c) v -= sS[i][c] * sr[c];
        v /= sS[i][i];
        sr[i] = v;
        g += v * v;
      }
    }
    sGamma = g;
  }
  __syncthreads();
  const double gamma = sGamma;
  const double th = a.chi2[rr];
  const bool out = bad || (th > 0.0 && gamma > th);
  if (lane == 0) {
    *gamma_out = gamma;
    if (out) atomicAdd((unsigned long long*)(a.gated + (long)filt * a.gated_stride), 1ull);
  }
  if (!out) return;
  for (int e = lane; e < rr * nc; e += 64) {
    const int i = e % rr, c = e / rr;
    if (sCol[c] >= 0) H[row0 + i + (long)sCol[c] * a.ldh] = 0.0;
  }
  if (lane < rr) inn[row0 + lane] = 0.0;
}

// ---------------------------------------------------------------- loop-closure rows
// Feature::ComputeLCJacobian (oos.cpp:92-145) as Estimator::CloseLoopInternal drives it (update.cpp:183-196): one thread per
// (filter, match). The OLD in-state feature's world position Xs = Feature::Xs(gbc) (feature.cpp:107-118: its own state and
// anchor group) is re-observed as pixel xp by the group in slot group_sind: row pair 2m, 2m+1 of a zeroed H gets
// d xp / d (Wsb_g, Tsb_g, Wbc, Tbc) [+ the intrinsics block under USE_ONLINE_CAMERA_CALIB, :125-142], inn = obs.xp - xp,
// diagR = Rlc. No block for the old feature's own state or its anchor group: as coded. feat < 0: an absent match (ragged
// batches) - a neutral row pair (H = 0, inn = 0, R = 1).
__global__ void lc_rows_kernel(LcArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.batch * a.n) return;
  const int filt = t / a.n, m = t % a.n;
  const xivo_lc_match& mt = a.matches[t];
  double* H = a.H + (long)filt * a.strideH;          // 2n x N column-major, ld = ldh, zero-filled by the caller
  double* inn = a.inn + (long)filt * a.strideV;
  double* dR = a.diagR + (long)filt * a.strideV;
  const int r0 = 2 * m;
  if (mt.feat < 0) { inn[r0] = 0.0; inn[r0 + 1] = 0.0; dR[r0] = 1.0; dR[r0 + 1] = 1.0; return; }
  const xivo_pose_in& pose = a.poses[filt];
  const xivo_feat_in& ft = a.feats[(long)filt * a.Fmax + mt.feat];
  // a matched feature that is not in the state (a free slot of a ragged batch: sind < 0) or whose anchor slot is out of range is
  // the caller's error, not an address: the pair stays neutral (the host checked feat / group_sind against the layout)
  if (ft.sind < 0 || ft.ref_sind < 0 || ft.ref_sind >= a.lay.n_groups) { inn[r0] = 0.0; inn[r0 + 1] = 0.0; dR[r0] = 1.0; dR[r0 + 1] = 1.0; return; }
  const xivo_group_in& gref = a.groups[(long)filt * a.lay.n_groups + ft.ref_sind];
  const xivo_group_in& g = a.groups[(long)filt * a.lay.n_groups + mt.group_sind];
  const xivo_cam cam = filter_cam(a.cam, a.calib, a.cl.cam_dim, filt);
  const V3 Xs = lc_world_point(pose, ft, gref, a.invdepth);
  lc_row_pair(Xs, g.Rsb, g.Tsb, a.lay.group_begin + 6 * mt.group_sind, pose, cam, a.cl.cam_begin, a.cl.cam_dim, mt.xp, a.Rlc,
              H, a.ldh, r0, inn, dR);
}

// ---------------------------------------------------------------- measurement compression of the OOS rows
// use_compression_ / compression_trigger_ratio_ (src/estimator.h:399-402) and xivo::QR (src/helpers.cpp:77-101, "QR-based
// measurement compression") are parsed / defined but never run by the reference's pipeline. Here the block of
// null-space-projected OOS rows appended under the in-state rows (rows [row0, row0 + rows_b) of the stacked H) is
// replaced by the triangular factor of its QR decomposition whenever it has more than `ratio` times as many rows as
// non-zero columns: the rows only touch the camera-extrinsics and group columns, so 7 rows per feature collapse to at
// most 6 + 6 * n_groups rows for the whole block. Orthogonal row operations with isotropic noise Roos leave the update
// (S, K, dx, P+) unchanged to rounding (tests compare against the uncompressed oracle update and check
// Hc^T Hc = H^T H, Hc^T rc = H^T r).
// One workgroup of four waves per filter: lane = candidate column (CPL columns per lane: [Wbc Tbc | group slots], the
// residual rides along as one more column), wave w keeps rows [w RW, (w + 1) RW) of its columns in registers.
// Householder reflections column by column (a column that is zero from the pivot row down is skipped), v broadcast
// from the pivot lane with v_readlane, the per-column dot products reduced over the four waves through LDS: two
// barriers per column, no dynamic register indexing (the row loops are unrolled and predicated on r >= pivot row).
template <int RW, int CPL>
__global__ __launch_bounds__(256) void oos_compress_kernel(OosCompressArgs a) {
  const int filt = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = a.rows[filt];
  const int ncand = 6 + 6 * a.lay.n_groups;            // candidate columns; column index ncand = the residual
  double* H = a.mb.H + (long)filt * a.mb.strideH;
  double* HT = a.mb.HT + (long)filt * a.mb.strideHT;
  double* inn = a.mb.inn + (long)filt * a.mb.strideInn;
  double* dR = a.mb.diagR + (long)filt * a.mb.strideR;
  __shared__ double sdot[4][64 * CPL];
  __shared__ double ssum[4], spiv[4];
  auto col_of = [&](int jj) -> int { return jj < 6 ? 15 + jj : a.lay.group_begin + (jj - 6); };
  double v[CPL][RW];
  // rows this wave holds, as a VECTOR value (a scalar one makes the compiler keep RW row predicates in SGPRs)
  int nloc;
  asm volatile("v_mov_b32 %0, %1" : "=v"(nloc) : "s"(rows - wave * RW));
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int jj = lane + 64 * q;
    // column jj of the block: contiguous over the rows (H is column-major); the residual is one more column
    const double* src = jj < ncand ? H + (a.row0 + wave * RW) + (long)col_of(jj) * a.mb.ldh : inn + (a.row0 + wave * RW);
    const bool have = jj <= ncand;
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) v[q][rr] = (have && rr < nloc) ? src[rr] : 0.0;
  }
  // trigger: rows > ratio * (non-zero candidate columns)
  __shared__ unsigned long long smask[4][CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    bool any = false;
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) any = any || v[q][rr] != 0.0;
    const unsigned long long m = __ballot(any && lane + 64 * q < ncand);
    if (lane == 0) smask[wave][q] = m;
  }
  __syncthreads();
  int nzc = 0;
#pragma unroll
  for (int q = 0; q < CPL; ++q) nzc += __popcll(smask[0][q] | smask[1][q] | smask[2][q] | smask[3][q]);
  if (!((double)rows > a.ratio * (double)nzc) || rows <= 1) {
    if (tid == 0) a.rows_out[filt] = rows;
    return;
  }
  // Per column (= per reflection) the work of a wave is two passes over its RW register rows: the dot products
  // v^T A[:, c] and the rank-1 update. Everything that depends on the row index relative to the pivot row is folded
  // into the broadcast vector the owner lane publishes in LDS (zero above the pivot row, x_p - alpha at it), so both
  // passes are ds_read (broadcast) + v_fma per row, nothing else: the kernel is bound by VALU issue.
  __shared__ double scol[4][RW];
  __shared__ double salpha[64 * CPL];
  __shared__ int spivrow[64 * CPL];
  for (int c = tid; c < 64 * CPL; c += 256) spivrow[c] = -1;
  __syncthreads();
  int p = 0;   // pivot row = number of reflections applied so far
  for (int j = 0; j < ncand && p < rows; ++j) {
    const int jl = j & 63, jq = j >> 6;
    // pivot row relative to this wave's first row, in a VECTOR register on purpose (a scalar one makes the compiler
    // keep the RW row predicates of the unrolled loop as 64-bit lane masks in SGPRs, which spill)
    int pl;
    asm volatile("v_mov_b32 %0, %1" : "=v"(pl) : "s"(p - wave * RW));
    if (lane == jl) {    // the owner lane publishes column j masked to the rows >= p, its squared norm, the pivot element
      double s = 0.0, x0 = 0.0;
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        if (q != jq) continue;
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
          const double e = rr >= pl ? v[q][rr] : 0.0;
          scol[wave][rr] = e;
          s = fma(e, e, s);
          if (rr == pl) x0 = e;
        }
      }
      ssum[wave] = s; spiv[wave] = x0;
    }
    __syncthreads();
    const double stot = ssum[0] + ssum[1] + ssum[2] + ssum[3];
    const double xp = spiv[p / RW];       // from the wave that owns row p
    if (stot == 0.0) { __syncthreads(); continue; }       // nothing from the pivot row down in this column: no reflection
    const double nrm = sqrt(stot);
    const double alpha = xp > 0.0 ? -nrm : nrm;
    const double beta = 1.0 / (stot - xp * alpha);        // H = I - beta v v^T, v = x - alpha e_p
    if (wave == p / RW && lane == jl) { scol[wave][p % RW] = xp - alpha; salpha[j] = alpha; spivrow[j] = p; }
    __syncthreads();
    double dot[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) dot[q] = 0.0;
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      const double vr = scol[wave][rr];
#pragma unroll
      for (int q = 0; q < CPL; ++q) dot[q] = fma(vr, v[q][rr], dot[q]);
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) sdot[wave][lane + 64 * q] = dot[q];
    __syncthreads();
    double w[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int c = lane + 64 * q;
      w[q] = beta * (sdot[0][c] + sdot[1][c] + sdot[2][c] + sdot[3][c]);
    }
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      const double vr = scol[wave][rr];
#pragma unroll
      for (int q = 0; q < CPL; ++q) v[q][rr] = fma(-vr, w[q], v[q][rr]);
    }
    ++p;
  }
  __syncthreads();
  // rows [0, p): the triangular factor - the reflected columns exactly (alpha on the pivot, zero below it; the
  // arithmetic leaves rounding-level residue there); rows [p, rows): exactly neutral
  int pl;
  asm volatile("v_mov_b32 %0, %1" : "=v"(pl) : "s"(p - wave * RW));
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int jj = lane + 64 * q;
    if (jj < ncand) {
      const int col = col_of(jj);
      const int prow = spivrow[jj];                       // -1: never a pivot column (zero from its turn on)
      const double al = prow >= 0 ? salpha[jj] : 0.0;
      int prl;                                            // pivot row of this column relative to the wave's rows
      asm volatile("v_mov_b32 %0, %1" : "=v"(prl) : "v"(prow - wave * RW));
      double* hd = H + (a.row0 + wave * RW) + (long)col * a.mb.ldh;
      double* ht = HT + col + (long)(a.row0 + wave * RW) * a.mb.ldht;
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        if (rr < nloc) {
          double x = rr < pl ? v[q][rr] : 0.0;
          if (prow >= 0 && rr >= prl) x = rr == prl ? al : 0.0;
          hd[rr] = x;
          if (a.mb.HT) *ht = x;
        }
        ht += a.mb.ldht;
      }
    } else if (jj == ncand) {
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        if (rr < nloc) {
          inn[a.row0 + wave * RW + rr] = rr < pl ? v[q][rr] : 0.0;
          dR[a.row0 + wave * RW + rr] = rr < pl ? a.Roos : 1.0;
        }
      }
    }
  }
  if (tid == 0) a.rows_out[filt] = p;
}

// ---------------------------------------------------------------- Givens / QR
// givens(a, b), helpers.cpp:27-46 (G&VL Alg. 5.1.3; eps = 1e-4f, common/alias.h:80): G = [c s; -s c]
__device__ __forceinline__ void givens_cs(double a, double b, double& c, double& s) {
  const double eps = (double)1e-4f;
  if (fabs(b) < eps) { c = 1.0; s = 0.0; return; }
  if (fabs(b) > fabs(a)) { const double t = -a / b; s = 1.0 / sqrt(1.0 + t * t); c = s * t; }
  else { const double t = -b / a; c = 1.0 / sqrt(1.0 + t * t); s = c * t; }
}

// One wave per problem. The rotations of one column sweep run bottom-up and each touches rows (r, r+1): every
// lane owns the matrix columns j = lane (mod 64) and carries the current row r+1 of its columns in registers,
// so within a sweep each element is loaded once and stored once, and the pivot pair (a, b) of the sweep's
// column comes from its owner lane by a shuffle - no lane ever reads what another lane wrote.
//   qr = 0  xivo::Givens: pivots from Hf [rows x nf]; rotated: Hf (all nf columns), Hx (only its first nf
//           columns - helpers.cpp:64 as coded), x; then rows 0.. are replaced by rows nf.. (helpers.cpp:69-73)
//   qr = 1  xivo::QR: pivots from Hx; rotated: Hx (all nx columns), x (helpers.cpp:78-101)
__global__ __launch_bounds__(64) void givens_kernel(GivensArgs a) {
  constexpr int MAXC = 8;                                  // column chunks of 64: nx <= 512 for QR
  const int prob = blockIdx.x, lane = threadIdx.x;
  double* x = a.x + (long)prob * a.rows;
  double* Hx = a.Hx + (long)prob * a.rows * a.nx;
  double* P = a.qr ? Hx : a.Hf + (long)prob * a.rows * a.nf;   // pivot matrix
  const int pc = a.qr ? a.nx : a.nf;                            // pivot / elimination columns
  const int rows = a.eff < 0 ? a.rows : a.eff;
  const long ld = a.rows;
  const int nchunk = (pc + 63) / 64;
  for (int c = 0; c < pc && c < rows - 1; ++c) {
    const int owner = c & 63, och = c >> 6;
    // carries: row r+1 of the columns this lane owns, in the pivot matrix and (Givens) in Hx, and of x
    double cp[MAXC], chx = 0.0, cx = 0.0;
#pragma unroll
    for (int q = 0; q < MAXC; ++q) { const int j = lane + 64 * q; cp[q] = (q < nchunk && j < pc) ? P[(rows - 1) + ld * j] : 0.0; }
    if (!a.qr && lane < a.nf && lane < a.nx) chx = Hx[(rows - 1) + ld * lane];
    if (lane == 0) cx = x[rows - 1];
    for (int r = rows - 2; r >= c; --r) {
      double pa = 0.0, pb = 0.0;
#pragma unroll
      for (int q = 0; q < MAXC; ++q) if (q == och) { pa = P[r + ld * c]; pb = cp[q]; }   // meaningful on the owner lane only
      pa = __shfl(pa, owner); pb = __shfl(pb, owner);
      double cs, sn;
      givens_cs(pa, pb, cs, sn);
      // Gt = givens(a, b)^T = [c -s; s c]:  row_r <- c row_r - s row_r+1 ;  row_r+1 <- s row_r + c row_r+1
#pragma unroll
      for (int q = 0; q < MAXC; ++q) {
        const int j = lane + 64 * q;
        if (q < nchunk && j < pc) {
          const double top = P[r + ld * j], bot = cp[q];
          P[(r + 1) + ld * j] = sn * top + cs * bot;
          cp[q] = cs * top - sn * bot;
        }
      }
      if (!a.qr && lane < a.nf && lane < a.nx) {
        const double top = Hx[r + ld * lane], bot = chx;
        Hx[(r + 1) + ld * lane] = sn * top + cs * bot;
        chx = cs * top - sn * bot;
      }
      if (lane == 0) {
        const double top = x[r], bot = cx;
        x[r + 1] = sn * top + cs * bot;
        cx = cs * top - sn * bot;
      }
    }
#pragma unroll
    for (int q = 0; q < MAXC; ++q) { const int j = lane + 64 * q; if (q < nchunk && j < pc) P[c + ld * j] = cp[q]; }
    if (!a.qr && lane < a.nf && lane < a.nx) Hx[c + ld * lane] = chx;
    if (lane == 0) x[c] = cx;
  }
  if (!a.qr) {   // strip the first nf rows (helpers.cpp:69-73); increasing r reads rows not yet overwritten
    for (int r = 0; r < rows - a.nf; ++r) {
      for (int j = lane; j < a.nx; j += 64) Hx[r + ld * j] = Hx[(r + a.nf) + ld * j];
      if (lane < a.nf) P[r + ld * lane] = P[(r + a.nf) + ld * lane];
      if (lane == 0) x[r] = x[r + a.nf];
    }
  }
}

// |res| as Eigen's res.norm() forms it (src/update.cpp:245): two rounded products, one rounded add. Contracted to a fused
// multiply-add the norm differs by one ulp on about 8 % of innovations, and a feature whose norm EQUALS ransac_thresh_ is then
// low-innovation with the contracted norm and not with this one (tests/test_gate_edges_gpu.py, the norm tie).
__device__ __forceinline__ double innovation_norm(double r0, double r1) {
#pragma clang fp contract(off)
  const double a = r0 * r0;
  const double b = r1 * r1;
  return sqrt(a + b);
}

// ---------------------------------------------------------------- Estimator::OnePointRANSAC (src/update.cpp:213-393)
// select: the low-innovation set among the MH inliers (:238-258 - the hypothesis index k is drawn but never used, so
// the maximal set is {f : |xp - Predict| < ransac_thresh_}; xp - Predict is the innovation of the Jacobian pass), the
// groups that hold one, the temporary reference group when gauge_group_ptr_ holds none (FindNewRefGroup,
// src/estimator.cpp:1394-1407: smallest summed 6 diagonal entries of P, ascending slot order) and what has to be
// zeroed in P (:299-316). state: 0 = every MH inlier is low-innovation (or there is none): nothing to do (:263-265);
// 1 = partial update + rescue; 2 = no low-innovation inlier: rescue against the prior (:287 guard).
__global__ __launch_bounds__(64) void ransac_select_kernel(RansacArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  const SceneBuffers& sb = a.sb;
  const double* P = a.P + (long)filt * a.strideP;
  unsigned long long active = 0, withlow = 0;
  int n_mh = 0, n_low = 0;
  for (int f0 = 0; f0 < sb.F; f0 += 64) {
    const int f = f0 + lane;
    bool mh = false, low = false;
    int ref = 0;
    if (f < sb.F) {
      const xivo_feat_in& ft = sb.feats[(long)filt * sb.Fmax + f];
      mh = sb.mask[(long)filt * sb.Fmax + f] && ft.sind >= 0;
      ref = mh ? ft.ref_sind : 0;
      const double r0 = sb.finn[((long)filt * sb.Fmax + f) * 2], r1 = sb.finn[((long)filt * sb.Fmax + f) * 2 + 1];
      low = mh && innovation_norm(r0, r1) < a.thresh;
      a.low[(long)filt * sb.Fmax + f] = low ? 1 : 0;
    }
    n_mh += __popcll(__ballot(mh));
    n_low += __popcll(__ballot(low));
    unsigned long long ma = mh ? 1ull << ref : 0ull, ml = low ? 1ull << ref : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      ma |= __shfl_xor(ma, o);
      ml |= __shfl_xor(ml, o);
    }
    active |= ma; withlow |= ml;
  }
  int state = 1;
  unsigned long long zg = 0;
  if (n_mh == 0 || n_low == n_mh) state = 0;
  else if (n_low == 0) state = 2;
  if (state == 1) {
    const int gauge = a.gauge ? a.gauge[filt] : -1;
    if (gauge < 0 || gauge >= 64 || !((withlow >> gauge) & 1ull)) {
      double best = __builtin_inf();
      int arg = -1;
      for (int g = 0; g < a.lay.n_groups; ++g) {                    // wave-uniform loop
        if (!((withlow >> g) & 1ull)) continue;
        const int off = a.lay.group_begin + 6 * g;
        double cov = 0.0;
        for (int i = 0; i < 6; ++i) cov += P[(off + i) + (long)(off + i) * a.ldp];
        if (cov < best) { best = cov; arg = g; }
      }
      if (arg >= 0) zg |= 1ull << arg;
    }
    zg |= active & ~withlow;
  } else {
    // nothing is updated for this filter: an all-neutral measurement set leaves P and the state untouched
    for (int f = lane; f < sb.F; f += 64) a.low[(long)filt * sb.Fmax + f] = 0;
  }
  if (lane == 0) { a.state[filt] = state; a.zero_groups[filt] = zg; }
}

// P rows / columns of the MH inliers outside the low-innovation set and of the groups named by select (:299-316)
__global__ __launch_bounds__(256) void ransac_zero_kernel(RansacArgs a, double* Pall) {
  const int filt = blockIdx.x, tid = threadIdx.x;
  if (a.state[filt] != 1) return;
  const SceneBuffers& sb = a.sb;
  double* P = Pall + (long)filt * a.strideP;
  const unsigned long long zg = a.zero_groups[filt];
  for (int g = 0; g < a.lay.n_groups; ++g) {
    if (!((zg >> g) & 1ull)) continue;
    const int off = a.lay.group_begin + 6 * g;
    for (int t = tid; t < a.Np; t += 256)
      for (int r = 0; r < 6; ++r) { P[(off + r) + (long)t * a.ldp] = 0.0; P[t + (long)(off + r) * a.ldp] = 0.0; }
  }
  for (int f = 0; f < sb.F; ++f) {
    const xivo_feat_in& ft = sb.feats[(long)filt * sb.Fmax + f];
    if (!(sb.mask[(long)filt * sb.Fmax + f] && ft.sind >= 0) || a.low[(long)filt * sb.Fmax + f]) continue;
    const int off = a.lay.feature_begin + 3 * ft.sind;
    for (int t = tid; t < a.Np; t += 256)
      for (int r = 0; r < 3; ++r) { P[(off + r) + (long)t * a.ldp] = 0.0; P[t + (long)(off + r) * a.ldp] = 0.0; }
  }
}

// rescue (:343-369): chi-square test of every MH inlier outside the low-innovation set with the Jacobians re-taken at
// the partially updated state against the partially updated P; the final inlier mask replaces the MH mask.
__global__ __launch_bounds__(256) void ransac_rescue_kernel(RansacArgs a) {
  const int filt = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneBuffers& sb = a.sb;
  const double* P = a.P + (long)filt * a.strideP;
  const int state = a.state[filt];
  __shared__ int s_rej;
  __shared__ double s_scr[4][484];   // feature_chi2_lds: the 21 x 21 sub-block of P and the two rows of J, per wave
  if (tid == 0) s_rej = 0;
  __syncthreads();
  for (int f = wave; f < sb.F; f += 4) {
    const long e = (long)filt * sb.Fmax + f;
    const xivo_feat_in& ft = sb.feats[e];
    const bool mh = sb.mask[e] && ft.sind >= 0;
    double d = 0.0;
    bool keep = mh;
    if (mh && state != 0 && !a.low_keep[e]) {
      d = feature_chi2_lds(P, a.ldp, a.lay, ft, sb.J + e * 42, sb.finn + e * 2, a.R, lane, s_scr[wave]);
      keep = d < a.chi2;
      if (!keep && lane == 0) atomicAdd(&s_rej, 1);
    }
    if (lane == 0) { a.keep[e] = keep ? 1 : 0; a.chi[e] = d; }
  }
  __syncthreads();
  if (tid == 0) a.n_rejected[filt] = s_rej;
}

// the same decision from distances that are already formed (online-calibration builds: the whole-row distances of the
// dense-row gate - J() carries the td / Cg / bg / intrinsics blocks there, which the compact 21-column form does not hold)
__global__ __launch_bounds__(256) void ransac_rescue_dist_kernel(RansacArgs a, const double* dist, int ld) {
  const int filt = blockIdx.x, tid = threadIdx.x;
  const SceneBuffers& sb = a.sb;
  const int state = a.state[filt];
  __shared__ int s_rej;
  if (tid == 0) s_rej = 0;
  __syncthreads();
  for (int f = tid; f < sb.F; f += 256) {
    const long e = (long)filt * sb.Fmax + f;
    const bool mh = sb.mask[e] && sb.feats[e].sind >= 0;
    double d = 0.0;
    bool keep = mh;
    if (mh && state != 0 && !a.low_keep[e]) {
      d = dist[(long)filt * ld + f];
      keep = d < a.chi2;
      if (!keep) atomicAdd(&s_rej, 1);
    }
    a.keep[e] = keep ? 1 : 0; a.chi[e] = d;
  }
  __syncthreads();
  if (tid == 0) a.n_rejected[filt] = s_rej;
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_jac_instate(const SceneBuffers& sb, const xivo_layout& lay, const xivo_cam& cam, int batch,
                       hipStream_t s) {
  const int tot = batch * sb.F;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(jac_instate_kernel, dim3((tot + 127) / 128), dim3(128), 0, s, sb, lay, cam, batch);
  CHECK_LAUNCH();
}
int launch_stack(const StackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(stack_kernel, dim3(a.batch), dim3(256), 0, s, a);
  CHECK_LAUNCH();
}
int launch_oos(const OosArgs& a, hipStream_t s) {
  if (a.n_oos <= 0) return 0;
  hipLaunchKernelGGL(oos_kernel, dim3(a.n_oos, a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_oos_block_init(const MeasBuffers& mb, int row0, int rows, double Roos, int batch, hipStream_t s) {
  const long tot = (long)batch * rows;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(oos_block_init_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, mb, row0, rows, Roos, batch);
  CHECK_LAUNCH();
}
int launch_oos_gate(const OosGateArgs& a, hipStream_t s) {
  if (a.n_oos <= 0 || a.batch <= 0) return 0;
  hipLaunchKernelGGL(oos_gate_kernel, dim3(a.n_oos, a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_lc_rows(const LcArgs& a, hipStream_t s) {
  const int tot = a.batch * a.n;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(lc_rows_kernel, dim3((tot + 63) / 64), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int oos_compress_pick(int n_groups, int rows_max, char* label, size_t n) {
  const int ncols = 6 + 6 * n_groups + 1;            // candidates + the residual column
  const int pick = (ncols <= 64 && rows_max <= 144) ? 0 : (ncols <= 64 && rows_max <= 256) ? 1 : (ncols <= 128 && rows_max <= 144) ? 2 : -1;
  static const char* const names[] = {"oos_compress_kernel<36,1>", "oos_compress_kernel<64,1>", "oos_compress_kernel<36,2>"};
  if (label && n) snprintf(label, n, "%s", pick < 0 ? "" : names[pick]);
  return pick;
}
int launch_oos_compress(const OosCompressArgs& a, int rows_max, hipStream_t s) {
  switch (oos_compress_pick(a.lay.n_groups, rows_max, nullptr, 0)) {
    case 0: hipLaunchKernelGGL((oos_compress_kernel<36, 1>), dim3(a.batch), dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((oos_compress_kernel<64, 1>), dim3(a.batch), dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((oos_compress_kernel<36, 2>), dim3(a.batch), dim3(256), 0, s, a); break;
    default: return -1;                               // not built for this size: the caller leaves the rows as they are
  }
  CHECK_LAUNCH();
}
int launch_givens(const GivensArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(givens_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_ransac_select(const RansacArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ransac_select_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_ransac_zero(const RansacArgs& a, double* P, hipStream_t s) {
  hipLaunchKernelGGL(ransac_zero_kernel, dim3(a.batch), dim3(256), 0, s, a, P);
  CHECK_LAUNCH();
}
int launch_ransac_rescue_dist(const RansacArgs& a, const double* dist, int ld, hipStream_t s) {
  hipLaunchKernelGGL(ransac_rescue_dist_kernel, dim3(a.batch), dim3(256), 0, s, a, dist, ld);
  CHECK_LAUNCH();
}
int launch_ransac_rescue(const RansacArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ransac_rescue_kernel, dim3(a.batch), dim3(256), 0, s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
