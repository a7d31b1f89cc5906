// The stand-alone kernels of Estimator::MHGating (src/update.cpp:50-116) on the in-state features (gfx950), one per form the
// candidate rows come in. The gate's own rules are gate_device.h; each kernel here adds how it obtains S_f.
//
//  gate_sparse_kernel   the scene's compact Jacobians (21 columns; 43 in online-calibration builds)   capi_glevel.hip
//  gate_dense_kernel    stacked dense rows and their P H^T                       capi_glevel.hip, capi_update.hip, capi_ransac.hip
//  gate_ell_kernel      compressed rows (ell.h) with S = H P H^T + diag(R) already formed             capi_update.hip
// The same gate runs inside fused_update_f64_kernel (fused_update.hip, section 3) and in the prologue of
// chol_reg_la_f64_kernel (chol_f64.hip, GATE).
#include <cstdio>

#include "ekf_kernels.h"
#include "feature_chi2_device.h"

namespace xivo_hip {

namespace {

// ---------------------------------------------------------------- compact-Jacobian gate
// One workgroup per filter (4 waves; 16 for fewer than 256 filters - latency); a wave64 per feature computes S = J P J^T + R I2
// from the 21 x 21 sub-block of P the feature touches (J is structurally
// sparse), reduces it across lanes, and the 2x2 LLT gives the Mahalanobis
// distance (feature_chi2_lds, feature_chi2_device.h). Then one wave runs the threshold-relaxation loop.
// Online-calibration builds: J() has 22 more columns EVERY feature shares - td, Cg (9), bg (3), the intrinsics (9 slots) - next
// to the 21 of the default build (src/feature.cpp:623-651); 12 of those 21 (Wsb, Tsb, Wbc, Tbc) are shared as well. The 34 x 34
// block of P on the shared columns is therefore the same for all features of a filter: the workgroup parks it in LDS once,
// and a feature gathers only its 9 private columns (group, feature) against the shared ones and themselves - 387 elements,
// seven wave-wide loads as in the default build, instead of the 43 x 43 = 1849 of a gather per feature (2.0 -> 0.46 ms per 4096
// filters x 60 features at N = 276). The sums run over the 43 columns in the order of the whole row, as before.
constexpr int WIDE_NS = 34, WIDE_NP = 9, WIDE_NC = 43;
constexpr int WIDE_X = WIDE_NS * WIDE_NP, WIDE_Y = WIDE_NP * WIDE_NP;         // P[shared, private] | P[private, private]
constexpr int WIDE_SCR = WIDE_X + WIDE_Y + 2 * WIDE_NC + 1;                   // doubles of LDS scratch per wave (474)
constexpr int WIDE_PSS = WIDE_NS * WIDE_NS;                                   // doubles of the per-filter shared block
__device__ __forceinline__ int wide_scol(const xivo_calib_layout& cl, int s) {   // state column of shared slot s
  if (s < 6) return s;                                    // Index::Wsb, Tsb
  if (s < 12) return 15 + (s - 6);                        // Index::Wbc, Tbc
  const int k = s - 12;                                   // the layout of Jc: td | Cg 9 | bg 3 | intrinsics 9
  if (k == 0) return cl.td >= 0 ? cl.td : 0;              // (a block that is switched off carries zeros in Jc: any valid column will do)
  if (k < 10) return cl.Cg >= 0 ? cl.Cg + (k - 1) : 0;
  if (k < 13) return 9 + (k - 10);                        // Index::bg
  return (k - 13) < cl.cam_dim ? cl.cam_begin + (k - 13) : 0;
}
__device__ __forceinline__ double feature_chi2_wide(const double* P, int ldp, const xivo_layout& lay, const xivo_calib_layout& cl,
                                                    const xivo_feat_in& ft, const double* J, const double* Jc, const double* inn, double R,
                                                    int lane, const double* sPss, double* scratch) {
  double* X = scratch;                        // [s + 34 p] = P[shared s, private p]
  double* Y = scratch + WIDE_X;               // [p + 9 q]
  double* sJ = scratch + WIDE_X + WIDE_Y;     // [row * 43 + w], w in the order of the whole row: 12 common | 9 private | 22 calibration
  auto pcol = [&](int q) -> int { return q < 6 ? lay.group_begin + 6 * ft.ref_sind + q : lay.feature_begin + 3 * ft.sind + (q - 6); };
  double pv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int e = lane + 64 * k;
    int row = 0, col = 0;
    if (e < WIDE_X) { row = wide_scol(cl, e % WIDE_NS); col = pcol(e / WIDE_NS); }
    else if (e < WIDE_X + WIDE_Y) { const int q = e - WIDE_X; row = pcol(q % WIDE_NP); col = pcol(q / WIDE_NP); }
    pv[k] = P[row + (long)col * ldp];
  }
  double j0 = 0.0, j1 = 0.0;
  if (lane < WIDE_NC) { j0 = lane < 21 ? J[lane] : Jc[lane - 21]; j1 = lane < 21 ? J[21 + lane] : Jc[22 + lane - 21]; }
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int e = lane + 64 * k;
    if (e < WIDE_X + WIDE_Y) scratch[e] = pv[k];
  }
  if (lane < WIDE_NC) { sJ[lane] = j0; sJ[WIDE_NC + lane] = j1; }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  double v0 = 0.0, v1 = 0.0;
  if (lane < WIDE_NC) {
    // lane a of the whole row: shared (a < 12 or a >= 21: slot a or a - 9) or private (slot a - 12)
    const bool ash = lane < 12 || lane >= 21;
    const int as = lane < 12 ? lane : lane - 9, ap = lane - 12;
    const double* ps = ash ? sPss + as : X + WIDE_NS * ap;   // P[a, shared b]: step over b
    const int ss = ash ? WIDE_NS : 1;
    const double* pp = ash ? X + as : Y + ap;                // P[a, private b]
    const int sp = ash ? WIDE_NS : WIDE_NP;
    for (int b = 0; b < 12; ++b) { const double p = ps[b * ss]; v0 = fma(p, sJ[b], v0); v1 = fma(p, sJ[WIDE_NC + b], v1); }
    for (int b = 12; b < 21; ++b) { const double p = pp[(b - 12) * sp]; v0 = fma(p, sJ[b], v0); v1 = fma(p, sJ[WIDE_NC + b], v1); }
    for (int b = 21; b < WIDE_NC; ++b) { const double p = ps[(b - 9) * ss]; v0 = fma(p, sJ[b], v0); v1 = fma(p, sJ[WIDE_NC + b], v1); }
  }
  __builtin_amdgcn_wave_barrier();
  return gate_dist(wave_sum(j0 * v0), wave_sum(j1 * v0), wave_sum(j1 * v1), R, inn[0], inn[1]);
}

__global__ __launch_bounds__(1024) void gate_sparse_kernel(GateArgs a) {
  const int filt = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;   // 4 waves per filter for a big batch, 16 when few filters must finish fast
  extern __shared__ double sdist[];
  const SceneBuffers& sb = a.sb;
  const double* P = a.P + (long)filt * a.strideP;
  __shared__ int s_present;
  // the two slot indices of every entry, parked in LDS by the counting pass: the per-feature loop below then starts its gathers
  // of P and J right away instead of behind a load of the entry (two dependent memory round trips per feature, fifteen
  // features per wave one after the other, were what the kernel's time was)
  int* s_slot = reinterpret_cast<int*>(sdist + sb.F + 1);   // [2 F]: sind, ref_sind
  double* s_pss = sdist + sb.F + 1 + (2 * sb.F + 1) / 2;    // online-calibration builds: P on the 34 shared columns
  double* s_scr = s_pss + (sb.Jc ? WIDE_PSS : 0) + (long)wave * (sb.Jc ? WIDE_SCR : 484);   // per wave: feature_chi2_lds / _wide scratch
  if (sb.Jc && a.use_gating) {
    for (int e = tid; e < WIDE_PSS; e += nt) s_pss[e] = P[wide_scol(sb.cl, e % WIDE_NS) + (long)wide_scol(sb.cl, e / WIDE_NS) * a.ldp];
  }
  const int present = gate_count_present(sb.feats + (long)filt * sb.Fmax, sb.F, &s_present, s_slot, tid, nt);
  const bool gating = a.use_gating && present > a.gp.min_inliers;
  double th = 1.0;
  if (gating) {
    // tuning table: the filter's own R and threshold, a load every lane shares; the same operands of the same expressions
    GateParams gp = a.gp;
    if (a.tune_R) { gp.R = a.tune_R[filt]; gp.thresh = a.tune_thresh[filt]; }
    for (int f = wave; f < sb.F; f += nw) {
      xivo_feat_in ft;                      // only the slots are read by feature_chi2 / jcol
      ft.sind = s_slot[2 * f]; ft.ref_sind = s_slot[2 * f + 1];
      if (ft.sind < 0) { if (lane == 0) sdist[f] = __builtin_inf(); continue; }
      const double* J = sb.J + ((long)filt * sb.Fmax + f) * 42;
      const double* inn = sb.finn + ((long)filt * sb.Fmax + f) * 2;
      const double d = sb.Jc ? feature_chi2_wide(P, a.ldp, a.lay, sb.cl, ft, J, sb.Jc + ((long)filt * sb.Fmax + f) * 44, inn, gp.R, lane, s_pss, s_scr)
                             : feature_chi2_lds(P, a.ldp, a.lay, ft, J, inn, gp.R, lane, s_scr);
      if (lane == 0) sdist[f] = d;
    }
    th = gate_threshold(sdist, sb.F, wave, lane, [&] { return relax_threshold(sdist, sb.F, gp, lane, present); });
  } else {
    // (not gating: present entries carry 0, absent ones +inf - any positive threshold keeps exactly the present ones; every
    //  thread reads back below what it wrote here)
    for (int f = tid; f < sb.F; f += nt) sdist[f] = s_slot[2 * f] >= 0 ? 0.0 : __builtin_inf();
  }
  for (int f = tid; f < sb.F; f += nt)
    gate_verdict(sdist, f, th, sb.mask, sb.dist, (long)filt * sb.Fmax + f, gating && s_slot[2 * f] >= 0);
}

// ---------------------------------------------------------------- dense-row gate
__global__ __launch_bounds__(256) void gate_dense_kernel(GateDenseArgs a) {
  const int filt = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  extern __shared__ double sdist[];  // F doubles + 1
  double* inn = a.inn + (long)filt * a.strideInn;
  // S_f = (HP)_f H_f^T + R I2 from the TRANSPOSED copies (P H^T and H^T are [Np x Mp] with
  // the state index contiguous), so every lane streams four contiguous columns.
  const double* PHT = a.PHTr + (long)filt * a.strideHT;
  const double* HT = a.HTw + (long)filt * a.strideHT;
  // ragged batches (a.feats given): absent entries (sind < 0) were stacked as zero rows; they are no candidates - distance
  // +inf, never an inlier, not counted - and a filter gates only with more than min_inliers present entries, exactly as
  // gate_sparse_kernel does (src/manager.cpp:635)
  __shared__ int s_present;
  const xivo_feat_in* feats = a.feats ? a.feats + (long)filt * a.Fmax : nullptr;
  const int present = feats ? gate_count_present(feats, a.F, &s_present, nullptr, tid, 256) : a.F;
  const bool gating = !feats || present > a.gp.min_inliers;
  for (int f = wave; f < a.F; f += 4) {
    const bool here = !feats || feats[f].sind >= 0;
    if (!here || !gating) { if (lane == 0) sdist[f] = here ? 0.0 : __builtin_inf(); continue; }
    double s00 = 0, s10 = 0, s11 = 0;
    const double* p0 = PHT + (long)(2 * f) * a.ldht;
    const double* p1 = p0 + a.ldht;
    const double* h0 = HT + (long)(2 * f) * a.ldht;
    const double* h1 = h0 + a.ldht;
    for (int n = lane; n < a.Np; n += 64) {
      const double hp0 = p0[n], hp1 = p1[n], hh0 = h0[n], hh1 = h1[n];
      s00 = fma(hp0, hh0, s00);
      s10 = fma(hp1, hh0, s10);
      s11 = fma(hp1, hh1, s11);
    }
    s00 = wave_sum(s00); s10 = wave_sum(s10); s11 = wave_sum(s11);
    if (lane == 0) sdist[f] = gate_dist(s00, s10, s11, a.gp.R, inn[2 * f], inn[2 * f + 1]);
  }
  // (not gating: present entries carry 0, absent ones +inf - any positive threshold keeps exactly the present ones)
  // (no_relax: a plain chi-square test against thresh - the rescue pass of OnePointRANSAC, update.cpp:352-356)
  const double th = gate_threshold(sdist, a.F, wave, lane, [&] {
    return gating ? (a.no_relax ? a.gp.thresh : relax_threshold(sdist, a.F, a.gp, lane, present)) : 1.0;
  });
  const long row = (long)filt * (a.mask_ld ? a.mask_ld : a.F);   // of mask / dist
  double* dr = a.diagR + (long)filt * a.strideR;
  for (int f = tid; f < a.F; f += 256) {
    if (gate_verdict(sdist, f, th, a.mask, a.dist, row + f, gating && sdist[f] != __builtin_inf())) continue;
    if (a.have_ell) gate_reject_pair(inn, dr, f, a.ell.val + (long)filt * a.ell.stride_val() + (long)f * ELL_W * 2, 2 * ELL_W);
    else gate_reject_pair(inn, dr, f);
  }
  // neutralise rejected rows of H / H^T (and of H P / P H^T where the caller goes on with them)
  double* Hw = a.Hw + (long)filt * a.strideH;
  double* HTw = a.HTw + (long)filt * a.strideHT;
  double* HPw = a.HPw ? a.HPw + (long)filt * a.strideHP : nullptr;
  double* PHTw = a.HPw ? a.PHTw + (long)filt * a.strideHT : nullptr;
  for (int f = 0; f < a.F; ++f) {
    if (gate_inlier(sdist, f, th)) continue;
    gate_zero_rows(Hw, a.ldh, HTw, a.ldht, f, a.Np, tid, 256);
    if (HPw) gate_zero_rows(HPw, a.ldhp, PHTw, a.ldht, f, a.Np, tid, 256);
  }
}

// ---------------------------------------------------------------- gating on ELL rows
// S = H P H^T + diag(R) of ALL candidate rows is formed (ell<S>): the 2 x 2 blocks S_f are read off its diagonal - from the
// compact copy the S kernel left (Sdiag) or from S itself - and the rows / columns of the rejected pairs are then decoupled
// in S in place (0, unit diagonal)
__global__ __launch_bounds__(1024) void gate_ell_kernel(GateEllArgs a) {
  extern __shared__ double sdist[];  // F doubles + 1; 256 threads for a big batch, 1024 when few filters must finish fast
  const int filt = blockIdx.x;
  const int nt = blockDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* val = a.ell.val + (long)filt * a.ell.stride_val();
  double* PHT = a.PHT + (long)filt * a.strideHT;
  double* inn = a.inn + (long)filt * a.strideInn;
  double* dr = a.diagR + (long)filt * a.strideR;
  double* Sm = a.S + (long)filt * a.strideS;
  for (int f = tid; f < a.F; f += nt) {
    const double* sd = a.Sdiag ? a.Sdiag + (long)filt * a.strideSdiag + 4 * f : nullptr;   // [row in block][column in block]
    sdist[f] = gate_dist_S(sd ? sd[0] : Sm[2 * f + (long)(2 * f) * a.lds], sd ? sd[2] : Sm[2 * f + 1 + (long)(2 * f) * a.lds],
                           sd ? sd[3] : Sm[2 * f + 1 + (long)(2 * f + 1) * a.lds], dr[2 * f], dr[2 * f + 1], a.gp.R,
                           inn[2 * f], inn[2 * f + 1]);
  }
  const double th = gate_threshold(sdist, a.F, wave, lane, [&] { return relax_threshold(sdist, a.F, a.gp, lane); });
  for (int f = tid; f < a.F; f += nt)
    if (!gate_verdict(sdist, f, th, a.mask, a.dist, (long)filt * a.F + f))
      gate_reject_pair(inn, dr, f, val + (long)f * ELL_W * 2, 2 * ELL_W);
  double* H = a.H ? a.H + (long)filt * a.strideH : nullptr;       // dense copies, when they are materialised
  double* HT = a.HT ? a.HT + (long)filt * a.strideHT : nullptr;
  for (int f = 0; f < a.F; ++f) {
    if (gate_inlier(sdist, f, th)) continue;
    if (H) gate_zero_rows(H, a.ldh, HT, a.ldht, f, a.Np, tid, nt);
    gate_zero_rows(PHT, a.ldht, f, a.Np, tid, nt);
    for (int jx = tid; jx < a.Mp; jx += nt) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = 2 * f + i;
        Sm[r + (long)jx * a.lds] = 0.0;
        Sm[jx + (long)r * a.lds] = 0.0;
      }
    }
  }
  __syncthreads();
  for (int f = tid; f < a.F; f += nt) {
    if (gate_inlier(sdist, f, th)) continue;
    Sm[2 * f + (long)(2 * f) * a.lds] = 1.0;
    Sm[2 * f + 1 + (long)(2 * f + 1) * a.lds] = 1.0;
  }
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

// distances + threshold | slot indices | per-wave scratch of feature_chi2_lds (64 KB without an opt-in: fewer waves if F is large)
static size_t gate_sparse_lds(int F, int wide, int nt) {
  const size_t scr = wide ? WIDE_SCR : 484, pss = wide ? WIDE_PSS : 0;
  return ((size_t)(F + 1) + (2 * F + 1) / 2 + pss + (size_t)(nt / 64) * scr) * sizeof(double);
}
int gate_sparse_threads(int batch, int F, int wide, char* label, size_t n) {
  int nt = batch < 256 ? 1024 : 256;
  while (nt > 64 && gate_sparse_lds(F, wide, nt) > 65536) nt /= 2;
  if (label && n) snprintf(label, n, "gate_sparse_kernel@%d", nt);
  return nt;
}
int launch_gate_sparse(const GateArgs& a, hipStream_t s) {
  const int wide = a.sb.Jc ? 1 : 0;
  const int nt = gate_sparse_threads(a.batch, a.sb.F, wide, nullptr, 0);
  hipLaunchKernelGGL(gate_sparse_kernel, dim3(a.batch), dim3(nt), gate_sparse_lds(a.sb.F, wide, nt), s, a);
  CHECK_LAUNCH();
}
int launch_gate_dense(const GateDenseArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gate_dense_kernel, dim3(a.batch), dim3(256), (a.F + 1) * sizeof(double), s, a);
  CHECK_LAUNCH();
}
int launch_gate_ell(const GateEllArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(gate_ell_kernel, dim3(a.batch), dim3(a.batch < 256 ? 1024 : 256), (size_t)(a.F + 1) * sizeof(double), s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
