// C ABI, feature level (include/xivo_hip.h): layout, scene, calibration, Jacobians, MH gating, stacking, OOS rows, RANSAC, loop
// closure, measurement compression, filter_update, Givens / QR, sub-filter, candidate order, absorb, edits, pixels. Host-side
// orchestration only (capi_internal.h).
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

int gate_impl(xivo_hip_ctx* c, int B, double R, double th, double mult, int min_inl, int use_gating) {
  GateArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; c->P.to(a.P, a.strideP, a.ldp);
  a.R = R; a.thresh = th; a.mult = mult; a.min_inliers = min_inl; a.batch = B; a.use_gating = use_gating;
  char label[64];
  gate_sparse_threads(B, a.sb.F, a.sb.Jc ? 1 : 0, label, sizeof(label));
  StageTimer st(c, ST_GATE, 0.0, label);
  c->rows.gate_wrote(GateLayout::strided);
  return launch_gate_sparse(a, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int stack_impl(xivo_hip_ctx* c, int B, double R, int write_dense, unsigned char* mask_override = nullptr, int full_rows = 0) {
  StackArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; a.mb = meas_buffers(c);
  if (mask_override) a.sb.mask = mask_override;
  a.Mp = c->Mpmax; a.Np = c->Np; a.batch = B; a.R = R;
  a.fix_group_block = (full_rows || (c->flags & XIVO_HIP_FLAG_FIX_GROUP_BLOCK)) ? 1 : 0;
  a.rows_instate = c->rows_instate;
  a.ell = c->ell; a.emit_ell = 1; a.write_dense = write_dense;
  // as-coded stacking of an online-calibration build on the sparse pipeline: compressed rows + the leading dense block
  // (full_rows - the whole-row stackings of the gate / RANSAC - stay dense rows)
  if (!full_rows && !write_dense && calib_sparse(c)) { a.lead = c->Hlead.p; a.strideLead = c->Hlead.stride; a.lead_k = LEAD_K; }
  StageTimer st(c, ST_STACK, 0.0, "stack_kernel");
  return launch_stack(a, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

// Estimator::MHGating of an online-calibration build: the gate needs the WHOLE row J() incl. the td / Cg / bg / intrinsics
// blocks (update.cpp:60-70), which is not the row FillJacobianBlock stacks (the :675-676 overwrite): every present feature is
// stacked once as its full J() (dense rows) and gated on (J P) J^T + R by the dense-row gate. gate = 0: every present feature
// is an inlier (Estimator::OutlierRejection does not gate F <= min_required_inliers_, src/manager.cpp:635).
int calib_gate(xivo_hip_ctx* c, int B, double R, double mh_thresh, double mh_mult, int min_inliers, int gate) {
  int rc = gate_impl(c, B, R, mh_thresh, mh_mult, min_inliers, 0);
  if (rc) return rc;
  if (gate) {
    c->rows.stacked(B, c->F, R, Stacking::full_rows, /*pw=*/9, /*dense=*/true, CalibCols::in_rows);
    c->dx_clear();
    rc = stack_impl(c, B, R, 1, nullptr, /*full_rows=*/1);
    if (rc) return rc;
    GateDenseArgs a{};
    a.mask = c->mask; a.dist = c->dist; a.F = c->F; a.mask_ld = c->Fmax;   // (the stride xivo_hip_stack reads the mask with)
    a.R = R; a.thresh = mh_thresh; a.mult = mh_mult; a.min_inliers = min_inliers; a.have_ell = 0;
    a.feats = c->feats; a.Fmax = c->Fmax;        // absent entries of ragged batches are no candidates (per-filter present count)
    return gate_dense_rows(c, B, a);   // (mask / dist stay in the strided layout gate_impl left)
  }
  return XIVO_HIP_OK;
}

}  // namespace

namespace xivo_hip::capi {

int ensure_gate_buffers(xivo_hip_ctx* c, int F) {
  // allocated once, for the most features a context can stage: every caller bounds 2 F by Mmax <= Mpmax. (Fmax stays 0 until
  // the whole group is there, so a call after a failed one starts over; the owner releases what a slot still holds.)
  const int Fm = c->Mpmax / 2;
  if (F > Fm) return XIVO_HIP_ERR_INVALID;
  if (c->Fmax == Fm) return XIVO_HIP_OK;
  const size_t B = c->Bmax;
  int rc = c->mem.zeroed(&c->feats, B * Fm);
  if (!rc) rc = c->mem.zeroed(&c->J, B * Fm * 42);
  if (!rc) rc = c->mem.zeroed(&c->finn, B * Fm * 2);
  if (!rc) rc = c->mem.zeroed(&c->dist, B * Fm);
  if (!rc) rc = c->mem.zeroed(&c->mask, B * Fm);
  if (!rc && c->calib_on) rc = c->mem.zeroed(&c->Jc, B * Fm * 44);
  if (!rc && !c->rows_instate) rc = c->mem.zeroed(&c->rows_instate, B);
  // every entry starts absent (sind = -1) and masked out until a scene / edit writes it
  if (!rc && hipMemsetAsync(c->feats, 0xFF, B * Fm * sizeof(xivo_feat_in), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(c->mask, 0, B * Fm, c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc) c->Fmax = Fm;
  return rc;
}

// the transposed dense copy: a G-level producer may have skipped it (mixed stacking); a consumer that needs it - the dense-row gate, the as-coded K H - I - rebuilds it from H here
int ensure_HT(xivo_hip_ctx* c) {
  if (c->rows.ht_alive()) return XIVO_HIP_OK;
  StageTimer st(c, ST_STACK, 0.0, "transpose_H_kernel");
  if (launch_transpose_H(c->H.p, c->H.stride, c->H.ld, c->HT.p, c->HT.stride, c->HT.ld, c->Mpmax, c->Np, c->Bmax, c->stream)) return XIVO_HIP_ERR_HIP;
  c->rows.ht_materialised();
  return XIVO_HIP_OK;
}

// the dense copies of the stacked rows, for the consumers that need them (dense pipeline, OOS rows, get_H)
int ensure_dense(xivo_hip_ctx* c) {
  if (c->rows.dense_alive()) return XIVO_HIP_OK;
  const int mr0 = c->rows.mixed_row0();
  if (mr0 >= 0 || c->rows.dense_from_compressed()) {
    // the compressed rows are the source. Mixed stacking: the in-state rows only, next to the OOS rows already in place (no H^T);
    // S-level hand-over: H and H^T (filters that do not fit hold dense rows already)
    StageTimer st(c, ST_STACK, 0.0, "ell_to_dense_kernel");
    if (launch_ell_to_dense(c->ell, c->H.p, c->H.stride, c->H.ld, mr0 >= 0 ? nullptr : c->HT.p, c->HT.stride, c->HT.ld, c->Mpmax, c->Np, c->Bmax, c->stream, mr0))
      return XIVO_HIP_ERR_HIP;
  } else {
    if (int rc = stack_impl(c, c->rows.restack_args().B, c->rows.restack_args().R, 1)) return rc;
    // online-calibration stacking on the sparse pipeline: dense rows carry the calibration columns themselves
    if (c->rows.has_lead()) c->rows.lead_demoted();
  }
  c->rows.dense_materialised();
  return XIVO_HIP_OK;
}

int gate_dense_rows(xivo_hip_ctx* c, int B, GateDenseArgs a) {
  int rc = ensure_HT(c);   // (the gate reads - and neutralises - the transposed rows too)
  if (rc) return rc;
  const int Np = c->Np;
  GemmExtra x; x.C2 = c->PHT;
  rc = gemm(c, ST_HP, B, c->rows.rows_padded(), Np, {c->H, c->P, Np}, c->HP, x);
  if (rc) return rc;
  c->H.to(a.H, a.strideH, a.ldh); c->HP.to(a.HP, a.strideHP, a.ldhp);
  a.Hw = c->H.p; c->HT.to(a.HTw, a.strideHT, a.ldht); a.HPw = nullptr; a.PHTw = nullptr; a.PHTr = c->PHT.p;
  c->inn.to(a.inn, a.strideInn); c->diagR.to(a.diagR, a.strideR); a.Np = Np; a.batch = B; a.ell = c->ell;
  StageTimer st(c, ST_GATE, 0.0, "gate_dense_kernel");
  HIP_TRY((hipError_t)launch_gate_dense(a, c->stream));
  return XIVO_HIP_OK;
}

}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_set_layout(xivo_hip_ctx* c, const xivo_layout* lay, const xivo_cam* cam) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !lay || !cam) return XIVO_HIP_ERR_INVALID;
  if (lay->N != c->N || lay->group_begin < 21 || lay->n_groups <= 0 || lay->n_features <= 0 ||
      lay->feature_begin < lay->group_begin + 6 * lay->n_groups ||
      lay->feature_begin + 3 * lay->n_features > lay->N)
    return XIVO_HIP_ERR_INVALID;
  if (cam->model < XIVO_CAM_PINHOLE || cam->model > XIVO_CAM_EQUI) return XIVO_HIP_ERR_INVALID;
  c->lay = *lay; c->cam = *cam; c->have_layout = true;
  if (!c->poses) {
    int rc = c->mem.zeroed(&c->poses, (size_t)c->Bmax);
    if (!rc) rc = c->mem.zeroed(&c->absorb_count, (size_t)c->Bmax);
    if (!rc) rc = c->mem.zeroed(&c->groups, (size_t)c->Bmax * lay->n_groups);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_set_scene(xivo_hip_ctx* c, int b0, int nb, int F, const xivo_pose_in* poses,
                       const xivo_group_in* groups, const xivo_feat_in* feats) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || F <= 0 || 2 * F > c->Mmax || !poses || !groups || !feats)
    return XIVO_HIP_ERR_INVALID;
  int rc = ensure_gate_buffers(c, F);
  if (rc) return rc;
  for (long i = 0; i < (long)nb * F; ++i) {
    const xivo_feat_in& f = feats[i];
    if (f.sind == -1) continue;   // absent entry
    if (f.ref_sind < 0 || f.ref_sind >= c->lay.n_groups || f.sind < 0 || f.sind >= c->lay.n_features)
      return XIVO_HIP_ERR_INVALID;
  }
  c->F = F;
  HIP_TRY(hipMemcpyAsync(c->poses + b0, poses, (size_t)nb * sizeof(xivo_pose_in), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->groups + (size_t)b0 * c->lay.n_groups, groups,
                         (size_t)nb * c->lay.n_groups * sizeof(xivo_group_in), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpy2DAsync(c->feats + (size_t)b0 * c->Fmax, (size_t)c->Fmax * sizeof(xivo_feat_in), feats,
                           (size_t)F * sizeof(xivo_feat_in), (size_t)F * sizeof(xivo_feat_in), nb,
                           hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_jacobians_instate(xivo_hip_ctx* c, int B) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  StageTimer st(c, ST_JAC, 0.0, "jac_instate_kernel");
  return launch_jac_instate(scene_buffers(c), c->lay, c->cam, B, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_get_jacobians(xivo_hip_ctx* c, int b0, int nb, double* J, double* inn) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  const size_t F = c->F, Fm = c->Fmax;
  if (J) {
    int rc = d2h_rows(c, J, F * 42 * sizeof(double), c->J + (size_t)b0 * Fm * 42, Fm * 42 * sizeof(double),
                      F * 42 * sizeof(double), nb);
    if (rc) return rc;
  }
  if (inn) {
    int rc = d2h_rows(c, inn, F * 2 * sizeof(double), c->finn + (size_t)b0 * Fm * 2, Fm * 2 * sizeof(double),
                      F * 2 * sizeof(double), nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_set_calib(xivo_hip_ctx* c, const xivo_calib_layout* layout) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout) return XIVO_HIP_ERR_INVALID;
  if (!layout) { c->calib_on = false; c->calib_motion = false; c->cl = xivo_calib_layout{-1, -1, 0, 0}; return XIVO_HIP_OK; }
  const xivo_calib_layout& l = *layout;
  const int N = c->N;
  if (l.td >= N || (l.Cg >= 0 && l.Cg + 15 > N) || l.cam_dim < 0 || l.cam_dim > 9 ||
      (l.cam_dim > 0 && (l.cam_begin < 0 || l.cam_begin + l.cam_dim > N)))
    return XIVO_HIP_ERR_INVALID;
  // slots as src/core.h:40-75 numbers them: td right behind Wsg, Cg behind td (or Wsg), the intrinsics behind the motion block
  if ((l.td >= 0 && l.td != 23) || (l.Cg >= 0 && l.Cg != (l.td >= 0 ? 24 : 23))) return XIVO_HIP_ERR_INVALID;
  if (!c->calib) { int rc = c->mem.zeroed(&c->calib, (size_t)c->Bmax); if (rc) return rc; }
  if (!c->Jc && c->Fmax > 0) { int rc = c->mem.zeroed(&c->Jc, (size_t)c->Bmax * c->Fmax * 44); if (rc) return rc; }
  if (!c->Hlead.p) { int rc = c->mem.zeroed(&c->Hlead.p, (size_t)c->Bmax * c->Hlead.stride); if (rc) return rc; }
  c->rows.lead_dropped();
  c->dx_clear();
  c->cl = l;
  c->calib_on = l.td >= 0 || l.cam_dim > 0;       // measurement side: blocks beyond the default build's (the Cg / bg blocks sit inside the td block)
  c->calib_motion = l.td >= 0 || l.Cg >= 0;       // motion side: kMotionSize > 23
  return XIVO_HIP_OK;
}

int xivo_hip_set_calib_state(xivo_hip_ctx* c, int b0, int nb, const xivo_calib_in* calib) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !calib || !c->calib) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(c->calib + b0, calib, (size_t)nb * sizeof(xivo_calib_in), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));    // host buffer is only borrowed for the call
  return XIVO_HIP_OK;
}

int xivo_hip_set_calib_gyro(xivo_hip_ctx* c, int b0, int nb, const double* gyro3) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !gyro3 || !c->calib) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  static_assert(offsetof(xivo_calib_in, gyro) == 0, "gyro leads xivo_calib_in");
  HIP_TRY(hipMemcpy2DAsync(c->calib + b0, sizeof(xivo_calib_in), gyro3, 3 * sizeof(double), 3 * sizeof(double), (size_t)nb,
                           hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_get_calib_state(xivo_hip_ctx* c, int b0, int nb, xivo_calib_in* calib) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !calib || !c->calib) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(calib, c->calib + b0, (size_t)nb * sizeof(xivo_calib_in), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_get_jacobians_calib(xivo_hip_ctx* c, int b0, int nb, double* Jc) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || c->F <= 0 || !Jc || !c->calib_on || !c->Jc) return XIVO_HIP_ERR_INVALID;
  const size_t F = c->F, Fm = c->Fmax;
  return d2h_rows(c, Jc, F * 44 * sizeof(double), c->Jc + (size_t)b0 * Fm * 44, Fm * 44 * sizeof(double), F * 44 * sizeof(double), nb);
}

int xivo_hip_mh_gate(xivo_hip_ctx* c, int B, double R, double mh_thresh, double mh_mult, int min_inliers,
                     unsigned char* mask_out, double* dist_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  // (online-calibration builds: the compact gate works on the whole row too - 43 columns, gate_sparse_kernel's wide form;
  //  with XIVO_HIP_FLAG_DENSE_H the dense-row gate of round 4)
  int rc = (c->calib_on && !calib_sparse(c)) ? calib_gate(c, B, R, mh_thresh, mh_mult, min_inliers, 1)
                                             : gate_impl(c, B, R, mh_thresh, mh_mult, min_inliers, 1);
  return rc ? rc : xivo_hip_get_gate(c, B, c->F, mask_out, dist_out);   // (in the strided layout the gate just left)
}

int xivo_hip_stack(xivo_hip_ctx* c, int B, double R) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  // (calibration blocks: up to 34 shared columns - dense rows, or compressed rows + the leading dense block)
  const CalibCols cc = !c->calib_on ? CalibCols::none : calib_sparse(c) ? CalibCols::lead_block : CalibCols::in_rows;
  // the sparse-H pipeline reads only the compressed rows: skip the 2 x Mp x Np dense zero-fill + scatter
  const int dense = ((c->flags & XIVO_HIP_FLAG_DENSE_H) || cc == CalibCols::in_rows) ? 1 : 0;
  const int pw = (c->flags & XIVO_HIP_FLAG_FIX_GROUP_BLOCK) ? 9 : 6;   // group block(s) + feature block
  c->rows.stacked(B, c->F, R, Stacking::in_state_as_coded, pw, /*dense=*/dense != 0, cc);
  c->dx_clear();
  return stack_impl(c, B, R, dense);
}

int xivo_hip_oos_project(xivo_hip_ctx* c, int b0, int nb, int n_oos, const xivo_oos_in* feats, double Roos,
                         int* rows_out) {
  return xivo_hip_oos_project_ex(c, b0, nb, n_oos, feats, Roos, rows_out, 0u);
}

int xivo_hip_oos_project_ex(xivo_hip_ctx* c, int b0, int nb, int n_oos, const xivo_oos_in* feats, double Roos,
                            int* rows_out, unsigned options) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || n_oos <= 0 || b0 != 0) return XIVO_HIP_ERR_INVALID;
  if (options & ~XIVO_HIP_OOS_WHOLE_BUFFER) return XIVO_HIP_ERR_INVALID;
  // XIVO_HIP_OOS_WHOLE_BUFFER (src/oos.cpp:28 as coded): SlowGivens sees the whole 2 kMaxGroup-row buffers of the feature, so
  // every feature contributes 2 kMaxGroup - 3 rows; the rows behind its 2 k observations are zero (include/xivo_hip.h)
  const int whole = (options & XIVO_HIP_OOS_WHOLE_BUFFER) ? 2 * c->lay.n_groups : 0;
  // feats == NULL: the list uploaded by the previous call is still resident (same nb, n_oos) - project it again
  if (!feats && (!c->oos || c->oos_nb != nb || c->oos_n != n_oos || c->oos_whole != whole)) return XIVO_HIP_ERR_INVALID;
  int max_rows = feats ? 0 : c->rows.oos_max_rows();
  for (int b = 0; feats && b < nb; ++b) {
    int rows = 0;
    for (int o = 0; o < n_oos; ++o) {
      const xivo_oos_in& f = feats[(size_t)b * n_oos + o];
      if (f.n_obs < 2 || f.n_obs > XIVO_OOS_MAX_OBS) return XIVO_HIP_ERR_INVALID;
      for (int q = 0; q < f.n_obs; ++q)
        if (f.group_sind[q] < 0 || f.group_sind[q] >= c->lay.n_groups) return XIVO_HIP_ERR_INVALID;
      if (whole && 2 * f.n_obs > whole) return XIVO_HIP_ERR_INVALID;     // (more observations than the reference's buffer has rows)
      rows += whole ? whole - 3 : 2 * f.n_obs - 3;
    }
    if (rows > max_rows) max_rows = rows;
  }
  const int M = c->rows.rows();
  if (M + max_rows > c->Mmax) return XIVO_HIP_ERR_INVALID;
  // Mixed stacking (round 3, default whenever the in-state rows were stacked in the compressed form only and nothing
  // forces the dense pipeline): the OOS rows go to the dense buffer behind the in-state rows and the update keeps the
  // sparse walk for the in-state rows - only the OOS block takes the MFMA products (update_sparse_range). Needs a
  // 16-row-padded OOS block inside the allocation; otherwise (and with XIVO_HIP_FLAG_DENSE_H) every row
  // becomes dense as before.
  const bool mixed = !c->calib_on && !c->rows.dense_alive() && !c->rows.dense_from_compressed() && c->rows.oos_row0() < 0 && b0 == 0 &&
                     !(c->flags & XIVO_HIP_FLAG_DENSE_H) && (M % 2 == 0) &&
                     M + round_up16(max_rows + 16) <= c->Mpmax && c->Np <= 512;
  if (!mixed) { int rcd = ensure_dense(c); if (rcd) return rcd; }
  else {
    // the OOS rows must start from zero: only the extrinsics and group columns are ever written there in this mode, so
    // those are cleared (whole rows once, if anything else has used the dense buffer since it was allocated)
    const int nz = std::min(round_up16(max_rows + 16), c->Mpmax - M);
    if (!c->rows.dense_clean()) {
      HIP_TRY((hipError_t)launch_zero_rows(c->H.p, c->H.stride, c->H.ld, 0, c->Mpmax, 0, c->Np, c->Bmax, c->stream));
      c->rows.dense_zeroed();
    } else {
      HIP_TRY((hipError_t)launch_zero_rows(c->H.p, c->H.stride, c->H.ld, M, nz, 15, 21, nb, c->stream));
      HIP_TRY((hipError_t)launch_zero_rows(c->H.p, c->H.stride, c->H.ld, M, nz, c->lay.group_begin, c->lay.group_begin + 6 * c->lay.n_groups, nb, c->stream));
    }
  }
  if ((size_t)n_oos * nb > c->oos_cap) {   // (a resident list - feats == NULL - fits by the check above)
    int rc = c->mem.grow(&c->oos, &c->oos_cap, (size_t)n_oos * c->Bmax);
    if (rc) return rc;
  }
  if (!c->oos_rows) { int rc = c->mem.zeroed(&c->oos_rows, (size_t)c->Bmax); if (rc) return rc; }
  if (feats) {
    HIP_TRY(hipMemcpyAsync(c->oos, feats, (size_t)nb * n_oos * sizeof(xivo_oos_in), hipMemcpyHostToDevice, c->stream));
    c->oos_nb = nb; c->oos_n = n_oos; c->oos_whole = whole;
  }
  OosArgs a{};
  a.feats = c->oos; a.n_oos = n_oos; a.poses = c->poses; a.groups = c->groups; a.lay = c->lay; a.cam = c->cam;
  a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  a.mb = meas_buffers(c); a.row0 = M; a.Mp = c->Mpmax; a.Np = c->Np; a.batch = nb; a.Roos = Roos; a.whole = whole;
  if (mixed) a.mb.HT = nullptr;
  a.rows_out = c->oos_rows;
  {
    StageTimer st(c, ST_OTHER, 0.0, "oos_kernel");
    HIP_TRY((hipError_t)launch_oos(a, c->stream));
  }
  if (rows_out) HIP_TRY(hipMemcpyAsync(rows_out, c->oos_rows, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->dx_clear();
  c->rows.oos_appended(max_rows, Roos, mixed, b0, nb);   // (not mixed: OOS rows are dense over the group blocks - dense path)
  return XIVO_HIP_OK;
}

// Estimator::OnePointRANSAC (src/update.cpp:213-393) for filters [0,B) on the resident state, after
// xivo_hip_jacobians_instate + xivo_hip_mh_gate (the MH inlier mask is the input set):
//   select (low-innovation set, temporary reference group)                       :238-301   ransac_select_kernel
//   BackupState: P, nominal state, groups                                        :283       device-to-device copies
//   zero P rows / cols of non-members                                            :299-316   ransac_zero_kernel
//   partial update on the FULL rows J() of the low-innovation set + AbsorbError  :320-333   stack (full rows) + update + absorb
//   re-Jacobians at the updated state, chi-square rescue                         :343-369   jac_instate + ransac_rescue_kernel
//   RestoreState, re-Jacobians at the original state                             :383-387
// The resulting inlier set replaces the MH mask (what xivo_hip_stack / xivo_hip_absorb_error read afterwards).
int xivo_hip_one_point_ransac(xivo_hip_ctx* c, int B, double R, double ransac_thresh, double ransac_chi2,
                              const int* gauge_group, const unsigned long long* absorb_groups,
                              unsigned char* inlier_mask_out, double* chi2_out, int* n_rejected_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0 || !c->mask || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (c->lay.n_groups > 64) return XIVO_HIP_ERR_UNSUPPORTED;
  const size_t Bm = c->Bmax, ng = c->lay.n_groups;
  // online-calibration builds: the calibration state is backed up / restored with X_ (imu_.BackupState, Camera::BackupState,
  // src/estimator.cpp:1421-1427), the partial update stacks the whole rows J() as dense rows, AbsorbError retracts td / Cg / Ca /
  // the intrinsics too, and the rescue test uses the whole-row distances of the dense-row gate
  const bool cal = c->calib_on;
  if (cal && !c->calib_rs) { int rc = c->mem.zeroed(&c->calib_rs, Bm); if (rc) return rc; }
  if (c->rs_Fmax != c->Fmax) {   // first use (Fmax never changes once it is set: ensure_gate_buffers)
    int rc = XIVO_HIP_OK;
    auto A = [&](auto** p, size_t n) { if (rc == XIVO_HIP_OK) rc = c->mem.zeroed(p, n); };
    A(&c->Prs, Bm * c->P.stride); A(&c->poses_rs, Bm); A(&c->groups_rs, Bm * ng);
    A(&c->rs_low, Bm * c->Fmax); A(&c->rs_lowkeep, Bm * c->Fmax); A(&c->rs_keep, Bm * c->Fmax); A(&c->rs_chi, Bm * c->Fmax);
    A(&c->rs_zg, Bm); A(&c->rs_gmask, Bm); A(&c->rs_state, Bm); A(&c->rs_gauge, Bm); A(&c->rs_nrej, Bm);
    if (rc) return rc;
    c->rs_Fmax = c->Fmax;
  }
  if (gauge_group) HIP_TRY(hipMemcpyAsync(c->rs_gauge, gauge_group, (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
  else HIP_TRY(hipMemsetAsync(c->rs_gauge, 0xFF, (size_t)B * sizeof(int), c->stream));
  if (absorb_groups) HIP_TRY(hipMemcpyAsync(c->rs_gmask, absorb_groups, (size_t)B * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  RansacArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; c->P.to(a.P, a.strideP, a.ldp); a.Np = c->Np;
  a.R = R; a.thresh = ransac_thresh; a.chi2 = ransac_chi2; a.gauge = c->rs_gauge;
  a.low = c->rs_low; a.low_keep = c->rs_lowkeep; a.zero_groups = c->rs_zg; a.state = c->rs_state;
  a.keep = c->rs_keep; a.chi = c->rs_chi; a.n_rejected = c->rs_nrej; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "ransac_select_kernel");
    HIP_TRY((hipError_t)launch_ransac_select(a, c->stream));
  }
  // the low-innovation set as select found it (filters with nothing to update get an all-neutral stacking mask)
  HIP_TRY(hipMemcpyAsync(c->rs_lowkeep, c->rs_low, (size_t)B * c->Fmax, hipMemcpyDeviceToDevice, c->stream));
  // BackupState (src/estimator.cpp:1410-1428)
  HIP_TRY(hipMemcpyAsync(c->Prs, c->P.p, (size_t)B * c->P.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->poses_rs, c->poses, (size_t)B * sizeof(xivo_pose_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->groups_rs, c->groups, (size_t)B * ng * sizeof(xivo_group_in), hipMemcpyDeviceToDevice, c->stream));
  if (cal) HIP_TRY(hipMemcpyAsync(c->calib_rs, c->calib, (size_t)B * sizeof(xivo_calib_in), hipMemcpyDeviceToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "ransac_zero_kernel");
    HIP_TRY((hipError_t)launch_ransac_zero(a, c->P.p, c->stream));
  }
  // partial update: H_ rows = the full J() of the low-innovation inliers (:326 - no FillJacobianBlock), R_ on the diagonal
  const int dense = ((c->flags & XIVO_HIP_FLAG_DENSE_H) || cal) ? 1 : 0;
  const CalibCols cc = cal ? CalibCols::in_rows : CalibCols::none;
  c->rows.stacked(B, c->F, R, Stacking::full_rows, /*pw=*/9, /*dense=*/dense != 0, cc);
  int rc = stack_impl(c, B, R, dense, c->rs_low, 1);
  if (rc) return rc;
  rc = xivo_hip_update_joseph(c, B);
  if (rc) return rc;
  c->dx_clear();   // (the partial update's dx is absorbed right here and the state restored: nothing to record)
  {  // AbsorbError (:333): in_current_ekf_update_ is empty at this point of Estimator::UpdateStep (cleared at
     // src/manager.cpp:28, filled after OutlierRejection), so no feature state moves; State::counter is restored with X_
    AbsorbArgs ab{};
    ab.poses = c->poses; ab.groups = c->groups; ab.feats = c->feats; ab.mask = nullptr; c->err.to(ab.err, ab.strideErr);
    ab.lay = c->lay; ab.F = c->F; ab.Fmax = c->Fmax; ab.batch = B; ab.counter = nullptr; ab.status = c->status;
    ab.group_mask = absorb_groups ? c->rs_gmask : nullptr;
    ab.calib = (c->calib_on || c->calib_motion) ? c->calib : nullptr; ab.cl = c->cl;
    StageTimer st(c, ST_OTHER, 0.0, "absorb_error_kernel");
    HIP_TRY((hipError_t)launch_absorb_error(ab, c->stream));
  }
  rc = xivo_hip_jacobians_instate(c, B);                                   // :348 at the updated state
  if (rc) return rc;
  if (!cal) {
    StageTimer st(c, ST_OTHER, 0.0, "ransac_rescue_kernel");
    HIP_TRY((hipError_t)launch_ransac_rescue(a, c->stream));
  } else {
    // S = J P J^T + R of every MH inlier on its WHOLE row at the updated state against the partially updated P (:350-356):
    // the rows stacked once more in full (scratch: xivo_hip_stack re-stacks the final inlier set), H P, the dense-row distances
    c->rows.stacked(B, c->F, R, Stacking::full_rows, /*pw=*/9, /*dense=*/true, cc);
    rc = stack_impl(c, B, R, 1, nullptr, /*full_rows=*/1);
    if (rc) return rc;
    GateDenseArgs ga{};
    // (scratch outputs: the mask goes to rs_low - dead once the partial update is stacked -, the distances to rs_chi, where the
    //  decision kernel below reads them and leaves chi2 per tested feature; c->dist keeps the MH distances)
    ga.mask = c->rs_low; ga.dist = c->rs_chi; ga.F = c->F; ga.mask_ld = c->Fmax;
    ga.R = R; ga.thresh = ransac_chi2; ga.mult = 1.0; ga.min_inliers = -1; ga.no_relax = 1;
    ga.have_ell = 0; ga.feats = c->feats; ga.Fmax = c->Fmax;
    rc = gate_dense_rows(c, B, ga);
    if (rc) return rc;
    StageTimer st(c, ST_OTHER, 0.0, "ransac_rescue_dist_kernel");
    HIP_TRY((hipError_t)launch_ransac_rescue_dist(a, c->rs_chi, c->Fmax, c->stream));
  }
  // RestoreState + Jacobians at the original state (:383-387)
  HIP_TRY(hipMemcpyAsync(c->P.p, c->Prs, (size_t)B * c->P.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->poses, c->poses_rs, (size_t)B * sizeof(xivo_pose_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->groups, c->groups_rs, (size_t)B * ng * sizeof(xivo_group_in), hipMemcpyDeviceToDevice, c->stream));
  if (cal) HIP_TRY(hipMemcpyAsync(c->calib, c->calib_rs, (size_t)B * sizeof(xivo_calib_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->mask, c->rs_keep, (size_t)B * c->Fmax, hipMemcpyDeviceToDevice, c->stream));
  rc = xivo_hip_jacobians_instate(c, B);
  if (rc) return rc;
  c->rows.gate_wrote(GateLayout::strided);
  const size_t F = c->F, Fm = c->Fmax;
  if (inlier_mask_out) { rc = d2h_rows(c, inlier_mask_out, F, c->mask, Fm, F, B); if (rc) return rc; }
  if (chi2_out) { rc = d2h_rows(c, chi2_out, F * sizeof(double), c->rs_chi, Fm * sizeof(double), F * sizeof(double), B); if (rc) return rc; }
  if (n_rejected_out) HIP_TRY(hipMemcpyAsync(n_rejected_out, c->rs_nrej, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // gauge_group / absorb_groups are borrowed host memory
  return XIVO_HIP_OK;
}

// Estimator::CloseLoopInternal's stacking (src/update.cpp:183-196) with Feature::ComputeLCJacobian (src/oos.cpp:92-145) on the
// resident scene: the 2n rows of every filter are built dense in a scratch block (lc_rows_kernel) and handed over like any
// device-resident H_ (stage_measurements: row-pair compressed where they fit - group block private, extrinsics [+ intrinsics]
// common -, so the update that follows takes the sparse pipeline). The inlier mask of the last gating pass is left alone:
// AbsorbError after a loop closure updates in_current_ekf_update_ as the last FilterUpdate left it (src/estimator.cpp:906-912).
int xivo_hip_close_loop_stack(xivo_hip_ctx* c, int b0, int nb, int n, const xivo_lc_match* matches, double Rlc) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || !c->feats || n <= 0 || 2 * n > c->Mmax || !matches || !(Rlc > 0.0))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  for (size_t i = 0; i < (size_t)nb * n; ++i) {
    const xivo_lc_match& m = matches[i];
    if (m.feat >= c->F || (m.feat >= 0 && (m.group_sind < 0 || m.group_sind >= c->lay.n_groups))) return XIVO_HIP_ERR_INVALID;
  }
  const int M = 2 * n, N = c->N;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_m = 0, o_H = al((size_t)nb * n * sizeof(xivo_lc_match)), o_inn = al(o_H + (size_t)nb * M * N * sizeof(double)),
               o_R = al(o_inn + (size_t)nb * M * sizeof(double)), total = al(o_R + (size_t)nb * M * sizeof(double));
  if (int rc = c->mem.grow(&c->lc_buf, &c->lc_cap, total)) return rc;
  char* base = c->lc_buf;
  HIP_TRY(hipMemcpyAsync(base + o_m, matches, (size_t)nb * n * sizeof(xivo_lc_match), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(base + o_H, 0, (size_t)nb * M * N * sizeof(double), c->stream));     // H_.setZero(2n, N) (update.cpp:184)
  LcArgs a{};
  a.matches = reinterpret_cast<const xivo_lc_match*>(base + o_m); a.n = n;
  a.poses = c->poses + b0; a.groups = c->groups + (size_t)b0 * c->lay.n_groups; a.feats = c->feats + (size_t)b0 * c->Fmax; a.Fmax = c->Fmax;
  a.lay = c->lay; a.cam = c->cam; a.calib = c->calib_on ? c->calib + b0 : nullptr;
  a.cl = c->calib_on ? c->cl : xivo_calib_layout{-1, -1, 0, 0}; a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  a.H = reinterpret_cast<double*>(base + o_H); a.strideH = (long)M * N; a.ldh = M;
  a.inn = reinterpret_cast<double*>(base + o_inn); a.diagR = reinterpret_cast<double*>(base + o_R); a.strideV = M;
  a.Rlc = Rlc; a.batch = nb;
  {
    StageTimer st(c, ST_OTHER, 0.0, "lc_rows_kernel");
    HIP_TRY((hipError_t)launch_lc_rows(a, c->stream));
  }
  return stage_measurements(c, b0, nb, M, a.H, a.strideH, a.ldh, a.inn, a.strideV, a.diagR, a.strideV);
}

// Measurement compression of the OOS rows appended by the last xivo_hip_oos_project (use_compression_ /
// compression_trigger_ratio_, src/estimator.h:399-402; xivo::QR, src/helpers.cpp:77-101): per filter, when the block
// has more than trigger_ratio times as many rows as non-zero columns, it is replaced by the triangular factor of its QR
// decomposition (oos_compress_kernel) and the row count of the stacked measurement shrinks accordingly.
int xivo_hip_compress_oos(xivo_hip_ctx* c, int B, double trigger_ratio, int* rows_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->rows.oos_row0() < 0 || !c->oos_rows || B != c->oos_nb || !(trigger_ratio >= 1.0))
    return XIVO_HIP_ERR_INVALID;
  OosCompressArgs a{};
  a.lay = c->lay; a.mb = meas_buffers(c); a.row0 = c->rows.oos_row0(); a.rows = c->oos_rows; a.rows_out = c->oos_rows;
  if (c->rows.mixed_row0() >= 0) a.mb.HT = nullptr;
  a.ratio = trigger_ratio; a.Roos = c->rows.oos_R(); a.batch = B;
  int rc = -1;
  char label[64];
  if (oos_compress_pick(c->lay.n_groups, c->rows.oos_max_rows(), label, sizeof(label)) >= 0) {
    StageTimer st(c, ST_OTHER, 0.0, label);
    rc = launch_oos_compress(a, c->rows.oos_max_rows(), c->stream);
  }
  if (rc > 0) return XIVO_HIP_ERR_HIP;
  std::vector<int> rows(B);
  HIP_TRY(hipMemcpyAsync(rows.data(), c->oos_rows, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int mx = 0;
  for (int b = 0; b < B; ++b) mx = rows[b] > mx ? rows[b] : mx;
  // (rc == -1: block larger than the built kernels - rows are left as they are, which is always valid)
  c->rows.oos_compressed(mx);
  c->dx_clear();
  if (rows_out) memcpy(rows_out, rows.data(), (size_t)B * sizeof(int));
  return XIVO_HIP_OK;
}

int xivo_hip_filter_update(xivo_hip_ctx* c, int B, double R, double mh_thresh, double mh_mult, int min_inliers,
                           int use_gating) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  int rc = xivo_hip_jacobians_instate(c, B);
  if (rc) return rc;
  // Estimator::OutlierRejection only gates when F > min_required_inliers_ (src/manager.cpp:635)
  const int gate = use_gating && c->F > min_inliers;
  // online-calibration builds on dense rows (XIVO_HIP_FLAG_DENSE_H): the gate needs the WHOLE row J() incl. the td / Cg / bg / intrinsics blocks (update.cpp:60-70),
  // which is not the row FillJacobianBlock stacks (the :675-676 overwrite): every present feature is stacked once as its
  // full J() (dense rows), gated on (J P) J^T + R by the dense-row gate, then the inliers are stacked as coded and updated
  rc = (c->calib_on && !calib_sparse(c)) ? calib_gate(c, B, R, mh_thresh, mh_mult, min_inliers, gate)
                                         : gate_impl(c, B, R, mh_thresh, mh_mult, min_inliers, gate);
  if (rc) return rc;
  rc = xivo_hip_stack(c, B, R);
  if (rc) return rc;
  return xivo_hip_update_joseph(c, B);
}

static int givens_impl(xivo_hip_ctx* c, int nb, int rows, int nx, int nf, double* x, double* Hx, double* Hf,
                       int effective_rows, int* rows_out, int qr) {
  if (!c || nb <= 0 || rows < 2 || nx <= 0 || !x || !Hx || (!qr && (!Hf || nf <= 0 || nf > 64)) || (qr && nx > 512))
    return XIVO_HIP_ERR_INVALID;
  const int eff = effective_rows < 0 ? rows : effective_rows;
  // the reference CHECKs these (helpers.cpp:49-53, 79-84); here they are an error code
  if (eff > rows || eff < 2 || (qr ? eff <= nx : eff < nf)) return XIVO_HIP_ERR_INVALID;
  const size_t ex = (size_t)nb * rows, ehx = (size_t)nb * rows * nx, ehf = qr ? 0 : (size_t)nb * rows * nf;
  int rc = ensure_staging(c, ex + ehx + ehf);
  if (rc) return rc;
  double* dx = c->staging; double* dHx = dx + ex; double* dHf = dHx + ehx;
  HIP_TRY(hipMemcpyAsync(dx, x, ex * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dHx, Hx, ehx * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (!qr) HIP_TRY(hipMemcpyAsync(dHf, Hf, ehf * sizeof(double), hipMemcpyHostToDevice, c->stream));
  GivensArgs a{}; a.x = dx; a.Hx = dHx; a.Hf = qr ? nullptr : dHf; a.rows = rows; a.nx = nx; a.nf = nf; a.eff = effective_rows;
  a.batch = nb; a.qr = qr;
  {
    StageTimer st(c, ST_OTHER, 0.0, "givens_kernel");
    HIP_TRY((hipError_t)launch_givens(a, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(x, dx, ex * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(Hx, dHx, ehx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (!qr) HIP_TRY(hipMemcpyAsync(Hf, dHf, ehf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (rows_out) for (int b = 0; b < nb; ++b) rows_out[b] = qr ? eff : eff - nf;
  return XIVO_HIP_OK;
}

int xivo_hip_givens(xivo_hip_ctx* c, int nb, int rows, int nx, int nf, double* x, double* Hx, double* Hf,
                    int effective_rows, int* rows_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  return givens_impl(c, nb, rows, nx, nf, x, Hx, Hf, effective_rows, rows_out, 0);
}

int xivo_hip_qr(xivo_hip_ctx* c, int nb, int rows, int nx, double* x, double* Hx, int effective_rows, int* rows_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  return givens_impl(c, nb, rows, nx, 0, x, Hx, nullptr, effective_rows, rows_out, 1);
}

int xivo_hip_subfilter_update(xivo_hip_ctx* c, int b0, int nb, int n, xivo_subfilter_feat* feats,
                              const xivo_subfilter_opts* opts) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || n <= 0 || !feats || !opts) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  for (size_t i = 0; i < (size_t)nb * n; ++i)
    if (feats[i].ref_sind < 0 || feats[i].ref_sind >= c->lay.n_groups) return XIVO_HIP_ERR_INVALID;
  const size_t bytes = (size_t)nb * n * sizeof(xivo_subfilter_feat);
  if (int rc = c->mem.grow(&c->sub, &c->sub_cap, (size_t)nb * n)) return rc;
  HIP_TRY(hipMemcpyAsync(c->sub, feats, bytes, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "subfilter_kernel");
    if (launch_subfilter(c->sub, n, c->poses + b0, c->groups + (size_t)b0 * c->lay.n_groups, c->lay.n_groups, c->cam,
                         *opts, nb, c->stream, c->calib_on ? c->calib + b0 : nullptr, c->calib_on ? c->cl.cam_dim : 0,
                         (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0))
      return XIVO_HIP_ERR_HIP;
  }
  HIP_TRY(hipMemcpyAsync(feats, c->sub, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

// Criteria::CandidateComparison (src/options.cpp:34-61) and the selection order of SelectAndAddNewFeatures /
// AddFeaturesToState-style loops (src/manager.cpp:364-376,417-421): host arithmetic on the array
// xivo_hip_subfilter_update returned - no device work.
int xivo_hip_candidate_order(const xivo_subfilter_feat* feats, int nb, int n, int strict, int score_type, int* order_out,
                             int* n_out, double* score_out) {
  if (!feats || nb < 0 || n <= 0 || !order_out || !n_out || score_type < 0 || score_type > 2) return XIVO_HIP_ERR_INVALID;
  for (int b = 0; b < nb; ++b) {
    const xivo_subfilter_feat* f = feats + (size_t)b * n;
    std::vector<int> idx;
    for (int i = 0; i < n; ++i) {
      if (score_out) {
        const double dn = sqrt(f[i].P[0] * f[i].P[0] + f[i].P[4] * f[i].P[4] + f[i].P[8] * f[i].P[8]);   // P().diagonal().norm()
        score_out[(size_t)b * n + i] = score_type == 0 ? -1.0 * f[i].P[8] : (score_type == 1 ? -1.0 * dn : -1.0 * (dn + f[i].outlier_counter));
      }
      if (f[i].candidate & (strict ? 2 : 1)) idx.push_back(i);
    }
    // as coded, the comparison ignores the score it has just computed from comparison_score_type and orders by
    // status, then Feature::score() = -P(2,2) (options.cpp:60); FeatureStatus READY = 2 > INITIALIZING = 1 (core.h:190-199).
    // std::sort leaves the order of equivalent elements unspecified: here ties keep the list order.
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int c2) {
      const int s1 = f[a].status == XIVO_FEAT_READY ? 2 : 1, s2 = f[c2].status == XIVO_FEAT_READY ? 2 : 1;
      return (s1 > s2) || (s1 == s2 && -f[a].P[8] > -f[c2].P[8]);
    });
    n_out[b] = (int)idx.size();
    for (int i = 0; i < n; ++i) order_out[(size_t)b * n + i] = i < (int)idx.size() ? idx[i] : -1;
  }
  return XIVO_HIP_OK;
}

// ---- out-of-state feature pool
}  // extern "C"
namespace xivo_hip::capi {
// one pool step of filters [0, B) on the context's pool: everything but where the pixels come from and the results go (xp, order,
// n, live) - xivo_hip_pool_step points them at its per-call staging, xivo_hip_pool_life_begin at its resident buffers
PoolStepArgs pool_step_args(xivo_hip_ctx* c, int B, int strict) {
  PoolStepArgs a{};
  a.pool = c->fpool; a.anchors = c->anchors; a.pool_max = c->pool_max; a.anchor_max = c->anchor_max;
  a.poses = c->poses; a.groups = c->groups; a.n_groups = c->lay.n_groups;
  a.cam = c->cam; a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  a.o = c->pool_opts; a.remove_outlier = c->pool_remove_outlier; a.strict = strict ? 1 : 0; a.batch = B;
  a.tri = c->pool_tri; a.tri_good = c->tri_counts; a.tri_bad = c->tri_counts + c->Bmax;
  return a;
}
}  // namespace xivo_hip::capi
extern "C" {
static int ensure_pool_io(xivo_hip_ctx* c, size_t bytes) { return c->mem.grow(&c->pool_io, &c->pool_io_cap, bytes); }

int xivo_hip_pool_config(xivo_hip_ctx* c, int pool_max, int anchor_max, const xivo_subfilter_opts* opts,
                         double remove_outlier_counter) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || pool_max < 1 || anchor_max < 1 || !opts) return XIVO_HIP_ERR_INVALID;
  if (pool_max > XIVO_POOL_MAX_ENTRIES) return XIVO_HIP_ERR_UNSUPPORTED;
  HIP_TRY(hipStreamSynchronize(c->stream));
  pool_life_release(c);   // the device pool life cycle's books describe the pool given back here
  c->mem.release(&c->fpool, &c->anchors, &c->tri_counts, &c->init_z);
  c->pool_max = c->anchor_max = 0;
  c->pool_tri = xivo_triangulate_opts{}; c->adapt = xivo_adapt_depth_opts{}; c->adapt_on = false;
  const size_t ne = (size_t)c->Bmax * pool_max, na = (size_t)c->Bmax * anchor_max;
  int rc = c->mem.raw(&c->fpool, ne);
  if (!rc) rc = c->mem.raw(&c->anchors, na);
  if (!rc) rc = c->mem.raw(&c->tri_counts, 2 * (size_t)c->Bmax);
  if (!rc) rc = c->mem.raw(&c->init_z, (size_t)c->Bmax);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->tri_counts, 0, 2 * (size_t)c->Bmax * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->init_z, 0, (size_t)c->Bmax * sizeof(double), c->stream));
  // all bytes 0xff: every entry's anchor (ref_sind) and every anchor's slot read -1 - free / unlinked
  HIP_TRY(hipMemsetAsync(c->fpool, 0xff, ne * sizeof(xivo_subfilter_feat), c->stream));
  HIP_TRY(hipMemsetAsync(c->anchors, 0xff, na * sizeof(PoolAnchor), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pool_anchor_h.assign(ne, -1);
  c->anchor_link_h.assign(na, -2);   // -2: never created (xivo_hip_pool_anchor), -1: unlinked, >= 0: linked slot
  c->pool_max = pool_max; c->anchor_max = anchor_max;
  c->pool_opts = *opts; c->pool_remove_outlier = remove_outlier_counter;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_anchor(xivo_hip_ctx* c, int b0, int nb, const int* slot) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->fpool || c->plife_on || !c->poses || (nb > 0 && !slot)) return XIVO_HIP_ERR_INVALID;
  for (int b = 0; b < nb; ++b) {
    if (slot[b] < -1 || slot[b] >= c->anchor_max) return XIVO_HIP_ERR_INVALID;
    if (slot[b] >= 0 && c->anchor_link_h[(size_t)(b0 + b) * c->anchor_max + slot[b]] >= 0) return XIVO_HIP_ERR_INVALID;   // linked
  }
  if (nb == 0) return XIVO_HIP_OK;
  int rc = ensure_pool_io(c, (size_t)nb * sizeof(int));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->pool_io, slot, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_anchor_kernel");
    HIP_TRY((hipError_t)launch_pool_anchor(c->anchors + (size_t)b0 * c->anchor_max, c->anchor_max, c->poses + b0,
                                           (const int*)c->pool_io, nb, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // slot is borrowed host memory
  for (int b = 0; b < nb; ++b)
    if (slot[b] >= 0) c->anchor_link_h[(size_t)(b0 + b) * c->anchor_max + slot[b]] = -1;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_add(xivo_hip_ctx* c, int n, const xivo_pool_new* recs) { return xivo_hip_pool_add_ex(c, n, recs, 0u); }

int xivo_hip_pool_add_ex(xivo_hip_ctx* c, int n, const xivo_pool_new* recs, unsigned options) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->fpool || c->plife_on || !c->have_layout || n < 0 || (n > 0 && !recs)) return XIVO_HIP_ERR_INVALID;
  if ((options & ~XIVO_POOL_ADD_ADAPTIVE_Z) != 0u) return XIVO_HIP_ERR_INVALID;
  const bool adaptive = (options & XIVO_POOL_ADD_ADAPTIVE_Z) != 0u;
  if (adaptive && !c->adapt_on) return XIVO_HIP_ERR_INVALID;
  std::vector<long> keys((size_t)n);
  for (int i = 0; i < n; ++i) {
    const xivo_pool_new& r = recs[i];
    if (r.b < 0 || r.b >= c->Bmax || r.entry < 0 || r.entry >= c->pool_max || r.anchor < 0 || r.anchor >= c->anchor_max ||
        c->anchor_link_h[(size_t)r.b * c->anchor_max + r.anchor] == -2 || (!adaptive && !(r.z0 > 0.0)))
      return XIVO_HIP_ERR_INVALID;
    keys[i] = (long)r.b * c->pool_max + r.entry;
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return XIVO_HIP_ERR_INVALID;   // one record per entry
  if (n == 0) return XIVO_HIP_OK;
  int rc = ensure_pool_io(c, (size_t)n * sizeof(xivo_pool_new));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->pool_io, recs, (size_t)n * sizeof(xivo_pool_new), hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_add_kernel");
    HIP_TRY((hipError_t)launch_pool_add(c->fpool, c->pool_max, (const xivo_pool_new*)c->pool_io, n, c->cam,
                                        c->calib_on ? c->calib : nullptr, c->calib_on ? c->cl.cam_dim : 0,
                                        (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0, c->stream, adaptive ? c->init_z : nullptr));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // recs is borrowed host memory
  for (int i = 0; i < n; ++i) c->pool_anchor_h[(size_t)recs[i].b * c->pool_max + recs[i].entry] = recs[i].anchor;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_step(xivo_hip_ctx* c, int B, const double* xp, int strict, int* order_out, int* n_out,
                       unsigned char* live_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->fpool || c->plife_on || !c->have_layout || !c->poses || B <= 0 || B > c->Bmax || !xp || !order_out || !n_out ||
      !live_out)
    return XIVO_HIP_ERR_INVALID;
  const size_t ne = (size_t)B * c->pool_max;
  const size_t b_xp = ne * 2 * sizeof(double), b_ord = ne * sizeof(int), b_n = (size_t)B * sizeof(int);
  int rc = ensure_pool_io(c, b_xp + b_ord + b_n + ne);
  if (rc) return rc;
  char* io = c->pool_io;
  PoolStepArgs a = pool_step_args(c, B, strict);
  a.xp = (const double*)io; a.order = (int*)(io + b_xp); a.n = (int*)(io + b_xp + b_ord);
  a.live = (unsigned char*)(io + b_xp + b_ord + b_n);
  HIP_TRY(hipMemcpyAsync(io, xp, b_xp, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_step_kernel");
    HIP_TRY((hipError_t)launch_pool_step(a, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(order_out, a.order, b_ord, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(n_out, a.n, b_n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(live_out, a.live, ne, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < ne; ++i)
    if (!live_out[i]) c->pool_anchor_h[i] = -1;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_get(xivo_hip_ctx* c, int b0, int nb, xivo_subfilter_feat* entries, xivo_group_in* anchor_poses,
                      int* anchor_slots) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->fpool) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (entries)
    HIP_TRY(hipMemcpyAsync(entries, c->fpool + (size_t)b0 * c->pool_max, (size_t)nb * c->pool_max * sizeof(xivo_subfilter_feat),
                           hipMemcpyDeviceToHost, c->stream));
  std::vector<PoolAnchor> anc;
  if (anchor_poses || anchor_slots) {
    anc.resize((size_t)nb * c->anchor_max);
    HIP_TRY(hipMemcpyAsync(anc.data(), c->anchors + (size_t)b0 * c->anchor_max, anc.size() * sizeof(PoolAnchor),
                           hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < anc.size(); ++i) {
    if (anchor_poses) anchor_poses[i] = anc[i].g;
    if (anchor_slots) anchor_slots[i] = anc[i].slot;
  }
  return XIVO_HIP_OK;
}

// ---- depth initialisation of new tracks: triangulation and AdaptInitialDepth
static bool tri_opts_ok(const xivo_triangulate_opts* o) {
  return o->struct_size == (int)sizeof(xivo_triangulate_opts) && o->method >= XIVO_TRI_OFF && o->method <= XIVO_TRI_LINF;
}

int xivo_hip_triangulate(xivo_hip_ctx* c, int n, const xivo_tri_in* in, xivo_tri_out* out, const xivo_triangulate_opts* o) {
  if (!c || n < 0 || !o || (n > 0 && (!in || !out)) || !tri_opts_ok(o) || o->method == XIVO_TRI_OFF) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (n == 0) return XIVO_HIP_OK;
  const size_t bi = (size_t)n * sizeof(xivo_tri_in), bo = (size_t)n * sizeof(xivo_tri_out);
  int rc = ensure_pool_io(c, bi + bo);
  if (rc) return rc;
  char* io = c->pool_io;
  HIP_TRY(hipMemcpyAsync(io, in, bi, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "triangulate_kernel");
    HIP_TRY((hipError_t)launch_triangulate((const xivo_tri_in*)io, (xivo_tri_out*)(io + bi), n, *o, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(out, io + bi, bo, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_triangulation(xivo_hip_ctx* c, const xivo_triangulate_opts* o) {
  if (!c || !c->fpool || (o && !tri_opts_ok(o))) return XIVO_HIP_ERR_INVALID;
  c->pool_tri = o ? *o : xivo_triangulate_opts{};
  return XIVO_HIP_OK;
}

int xivo_hip_pool_tri_counts(xivo_hip_ctx* c, int b0, int nb, int* good_out, int* bad_out) {
  if (bad_range(c, b0, nb) || !c->tri_counts) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (nb == 0) return XIVO_HIP_OK;
  if (good_out)
    HIP_TRY(hipMemcpyAsync(good_out, c->tri_counts + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (bad_out)
    HIP_TRY(hipMemcpyAsync(bad_out, c->tri_counts + c->Bmax + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_adapt_depth_config(xivo_hip_ctx* c, const xivo_adapt_depth_opts* o) {
  if (!c || !c->init_z || !o || o->struct_size != (int)sizeof(xivo_adapt_depth_opts) || !(o->initial_z > 0.0) ||
      !(o->median_weight >= 0.0 && o->median_weight <= 1.0))
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  std::vector<double> z((size_t)c->Bmax, o->initial_z);
  HIP_TRY(hipMemcpyAsync(c->init_z, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->adapt = *o; c->adapt_on = true;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_adapt_depth(xivo_hip_ctx* c, int B, double* init_z_out) {
  if (!c || !c->fpool || !c->adapt_on || B <= 0 || B > c->Bmax) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (adapt_depth_lds(c->feats ? c->F : 0, c->pool_max) > 60 * 1024) return XIVO_HIP_ERR_UNSUPPORTED;
  int rc = ensure_pool_io(c, (size_t)B * sizeof(double));
  if (rc) return rc;
  AdaptDepthArgs a{};
  a.feats = c->feats; a.F = c->feats ? c->F : 0; a.Fmax = c->Fmax;
  a.pool = c->fpool; a.pool_max = c->pool_max;
  a.init_z = c->init_z; a.init_z_out = (double*)c->pool_io;
  a.beta = c->adapt.median_weight; a.min_z = c->adapt.min_z; a.max_z = c->adapt.max_z;
  a.min_lifetime = c->adapt.min_feature_lifetime; a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "adapt_depth_kernel");
    HIP_TRY((hipError_t)launch_adapt_depth(a, c->stream));
  }
  if (init_z_out) HIP_TRY(hipMemcpyAsync(init_z_out, a.init_z_out, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_get_init_z(xivo_hip_ctx* c, int b0, int nb, double* init_z_out) {
  if (bad_range(c, b0, nb) || !c->init_z || !c->adapt_on || (nb > 0 && !init_z_out)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(init_z_out, c->init_z + b0, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_absorb_error(xivo_hip_ctx* c, int B) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0 || !c->mask) return XIVO_HIP_ERR_INVALID;
  AbsorbArgs a{};
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.mask = c->mask; c->err.to(a.err, a.strideErr);
  a.lay = c->lay; a.F = c->F; a.Fmax = c->Fmax; a.batch = B; a.counter = c->absorb_count; a.status = c->status;
  a.calib = (c->calib_on || c->calib_motion) ? c->calib : nullptr; a.cl = c->cl;
  c->dx_clear();   // the kernel zeroes dx
  StageTimer st(c, ST_OTHER, 0.0, "absorb_error_kernel");
  return launch_absorb_error(a, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_edit_batch(xivo_hip_ctx* c, int F, int n_ops, const xivo_edit_op* ops) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || !c->poses || F <= 0 || 2 * F > c->Mmax || n_ops < 0 || (n_ops > 0 && !ops))
    return XIVO_HIP_ERR_INVALID;
  int rc = ensure_gate_buffers(c, F);
  if (rc) return rc;
  const xivo_layout& L = c->lay;
  std::vector<int> wg_filter, wg_begin;
  std::vector<std::pair<int*, int>> undo;
  for (int o = 0; o < n_ops; ++o) {
    const xivo_edit_op& e = ops[o];
    if (e.b < 0 || e.b >= c->Bmax || (o > 0 && e.b < ops[o - 1].b)) {
      for (size_t k = undo.size(); k-- > 0;) *undo[k].first = undo[k].second;
      return XIVO_HIP_ERR_INVALID;
    }
    bool ok = false;
    switch (e.kind) {
      case XIVO_EDIT_P_ZERO_RC: ok = e.i0 >= 0 && e.i1 >= 0 && e.i0 + e.i1 <= c->N; break;
      case XIVO_EDIT_P_COPY_RC: ok = e.i0 >= 0 && e.i1 >= 0 && e.i2 >= 0 && e.i0 + e.i2 <= c->N && e.i1 + e.i2 <= c->N; break;
      case XIVO_EDIT_P_SET_BLOCK3: ok = e.i0 >= 0 && e.i0 + 3 <= c->N; break;
      case XIVO_EDIT_ADD_GROUP: case XIVO_EDIT_REMOVE_GROUP: ok = e.i0 >= 0 && e.i0 < L.n_groups; break;
      case XIVO_EDIT_ADD_FEATURE:
        ok = e.i0 >= 0 && e.i0 < F && e.i1 >= 0 && e.i1 < L.n_features && e.i2 >= 0 && e.i2 < L.n_groups; break;
      case XIVO_EDIT_REMOVE_FEATURE: case XIVO_EDIT_SET_XP: ok = e.i0 >= 0 && e.i0 < F; break;
      case XIVO_EDIT_ADD_GROUP_ANCHOR:
        ok = c->fpool && !c->plife_on && e.i0 >= 0 && e.i0 < L.n_groups && e.i1 >= 0 && e.i1 < c->anchor_max &&
             c->anchor_link_h[(size_t)e.b * c->anchor_max + e.i1] == -1;
        for (int k = 0; ok && k < c->anchor_max; ++k) ok = c->anchor_link_h[(size_t)e.b * c->anchor_max + k] != e.i0;
        break;
      case XIVO_EDIT_ADMIT_POOL:
        ok = c->fpool && !c->plife_on && e.i0 >= 0 && e.i0 < F && e.i1 >= 0 && e.i1 < L.n_features && e.i2 >= 0 && e.i2 < c->pool_max;
        if (ok) {
          const int anc = c->pool_anchor_h[(size_t)e.b * c->pool_max + e.i2];
          ok = anc >= 0 && c->anchor_link_h[(size_t)e.b * c->anchor_max + anc] >= 0;
        }
        break;
      default: ok = false;
    }
    // the pool's host mirrors follow the ops in order (an op may rely on a link an earlier op of the call makes); undone
    // when a later op is rejected
    if (ok && c->fpool) {
      auto set = [&](int& slot, int v) { undo.emplace_back(&slot, slot); slot = v; };
      if (e.kind == XIVO_EDIT_ADD_GROUP_ANCHOR) set(c->anchor_link_h[(size_t)e.b * c->anchor_max + e.i1], e.i0);
      if (e.kind == XIVO_EDIT_REMOVE_GROUP)
        for (int k = 0; k < c->anchor_max; ++k)
          if (c->anchor_link_h[(size_t)e.b * c->anchor_max + k] == e.i0) set(c->anchor_link_h[(size_t)e.b * c->anchor_max + k], -1);
      if (e.kind == XIVO_EDIT_ADMIT_POOL) set(c->pool_anchor_h[(size_t)e.b * c->pool_max + e.i2], -1);
    }
    if (!ok) {
      for (size_t k = undo.size(); k-- > 0;) *undo[k].first = undo[k].second;
      return XIVO_HIP_ERR_INVALID;
    }
    if (o == 0 || e.b != ops[o - 1].b) { wg_filter.push_back(e.b); wg_begin.push_back(o); }
  }
  c->F = F;
  if (n_ops == 0) return XIVO_HIP_OK;
  wg_begin.push_back(n_ops);
  const int n_wg = (int)wg_filter.size();
  const size_t bytes_ops = (size_t)n_ops * sizeof(xivo_edit_op);
  const size_t bytes = bytes_ops + (size_t)(2 * n_wg + 1) * sizeof(int);
  if (bytes > c->edit_cap) {   // (twice the request: the op lists of consecutive frames differ by a few entries)
    rc = c->mem.grow(&c->edit_buf, &c->edit_cap, bytes * 2);
    if (rc) return rc;
  }
  char* d = c->edit_buf;
  HIP_TRY(hipMemcpyAsync(d, ops, bytes_ops, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + bytes_ops, wg_filter.data(), (size_t)n_wg * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + bytes_ops + (size_t)n_wg * sizeof(int), wg_begin.data(), (size_t)(n_wg + 1) * sizeof(int),
                         hipMemcpyHostToDevice, c->stream));
  EditArgs a{};
  a.ops = (const xivo_edit_op*)d; a.wg_filter = (const int*)(d + bytes_ops); a.wg_begin = a.wg_filter + n_wg;
  c->P.to(a.P, a.strideP, a.ldp); a.Np = c->Np; a.lay = L;
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.Fmax = c->Fmax;
  a.pool = c->fpool; a.anchors = c->anchors; a.pool_max = c->pool_max; a.anchor_max = c->anchor_max;
  {
    StageTimer st(c, ST_OTHER, 0.0, "edit_batch_kernel");
    HIP_TRY((hipError_t)launch_edit_batch(a, n_wg, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // the host vectors above are pageable staging
  return XIVO_HIP_OK;
}

int xivo_hip_set_pixels(xivo_hip_ctx* c, int b0, int nb, int F, const double* xp) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || F <= 0 || 2 * F > c->Mmax || !xp) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  int rc = ensure_gate_buffers(c, F);
  if (rc) return rc;
  rc = ensure_staging(c, (size_t)nb * F * 2);
  if (rc) return rc;
  c->F = F;
  HIP_TRY(hipMemcpyAsync(c->staging, xp, (size_t)nb * F * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY((hipError_t)launch_set_pixels(c->feats + (size_t)b0 * c->Fmax, c->Fmax, F, c->staging, nb, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // xp is borrowed host memory
  return XIVO_HIP_OK;
}

int xivo_hip_get_scene(xivo_hip_ctx* c, int b0, int nb, xivo_pose_in* poses, xivo_group_in* groups, xivo_feat_in* feats) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (poses) HIP_TRY(hipMemcpyAsync(poses, c->poses + b0, (size_t)nb * sizeof(xivo_pose_in), hipMemcpyDeviceToHost, c->stream));
  if (groups) HIP_TRY(hipMemcpyAsync(groups, c->groups + (size_t)b0 * c->lay.n_groups,
                                     (size_t)nb * c->lay.n_groups * sizeof(xivo_group_in), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (feats && c->F > 0) {
    int rc = d2h_rows(c, feats, (size_t)c->F * sizeof(xivo_feat_in), c->feats + (size_t)b0 * c->Fmax,
                      (size_t)c->Fmax * sizeof(xivo_feat_in), (size_t)c->F * sizeof(xivo_feat_in), nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_get_H(xivo_hip_ctx* c, int b, int* M_out, double* H, int ldh, double* inn, double* diagR) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const int M = c ? c->rows.rows() : 0;
  if (bad_range(c, b, 1) || M <= 0) return XIVO_HIP_ERR_INVALID;
  if (M_out) *M_out = M;
  if (H) {
    if (ldh < M) return XIVO_HIP_ERR_INVALID;
    { int rcd = ensure_dense(c); if (rcd) return rcd; }
    HIP_TRY(hipMemcpy2DAsync(H, (size_t)ldh * sizeof(double), c->H.from(b).p, (size_t)c->H.ld * sizeof(double),
                             (size_t)M * sizeof(double), c->N, hipMemcpyDeviceToHost, c->stream));
  }
  if (inn) HIP_TRY(hipMemcpyAsync(inn, c->inn.from(b).p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (diagR) HIP_TRY(hipMemcpyAsync(diagR, c->diagR.from(b).p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

// test hook (no device, no context): the launch choice of a feature-level or propagation kernel for a shape, from the same
// function the launch calls (include/xivo_hip.h)
int xivo_hip_selftest_glevel_launch(int kind, int a, int b, int c, char* label, int n) {
  const size_t ln = label && n > 0 ? (size_t)n : 0;
  if (ln) label[0] = 0;
  switch (kind) {
    case XIVO_HIP_LAUNCH_GATE:
      if (a <= 0 || b <= 0) return XIVO_HIP_ERR_INVALID;
      return gate_sparse_threads(a, b, c ? 1 : 0, label, ln);
    case XIVO_HIP_LAUNCH_OOS_COMPRESS:
      if (a <= 0 || b <= 0) return XIVO_HIP_ERR_INVALID;
      return oos_compress_pick(a, b, label, ln);
    case XIVO_HIP_LAUNCH_PROP_TAIL:
      return propagate_cov_pick(a, b, label, ln);
    default:
      return XIVO_HIP_ERR_INVALID;
  }
}

}  // extern "C"
