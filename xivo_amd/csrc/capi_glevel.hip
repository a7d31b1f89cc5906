// C ABI, feature level (include/xivo_hip.h): layout, scene, calibration, Jacobians, MH gating, stacking, filter_update, absorb,
// edits, pixels, read-back of the scene and the stacked rows. Host-side orchestration only (capi_internal.h).
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

int gate_impl(xivo_hip_ctx* c, int B, const GateParams& gp, int use_gating) {
  GateArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; c->P.to(a.P, a.strideP, a.ldp);
  a.gp = gp; a.batch = B; a.use_gating = use_gating;
  a.tune_R = c->tune.R; a.tune_thresh = c->tune.thresh;   // (tuning table: null without one)
  char label[64];
  gate_sparse_threads(B, a.sb.F, a.sb.Jc ? 1 : 0, label, sizeof(label));
  StageTimer st(c, ST_GATE, 0.0, label);
  c->rows.gate_wrote(GateLayout::strided);
  return launch_gate_sparse(a, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

// Estimator::MHGating of an online-calibration build: the gate needs the WHOLE row J() incl. the td / Cg / bg / intrinsics
// blocks (update.cpp:60-70), which is not the row FillJacobianBlock stacks (the :675-676 overwrite): every present feature is
// stacked once as its full J() (dense rows) and gated on (J P) J^T + R by the dense-row gate. gate = 0: every present feature
// is an inlier (Estimator::OutlierRejection does not gate F <= min_required_inliers_, src/manager.cpp:635).
int calib_gate(xivo_hip_ctx* c, int B, const GateParams& gp, int gate) {
  int rc = gate_impl(c, B, gp, 0);
  if (rc) return rc;
  if (gate) {
    c->rows.stacked(B, c->F, gp.R, Stacking::full_rows, /*pw=*/9, /*dense=*/true, CalibCols::in_rows);
    c->dx_clear();
    rc = stack_impl(c, B, gp.R, 1, nullptr, /*full_rows=*/1);
    if (rc) return rc;
    GateDenseArgs a{};
    a.mask = c->mask; a.dist = c->dist; a.F = c->F; a.mask_ld = c->Fmax;   // (the stride xivo_hip_stack reads the mask with)
    a.gp = gp; a.have_ell = 0;
    a.feats = c->feats; a.Fmax = c->Fmax;        // absent entries of ragged batches are no candidates (per-filter present count)
    return gate_dense_rows(c, B, a);   // (mask / dist stay in the strided layout gate_impl left)
  }
  return XIVO_HIP_OK;
}

}  // namespace

namespace xivo_hip::capi {

int stack_impl(xivo_hip_ctx* c, int B, double R, int write_dense, unsigned char* mask_override, int full_rows) {
  StackArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; a.mb = meas_buffers(c);
  if (mask_override) a.sb.mask = mask_override;
  a.Mp = c->Mpmax; a.Np = c->Np; a.batch = B; a.R = R;
  a.fix_group_block = (full_rows || (c->flags & XIVO_HIP_FLAG_FIX_GROUP_BLOCK)) ? 1 : 0;
  a.rows_instate = c->rows_instate;
  a.tune_R = c->tune.R;   // (tuning table: filter b's R in place of R - also when ensure_dense stacks again from restack_args())
  a.ell = c->ell; a.emit_ell = 1; a.write_dense = write_dense;
  // as-coded stacking of an online-calibration build on the sparse pipeline: compressed rows + the leading dense block
  // (full_rows - the whole-row stackings of the gate / RANSAC - stay dense rows)
  if (!full_rows && !write_dense && calib_sparse(c)) { a.lead = c->Hlead.p; a.strideLead = c->Hlead.stride; a.lead_k = LEAD_K; }
  StageTimer st(c, ST_STACK, 0.0, "stack_kernel");
  return launch_stack(a, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

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
  c->H.to(a.Hw, a.strideH, a.ldh); c->HT.to(a.HTw, a.strideHT, a.ldht); a.HPw = nullptr; a.PHTw = nullptr; a.PHTr = c->PHT.p;
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
  if (layout && c->tune.configured()) return XIVO_HIP_ERR_UNSUPPORTED;   // the tuning table has no calibration form
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
  const GateParams gp{R, mh_thresh, mh_mult, min_inliers};
  if (bad_gate_params(gp)) return XIVO_HIP_ERR_INVALID;
  // (online-calibration builds: the compact gate works on the whole row too - 43 columns, gate_sparse_kernel's wide form;
  //  with XIVO_HIP_FLAG_DENSE_H the dense-row gate of round 4)
  int rc = (c->calib_on && !calib_sparse(c)) ? calib_gate(c, B, gp, 1) : gate_impl(c, B, gp, 1);
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

int xivo_hip_filter_update(xivo_hip_ctx* c, int B, double R, double mh_thresh, double mh_mult, int min_inliers,
                           int use_gating) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  const GateParams gp{R, mh_thresh, mh_mult, min_inliers};
  if (bad_gate_params(gp)) return XIVO_HIP_ERR_INVALID;
  int rc = xivo_hip_jacobians_instate(c, B);
  if (rc) return rc;
  // Estimator::OutlierRejection only gates when F > min_required_inliers_ (src/manager.cpp:635)
  const int gate = use_gating && c->F > min_inliers;
  // online-calibration builds on dense rows (XIVO_HIP_FLAG_DENSE_H): the gate needs the WHOLE row J() incl. the td / Cg / bg / intrinsics blocks (update.cpp:60-70),
  // which is not the row FillJacobianBlock stacks (the :675-676 overwrite): every present feature is stacked once as its
  // full J() (dense rows), gated on (J P) J^T + R by the dense-row gate, then the inliers are stacked as coded and updated
  rc = (c->calib_on && !calib_sparse(c)) ? calib_gate(c, B, gp, gate) : gate_impl(c, B, gp, gate);
  if (rc) return rc;
  rc = xivo_hip_stack(c, B, R);
  if (rc) return rc;
  return xivo_hip_update_joseph(c, B);
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
  // the pool's host mirrors follow the ops in order (an op may rely on a link an earlier op of the call makes); a refused call
  // leaves them as they were (the Edit's destructor)
  const bool pool_edits = c->pool.configured() && !c->plife.configured();
  PoolMirror::Edit mirror(c->pool.mirror);
  for (int o = 0; o < n_ops; ++o) {
    const xivo_edit_op& e = ops[o];
    if (e.b < 0 || e.b >= c->Bmax || (o > 0 && e.b < ops[o - 1].b)) return XIVO_HIP_ERR_INVALID;
    bool ok = false;
    switch (e.kind) {
      case XIVO_EDIT_P_ZERO_RC: ok = e.i0 >= 0 && e.i1 >= 0 && e.i0 + e.i1 <= c->N; break;
      case XIVO_EDIT_P_COPY_RC: ok = e.i0 >= 0 && e.i1 >= 0 && e.i2 >= 0 && e.i0 + e.i2 <= c->N && e.i1 + e.i2 <= c->N; break;
      case XIVO_EDIT_P_SET_BLOCK3: ok = e.i0 >= 0 && e.i0 + 3 <= c->N; break;
      case XIVO_EDIT_ADD_GROUP: ok = e.i0 >= 0 && e.i0 < L.n_groups; break;
      case XIVO_EDIT_REMOVE_GROUP:
        ok = e.i0 >= 0 && e.i0 < L.n_groups;
        if (ok && c->pool.configured()) mirror.group_removed(e.b, e.i0);
        break;
      case XIVO_EDIT_ADD_FEATURE:
        ok = e.i0 >= 0 && e.i0 < F && e.i1 >= 0 && e.i1 < L.n_features && e.i2 >= 0 && e.i2 < L.n_groups; break;
      case XIVO_EDIT_REMOVE_FEATURE: case XIVO_EDIT_SET_XP: ok = e.i0 >= 0 && e.i0 < F; break;
      case XIVO_EDIT_ADD_GROUP_ANCHOR:
        ok = pool_edits && e.i0 >= 0 && e.i0 < L.n_groups && c->pool.mirror.can_anchor_group(e.b, e.i0, e.i1);
        if (ok) mirror.group_anchored(e.b, e.i0, e.i1);
        break;
      case XIVO_EDIT_ADMIT_POOL:
        ok = pool_edits && e.i0 >= 0 && e.i0 < F && e.i1 >= 0 && e.i1 < L.n_features && c->pool.mirror.can_admit(e.b, e.i2);
        if (ok) mirror.entry_admitted(e.b, e.i2);
        break;
      default: ok = false;
    }
    if (!ok) return XIVO_HIP_ERR_INVALID;
    if (o == 0 || e.b != ops[o - 1].b) { wg_filter.push_back(e.b); wg_begin.push_back(o); }
  }
  mirror.commit();
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
  a.pool = c->pool.entries; a.anchors = c->pool.anchors; a.pool_max = c->pool.pool_max(); a.anchor_max = c->pool.anchor_max();
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
