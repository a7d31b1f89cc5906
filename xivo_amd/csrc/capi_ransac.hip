// C ABI, OnePointRANSAC on the resident state (include/xivo_hip.h). Host-side orchestration only (capi_internal.h).
#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

extern "C" {

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
  if (bad_gate_params({R, ransac_thresh, 1.0, 0}) || ransac_chi2 != ransac_chi2) return XIVO_HIP_ERR_INVALID;
  if (c->tune.configured()) return XIVO_HIP_ERR_UNSUPPORTED;   // tuning table: one parameter set for all filters is not applied silently
  const size_t Bm = c->Bmax, ng = c->lay.n_groups;
  // online-calibration builds: the calibration state is backed up / restored with X_ (imu_.BackupState, Camera::BackupState,
  // src/estimator.cpp:1421-1427), the partial update stacks the whole rows J() as dense rows, AbsorbError retracts td / Cg / Ca /
  // the intrinsics too, and the rescue test uses the whole-row distances of the dense-row gate
  const bool cal = c->calib_on;
  if (cal && !c->rs.calib) { int rc = c->mem.zeroed(&c->rs.calib, Bm); if (rc) return rc; }
  if (!c->rs.sized_for(c->Fmax)) {   // first use (Fmax never changes once it is set: ensure_gate_buffers)
    int rc = XIVO_HIP_OK;
    auto A = [&](auto** p, size_t n) { if (rc == XIVO_HIP_OK) rc = c->mem.zeroed(p, n); };
    A(&c->rs.P, Bm * c->P.stride); A(&c->rs.poses, Bm); A(&c->rs.groups, Bm * ng);
    A(&c->rs.low, Bm * c->Fmax); A(&c->rs.lowkeep, Bm * c->Fmax); A(&c->rs.keep, Bm * c->Fmax); A(&c->rs.chi, Bm * c->Fmax);
    A(&c->rs.zg, Bm); A(&c->rs.gmask, Bm); A(&c->rs.state, Bm); A(&c->rs.gauge, Bm); A(&c->rs.nrej, Bm);
    if (rc) return rc;
    c->rs.Fmax = c->Fmax;
  }
  if (gauge_group) HIP_TRY(hipMemcpyAsync(c->rs.gauge, gauge_group, (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
  else HIP_TRY(hipMemsetAsync(c->rs.gauge, 0xFF, (size_t)B * sizeof(int), c->stream));
  if (absorb_groups) HIP_TRY(hipMemcpyAsync(c->rs.gmask, absorb_groups, (size_t)B * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  RansacArgs a{};
  a.sb = scene_buffers(c); a.lay = c->lay; c->P.to(a.P, a.strideP, a.ldp); a.Np = c->Np;
  a.R = R; a.thresh = ransac_thresh; a.chi2 = ransac_chi2; a.gauge = c->rs.gauge;
  a.low = c->rs.low; a.low_keep = c->rs.lowkeep; a.zero_groups = c->rs.zg; a.state = c->rs.state;
  a.keep = c->rs.keep; a.chi = c->rs.chi; a.n_rejected = c->rs.nrej; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "ransac_select_kernel");
    HIP_TRY((hipError_t)launch_ransac_select(a, c->stream));
  }
  // the low-innovation set as select found it (filters with nothing to update get an all-neutral stacking mask)
  HIP_TRY(hipMemcpyAsync(c->rs.lowkeep, c->rs.low, (size_t)B * c->Fmax, hipMemcpyDeviceToDevice, c->stream));
  // BackupState (src/estimator.cpp:1410-1428)
  HIP_TRY(hipMemcpyAsync(c->rs.P, c->P.p, (size_t)B * c->P.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->rs.poses, c->poses, (size_t)B * sizeof(xivo_pose_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->rs.groups, c->groups, (size_t)B * ng * sizeof(xivo_group_in), hipMemcpyDeviceToDevice, c->stream));
  if (cal) HIP_TRY(hipMemcpyAsync(c->rs.calib, c->calib, (size_t)B * sizeof(xivo_calib_in), hipMemcpyDeviceToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "ransac_zero_kernel");
    HIP_TRY((hipError_t)launch_ransac_zero(a, c->P.p, c->stream));
  }
  // partial update: H_ rows = the full J() of the low-innovation inliers (:326 - no FillJacobianBlock), R_ on the diagonal
  const int dense = ((c->flags & XIVO_HIP_FLAG_DENSE_H) || cal) ? 1 : 0;
  const CalibCols cc = cal ? CalibCols::in_rows : CalibCols::none;
  c->rows.stacked(B, c->F, R, Stacking::full_rows, /*pw=*/9, /*dense=*/dense != 0, cc);
  int rc = stack_impl(c, B, R, dense, c->rs.low, 1);
  if (rc) return rc;
  rc = xivo_hip_update_joseph(c, B);
  if (rc) return rc;
  c->dx_clear();   // (the partial update's dx is absorbed right here and the state restored: nothing to record)
  {  // AbsorbError (:333): in_current_ekf_update_ is empty at this point of Estimator::UpdateStep (cleared at
     // src/manager.cpp:28, filled after OutlierRejection), so no feature state moves; State::counter is restored with X_
    AbsorbArgs ab{};
    ab.poses = c->poses; ab.groups = c->groups; ab.feats = c->feats; ab.mask = nullptr; c->err.to(ab.err, ab.strideErr);
    ab.lay = c->lay; ab.F = c->F; ab.Fmax = c->Fmax; ab.batch = B; ab.counter = nullptr; ab.status = c->status;
    ab.group_mask = absorb_groups ? c->rs.gmask : nullptr;
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
    ga.mask = c->rs.low; ga.dist = c->rs.chi; ga.F = c->F; ga.mask_ld = c->Fmax;
    ga.gp = {R, ransac_chi2, 1.0, -1}; ga.no_relax = 1;
    ga.have_ell = 0; ga.feats = c->feats; ga.Fmax = c->Fmax;
    rc = gate_dense_rows(c, B, ga);
    if (rc) return rc;
    StageTimer st(c, ST_OTHER, 0.0, "ransac_rescue_dist_kernel");
    HIP_TRY((hipError_t)launch_ransac_rescue_dist(a, c->rs.chi, c->Fmax, c->stream));
  }
  // RestoreState + Jacobians at the original state (:383-387)
  HIP_TRY(hipMemcpyAsync(c->P.p, c->rs.P, (size_t)B * c->P.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->poses, c->rs.poses, (size_t)B * sizeof(xivo_pose_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->groups, c->rs.groups, (size_t)B * ng * sizeof(xivo_group_in), hipMemcpyDeviceToDevice, c->stream));
  if (cal) HIP_TRY(hipMemcpyAsync(c->calib, c->rs.calib, (size_t)B * sizeof(xivo_calib_in), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->mask, c->rs.keep, (size_t)B * c->Fmax, hipMemcpyDeviceToDevice, c->stream));
  rc = xivo_hip_jacobians_instate(c, B);
  if (rc) return rc;
  c->rows.gate_wrote(GateLayout::strided);
  const size_t F = c->F, Fm = c->Fmax;
  if (inlier_mask_out) { rc = d2h_rows(c, inlier_mask_out, F, c->mask, Fm, F, B); if (rc) return rc; }
  if (chi2_out) { rc = d2h_rows(c, chi2_out, F * sizeof(double), c->rs.chi, Fm * sizeof(double), F * sizeof(double), B); if (rc) return rc; }
  if (n_rejected_out) HIP_TRY(hipMemcpyAsync(n_rejected_out, c->rs.nrej, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // gauge_group / absorb_groups are borrowed host memory
  return XIVO_HIP_OK;
}

}  // extern "C"
