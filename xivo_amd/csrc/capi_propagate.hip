// C ABI, propagation (include/xivo_hip.h): the covariance tail on given transition matrices, and Estimator::Propagate of the
// default and the online-calibration builds (propagate_state* kernels + the tail). Host-side orchestration only
// (capi_internal.h).
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// What no sub-step loop may be handed (rk4.cpp:19, princedormand.cpp:38, :68 loop `while (total_step < dt)` with no cap on
// the count): a step that is NaN or in [0, 1e-6), and under control_stepsize (Dormand-Prince with a positive cfg step only) a
// growth factor below 1 - as coded the error estimate is 0 (:216-220), every step is followed by h *= max_scale_factor, and
// with a factor below 1 the steps form a convergent series: where its sum stays below dt, h underflows and the loop never ends.
bool prop_opts_bad(const xivo_prop_opts* o) {
  if (std::isnan(o->stepsize) || (o->stepsize >= 0 && o->stepsize < 1e-6)) return true;
  if (o->control_stepsize && (o->method != 1 || !(o->stepsize > 0) || !(o->max_scale_factor >= 1.0))) return true;
  return false;
}

// a sample's length: positive and finite (`while (total_step < dt)` never ends on dt = +inf)
bool prop_dt_bad(const xivo_imu_in* imu, size_t n) {
  for (size_t b = 0; b < n; ++b)
    if (!(imu[b].dt > 0.0) || !std::isfinite(imu[b].dt)) return true;
  return false;
}

// control_stepsize (src/princedormand.cpp:26-60). The reference's function-local static `h` starts at the cfg step (:23): one
// per filter here, reset when the cfg step changes. The options have passed prop_opts_bad.
int prop_step_control(xivo_hip_ctx* c, const xivo_prop_opts* o) {
  if (!o->control_stepsize) return XIVO_HIP_OK;
  if (c->pd_h && c->pd_h0 == o->stepsize) return XIVO_HIP_OK;
  if (!c->pd_h) { int rcd = c->mem.zeroed(&c->pd_h, (size_t)c->Bmax); if (rcd) return rcd; }
  std::vector<double> h0((size_t)c->Bmax, o->stepsize);
  HIP_TRY(hipMemcpy(c->pd_h, h0.data(), h0.size() * sizeof(double), hipMemcpyHostToDevice));
  c->pd_h0 = o->stepsize;
  return XIVO_HIP_OK;
}

// the arguments of the state kernel over device blocks: records, noise, and where Phi / P_mm go
void prop_args(xivo_hip_ctx* c, int b0, int nb, int n_imu, const xivo_imu_in* dImu, const double* dQi, const double* dQm,
               double* dPhi, double* dPmm, const xivo_prop_opts* o, PropStateArgs& a) {
  a = PropStateArgs{};
  a.poses = c->poses + b0; a.imu = dImu; a.n_imu = n_imu; a.Qimu = dQi; a.Qmodel = dQm;
  if (c->tune.configured()) {   // tuning table: the entries of filters [b0, b0 + nb) in place of the call's pair
    a.Qimu = c->tune.Qimu + (size_t)b0 * 144; a.strideQimu = 144;
    a.Qmodel = c->tune.Qmodel + (size_t)b0 * 529; a.strideQmodel = 529;
  }
  a.g[0] = o->g[0]; a.g[1] = o->g[1]; a.g[2] = o->g[2]; a.method = o->method; a.stepsize = o->stepsize;
  c->P.from(b0).to(a.P, a.strideP, a.ldp); a.Phi_out = dPhi; a.Pmm_out = dPmm; a.batch = nb;
  if (o->control_stepsize) {
    a.pd_h = c->pd_h + b0; a.pd_tol = o->tolerance; a.pd_min_scale = o->min_scale_factor; a.pd_max_scale = o->max_scale_factor;
  }
}

// the two launches of the default build: the state kernel and the tail over the 23 motion rows and columns; substeps: integrator
// sub-steps of one filter over the call (for the profile's flop count)
int prop_launch(xivo_hip_ctx* c, int b0, int nb, int n_imu, const PropStateArgs& a, double substeps) {
  {
    char plabel[64];
    snprintf(plabel, sizeof(plabel), "propagate_state_wave_kernel<%d>", a.method ? 7 : 4);
    // algorithmic flops: per integrator sub-step and stage the 23 x 23 Lyapunov right-hand side
    // F P + P F^T (2 * 2 * 23^3) and the transition recursion F + c F FK (2 * 23^3), as the reference codes them (dense);
    // sub-steps as src/rk4.cpp:19-31 cuts a sample: ceil(dt / stepsize), the sample's own dt when stepsize <= 0
    const double stage_flops = 6.0 * 23.0 * 23.0 * 23.0 + 2.0 * 23.0 * 12.0 * (12.0 + 23.0);
    StageTimer st(c, ST_PROP_STATE, (double)nb * substeps * (a.method ? 7.0 : 4.0) * stage_flops, plabel,
                  (double)nb * (3.0 * 529 + n_imu * sizeof(xivo_imu_in) / 8.0 + 60.0) * sizeof(double));
    HIP_TRY((hipError_t)launch_propagate_state(a, c->stream));
  }
  {
    // tail: reads and writes the 23 rows and 23 columns of P that change (+ Phi, P_mm)
    StageTimer st(c, ST_PROP_TAIL, (double)nb * 2.0 * (2.0 * 23.0 * 23.0 * (c->N - 23)), "propagate_cov_fixed_kernel<23>",
                  (double)nb * (4.0 * 23 * c->N + 2.0 * 529) * sizeof(double));
    HIP_TRY((hipError_t)launch_propagate_cov(c->P.p, c->P.stride, c->P.ld, c->N, c->Np, 23, a.Phi_out, a.Pmm_out, b0, nb, c->stream));
  }
  return XIVO_HIP_OK;
}

// What both integrators take: the staging block (Phi [nb][nm x nm] | P_mm [nb][nm x nm] | Qimu 12 x 12 | Qmodel nm x nm | imu),
// its uploads and the arguments of the state kernel the two share. The caller adds its own (nm, iCg, calib) and launches.
int prop_stage(xivo_hip_ctx* c, int b0, int nb, int n_imu, const xivo_imu_in* imu, const xivo_prop_opts* o, int nm,
               const double* Qmodel, PropStateArgs& a) {
  const size_t per = (size_t)nm * nm;
  const size_t imu_d = ((size_t)nb * n_imu * sizeof(xivo_imu_in) + 7) / 8;      // in doubles
  int rc = ensure_staging(c, 2 * per * nb + 144 + per + imu_d);
  if (rc) return rc;
  double* dPhi = c->staging; double* dPmm = dPhi + per * nb; double* dQi = dPmm + per * nb; double* dQm = dQi + 144;
  xivo_imu_in* dImu = reinterpret_cast<xivo_imu_in*>(dQm + per);
  HIP_TRY(hipMemcpyAsync(dQi, o->Qimu, 144 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dQm, Qmodel, per * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dImu, imu, (size_t)nb * n_imu * sizeof(xivo_imu_in), hipMemcpyHostToDevice, c->stream));
  prop_args(c, b0, nb, n_imu, dImu, dQi, dQm, dPhi, dPmm, o, a);
  return XIVO_HIP_OK;
}

}  // namespace

namespace xivo_hip::capi {

int propagate_device(xivo_hip_ctx* c, int B, int n_imu, const xivo_imu_in* recs, const double* dQimu, const double* dQmodel,
                     const xivo_prop_opts* o, double mean_dt) {
  if (bad_range(c, 0, B) || B <= 0 || !c->have_layout || !c->poses || !recs || !o || n_imu <= 0 || c->N < 23 || c->lay.group_begin < 23 ||
      prop_opts_bad(o))
    return XIVO_HIP_ERR_INVALID;
  // (the records' dt cannot be read here: they are device memory. xivo_hip_trajsim_frame, their only producer, refuses a
  //  sample index at which t_k = k imu_dt leaves the finite range, so every dt_k it writes is positive and finite)
  if (c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
  int rc = prop_step_control(c, o);
  if (rc) return rc;
  rc = ensure_staging(c, 2 * (size_t)529 * B);   // (sized by xivo_hip_trajsim_config: nothing happens here)
  if (rc) return rc;
  PropStateArgs a;
  prop_args(c, 0, B, n_imu, recs, dQimu, dQmodel, c->staging, c->staging + (size_t)529 * B, o, a);
  return prop_launch(c, 0, B, n_imu, a, n_imu * (o->stepsize > 0 ? std::ceil(mean_dt / o->stepsize) : 1.0));
}

}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_propagate_cov(xivo_hip_ctx* c, int b0, int nb, int nm, const double* Phi, const double* Pmm) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || nm <= 0 || nm > 40 || nm > c->N || !Phi || !Pmm) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t per = (size_t)nm * nm;
  int rc = ensure_staging(c, 2 * per * nb);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->staging, Phi, per * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->staging + per * nb, Pmm, per * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
  {
    char label[64];
    propagate_cov_pick(nm, c->N, label, sizeof(label));
    StageTimer st(c, ST_OTHER, 0.0, label);
    if (launch_propagate_cov(c->P.p, c->P.stride, c->P.ld, c->N, c->Np, nm, c->staging, c->staging + per * nb, b0, nb, c->stream))
      return XIVO_HIP_ERR_HIP;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_propagate(xivo_hip_ctx* c, int b0, int nb, int n_imu, const xivo_imu_in* imu, const xivo_prop_opts* o) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || !imu || !o || n_imu <= 0 || c->N < 23 || c->lay.group_begin < 23)
    return XIVO_HIP_ERR_INVALID;
  if (c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;   // kMotionSize > 23: xivo_hip_propagate_calib
  if (nb == 0) return XIVO_HIP_OK;
  if (prop_opts_bad(o) || prop_dt_bad(imu, (size_t)nb * n_imu)) return XIVO_HIP_ERR_INVALID;   // before any upload or launch
  int rc = prop_step_control(c, o);
  if (rc) return rc;
  PropStateArgs a;
  rc = prop_stage(c, b0, nb, n_imu, imu, o, 23, o->Qmodel, a);
  if (rc) return rc;
  double substeps = 0.0;
  for (int s = 0; s < n_imu; ++s) substeps += o->stepsize > 0 ? std::ceil(imu[s].dt / o->stepsize) : 1.0;
  rc = prop_launch(c, b0, nb, n_imu, a, substeps);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));   // imu / opts are borrowed host memory
  return XIVO_HIP_OK;
}

// Estimator::Propagate of an online-calibration build (kMotionSize = 24 / 38 / 39): propagate_state_calib_kernel + the
// run-time-nm tail
int xivo_hip_propagate_calib(xivo_hip_ctx* c, int b0, int nb, int n_imu, const xivo_imu_in* imu, const xivo_prop_opts* o,
                             const double* Qmodel) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // a tuning table: this call takes one Qimu / Qmodel for its range and must not apply it silently (such a context has no
  // calibration layout either, which the check below would refuse as invalid)
  if (c && c->tune.configured()) return XIVO_HIP_ERR_UNSUPPORTED;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || !imu || !o || !Qmodel || n_imu <= 0 || !c->calib_motion || !c->calib)
    return XIVO_HIP_ERR_INVALID;
  const int nm = c->cl.Cg >= 0 ? c->cl.Cg + 15 : c->cl.td + 1;
  if (nm > 40 || c->N < nm || c->lay.group_begin < nm) return XIVO_HIP_ERR_INVALID;
  // the options are judged before the empty-range return (unlike xivo_hip_propagate), every refusal before any upload or launch
  if (prop_opts_bad(o) || (nb > 0 && prop_dt_bad(imu, (size_t)nb * n_imu))) return XIVO_HIP_ERR_INVALID;
  int rc = prop_step_control(c, o);
  if (rc) return rc;
  if (nb == 0) return XIVO_HIP_OK;
  PropStateArgs a;
  rc = prop_stage(c, b0, nb, n_imu, imu, o, nm, Qmodel, a);
  if (rc) return rc;
  a.nm = nm; a.iCg = c->cl.Cg; a.calib = c->calib + b0;
  {
    char plabel[64];
    snprintf(plabel, sizeof(plabel), "propagate_state_calib_kernel<%d>", a.method ? 7 : 4);
    StageTimer st(c, ST_PROP_STATE, 0.0, plabel);
    HIP_TRY((hipError_t)launch_propagate_state_calib(a, c->stream));
  }
  {
    char label[64];
    propagate_cov_pick(nm, c->N, label, sizeof(label));
    StageTimer st(c, ST_PROP_TAIL, 0.0, label, (double)nb * (4.0 * nm * c->N + 2.0 * nm * nm) * sizeof(double));
    HIP_TRY((hipError_t)launch_propagate_cov(c->P.p, c->P.stride, c->P.ld, c->N, c->Np, nm, a.Phi_out, a.Pmm_out, b0, nb, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // imu / opts / Qmodel are borrowed host memory
  return XIVO_HIP_OK;
}

}  // extern "C"
