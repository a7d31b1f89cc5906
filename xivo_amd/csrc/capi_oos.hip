// C ABI, rows of out-of-state measurements (include/xivo_hip.h): OOS projection, loop-closure stacking, measurement compression of
// the OOS rows, Givens / QR. Host-side orchestration only (capi_internal.h).
#include <algorithm>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace xivo_hip::capi {

int oos_rows_begin(xivo_hip_ctx* c, int b0, int nb, int max_rows, bool* mixed_out) {
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
  *mixed_out = mixed;
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
  return XIVO_HIP_OK;
}

int oos_rows_launch(xivo_hip_ctx* c, int nb, int n_oos, int M, double Roos, int whole, bool mixed) {
  OosArgs a{};
  a.feats = c->resident_oos.feats; a.n_oos = n_oos; a.poses = c->poses; a.groups = c->groups; a.lay = c->lay; a.cam = c->cam;
  a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  a.mb = meas_buffers(c); a.row0 = M; a.Mp = c->Mpmax; a.Np = c->Np; a.batch = nb; a.Roos = Roos; a.whole = whole;
  if (mixed) a.mb.HT = nullptr;
  a.rows_out = c->resident_oos.rows;
  StageTimer st(c, ST_OTHER, 0.0, "oos_kernel");
  HIP_TRY((hipError_t)launch_oos(a, c->stream));
  return XIVO_HIP_OK;
}

}  // namespace xivo_hip::capi

extern "C" {

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
  if (!feats && !c->resident_oos.holds(nb, n_oos, whole)) return XIVO_HIP_ERR_INVALID;
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
  bool mixed = false;
  if (int rc = oos_rows_begin(c, b0, nb, max_rows, &mixed)) return rc;
  if ((size_t)n_oos * nb > c->resident_oos.cap) {   // (a resident list - feats == NULL - fits by the check above)
    int rc = c->mem.grow(&c->resident_oos.feats, &c->resident_oos.cap, (size_t)n_oos * c->Bmax);
    if (rc) return rc;
  }
  if (!c->resident_oos.rows) { int rc = c->mem.zeroed(&c->resident_oos.rows, (size_t)c->Bmax); if (rc) return rc; }
  if (feats) {
    HIP_TRY(hipMemcpyAsync(c->resident_oos.feats, feats, (size_t)nb * n_oos * sizeof(xivo_oos_in), hipMemcpyHostToDevice, c->stream));
    c->resident_oos.nb = nb; c->resident_oos.n = n_oos; c->resident_oos.whole = whole;
  }
  if (int rc = oos_rows_launch(c, nb, n_oos, M, Roos, whole, mixed)) return rc;
  if (rows_out) HIP_TRY(hipMemcpyAsync(rows_out, c->resident_oos.rows, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->dx_clear();
  c->rows.oos_appended(max_rows, Roos, mixed, b0, nb);   // (not mixed: OOS rows are dense over the group blocks - dense path)
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
  if (!c || !c->have_layout || B <= 0 || B > c->Bmax || c->rows.oos_row0() < 0 || !c->resident_oos.rows || B != c->resident_oos.nb || !(trigger_ratio >= 1.0))
    return XIVO_HIP_ERR_INVALID;
  OosCompressArgs a{};
  a.lay = c->lay; a.mb = meas_buffers(c); a.row0 = c->rows.oos_row0(); a.rows = c->resident_oos.rows; a.rows_out = c->resident_oos.rows;
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
  HIP_TRY(hipMemcpyAsync(rows.data(), c->resident_oos.rows, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int mx = 0;
  for (int b = 0; b < B; ++b) mx = rows[b] > mx ? rows[b] : mx;
  // (rc == -1: block larger than the built kernels - rows are left as they are, which is always valid)
  c->rows.oos_compressed(mx);
  c->dx_clear();
  if (rows_out) memcpy(rows_out, rows.data(), (size_t)B * sizeof(int));
  return XIVO_HIP_OK;
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
}  // extern "C"
