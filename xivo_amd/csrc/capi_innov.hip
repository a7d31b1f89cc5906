// C ABI, innovation log (include/xivo_hip.h, "innovation log"): configuration, the per-frame record launch, read-out in slices
// and the ensemble / per-filter sums. Host orchestration only - the kernels are in innov_kernels.hip, the arithmetic in
// innov_device.h. Every entry point checks its arguments before it touches the device. The staged rows (StagedRows) are only
// read here: the record picks the representation the update left and materialises nothing.
#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

static_assert(LEAD_K <= 64, "innov_record_kernel: one lane of a wave per column of the lead block");
// output staging of xivo_hip_innov_stats, sized once for the largest slice: per frame and per filter a sum, a dof and a count
constexpr size_t kStatBytes = sizeof(double) + sizeof(long long) + sizeof(int);

}  // namespace

extern "C" {

int xivo_hip_innov_config(xivo_hip_ctx* c, const xivo_innov_opts* o) {
  if (!c || !o || o->T_max < 0) return XIVO_HIP_ERR_INVALID;
  size_t n_rec = 0;
  if (o->T_max > 0 && !FrameLog::fits(o->T_max, c->Bmax, sizeof(xivo_innov_rec), &n_rec)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a record launch may still be writing the blocks given back here
  c->mem.release(&c->innov.rec, &c->innov.io);
  c->innov = InnovLog{};
  return log_alloc(c, c->innov.log, o->T_max, &c->innov.rec, n_rec, &c->innov.io,
                     ((size_t)o->T_max + (size_t)c->Bmax) * 2 * sizeof(double) * 2);
}

int xivo_hip_innov_record(xivo_hip_ctx* c, int B, long long ts_ns, int* frame_out) {
  if (!c || B <= 0 || B > c->Bmax || !c->innov.configured() || !c->dx_current(B) || c->rows.rows() <= 0) return XIVO_HIP_ERR_INVALID;
  if (c->innov.log.full()) return XIVO_HIP_ERR_FULL;
  const StagedRows& r = c->rows;
  const int M = r.rows(), N = c->N;
  if (innov_record_lds(M, N) > 48 * 1024) return XIVO_HIP_ERR_UNSUPPORTED;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  InnovRecordArgs a{};
  a.ell_idx = c->ell.idx; a.ell_val = c->ell.val; a.over = c->ell.over;
  a.stride_idx = c->ell.stride_idx(); a.stride_val = c->ell.stride_val();
  c->H.to(a.H, a.strideH, a.ldh);
  // which representation holds the rows right now (staged_rows.h): the dense copy once it is alive - the gates keep it
  // neutralised alongside -, else per filter its compressed rows (or its dense ones where they do not fit), the dense OOS rows
  // of a mixed stacking behind them, the calibration columns of a lead stacking next to them
  a.dense_all = r.dense_alive() ? 1 : 0;
  a.ell_rows = r.mixed_row0() >= 0 ? r.mixed_row0() : M;
  // (a pair's lane and a dense row's thread must not share a row: the compressed rows end on a pair boundary unless they are all)
  if (a.ell_rows != M && (a.ell_rows & 1)) return XIVO_HIP_ERR_INVALID;
  if (r.has_lead()) { c->Hlead.to(a.lead, a.strideLead, a.ldlead); a.lead_k = LEAD_K; }
  c->inn.to(a.inn, a.strideInn); c->diagR.to(a.diagR, a.strideR); c->err.to(a.err, a.strideErr);
  a.status = c->status; a.ldlt_used = c->ldlt_used; a.M = M; a.N = N;
  a.rec = c->innov.rec + FrameLog::at(c->innov.log.count(), c->Bmax, 0);
  {
    // per filter: dx, inn and diagR once, the rows in their representation, the record out
    const double rows_bytes = a.dense_all ? 8.0 * M * N
                                          : (double)((a.ell_rows + 1) / 2) * ELL_W * 20.0 + 8.0 * (M - a.ell_rows) * N + (a.lead ? 8.0 * M * LEAD_K : 0.0);
    StageTimer st(c, ST_OTHER, 0.0, "innov_record_kernel", (double)B * (8.0 * N + 16.0 * M + rows_bytes + sizeof(xivo_innov_rec)));
    if (launch_innov_record(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  log_commit(c->innov.log, ts_ns, frame_out);
  return XIVO_HIP_OK;
}

int xivo_hip_innov_count(xivo_hip_ctx* c) {
  if (!c || !c->innov.configured()) return XIVO_HIP_ERR_INVALID;
  return c->innov.log.count();
}

int xivo_hip_innov_reset(xivo_hip_ctx* c) {
  if (!c || !c->innov.configured()) return XIVO_HIP_ERR_INVALID;
  c->innov.log.reset();
  return XIVO_HIP_OK;
}

int xivo_hip_innov_read(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, xivo_innov_rec* recs, long long* ts) {
  if (!c || bad_slice(c, c->innov.log, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  c->innov.log.stamps(t0, nt, ts);
  if (nb == 0 || nt == 0 || !recs) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (d2h_frames(c, recs, c->innov.rec, sizeof(xivo_innov_rec), b0, nb, t0, nt)) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_innov_stats(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, double* frame_nis, long long* frame_dof,
                         int* frame_used, double* filt_nis, long long* filt_dof, int* filt_used) {
  if (!c || bad_slice(c, c->innov.log, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  static_assert(kStatBytes <= 4 * sizeof(double), "the staging xivo_hip_innov_config allocates holds every output");
  // staging (allocated by xivo_hip_innov_config for T_max frames and Bmax filters): sums | dofs | counts, frames then filters
  const size_t n = (size_t)nt + nb;
  double* d_nis = reinterpret_cast<double*>(c->innov.io);
  long long* d_dof = reinterpret_cast<long long*>(d_nis + n);
  int* d_used = reinterpret_cast<int*>(d_dof + n);
  const long at = (long)FrameLog::at(t0, c->Bmax, b0);
  InnovStatsArgs f{c->innov.rec, at, (long)c->Bmax, 1, nt, nb, d_nis, d_dof, d_used};                 // a frame: its filters
  InnovStatsArgs g{c->innov.rec, at, 1, (long)c->Bmax, nb, nt, d_nis + nt, d_dof + nt, d_used + nt};  // a filter: its frames
  if (launch_innov_stats(f, c->stream) || launch_innov_stats(g, c->stream)) return XIVO_HIP_ERR_HIP;
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIP_TRY(down(frame_nis, d_nis, nt * sizeof(double)));       HIP_TRY(down(filt_nis, d_nis + nt, nb * sizeof(double)));
  HIP_TRY(down(frame_dof, d_dof, nt * sizeof(long long)));    HIP_TRY(down(filt_dof, d_dof + nt, nb * sizeof(long long)));
  HIP_TRY(down(frame_used, d_used, nt * sizeof(int)));        HIP_TRY(down(filt_used, d_used + nt, nb * sizeof(int)));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
