// C ABI, trajectory log (include/xivo_hip.h, "trajectory log"): configuration, the per-frame record launch, read-out in slices and
// the NEES of the logged poses against ground truth. Host orchestration only - the kernels are in traj_kernels.hip. Every
// entry point checks its arguments before it touches the device.
#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

int traj_pack(const xivo_hip_ctx* c) { return c->traj.ncols * (c->traj.ncols + 1) / 2; }

}  // namespace

extern "C" {

int xivo_hip_traj_config(xivo_hip_ctx* c, const xivo_traj_opts* o) {
  if (!c || !o || o->T_max < 0) return XIVO_HIP_ERR_INVALID;
  size_t n_rec = 0, n_cov = 0;
  if (o->T_max > 0) {
    if (o->n_cols < 1 || o->n_cols > XIVO_TRAJ_MAX_COLS) return XIVO_HIP_ERR_INVALID;
    for (int i = 0; i < o->n_cols; ++i) {
      if (o->cols[i] < 0 || o->cols[i] >= c->N) return XIVO_HIP_ERR_INVALID;
      for (int j = 0; j < i; ++j) if (o->cols[j] == o->cols[i]) return XIVO_HIP_ERR_INVALID;
    }
    // [T_max][Bmax] entries of at most 22 + 528 doubles
    const size_t pack = (size_t)o->n_cols * (o->n_cols + 1) / 2;
    if (!FrameLog::fits(o->T_max, c->Bmax, sizeof(xivo_traj_rec) + pack * sizeof(double), &n_rec)) return XIVO_HIP_ERR_INVALID;
    n_cov = n_rec * pack;
  }
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a record launch may still be writing the blocks given back here
  c->mem.release(&c->traj.io, &c->traj.rec, &c->traj.cov);
  c->traj = TrajLog{};
  const int rc = log_alloc(c, c->traj.log, o->T_max, &c->traj.rec, n_rec, &c->traj.cov, n_cov);
  if (rc || o->T_max == 0) return rc;
  c->traj.ncols = o->n_cols;
  for (int i = 0; i < o->n_cols; ++i) c->traj.cols[i] = o->cols[i];
  return XIVO_HIP_OK;
}

int xivo_hip_traj_record(xivo_hip_ctx* c, int B, long long ts_ns, int* frame_out) {
  if (!c || B <= 0 || B > c->Bmax || !c->traj.configured() || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (c->traj.log.full()) return XIVO_HIP_ERR_FULL;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const int pack = traj_pack(c);
  const size_t at = FrameLog::at(c->traj.log.count(), c->Bmax, 0);
  TrajRecordArgs a{};
  a.poses = c->poses; a.status = c->status; c->P.to(a.P, a.strideP, a.ldp);
  a.rec = c->traj.rec + at; a.cov = c->traj.cov + at * pack; a.n_cols = c->traj.ncols; a.pack = pack;
  for (int i = 0; i < c->traj.ncols; ++i) a.cols[i] = c->traj.cols[i];
  {
    StageTimer st(c, ST_OTHER, 0.0, "traj_record_kernel", (double)B * (2.0 * sizeof(xivo_traj_rec) + 16.0 * pack));
    if (launch_traj_record(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  log_commit(c->traj.log, ts_ns, frame_out);
  return XIVO_HIP_OK;
}

int xivo_hip_traj_count(xivo_hip_ctx* c) {
  if (!c || !c->traj.configured()) return XIVO_HIP_ERR_INVALID;
  return c->traj.log.count();
}

int xivo_hip_traj_reset(xivo_hip_ctx* c) {
  if (!c || !c->traj.configured()) return XIVO_HIP_ERR_INVALID;
  c->traj.log.reset();
  return XIVO_HIP_OK;
}

int xivo_hip_traj_read(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, xivo_traj_rec* recs, double* cov, long long* ts) {
  if (!c || bad_slice(c, c->traj.log, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  c->traj.log.stamps(t0, nt, ts);
  if (nb == 0 || nt == 0 || (!recs && !cov)) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (d2h_frames(c, recs, c->traj.rec, sizeof(xivo_traj_rec), b0, nb, t0, nt) ||
      d2h_frames(c, cov, c->traj.cov, (size_t)traj_pack(c) * sizeof(double), b0, nb, t0, nt)) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_traj_nees(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, const double* gt, double* err6, double* nees,
                       double* anees, int* n_used) {
  if (!c || bad_slice(c, c->traj.log, b0, nb, t0, nt) || !gt) return XIVO_HIP_ERR_INVALID;
  TrajNeesArgs a{};
  for (int k = 0; k < 6; ++k) {
    a.pos6[k] = -1;
    for (int i = 0; i < c->traj.ncols; ++i) if (c->traj.cols[i] == k) a.pos6[k] = i;
    if (a.pos6[k] < 0) return XIVO_HIP_ERR_INVALID;   // the pose block (Wsb, Tsb) is not in the log
  }
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  NeesStaging io;
  const int rc = io.up(c, &c->traj.io, &c->traj.io_cap, (size_t)nb, nt, 12, 6, gt);
  if (rc) return rc;
  a.rec = c->traj.rec; a.cov = c->traj.cov; a.Bmax = c->Bmax; a.pack = traj_pack(c);
  a.b0 = b0; a.nb = nb; a.t0 = t0; a.nt = nt;
  a.gt = io.gt; a.err6 = err6 ? io.err : nullptr; a.nees = io.nees; a.anees = io.anees; a.n_used = io.n_used;
  if (launch_traj_nees(a, c->stream)) return XIVO_HIP_ERR_HIP;
  return io.down(c, err6, nees, anees, n_used);
}

}  // extern "C"
