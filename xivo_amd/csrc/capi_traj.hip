// C ABI, trajectory log (include/xivo_hip.h, "trajectory log"): configuration, the per-frame record launch, read-out in slices and
// the NEES of the logged poses against ground truth. Host orchestration only - the kernels are in traj_kernels.hip. Every
// entry point checks its arguments before it touches the device.
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

int traj_pack(const xivo_hip_ctx* c) { return c->traj_ncols * (c->traj_ncols + 1) / 2; }

// a slice of recorded frames and of the context's filters (an empty slice is fine)
bool bad_slice(xivo_hip_ctx* c, int b0, int nb, int t0, int nt) {
  return bad_range(c, b0, nb) || !c->traj_rec || t0 < 0 || nt < 0 || t0 > c->traj_n || nt > c->traj_n - t0;
}

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
    // [T_max][Bmax] entries of at most 22 + 528 doubles: the byte count must fit the 63 bits an element offset is held in
    const size_t pack = (size_t)o->n_cols * (o->n_cols + 1) / 2, per = sizeof(xivo_traj_rec) + pack * sizeof(double);
    n_rec = (size_t)o->T_max * (size_t)c->Bmax;   // (two ints: no overflow in 64 bits)
    if (n_rec > (size_t)INT64_MAX / per) return XIVO_HIP_ERR_INVALID;
    n_cov = n_rec * pack;
  }
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a record launch may still be writing the blocks given back here
  c->mem.release(&c->traj_rec, &c->traj_cov, &c->traj_io);
  c->traj_io_cap = 0; c->traj_T = 0; c->traj_n = 0; c->traj_ncols = 0;
  c->traj_ts.clear();
  if (o->T_max == 0) return XIVO_HIP_OK;
  int rc = c->mem.raw(&c->traj_rec, n_rec);
  if (!rc) rc = c->mem.raw(&c->traj_cov, n_cov);
  if (rc) { c->mem.release(&c->traj_rec, &c->traj_cov); return rc; }
  c->traj_T = o->T_max; c->traj_ncols = o->n_cols;
  for (int i = 0; i < o->n_cols; ++i) c->traj_cols[i] = o->cols[i];
  return XIVO_HIP_OK;
}

int xivo_hip_traj_record(xivo_hip_ctx* c, int B, long long ts_ns, int* frame_out) {
  if (!c || B <= 0 || B > c->Bmax || !c->traj_rec || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (c->traj_n >= c->traj_T) return XIVO_HIP_ERR_FULL;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const int pack = traj_pack(c);
  const size_t at = (size_t)c->traj_n * c->Bmax;
  TrajRecordArgs a{};
  a.poses = c->poses; a.status = c->status; c->P.to(a.P, a.strideP, a.ldp);
  a.rec = c->traj_rec + at; a.cov = c->traj_cov + at * pack; a.n_cols = c->traj_ncols; a.pack = pack;
  for (int i = 0; i < c->traj_ncols; ++i) a.cols[i] = c->traj_cols[i];
  {
    StageTimer st(c, ST_OTHER, 0.0, "traj_record_kernel", (double)B * (2.0 * sizeof(xivo_traj_rec) + 16.0 * pack));
    if (launch_traj_record(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  if (frame_out) *frame_out = c->traj_n;
  c->traj_ts.push_back(ts_ns);
  c->traj_n++;
  return XIVO_HIP_OK;
}

int xivo_hip_traj_count(xivo_hip_ctx* c) {
  if (!c || !c->traj_rec) return XIVO_HIP_ERR_INVALID;
  return c->traj_n;
}

int xivo_hip_traj_reset(xivo_hip_ctx* c) {
  if (!c || !c->traj_rec) return XIVO_HIP_ERR_INVALID;
  c->traj_n = 0;
  c->traj_ts.clear();
  return XIVO_HIP_OK;
}

int xivo_hip_traj_read(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, xivo_traj_rec* recs, double* cov, long long* ts) {
  if (!c || bad_slice(c, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  if (ts) for (int t = 0; t < nt; ++t) ts[t] = c->traj_ts[(size_t)t0 + t];
  if (nb == 0 || nt == 0 || (!recs && !cov)) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // frame-major storage: the filters [b0, b0 + nb) of one frame are contiguous, frames are Bmax entries apart
  const size_t at = (size_t)t0 * c->Bmax + b0, pack = (size_t)traj_pack(c);
  if (recs)
    HIP_TRY(hipMemcpy2DAsync(recs, (size_t)nb * sizeof(xivo_traj_rec), c->traj_rec + at, (size_t)c->Bmax * sizeof(xivo_traj_rec),
                             (size_t)nb * sizeof(xivo_traj_rec), nt, hipMemcpyDeviceToHost, c->stream));
  if (cov)
    HIP_TRY(hipMemcpy2DAsync(cov, (size_t)nb * pack * sizeof(double), c->traj_cov + at * pack,
                             (size_t)c->Bmax * pack * sizeof(double), (size_t)nb * pack * sizeof(double), nt,
                             hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_traj_nees(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, const double* gt, double* err6, double* nees,
                       double* anees, int* n_used) {
  if (!c || bad_slice(c, b0, nb, t0, nt) || !gt) return XIVO_HIP_ERR_INVALID;
  TrajNeesArgs a{};
  for (int k = 0; k < 6; ++k) {
    a.pos6[k] = -1;
    for (int i = 0; i < c->traj_ncols; ++i) if (c->traj_cols[i] == k) a.pos6[k] = i;
    if (a.pos6[k] < 0) return XIVO_HIP_ERR_INVALID;   // the pose block (Wsb, Tsb) is not in the log
  }
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // per-call staging: gt in | err6, nees, anees out (doubles), then n_used (ints)
  const size_t n = (size_t)nt * nb;
  const size_t o_gt = 0, o_err = o_gt + n * 12, o_nees = o_err + n * 6, o_an = o_nees + n, dbl = o_an + (size_t)nt;
  const size_t bytes = dbl * sizeof(double) + (size_t)nt * sizeof(int);
  int rc = c->mem.grow(&c->traj_io, &c->traj_io_cap, bytes);
  if (rc) return rc;
  double* io = reinterpret_cast<double*>(c->traj_io);
  a.rec = c->traj_rec; a.cov = c->traj_cov; a.Bmax = c->Bmax; a.pack = traj_pack(c);
  a.b0 = b0; a.nb = nb; a.t0 = t0; a.nt = nt;
  a.gt = io + o_gt; a.err6 = err6 ? io + o_err : nullptr; a.nees = io + o_nees; a.anees = io + o_an;
  a.n_used = reinterpret_cast<int*>(io + dbl);
  HIP_TRY(hipMemcpyAsync(io + o_gt, gt, n * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (launch_traj_nees(a, c->stream)) return XIVO_HIP_ERR_HIP;
  if (err6) HIP_TRY(hipMemcpyAsync(err6, a.err6, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (nees) HIP_TRY(hipMemcpyAsync(nees, a.nees, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (anees) HIP_TRY(hipMemcpyAsync(anees, a.anees, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n_used) HIP_TRY(hipMemcpyAsync(n_used, a.n_used, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
