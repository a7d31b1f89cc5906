// C ABI, landmark log (include/xivo_hip.h, "landmark log"): configuration, the per-frame record launch, read-out in slices and
// the NEES of the logged world points against true points. Host orchestration only - the kernels are in map_kernels.hip. Every
// entry point checks its arguments before it touches the device.
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// a slice of recorded frames and of the context's filters (an empty slice is fine)
bool bad_slice(xivo_hip_ctx* c, int b0, int nb, int t0, int nt) {
  return bad_range(c, b0, nb) || !c->map_pts || t0 < 0 || nt < 0 || t0 > c->map_n || nt > c->map_n - t0;
}

}  // namespace

extern "C" {

int xivo_hip_map_config(xivo_hip_ctx* c, const xivo_map_opts* o) {
  if (!c || !o || o->T_max < 0) return XIVO_HIP_ERR_INVALID;
  size_t n_fr = 0, n_pt = 0;
  if (o->T_max > 0) {
    if (o->n_out < 1 || o->n_out > XIVO_MAP_MAX_OUT || (o->flags & ~(unsigned)XIVO_MAP_WORLD_COV) || !c->have_layout)
      return XIVO_HIP_ERR_INVALID;
    if (c->lay.n_features > XIVO_MAP_MAX_OUT) return XIVO_HIP_ERR_UNSUPPORTED;   // one sorting network of that many keys
    // [T_max][Bmax] filters of n_out entries and one count: the byte count must fit the 63 bits an element offset is held in
    const size_t per = (size_t)o->n_out * sizeof(xivo_map_pt) + sizeof(int);
    n_fr = (size_t)o->T_max * (size_t)c->Bmax;   // (two ints: no overflow in 64 bits)
    if (n_fr > (size_t)INT64_MAX / per) return XIVO_HIP_ERR_INVALID;
    n_pt = n_fr * (size_t)o->n_out;
  }
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a record launch may still be writing the blocks given back here
  c->mem.release(&c->map_pts, &c->map_npts, &c->map_io);
  c->map_io_cap = 0; c->map_T = 0; c->map_n = 0; c->map_nout = 0; c->map_flags = 0;
  c->map_ts.clear();
  if (o->T_max == 0) return XIVO_HIP_OK;
  int rc = c->mem.raw(&c->map_pts, n_pt);
  if (!rc) rc = c->mem.raw(&c->map_npts, n_fr);
  if (rc) { c->mem.release(&c->map_pts, &c->map_npts); return rc; }
  c->map_T = o->T_max; c->map_nout = o->n_out; c->map_flags = o->flags;
  return XIVO_HIP_OK;
}

int xivo_hip_map_record(xivo_hip_ctx* c, int B, long long ts_ns, int* frame_out) {
  if (!c || B <= 0 || B > c->Bmax || !c->map_pts || !c->poses || !c->feats || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (c->F > XIVO_MAP_MAX_OUT) return XIVO_HIP_ERR_UNSUPPORTED;
  if (c->map_n >= c->map_T) return XIVO_HIP_ERR_FULL;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const size_t at = (size_t)c->map_n * c->Bmax;
  MapRecordArgs a{};
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.F = c->F; a.Fmax = c->Fmax;
  c->P.to(a.P, a.strideP, a.ldp); a.lay = c->lay;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.world = (c->map_flags & XIVO_MAP_WORLD_COV) ? 1 : 0;
  a.pts = c->map_pts + at * c->map_nout; a.n_pts = c->map_npts + at; a.n_out = c->map_nout;
  {
    // per filter: the nine stored entries of every block, the 120 gathered entries of every kept one, the records out
    const double per = 72.0 * c->F + (double)c->map_nout * (sizeof(xivo_map_pt) + (a.world ? 960.0 : 48.0));
    StageTimer st(c, ST_OTHER, 0.0, "map_record_kernel", (double)B * per);
    if (launch_map_record(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  if (frame_out) *frame_out = c->map_n;
  c->map_ts.push_back(ts_ns);
  c->map_n++;
  return XIVO_HIP_OK;
}

int xivo_hip_map_count(xivo_hip_ctx* c) {
  if (!c || !c->map_pts) return XIVO_HIP_ERR_INVALID;
  return c->map_n;
}

int xivo_hip_map_reset(xivo_hip_ctx* c) {
  if (!c || !c->map_pts) return XIVO_HIP_ERR_INVALID;
  c->map_n = 0;
  c->map_ts.clear();
  return XIVO_HIP_OK;
}

int xivo_hip_map_read(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, xivo_map_pt* pts, int* n_pts, long long* ts) {
  if (!c || bad_slice(c, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  if (ts) for (int t = 0; t < nt; ++t) ts[t] = c->map_ts[(size_t)t0 + t];
  if (nb == 0 || nt == 0 || (!pts && !n_pts)) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // frame-major storage: the filters [b0, b0 + nb) of one frame are contiguous, frames are Bmax filters apart
  const size_t at = (size_t)t0 * c->Bmax + b0, row = (size_t)c->map_nout * sizeof(xivo_map_pt);
  if (pts)
    HIP_TRY(hipMemcpy2DAsync(pts, (size_t)nb * row, c->map_pts + at * c->map_nout, (size_t)c->Bmax * row, (size_t)nb * row, nt,
                             hipMemcpyDeviceToHost, c->stream));
  if (n_pts)
    HIP_TRY(hipMemcpy2DAsync(n_pts, (size_t)nb * sizeof(int), c->map_npts + at, (size_t)c->Bmax * sizeof(int),
                             (size_t)nb * sizeof(int), nt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_map_nees(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, const double* gt, double* err3, double* nees,
                      double* anees, int* n_used) {
  if (!c || bad_slice(c, b0, nb, t0, nt) || !gt || !(c->map_flags & XIVO_MAP_WORLD_COV)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // per-call staging: gt in | err3, nees, anees out (doubles), then n_used (ints)
  const size_t n = (size_t)nt * nb * c->map_nout;
  const size_t o_gt = 0, o_err = o_gt + n * 3, o_nees = o_err + n * 3, o_an = o_nees + n, dbl = o_an + (size_t)nt;
  const size_t bytes = dbl * sizeof(double) + (size_t)nt * sizeof(int);
  int rc = c->mem.grow(&c->map_io, &c->map_io_cap, bytes);
  if (rc) return rc;
  double* io = reinterpret_cast<double*>(c->map_io);
  MapNeesArgs a{};
  a.pts = c->map_pts; a.n_pts = c->map_npts; a.Bmax = c->Bmax; a.n_out = c->map_nout;
  a.b0 = b0; a.nb = nb; a.t0 = t0; a.nt = nt;
  a.gt = io + o_gt; a.err3 = err3 ? io + o_err : nullptr; a.nees = io + o_nees; a.anees = io + o_an;
  a.n_used = reinterpret_cast<int*>(io + dbl);
  HIP_TRY(hipMemcpyAsync(io + o_gt, gt, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (launch_map_nees(a, c->stream)) return XIVO_HIP_ERR_HIP;
  if (err3) HIP_TRY(hipMemcpyAsync(err3, a.err3, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (nees) HIP_TRY(hipMemcpyAsync(nees, a.nees, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (anees) HIP_TRY(hipMemcpyAsync(anees, a.anees, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n_used) HIP_TRY(hipMemcpyAsync(n_used, a.n_used, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
