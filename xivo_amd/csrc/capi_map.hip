// C ABI, landmark log (include/xivo_hip.h, "landmark log"): configuration, the per-frame record launch, read-out in slices and
// the NEES of the logged world points against true points. Host orchestration only - the kernels are in map_kernels.hip. Every
// entry point checks its arguments before it touches the device.
#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

extern "C" {

int xivo_hip_map_config(xivo_hip_ctx* c, const xivo_map_opts* o) {
  if (!c || !o || o->T_max < 0) return XIVO_HIP_ERR_INVALID;
  size_t n_fr = 0, n_pt = 0;
  if (o->T_max > 0) {
    if (o->n_out < 1 || o->n_out > XIVO_MAP_MAX_OUT || (o->flags & ~(unsigned)XIVO_MAP_WORLD_COV) || !c->have_layout)
      return XIVO_HIP_ERR_INVALID;
    if (c->lay.n_features > XIVO_MAP_MAX_OUT) return XIVO_HIP_ERR_UNSUPPORTED;   // one sorting network of that many keys
    // [T_max][Bmax] filters of n_out entries and one count
    if (!FrameLog::fits(o->T_max, c->Bmax, (size_t)o->n_out * sizeof(xivo_map_pt) + sizeof(int), &n_fr)) return XIVO_HIP_ERR_INVALID;
    n_pt = n_fr * (size_t)o->n_out;
  }
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a record launch may still be writing the blocks given back here
  c->mem.release(&c->map.io, &c->map.pts, &c->map.npts);
  c->map = MapLog{};
  const int rc = log_alloc(c, c->map.log, o->T_max, &c->map.pts, n_pt, &c->map.npts, n_fr);
  if (rc || o->T_max == 0) return rc;
  c->map.nout = o->n_out; c->map.flags = o->flags;
  return XIVO_HIP_OK;
}

int xivo_hip_map_record(xivo_hip_ctx* c, int B, long long ts_ns, int* frame_out) {
  if (!c || B <= 0 || B > c->Bmax || !c->map.configured() || !c->poses || !c->feats || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (c->F > XIVO_MAP_MAX_OUT) return XIVO_HIP_ERR_UNSUPPORTED;
  if (c->map.log.full()) return XIVO_HIP_ERR_FULL;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const size_t at = FrameLog::at(c->map.log.count(), c->Bmax, 0);
  MapRecordArgs a{};
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.F = c->F; a.Fmax = c->Fmax;
  c->P.to(a.P, a.strideP, a.ldp); a.lay = c->lay;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.world = (c->map.flags & XIVO_MAP_WORLD_COV) ? 1 : 0;
  a.pts = c->map.pts + at * c->map.nout; a.n_pts = c->map.npts + at; a.n_out = c->map.nout;
  {
    // per filter: the nine stored entries of every block, the 120 gathered entries of every kept one, the records out
    const double per = 72.0 * c->F + (double)c->map.nout * (sizeof(xivo_map_pt) + (a.world ? 960.0 : 48.0));
    StageTimer st(c, ST_OTHER, 0.0, "map_record_kernel", (double)B * per);
    if (launch_map_record(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  log_commit(c->map.log, ts_ns, frame_out);
  return XIVO_HIP_OK;
}

int xivo_hip_map_count(xivo_hip_ctx* c) {
  if (!c || !c->map.configured()) return XIVO_HIP_ERR_INVALID;
  return c->map.log.count();
}

int xivo_hip_map_reset(xivo_hip_ctx* c) {
  if (!c || !c->map.configured()) return XIVO_HIP_ERR_INVALID;
  c->map.log.reset();
  return XIVO_HIP_OK;
}

int xivo_hip_map_read(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, xivo_map_pt* pts, int* n_pts, long long* ts) {
  if (!c || bad_slice(c, c->map.log, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  c->map.log.stamps(t0, nt, ts);
  if (nb == 0 || nt == 0 || (!pts && !n_pts)) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (d2h_frames(c, pts, c->map.pts, (size_t)c->map.nout * sizeof(xivo_map_pt), b0, nb, t0, nt) ||
      d2h_frames(c, n_pts, c->map.npts, sizeof(int), b0, nb, t0, nt)) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_map_nees(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, const double* gt, double* err3, double* nees,
                      double* anees, int* n_used) {
  if (!c || bad_slice(c, c->map.log, b0, nb, t0, nt) || !gt || !(c->map.flags & XIVO_MAP_WORLD_COV)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  NeesStaging io;
  const int rc = io.up(c, &c->map.io, &c->map.io_cap, (size_t)nb * c->map.nout, nt, 3, 3, gt);
  if (rc) return rc;
  MapNeesArgs a{};
  a.pts = c->map.pts; a.n_pts = c->map.npts; a.Bmax = c->Bmax; a.n_out = c->map.nout;
  a.b0 = b0; a.nb = nb; a.t0 = t0; a.nt = nt;
  a.gt = io.gt; a.err3 = err3 ? io.err : nullptr; a.nees = io.nees; a.anees = io.anees; a.n_used = io.n_used;
  if (launch_map_nees(a, c->stream)) return XIVO_HIP_ERR_HIP;
  return io.down(c, err3, nees, anees, n_used);
}

}  // extern "C"
