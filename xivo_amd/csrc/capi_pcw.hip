// C ABI, point-cloud world (include/xivo_hip.h, "point-cloud world"): the resident worlds, the per-frame track producer and the
// read-back of what it left. Host orchestration only - the kernel is in pcw_kernels.hip, its rules in pcw_device.h. The frame
// call checks its arguments before it touches the device, allocates nothing and does not synchronise the stream; the tracks
// land in the strided form of the life cycles' track block (capi_lifecycle.hip), where xivo_hip_life_begin_tracks and
// xivo_hip_pool_life_begin_tracks find them.
#include <math.h>
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace xivo_hip::capi {

void pcw_release(xivo_hip_ctx* c) {
  c->mem.release(&c->world.Xs, &c->world.ids, &c->world.next_id, &c->world.cnt, &c->world.gsc);
  c->mem.release(&c->world.bias, &c->world.flags, &c->world.fstats);   // the fault path's blocks go with the worlds
  c->world = World{};   // (the page-locked staging of the poses goes with it)
}

int pcw_produce(xivo_hip_ctx* c, int B, const double* gsc, double noise_px_std, unsigned long long seed, unsigned long long frame) {
  const xivo_pcw_opts& o = c->world.opts;
  PcwArgs a{};
  a.Xs = c->world.Xs; a.ids = c->world.ids; a.next_id = c->world.next_id; a.gsc = gsc; a.npts = o.npts;
  a.fx = o.fx; a.fy = o.fy; a.cx = o.cx; a.cy = o.cy; a.imw = o.imw; a.imh = o.imh;
  a.noise_px_std = noise_px_std; a.seed = seed; a.frame = frame;
  a.use_cam = c->world.use_cam ? 1 : 0; a.cam = c->world.cam; a.max_radius = c->world.max_radius;
  a.track_ids = track_block_strided_ids(c); a.track_meas = track_block_strided_meas(c); a.cnt = c->world.cnt; a.track_ld = track_block_row(c);
  a.track_keys = c->lclife.keys;   // (null unless xivo_hip_lcmap_life_config is on: the keys go where the begin_tracks call reads them)
  // the fault path: its own instances of the kernel, picked when faults are configured or a stream is shared (thresholds 0 and
  // no blocks: a shared stream alone)
  const World& w = c->world;
  a.fault_path = (w.faults_on() || w.stream_mod > 0) ? 1 : 0; a.stream_mod = w.stream_mod;
  if (w.faults_on()) {
    const xivo_pcw_fault_opts& f = w.fault;
    a.sticky = f.sticky; a.t1 = f.p_drop; a.t2 = a.t1 + f.p_outlier; a.t3 = a.t2 + f.p_tail;
    a.outlier_min_px = f.outlier_min_px; a.outlier_max_px = f.outlier_max_px; a.tail_scale = f.tail_scale;
    a.bias = w.bias; a.flags = w.flags; a.fstats = w.fstats;
  }
  c->world.tracks_overwritten();   // (whatever the block held)
  c->world.scored = false;
  {
    // per filter: the points and their ids in, the ids that changed and at most npts tracks of 32 bytes out
    char label[32];   // the instance launch_pcw_tracks picks, as the tracer prints it
    snprintf(label, sizeof(label), a.fault_path ? "pcw_tracks_kernel<%d, true>" : "pcw_tracks_kernel<%d>", a.use_cam ? a.cam.model : -1);
    StageTimer st(c, ST_OTHER, 0.0, label, (double)B * o.npts * (24.0 + 8.0 + 8.0 + 32.0));
    if (launch_pcw_tracks(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->world.tracks_B = B; c->world.fresh = true;
  return XIVO_HIP_OK;
}

}  // namespace xivo_hip::capi

namespace {

bool pcw_ready(const xivo_hip_ctx* c) { return c && c->world.configured() && track_block_row(c) > 0 && c->world.opts.npts > 0; }

}  // namespace

extern "C" {

int xivo_hip_pcw_config(xivo_hip_ctx* c, const xivo_pcw_opts* o) {
  if (!c || !o || o->struct_size != (int)sizeof(xivo_pcw_opts) || o->npts < 0) return XIVO_HIP_ERR_INVALID;
  if (o->npts > 0) {
    if (!c->life_cycle_configured() || o->npts > track_block_row(c)) return XIVO_HIP_ERR_INVALID;   // either device life cycle
    const double v[6] = {o->fx, o->fy, o->cx, o->cy, o->imw, o->imh};
    for (double x : v) if (!isfinite(x)) return XIVO_HIP_ERR_INVALID;
  }
  if (track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;   // an open frame may be reading the producer's tracks
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
  pcw_release(c);
  if (o->npts == 0) return XIVO_HIP_OK;
  const size_t B = c->Bmax, n = o->npts;
  int rc = c->mem.raw(&c->world.Xs, B * n * 3);
  if (!rc) rc = c->mem.raw(&c->world.ids, B * n);
  if (!rc) rc = c->mem.raw(&c->world.next_id, B);
  if (!rc) rc = c->mem.zeroed(&c->world.cnt, B);
  if (!rc) rc = c->mem.zeroed(&c->world.gsc, B * 12);
  // the poses as the tracks of xivo_hip_life_begin: one device block behind the stream's order, two page-locked blocks so that
  // the host writes the next frame's poses while the previous upload may still be reading
  if (!rc) rc = c->world.up.alloc(B * 12 * sizeof(double));
  // an empty world until xivo_hip_pcw_set_world: points at the origin, no track (all bytes 0xff: -1), ids from 0
  if (!rc && hipMemsetAsync(c->world.Xs, 0, B * n * 3 * sizeof(double), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(c->world.ids, 0xff, B * n * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(c->world.next_id, 0, B * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { pcw_release(c); return rc; }
  c->world.opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_camera(xivo_hip_ctx* c, const xivo_cam* cam, double max_radius) {
  if (!pcw_ready(c) || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  if (!cam) {   // back to the pinhole of xivo_pcw_opts
    c->world.use_cam = false; c->world.cam = xivo_cam{}; c->world.max_radius = 0.0;
    return XIVO_HIP_OK;
  }
  if (cam->model != XIVO_CAM_PINHOLE && cam->model != XIVO_CAM_ATAN && cam->model != XIVO_CAM_RADTAN && cam->model != XIVO_CAM_EQUI)
    return XIVO_HIP_ERR_INVALID;
  if (!(max_radius > 0.0) || cam->rows <= 0 || cam->cols <= 0) return XIVO_HIP_ERR_INVALID;   // (a NaN radius fails the comparison)
  const double v[4] = {cam->fx, cam->fy, cam->cx, cam->cy};
  for (double x : v) if (!isfinite(x)) return XIVO_HIP_ERR_INVALID;
  for (double x : cam->d) if (!isfinite(x)) return XIVO_HIP_ERR_INVALID;
  // the frame calls hand the camera to the kernel by value: frames already enqueued keep the one they were launched with
  c->world.use_cam = true; c->world.cam = *cam; c->world.max_radius = max_radius;
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_set_world(xivo_hip_ctx* c, int b0, int nb, const double* Xs, const long long* ids, const long long* next_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !pcw_ready(c) || track_block_frame_open(c) || (nb > 0 && !Xs)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t n = c->world.opts.npts;
  std::vector<long long> fill;
  if (!ids) { fill.assign((size_t)nb * n, -1); ids = fill.data(); }
  std::vector<long long> first;
  if (!next_id) { first.assign((size_t)nb, 10000); next_id = first.data(); }   // counter0 of src/feature.h
  HIP_TRY(hipMemcpyAsync(c->world.Xs + (size_t)b0 * n * 3, Xs, (size_t)nb * n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->world.ids + (size_t)b0 * n, ids, (size_t)nb * n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->world.next_id + b0, next_id, (size_t)nb * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  if (c->world.bias) HIP_TRY(hipMemsetAsync(c->world.bias + (size_t)b0 * n * 2, 0, (size_t)nb * n * 2 * sizeof(double), c->stream));   // new worlds carry no bias
  HIP_TRY(hipStreamSynchronize(c->stream));   // pageable sources
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_get_world(xivo_hip_ctx* c, int b0, int nb, long long* ids, long long* next_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !pcw_ready(c)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t n = c->world.opts.npts;
  if (ids) {
    int rc = d2h_rows(c, ids, n * sizeof(long long), c->world.ids + (size_t)b0 * n, n * sizeof(long long), n * sizeof(long long), nb);
    if (rc) return rc;
  }
  if (next_id) {
    int rc = d2h_rows(c, next_id, sizeof(long long), c->world.next_id + b0, sizeof(long long), sizeof(long long), nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_tracks(xivo_hip_ctx* c, int B, const double* gsc, double noise_px_std, unsigned long long seed,
                        unsigned long long frame) {
  if (!pcw_ready(c) || B <= 0 || B > c->Bmax || !gsc || track_block_frame_open(c) || !isfinite(noise_px_std)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // the staging block the previous frame did not use; it is free once its upload (two frames back) has finished
  char* h = nullptr;
  if (int rc = c->world.up.stage(&h)) return rc;
  const size_t bytes = (size_t)B * 12 * sizeof(double);
  memcpy(h, gsc, bytes);
  if (int rc = c->world.up.enqueue(c->world.gsc, bytes, c->stream)) return rc;
  return pcw_produce(c, B, c->world.gsc, noise_px_std, seed, frame);
}

int xivo_hip_pcw_tracks_resident(xivo_hip_ctx* c, int B, double noise_px_std, unsigned long long seed, unsigned long long frame) {
  if (!pcw_ready(c) || B <= 0 || B > c->Bmax || track_block_frame_open(c) || !isfinite(noise_px_std) || !c->trajsim.frame_poses(B))
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  return pcw_produce(c, B, c->trajsim.frame_poses(B), noise_px_std, seed, frame);
}

int xivo_hip_pcw_get_tracks(xivo_hip_ctx* c, int b0, int nb, int* cnt, long long* ids, double* meas) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !pcw_ready(c) || b0 + nb > c->world.tracks_B) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t ld = track_block_row(c);
  std::vector<int> n((size_t)nb);
  int rc = d2h_rows(c, n.data(), sizeof(int), c->world.cnt + b0, sizeof(int), sizeof(int), nb);
  if (rc) return rc;
  if (ids) {
    rc = d2h_rows(c, ids, ld * sizeof(long long), track_block_strided_ids(c) + (size_t)b0 * ld, ld * sizeof(long long), ld * sizeof(long long), nb);
    if (rc) return rc;
  }
  if (meas) {
    rc = d2h_rows(c, meas, 3 * ld * sizeof(double), track_block_strided_meas(c) + 3 * (size_t)b0 * ld, 3 * ld * sizeof(double), 3 * ld * sizeof(double), nb);
    if (rc) return rc;
  }
  // behind cnt[b] a row holds whatever an earlier frame left: blanked, so that two read-backs compare equal
  for (int b = 0; b < nb; ++b) {
    if (ids) std::fill(ids + (size_t)b * ld + n[b], ids + (size_t)(b + 1) * ld, -1LL);
    if (meas) std::fill(meas + 3 * ((size_t)b * ld + n[b]), meas + 3 * (size_t)(b + 1) * ld, 0.0);
    if (cnt) cnt[b] = n[b];
  }
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_fault_config(xivo_hip_ctx* c, const xivo_pcw_fault_opts* o) {
  if (!pcw_ready(c) || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  if (o) {
    if (o->struct_size != (int)sizeof(xivo_pcw_fault_opts) || (o->sticky != 0 && o->sticky != 1)) return XIVO_HIP_ERR_INVALID;
    const double v[6] = {o->p_drop, o->p_outlier, o->p_tail, o->outlier_min_px, o->outlier_max_px, o->tail_scale};
    for (double x : v) if (!isfinite(x)) return XIVO_HIP_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (v[i] < 0.0 || v[i] > 1.0) return XIVO_HIP_ERR_INVALID;
    if ((o->p_drop + o->p_outlier) + o->p_tail > 1.0) return XIVO_HIP_ERR_INVALID;   // t3 as the frame calls sum it
    if (o->outlier_min_px < 0.0 || o->outlier_min_px > o->outlier_max_px || o->tail_scale < 1.0) return XIVO_HIP_ERR_INVALID;
  }
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
  World& w = c->world;
  c->mem.release(&w.bias, &w.flags, &w.fstats);
  w.fault = xivo_pcw_fault_opts{}; w.scored = false;
  if (!o) return XIVO_HIP_OK;
  const size_t B = c->Bmax, n = w.opts.npts, ld = track_block_row(c);
  int rc = c->mem.zeroed(&w.bias, B * n * 2);
  if (!rc) rc = c->mem.zeroed(&w.flags, B * ld);
  if (!rc) rc = c->mem.zeroed(&w.fstats, B);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { c->mem.release(&w.bias, &w.flags, &w.fstats); return rc; }
  w.fault = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_stream_share(xivo_hip_ctx* c, int W) {
  if (!pcw_ready(c) || W < 0 || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  c->world.stream_mod = W;   // (a kernel argument: frames already enqueued keep the one they were launched with)
  return XIVO_HIP_OK;
}

int xivo_hip_pcw_fault_score(xivo_hip_ctx* c, int B) {
  if (!pcw_ready(c) || !c->world.faults_on() || B <= 0 || B != track_block_frame(c) || !c->tracks.strided || c->world.tracks_B != B ||
      c->world.scored || !c->mask || c->F <= 0)
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  PcwScoreArgs a{};
  a.life = life_args_common(c, B);
  life_args_update(c, a.life);
  a.flags = c->world.flags; a.stats = c->world.fstats;
  c->world.scored = true;
  StageTimer st(c, ST_OTHER, 0.0, "pcw_fault_score_kernel");
  return launch_pcw_fault_score(a, B, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_pcw_fault_get_stats(xivo_hip_ctx* c, int b0, int nb, xivo_pcw_fault_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !pcw_ready(c) || !c->world.faults_on() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, out, sizeof(xivo_pcw_fault_stats), c->world.fstats + b0, sizeof(xivo_pcw_fault_stats), sizeof(xivo_pcw_fault_stats), nb);
}

int xivo_hip_pcw_fault_get_flags(xivo_hip_ctx* c, int b0, int nb, unsigned char* flags) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !pcw_ready(c) || !c->world.faults_on() || b0 + nb > c->world.tracks_B || (nb > 0 && !flags)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t ld = track_block_row(c);
  std::vector<int> n((size_t)nb);
  int rc = d2h_rows(c, n.data(), sizeof(int), c->world.cnt + b0, sizeof(int), sizeof(int), nb);
  if (!rc) rc = d2h_rows(c, flags, ld, c->world.flags + (size_t)b0 * ld, ld, ld, nb);
  if (rc) return rc;
  for (int b = 0; b < nb; ++b) std::fill(flags + (size_t)b * ld + n[b], flags + (size_t)(b + 1) * ld, (unsigned char)0);   // as get_tracks blanks its rows
  return XIVO_HIP_OK;
}

}  // extern "C"
