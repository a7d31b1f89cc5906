// C ABI, device-resident feature life cycle of the "subfilter" mode (include/xivo_hip.h, "the pool life cycle"): configuration,
// the books' set-up and read-out, the frame calls (pool_life_begin on uploaded tracks, pool_life_begin_tracks on the
// tracks capi_pcw.hip's producer left in the block, pool_life_end) and the counters. Host orchestration only - the kernels are in
// pool_lifecycle_kernels.hip (and pool_kernels.hip for the step), the decisions in pool_lifecycle_device.h. The in-state book,
// the track block and the frame calls' common check and kernel arguments are capi_lifecycle.hip's (book_*, track_block_*,
// frame_can_begin, life_args_*). Every entry point checks its arguments before it touches the device; the frame calls
// allocate nothing and do not synchronise the stream.
#include <math.h>
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// what the three kernels take: the common arguments of a frame (P, the scene, the in-state book, the tracks), the pool and its book
PoolLifeArgs plife_args(xivo_hip_ctx* c, int B) {
  PoolLifeArgs a{};
  a.life = life_args_common(c, B);
  a.pool = c->fpool; a.anchors = c->anchors; a.pool_max = c->pool_max; a.anchor_max = c->anchor_max;
  a.ent_id = c->plife_ent_id; a.ent_born = c->plife_ent_born; a.anc_used = c->plife_anc_used; a.anc_life = c->plife_anc_life;
  a.stats = c->plife_stats;
  a.slot_track = c->plife_slot_track; a.ent_track = c->plife_ent_track;
  a.xp = c->plife_xp; a.order = c->plife_order; a.n = c->plife_n; a.live = c->plife_live;
  a.frame = c->plife_frame;
  return a;
}

// the host mirrors of the pool (capi_internal.h) as the device has them now: an entry's anchor, an anchor's link (-2: the anchor
// does not exist - the host life cycle creates it before it adds to it)
int reread_mirrors(xivo_hip_ctx* c) {
  const size_t ne = (size_t)c->Bmax * c->pool_max, na = (size_t)c->Bmax * c->anchor_max;
  std::vector<xivo_subfilter_feat> ent(ne);
  std::vector<PoolAnchor> anc(na);
  std::vector<int> used(na);
  HIP_TRY(hipMemcpyAsync(ent.data(), c->fpool, ne * sizeof(xivo_subfilter_feat), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(anc.data(), c->anchors, na * sizeof(PoolAnchor), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(used.data(), c->plife_anc_used, na * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < ne; ++i) c->pool_anchor_h[i] = ent[i].ref_sind >= 0 && ent[i].ref_sind < c->anchor_max ? ent[i].ref_sind : -1;
  for (size_t i = 0; i < na; ++i) c->anchor_link_h[i] = !used[i] ? -2 : (anc[i].slot >= 0 ? anc[i].slot : -1);
  return XIVO_HIP_OK;
}

// the begin kernel, the step and the admit kernel on the tracks the block holds
int plife_begin_frame(xivo_hip_ctx* c, int B, int F, int strict) {
  c->F = F;   // the list length, as xivo_hip_edit_batch / xivo_hip_set_pixels set it
  // the frame counter advances and the frame opens only once everything is enqueued: a failed launch leaves neither behind
  PoolLifeArgs a = plife_args(c, B);
  a.frame = c->plife_frame + 1;
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_begin_kernel");
    if (launch_pool_life_begin(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  // the step of xivo_hip_pool_step, on the pixels the begin kernel left and into device outputs
  PoolStepArgs p = pool_step_args(c, B, strict);
  p.xp = c->plife_xp; p.order = c->plife_order; p.n = c->plife_n; p.live = c->plife_live;
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_step_kernel");
    HIP_TRY((hipError_t)launch_pool_step(p, c->stream));
  }
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_admit_kernel");
    if (launch_pool_life_admit(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->plife_frame += 1;
  track_block_open_frame(c, B);
  return XIVO_HIP_OK;
}

}  // namespace

namespace xivo_hip::capi {
void pool_life_release(xivo_hip_ctx* c) {
  if (!c->plife_on) return;
  pcw_release(c);   // the producer writes into the track block: it goes with it
  c->mem.release(&c->plife_ent_id, &c->plife_ent_born, &c->plife_anc_used, &c->plife_anc_life, &c->plife_stats);
  c->mem.release(&c->plife_slot_track, &c->plife_ent_track, &c->plife_xp, &c->plife_order, &c->plife_n, &c->plife_live);
  book_release(c);
  track_block_release(c);
  c->plife_on = false; c->plife_frame = 0;
  c->plife_opts = xivo_pool_life_opts{};
}
}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_pool_life_config(xivo_hip_ctx* c, const xivo_pool_life_opts* o) {
  if (!c || !o || o->struct_size != (int)sizeof(xivo_pool_life_opts) || o->tracks_max < 0 || o->tracks_max > XIVO_LIFE_MAX_TRACKS)
    return XIVO_HIP_ERR_INVALID;
  if (o->tracks_max == 0) {
    if (!c->plife_on) return XIVO_HIP_OK;
    if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
    const int rc = reread_mirrors(c);
    pool_life_release(c);
    return rc;
  }
  if (c->plife_on || !c->fpool || c->life_stats || !c->have_layout || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (o->max_group_lifetime < 0 || !isfinite(o->initial_z) || !(o->initial_z > 0.0) || (o->adaptive_z && !c->adapt_on))
    return XIVO_HIP_ERR_INVALID;
  for (int i = 0; i < 3; ++i) if (!isfinite(o->std_xyz[i])) return XIVO_HIP_ERR_INVALID;
  // an empty pool: no live entry, no anchor created (the books start empty and nothing could tell what is there)
  for (int v : c->pool_anchor_h) if (v != -1) return XIVO_HIP_ERR_INVALID;
  for (int v : c->anchor_link_h) if (v != -2) return XIVO_HIP_ERR_INVALID;
  if (c->lay.n_features > XIVO_LIFE_MAX_SLOTS || c->lay.n_groups > XIVO_LIFE_MAX_SLOTS || c->pool_max > XIVO_POOL_MAX_ENTRIES ||
      c->anchor_max > XIVO_POOL_LIFE_MAX_ANCHORS)
    return XIVO_HIP_ERR_UNSUPPORTED;
  if (c->adapt_on && adapt_depth_lds(c->lay.n_features, c->pool_max) > 60 * 1024) return XIVO_HIP_ERR_UNSUPPORTED;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = ensure_gate_buffers(c, 1);   // the resident feature list, so that the frame calls allocate nothing
  if (rc) return rc;
  c->plife_on = true;                   // (pool_life_release gives back whatever the steps below got)
  const size_t B = c->Bmax, ld = c->lay.n_features, pm = c->pool_max, am = c->anchor_max;
  rc = book_alloc(c);
  if (!rc) rc = c->mem.raw(&c->plife_ent_id, B * pm);
  if (!rc) rc = c->mem.zeroed(&c->plife_ent_born, B * pm);
  if (!rc) rc = c->mem.zeroed(&c->plife_anc_used, B * am);
  if (!rc) rc = c->mem.zeroed(&c->plife_anc_life, B * am);
  if (!rc) rc = c->mem.zeroed(&c->plife_stats, B);
  if (!rc) rc = c->mem.raw(&c->plife_slot_track, B * ld);
  if (!rc) rc = c->mem.raw(&c->plife_ent_track, B * pm);
  if (!rc) rc = c->mem.raw(&c->plife_xp, B * pm * 2);
  if (!rc) rc = c->mem.raw(&c->plife_order, B * pm);
  if (!rc) rc = c->mem.raw(&c->plife_n, B);
  if (!rc) rc = c->mem.raw(&c->plife_live, B * pm);
  if (!rc) rc = track_block_alloc(c, o->tracks_max);
  // all bytes 0xff: every pool entry reads -1 - free
  if (!rc && hipMemsetAsync(c->plife_ent_id, 0xff, B * pm * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { pool_life_release(c); return rc; }
  c->plife_opts = *o; c->plife_frame = 0;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_set_book(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife_on || track_block_frame_open(c) || c->F <= 0 || c->F > c->book.ld || (nb > 0 && !feat_id))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return book_set(c, b0, nb, feat_id);
}

int xivo_hip_pool_life_get_book(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs,
                                long long* ent_id, int* ent_born, int* anc_used, int* anc_life) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife_on) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (feat_id || feat_ref || group_refs) {
    if (c->F <= 0 || c->F > c->book.ld) return XIVO_HIP_ERR_INVALID;
    int rc = book_get(c, b0, nb, feat_id, feat_ref, group_refs);
    if (rc) return rc;
  }
  const size_t pm = c->pool_max, am = c->anchor_max;
  if (ent_id) HIP_TRY(hipMemcpyAsync(ent_id, c->plife_ent_id + b0 * pm, nb * pm * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  if (ent_born) HIP_TRY(hipMemcpyAsync(ent_born, c->plife_ent_born + b0 * pm, nb * pm * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (anc_used) HIP_TRY(hipMemcpyAsync(anc_used, c->plife_anc_used + b0 * am, nb * am * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (anc_life) HIP_TRY(hipMemcpyAsync(anc_life, c->plife_anc_life + b0 * am, nb * am * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_begin(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas, int strict) {
  if (!frame_can_begin(c, B, F) || !c->plife_on || !c->fpool || !track_block_frame_ok(c, B, off, ids, meas)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by pool_life_config: checks F only)
  if (rc) return rc;
  rc = track_block_upload(c, B, off, ids, meas);
  if (rc) return rc;
  return plife_begin_frame(c, B, F, strict);
}

int xivo_hip_pool_life_begin_tracks(xivo_hip_ctx* c, int B, int F, int strict) {
  if (!frame_can_begin(c, B, F) || !c->plife_on || !c->fpool || !c->pcw_cnt || !c->pcw_fresh || c->pcw_tracks_B != B)
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by pool_life_config: checks F only)
  if (rc) return rc;
  track_block_use_strided(c); c->pcw_fresh = false;
  return plife_begin_frame(c, B, F, strict);
}

int xivo_hip_pool_life_end(xivo_hip_ctx* c, int B) {
  if (!c || !c->plife_on || !c->fpool || B <= 0 || B != track_block_frame(c) || !c->mask || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  PoolLifeArgs a = plife_args(c, B);
  life_args_update(c, a.life);
  const xivo_pool_life_opts& o = c->plife_opts;
  a.max_group_lifetime = o.max_group_lifetime; a.initial_z = o.initial_z;
  for (int i = 0; i < 3; ++i) a.std_xyz[i] = o.std_xyz[i];
  a.init_z = o.adaptive_z ? c->init_z : nullptr;
  a.cam = c->cam; a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  track_block_close_frame(c);
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_end_kernel");
    if (launch_pool_life_end(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  if (c->adapt_on) {   // AdaptInitialDepth (src/manager.cpp:131), after the new tracks took the old init_z; no copy out
    AdaptDepthArgs d{};
    d.feats = c->feats; d.F = c->F; d.Fmax = c->Fmax;
    d.pool = c->fpool; d.pool_max = c->pool_max;
    d.init_z = c->init_z; d.init_z_out = nullptr;
    d.beta = c->adapt.median_weight; d.min_z = c->adapt.min_z; d.max_z = c->adapt.max_z;
    d.min_lifetime = c->adapt.min_feature_lifetime; d.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; d.batch = B;
    StageTimer st(c, ST_OTHER, 0.0, "adapt_depth_kernel");
    HIP_TRY((hipError_t)launch_adapt_depth(d, c->stream));
  }
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_stats(xivo_hip_ctx* c, int b0, int nb, xivo_pool_life_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife_on || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, out, sizeof(xivo_pool_life_stats), c->plife_stats + b0, sizeof(xivo_pool_life_stats),
                  sizeof(xivo_pool_life_stats), nb);
}

}  // extern "C"
