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
  a.pool = c->pool.entries; a.anchors = c->pool.anchors; a.pool_max = c->pool.pool_max(); a.anchor_max = c->pool.anchor_max();
  a.ent_id = c->plife.ent_id; a.ent_born = c->plife.ent_born; a.anc_used = c->plife.anc_used; a.anc_life = c->plife.anc_life;
  a.stats = c->plife.stats;
  a.slot_track = c->plife.slot_track; a.ent_track = c->plife.ent_track;
  a.xp = c->plife.xp; a.order = c->plife.order; a.n = c->plife.n; a.live = c->plife.live;
  a.frame = c->plife.frame;
  return a;
}

// the host mirrors of the pool (capi_internal.h) as the device has them now: an entry's anchor, an anchor's link (-2: the anchor
// does not exist - the host life cycle creates it before it adds to it)
int reread_mirrors(xivo_hip_ctx* c) {
  const size_t ne = (size_t)c->Bmax * c->pool.pool_max(), na = (size_t)c->Bmax * c->pool.anchor_max();   // (the mirrors' sizes)
  std::vector<xivo_subfilter_feat> ent(ne);
  std::vector<PoolAnchor> anc(na);
  std::vector<int> used(na);
  HIP_TRY(hipMemcpyAsync(ent.data(), c->pool.entries, ne * sizeof(xivo_subfilter_feat), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(anc.data(), c->pool.anchors, na * sizeof(PoolAnchor), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(used.data(), c->plife.anc_used, na * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pool.mirror.reread(ent.data(), anc.data(), used.data());
  return XIVO_HIP_OK;
}

// the begin kernel, the step and the admit kernel on the tracks the block holds
int plife_begin_frame(xivo_hip_ctx* c, int B, int F, int strict) {
  c->F = F;   // the list length, as xivo_hip_edit_batch / xivo_hip_set_pixels set it
  // the frame counter advances and the frame opens only once everything is enqueued: a failed launch leaves neither behind
  PoolLifeArgs a = plife_args(c, B);
  a.frame = c->plife.frame + 1;
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_begin_kernel");
    if (launch_pool_life_begin(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  // use_oos: the frame's OOS list from the entries the tracker dropped, before the step frees them (capi_pool_oos.hip)
  if (int rc = pool_oos_life_select(c, B)) return rc;
  // the step of xivo_hip_pool_step, on the pixels the begin kernel left and into device outputs
  PoolStepArgs p = pool_step_args(c, B, strict);
  p.xp = c->plife.xp; p.order = c->plife.order; p.n = c->plife.n; p.live = c->plife.live;
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_step_kernel");
    HIP_TRY((hipError_t)launch_pool_step(p, c->stream));
  }
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_admit_kernel");
    if (launch_pool_life_admit(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->plife.frame += 1;
  track_block_open_frame(c, B);
  return XIVO_HIP_OK;
}

}  // namespace

namespace xivo_hip::capi {
void pool_life_release(xivo_hip_ctx* c) {
  if (!c->plife.configured()) return;
  pool_oos_release(c);   // its rings follow this life cycle's books
  pcw_release(c);   // the producer writes into the track block: it goes with it
  c->mem.release(&c->plife.ent_id, &c->plife.ent_born, &c->plife.anc_used, &c->plife.anc_life, &c->plife.stats);
  c->mem.release(&c->plife.slot_track, &c->plife.ent_track, &c->plife.xp, &c->plife.order, &c->plife.n, &c->plife.live);
  book_release(c);
  track_block_release(c);
  c->plife = PoolLife{};
}
}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_pool_life_config(xivo_hip_ctx* c, const xivo_pool_life_opts* o) {
  if (!c || !o || o->struct_size != (int)sizeof(xivo_pool_life_opts) || o->tracks_max < 0 || o->tracks_max > XIVO_LIFE_MAX_TRACKS)
    return XIVO_HIP_ERR_INVALID;
  if (o->tracks_max == 0) {
    if (!c->plife.configured()) return XIVO_HIP_OK;
    if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
    const int rc = reread_mirrors(c);
    pool_life_release(c);
    return rc;
  }
  if (c->plife.configured() || !c->pool.configured() || c->life.configured() || !c->have_layout || !c->poses) return XIVO_HIP_ERR_INVALID;
  if (c->pool_oos.configured()) return XIVO_HIP_ERR_INVALID;   // (xivo_hip_pool_oos_config comes after: it sizes the rings by this)
  if (o->max_group_lifetime < 0 || !isfinite(o->initial_z) || !(o->initial_z > 0.0) || (o->adaptive_z && !c->pool.adapt_on))
    return XIVO_HIP_ERR_INVALID;
  for (int i = 0; i < 3; ++i) if (!isfinite(o->std_xyz[i])) return XIVO_HIP_ERR_INVALID;
  // an empty pool: no live entry, no anchor created (the books start empty and nothing could tell what is there)
  if (!c->pool.mirror.empty()) return XIVO_HIP_ERR_INVALID;
  if (c->lay.n_features > XIVO_LIFE_MAX_SLOTS || c->lay.n_groups > XIVO_LIFE_MAX_SLOTS || c->pool.pool_max() > XIVO_POOL_MAX_ENTRIES ||
      c->pool.anchor_max() > XIVO_POOL_LIFE_MAX_ANCHORS)
    return XIVO_HIP_ERR_UNSUPPORTED;
  if (c->pool.adapt_on && adapt_depth_lds(c->lay.n_features, c->pool.pool_max()) > 60 * 1024) return XIVO_HIP_ERR_UNSUPPORTED;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = ensure_gate_buffers(c, 1);   // the resident feature list, so that the frame calls allocate nothing
  if (rc) return rc;
  c->plife.on = true;                   // (pool_life_release gives back whatever the steps below got)
  const size_t B = c->Bmax, ld = c->lay.n_features, pm = c->pool.pool_max(), am = c->pool.anchor_max();
  rc = book_alloc(c);
  if (!rc) rc = c->mem.raw(&c->plife.ent_id, B * pm);
  if (!rc) rc = c->mem.zeroed(&c->plife.ent_born, B * pm);
  if (!rc) rc = c->mem.zeroed(&c->plife.anc_used, B * am);
  if (!rc) rc = c->mem.zeroed(&c->plife.anc_life, B * am);
  if (!rc) rc = c->mem.zeroed(&c->plife.stats, B);
  if (!rc) rc = c->mem.raw(&c->plife.slot_track, B * ld);
  if (!rc) rc = c->mem.raw(&c->plife.ent_track, B * pm);
  if (!rc) rc = c->mem.raw(&c->plife.xp, B * pm * 2);
  if (!rc) rc = c->mem.raw(&c->plife.order, B * pm);
  if (!rc) rc = c->mem.raw(&c->plife.n, B);
  if (!rc) rc = c->mem.raw(&c->plife.live, B * pm);
  if (!rc) rc = track_block_alloc(c, o->tracks_max);
  // all bytes 0xff: every pool entry reads -1 - free
  if (!rc && hipMemsetAsync(c->plife.ent_id, 0xff, B * pm * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { pool_life_release(c); return rc; }
  c->plife.opts = *o; c->plife.frame = 0;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_set_book(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife.configured() || track_block_frame_open(c) || c->F <= 0 || c->F > c->book.ld || (nb > 0 && !feat_id))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return book_set(c, b0, nb, feat_id);
}

int xivo_hip_pool_life_get_book(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs,
                                long long* ent_id, int* ent_born, int* anc_used, int* anc_life) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife.configured()) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (feat_id || feat_ref || group_refs) {
    if (c->F <= 0 || c->F > c->book.ld) return XIVO_HIP_ERR_INVALID;
    int rc = book_get(c, b0, nb, feat_id, feat_ref, group_refs);
    if (rc) return rc;
  }
  const size_t pm = c->pool.pool_max(), am = c->pool.anchor_max();
  if (ent_id) HIP_TRY(hipMemcpyAsync(ent_id, c->plife.ent_id + b0 * pm, nb * pm * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  if (ent_born) HIP_TRY(hipMemcpyAsync(ent_born, c->plife.ent_born + b0 * pm, nb * pm * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (anc_used) HIP_TRY(hipMemcpyAsync(anc_used, c->plife.anc_used + b0 * am, nb * am * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (anc_life) HIP_TRY(hipMemcpyAsync(anc_life, c->plife.anc_life + b0 * am, nb * am * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_begin(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas, int strict) {
  if (!frame_can_begin(c, B, F) || !c->plife.configured() || !c->pool.configured() || !track_block_frame_ok(c, B, off, ids, meas)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by pool_life_config: checks F only)
  if (rc) return rc;
  rc = track_block_upload(c, B, off, ids, meas);
  if (rc) return rc;
  return plife_begin_frame(c, B, F, strict);
}

int xivo_hip_pool_life_begin_tracks(xivo_hip_ctx* c, int B, int F, int strict) {
  if (!frame_can_begin(c, B, F) || !c->plife.configured() || !c->pool.configured() || !c->world.tracks_fresh_for(B))
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by pool_life_config: checks F only)
  if (rc) return rc;
  track_block_use_strided(c); c->world.tracks_consumed();
  return plife_begin_frame(c, B, F, strict);
}

int xivo_hip_pool_life_end(xivo_hip_ctx* c, int B) {
  if (!c || !c->plife.configured() || !c->pool.configured() || B <= 0 || B != track_block_frame(c) || !c->mask || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  PoolLifeArgs a = plife_args(c, B);
  life_args_update(c, a.life);
  const xivo_pool_life_opts& o = c->plife.opts;
  a.max_group_lifetime = o.max_group_lifetime; a.initial_z = o.initial_z;
  for (int i = 0; i < 3; ++i) a.std_xyz[i] = o.std_xyz[i];
  a.init_z = o.adaptive_z ? c->pool.init_z : nullptr;
  a.cam = c->cam; a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  track_block_close_frame(c);
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_life_end_kernel");
    if (launch_pool_life_end(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  if (int rc = pool_oos_life_record(c, B, c->plife.frame)) return rc;   // use_oos: the frame's anchor observes the live entries
  if (c->pool.adapt_on) {   // AdaptInitialDepth (src/manager.cpp:131), after the new tracks took the old init_z; no copy out
    AdaptDepthArgs d{};
    d.feats = c->feats; d.F = c->F; d.Fmax = c->Fmax;
    d.pool = c->pool.entries; d.pool_max = c->pool.pool_max();
    d.init_z = c->pool.init_z; d.init_z_out = nullptr;
    d.beta = c->pool.adapt.median_weight; d.min_z = c->pool.adapt.min_z; d.max_z = c->pool.adapt.max_z;
    d.min_lifetime = c->pool.adapt.min_feature_lifetime; d.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; d.batch = B;
    StageTimer st(c, ST_OTHER, 0.0, "adapt_depth_kernel");
    HIP_TRY((hipError_t)launch_adapt_depth(d, c->stream));
  }
  return XIVO_HIP_OK;
}

int xivo_hip_pool_life_stats(xivo_hip_ctx* c, int b0, int nb, xivo_pool_life_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->plife.configured() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, out, sizeof(xivo_pool_life_stats), c->plife.stats + b0, sizeof(xivo_pool_life_stats),
                  sizeof(xivo_pool_life_stats), nb);
}

}  // extern "C"
