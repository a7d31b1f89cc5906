// C ABI, device-resident feature life cycle (include/xivo_hip.h, "device-resident feature life cycle"): configuration, the
// book's set-up and read-out, the frame calls (life_begin on uploaded tracks, life_begin_tracks on the tracks capi_pcw.hip's
// producer left in the block, life_end) and the counters; and what this life cycle shares with the pool's
// (capi_pool_lifecycle.hip): the in-state book, the track block, the frame calls' common check and kernel arguments. Host
// orchestration only - the kernels are in lifecycle_kernels.hip, the decisions in lifecycle_device.h. Every entry point checks
// its arguments before it touches the device; the frame calls allocate nothing and do not synchronise the stream.
#include <math.h>
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
// one block of track storage: off [Bmax + 1] | ids [n] | meas [n][3], n <= Bmax * tracks_max
size_t set_bytes(int Bmax, int tracks_max) {
  return pad8(((size_t)Bmax + 1) * sizeof(int)) + (size_t)Bmax * tracks_max * (sizeof(long long) + 3 * sizeof(double));
}

void life_release(xivo_hip_ctx* c) {
  pcw_release(c);   // the producer writes into the track block: it goes with it
  c->mem.release(&c->life.stats);
  book_release(c);
  track_block_release(c);
  c->life = ImmediateLife{};
}

// the begin kernel on the tracks the block holds; the frame opens once it is enqueued
int life_begin_frame(xivo_hip_ctx* c, int B, int F) {
  c->F = F;   // the list length, as xivo_hip_edit_batch / xivo_hip_set_pixels set it (neither touches the staged rows or dx_ok)
  LifeArgs a = life_args_common(c, B);
  a.stats = c->life.stats;
  {
    StageTimer st(c, ST_OTHER, 0.0, "life_begin_kernel");
    if (launch_life_begin(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  track_block_open_frame(c, B);
  // (loop closure inside the life cycle: the kernel decided only - xivo_hip_lcmap_add_resident makes the removals)
  c->lclife.stage = c->lclife.configured() ? LcLife::kBegun : LcLife::kNone;
  return XIVO_HIP_OK;
}

// xivo_hip_life_begin / _begin_keys: keys null - the plain call
int life_begin_uploaded(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas, const long long* keys) {
  if (!frame_can_begin(c, B, F) || !c->life.configured() || c->pool.configured() || !track_block_frame_ok(c, B, off, ids, meas)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by life_config: checks F only)
  if (rc) return rc;
  rc = track_block_upload(c, B, off, ids, meas);
  if (rc) return rc;
  if (c->lclife.configured()) {
    rc = lclife_upload_keys(c, off[B], keys);
    if (rc) return rc;
  }
  return life_begin_frame(c, B, F);
}

}  // namespace

namespace xivo_hip::capi {
// ---- the track block
void track_block_release(xivo_hip_ctx* c) {
  lclife_release(c);   // the keys lie beside the tracks: they go with them
  c->mem.release(&c->tracks.dev);
  c->tracks = TrackBlock{};
}
// one device block: everything runs on the context's stream, so the upload of frame t + 1 is ordered behind the last kernel of
// frame t. Two page-locked blocks: the host writes the next frame's tracks while the previous upload may still be reading.
int track_block_alloc(xivo_hip_ctx* c, int tracks_max) {
  TrackBlock& t = c->tracks;
  const size_t bytes = set_bytes(c->Bmax, tracks_max);
  int rc = c->mem.raw(&t.dev, bytes);
  if (!rc) rc = t.up.alloc(bytes);
  if (!rc) { t.set_bytes = bytes; t.tracks_max = tracks_max; }
  return rc;
}
bool track_block_frame_ok(const xivo_hip_ctx* c, int B, const int* off, const long long* ids, const double* meas) {
  if (!off || off[0] != 0) return false;
  for (int b = 0; b < B; ++b) {
    const long d = (long)off[b + 1] - off[b];
    if (d < 0 || d > c->tracks.tracks_max) return false;
  }
  return off[B] == 0 || (ids && meas);
}
// the frame's tracks into the staging block the previous frame did not use (free once its upload, two frames back, has
// finished), then their upload - over whatever the producer left
int track_block_upload(xivo_hip_ctx* c, int B, const int* off, const long long* ids, const double* meas) {
  TrackBlock& t = c->tracks;
  const int n = off[B];
  char* h = nullptr;
  if (int rc = t.up.stage(&h)) return rc;
  const size_t off_bytes = pad8(((size_t)B + 1) * sizeof(int));
  const size_t bytes = off_bytes + (size_t)n * (sizeof(long long) + 3 * sizeof(double));
  if (bytes > t.set_bytes) return XIVO_HIP_ERR_INVALID;
  memcpy(h, off, ((size_t)B + 1) * sizeof(int));
  if (n > 0) {
    memcpy(h + off_bytes, ids, (size_t)n * sizeof(long long));
    memcpy(h + off_bytes + (size_t)n * sizeof(long long), meas, (size_t)n * 3 * sizeof(double));
  }
  if (int rc = t.up.enqueue(t.dev, bytes, c->stream)) return rc;
  t.n = n; t.strided = false;
  c->world.tracks_overwritten();
  return XIVO_HIP_OK;
}
long long* track_block_strided_ids(xivo_hip_ctx* c) {
  return reinterpret_cast<long long*>(c->tracks.dev + pad8(((size_t)c->Bmax + 1) * sizeof(int)));
}
double* track_block_strided_meas(xivo_hip_ctx* c) {
  return reinterpret_cast<double*>(track_block_strided_ids(c) + (size_t)c->Bmax * c->tracks.tracks_max);
}

// ---- the in-state book
void book_release(xivo_hip_ctx* c) {
  c->mem.release(&c->book.feat_id, &c->book.group_refs);
  c->book.ld = 0;
}
int book_alloc(xivo_hip_ctx* c) {
  InstateBookBuffers& k = c->book;
  const size_t B = c->Bmax, ld = c->lay.n_features, G = c->lay.n_groups;
  int rc = c->mem.raw(&k.feat_id, B * ld);
  if (!rc) rc = c->mem.raw(&k.group_refs, B * G);
  // all bytes 0xff: every feature slot and every group slot reads -1 - free
  if (!rc && hipMemsetAsync(k.feat_id, 0xff, B * ld * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(k.group_refs, 0xff, B * G * sizeof(int), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc) k.ld = (int)ld;
  return rc;
}
int book_set(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id) {
  const int F = c->F, G = c->lay.n_groups, ld = c->book.ld;
  std::vector<xivo_feat_in> feats((size_t)nb * F);
  int rc = d2h_rows(c, feats.data(), (size_t)F * sizeof(xivo_feat_in), c->feats + (size_t)b0 * c->Fmax,
                    (size_t)c->Fmax * sizeof(xivo_feat_in), (size_t)F * sizeof(xivo_feat_in), nb);
  if (rc) return rc;
  std::vector<long long> ids((size_t)nb * ld, -1);
  std::vector<int> refs((size_t)nb * G, -1);
  for (int b = 0; b < nb; ++b)
    for (int j = 0; j < F; ++j) {
      const xivo_feat_in& f = feats[(size_t)b * F + j];
      const long long id = feat_id[(size_t)b * F + j];
      if ((id >= 0) != (f.sind >= 0)) return XIVO_HIP_ERR_INVALID;
      if (id < 0) continue;
      if (f.sind != j || f.ref_sind < 0 || f.ref_sind >= G) return XIVO_HIP_ERR_INVALID;
      ids[(size_t)b * ld + j] = id;
      int& r = refs[(size_t)b * G + f.ref_sind];
      r = r < 0 ? 1 : r + 1;
    }
  HIP_TRY(hipMemcpyAsync(c->book.feat_id + (size_t)b0 * ld, ids.data(), ids.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->book.group_refs + (size_t)b0 * G, refs.data(), refs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the vectors above are pageable staging
  return XIVO_HIP_OK;
}
int book_get(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs) {
  const int F = c->F, G = c->lay.n_groups, ld = c->book.ld;
  std::vector<long long> ids;
  long long* idp = feat_id;
  if (!idp && feat_ref) { ids.resize((size_t)nb * F); idp = ids.data(); }
  if (idp) {
    int rc = d2h_rows(c, idp, (size_t)F * sizeof(long long), c->book.feat_id + (size_t)b0 * ld, (size_t)ld * sizeof(long long),
                      (size_t)F * sizeof(long long), nb);
    if (rc) return rc;
  }
  if (feat_ref) {
    std::vector<xivo_feat_in> feats((size_t)nb * F);
    int rc = d2h_rows(c, feats.data(), (size_t)F * sizeof(xivo_feat_in), c->feats + (size_t)b0 * c->Fmax,
                      (size_t)c->Fmax * sizeof(xivo_feat_in), (size_t)F * sizeof(xivo_feat_in), nb);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)nb * F; ++i) feat_ref[i] = idp[i] >= 0 ? feats[i].ref_sind : -1;
  }
  if (group_refs) {
    int rc = d2h_rows(c, group_refs, (size_t)G * sizeof(int), c->book.group_refs + (size_t)b0 * G, (size_t)G * sizeof(int),
                      (size_t)G * sizeof(int), nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

// ---- a frame of either life cycle
bool frame_can_begin(const xivo_hip_ctx* c, int B, int F) {
  return c && c->have_layout && c->poses && B > 0 && B <= c->Bmax && F > 0 && F <= c->book.ld && 2 * F <= c->Mmax && c->tracks.B == 0;
}
LifeArgs life_args_common(xivo_hip_ctx* c, int B) {
  LifeArgs a{};
  c->P.to(a.P, a.strideP, a.ldp); a.Np = c->Np; a.lay = c->lay;
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.Fmax = c->Fmax; a.F = c->F;
  a.feat_id = c->book.feat_id; a.slot_ld = c->book.ld; a.group_refs = c->book.group_refs;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  const TrackBlock& t = c->tracks;
  if (t.strided) {   // one row of tracks_max per filter with the counts next to them, as the producer left them
    a.ids = track_block_strided_ids(c); a.meas = track_block_strided_meas(c);
    a.cnt = c->world.track_counts(); a.track_ld = t.tracks_max;
  } else {           // packed behind the B + 1 offsets, as the host uploaded them
    const size_t off_bytes = pad8(((size_t)B + 1) * sizeof(int));
    a.off = reinterpret_cast<const int*>(t.dev);
    a.ids = reinterpret_cast<const long long*>(t.dev + off_bytes);
    a.meas = reinterpret_cast<const double*>(t.dev + off_bytes + (size_t)t.n * sizeof(long long));
  }
  lclife_args(c, a);
  return a;
}
// the inlier mask where the update left it (xivo_hip_get_gate): the layout-faithful gate strides by Fmax, the dense-row gate by F
void life_args_update(xivo_hip_ctx* c, LifeArgs& a) {
  a.mask = c->mask; a.mask_ld = c->rows.gate_layout() == GateLayout::strided ? c->Fmax : c->F;
  a.status = c->status;
}
}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_life_config(xivo_hip_ctx* c, const xivo_life_opts* o) {
  if (!c || !o || o->tracks_max < 0 || o->tracks_max > XIVO_LIFE_MAX_TRACKS) return XIVO_HIP_ERR_INVALID;
  if (o->tracks_max > 0) {
    if (c->pool.configured() || !c->have_layout) return XIVO_HIP_ERR_INVALID;
    if (!isfinite(o->min_depth) || !isfinite(o->max_depth) || o->min_new_features < 0) return XIVO_HIP_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (!isfinite(o->var_xyz[i])) return XIVO_HIP_ERR_INVALID;
    if (c->lay.n_features > XIVO_LIFE_MAX_SLOTS || c->lay.n_groups > XIVO_LIFE_MAX_SLOTS || c->cam.model != XIVO_CAM_PINHOLE)
      return XIVO_HIP_ERR_UNSUPPORTED;
  }
  if (c->plife.configured()) return XIVO_HIP_OK;   // (tracks_max = 0; the book and the track block are the pool life cycle's: nothing of this one to release)
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
  life_release(c);
  if (o->tracks_max == 0) return XIVO_HIP_OK;
  int rc = ensure_gate_buffers(c, 1);         // the resident feature list, so that the frame calls allocate nothing
  if (rc) return rc;
  rc = c->mem.zeroed(&c->life.stats, (size_t)c->Bmax);
  if (!rc) rc = book_alloc(c);
  if (!rc) rc = track_block_alloc(c, o->tracks_max);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { life_release(c); return rc; }
  c->life.opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_life_set_book(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life.configured() || track_block_frame_open(c) || c->F <= 0 || c->F > c->book.ld || (nb > 0 && !feat_id))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (c->lclife.configured())   // a book set from outside brings no keys: all bytes 0xff, every slot reads -1
    HIP_TRY(hipMemsetAsync(c->lclife.feat_key + (size_t)b0 * c->book.ld, 0xff, (size_t)nb * c->book.ld * sizeof(long long), c->stream));
  return book_set(c, b0, nb, feat_id);
}

int xivo_hip_life_get_book(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life.configured() || c->F <= 0 || c->F > c->book.ld) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return book_get(c, b0, nb, feat_id, feat_ref, group_refs);
}

int xivo_hip_life_begin(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas) {
  return life_begin_uploaded(c, B, F, off, ids, meas, nullptr);
}

int xivo_hip_life_begin_keys(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas, const long long* keys) {
  if (!c || !c->lclife.configured() || !off || B <= 0 || B > c->Bmax || (off[B] > 0 && !keys)) return XIVO_HIP_ERR_INVALID;
  return life_begin_uploaded(c, B, F, off, ids, meas, keys);
}

int xivo_hip_life_begin_tracks(xivo_hip_ctx* c, int B, int F) {
  if (!frame_can_begin(c, B, F) || !c->life.configured() || c->pool.configured() || !c->world.tracks_fresh_for(B))
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by life_config: checks F only)
  if (rc) return rc;
  track_block_use_strided(c); c->world.tracks_consumed();
  return life_begin_frame(c, B, F);
}

int xivo_hip_life_end(xivo_hip_ctx* c, int B) {
  if (!c || !c->life.configured() || c->pool.configured() || B <= 0 || B != track_block_frame(c) || !c->mask || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // loop closure inside the life cycle: the removals the begin call decided must have been made (xivo_hip_lcmap_add_resident),
  // and after a close call the status to count is the first update's, which it kept - the second update overwrote c->status
  if (c->lclife.configured() && c->lclife.stage == LcLife::kBegun) return XIVO_HIP_ERR_INVALID;
  LifeArgs a = life_args_common(c, B);
  life_args_update(c, a);
  if (c->lclife.configured() && c->lclife.stage == LcLife::kClosed) a.status = c->lclife.status;
  c->lclife.stage = LcLife::kNone;
  a.stats = c->life.stats;
  const xivo_life_opts& o = c->life.opts;
  a.min_new_features = o.min_new_features; a.min_depth = o.min_depth; a.max_depth = o.max_depth;
  for (int i = 0; i < 3; ++i) a.var_xyz[i] = o.var_xyz[i];
  a.tune_var = c->tune.var;   // (tuning table: filter b's variances in place of var_xyz)
  a.fx = c->cam.fx; a.fy = c->cam.fy; a.cx = c->cam.cx; a.cy = c->cam.cy;
  track_block_close_frame(c);
  StageTimer st(c, ST_OTHER, 0.0, "life_end_kernel");
  return launch_life_end(a, B, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_life_stats(xivo_hip_ctx* c, int b0, int nb, xivo_life_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life.configured() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, out, sizeof(xivo_life_stats), c->life.stats + b0, sizeof(xivo_life_stats), sizeof(xivo_life_stats), nb);
}

}  // extern "C"
