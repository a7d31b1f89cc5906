// C ABI, device-resident feature life cycle (include/xivo_hip.h, "device-resident feature life cycle"): configuration, the
// book's set-up and read-out, the frame calls (life_begin on uploaded tracks, life_begin_tracks on the tracks capi_pcw.hip's
// producer left in the block, life_end) and the counters. Host orchestration only - the kernels are in
// lifecycle_kernels.hip, the decisions in lifecycle_device.h. Every entry point checks its arguments before it touches the
// device; the frame calls allocate nothing and do not synchronise the stream.
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
  pcw_release(c);   // the producer writes into life_dev: it goes with it
  c->mem.release(&c->life_feat_id, &c->life_group_refs, &c->life_stats);
  track_block_release(c);
  c->life_ld = 0; c->life_strided = false;
  c->life_opts = xivo_life_opts{};
}

// what both kernels take; the tracks are those of the frame in the device block: packed behind the B + 1 offsets as the host
// uploaded them, or (c->life_strided) one row of tracks_max per filter with the counts next to them, as the producer left them
LifeArgs life_args(xivo_hip_ctx* c, int B, int n) {
  LifeArgs a{};
  c->P.to(a.P, a.strideP, a.ldp); a.Np = c->Np; a.lay = c->lay;
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.Fmax = c->Fmax; a.F = c->F;
  a.feat_id = c->life_feat_id; a.slot_ld = c->life_ld; a.group_refs = c->life_group_refs; a.stats = c->life_stats;
  track_block_args(c, B, n, a);
  if (c->life_strided) {
    a.ids = life_strided_ids(c); a.meas = life_strided_meas(c);
    a.cnt = c->pcw_cnt; a.track_ld = c->life_opts.tracks_max;
  }
  return a;
}

}  // namespace

namespace xivo_hip::capi {
// ---- the track block: what both device life cycles (this file, capi_pool_lifecycle.hip) keep a frame's tracks in
void track_block_release(xivo_hip_ctx* c) {
  c->mem.release(&c->life_dev);
  for (int i = 0; i < 2; ++i) {
    if (c->life_pin[i]) { hipHostFree(c->life_pin[i]); c->life_pin[i] = nullptr; }
    if (c->life_ev[i]) { hipEventDestroy(c->life_ev[i]); c->life_ev[i] = nullptr; }
  }
  c->life_set_bytes = 0; c->life_cur = 0; c->life_B = 0; c->life_n = 0;
}
// one device block: everything runs on the context's stream, so the upload of frame t + 1 is ordered behind the last kernel of
// frame t. Two page-locked blocks: the host writes the next frame's tracks while the previous upload may still be reading.
int track_block_alloc(xivo_hip_ctx* c, int tracks_max) {
  const size_t bytes = set_bytes(c->Bmax, tracks_max);
  int rc = c->mem.raw(&c->life_dev, bytes);
  for (int i = 0; i < 2 && !rc; ++i) {
    if (hipHostMalloc(reinterpret_cast<void**>(&c->life_pin[i]), bytes, hipHostMallocDefault) != hipSuccess) {
      c->life_pin[i] = nullptr; (void)hipGetLastError(); rc = XIVO_HIP_ERR_NOMEM;
    }
    if (!rc && hipEventCreateWithFlags(&c->life_ev[i], hipEventDisableTiming) != hipSuccess) { c->life_ev[i] = nullptr; rc = XIVO_HIP_ERR_HIP; }
  }
  if (!rc) c->life_set_bytes = bytes;
  return rc;
}
// off [B + 1]: off[0] = 0, non-decreasing, no filter above tracks_max; ids / meas present when there is a track
bool track_block_frame_ok(int B, const int* off, const long long* ids, const double* meas, int tracks_max) {
  if (!off || off[0] != 0) return false;
  for (int b = 0; b < B; ++b) {
    const long d = (long)off[b + 1] - off[b];
    if (d < 0 || d > tracks_max) return false;
  }
  return off[B] == 0 || (ids && meas);
}
// the frame's tracks into the staging block the previous frame did not use (free once its upload, two frames back, has
// finished), then their upload
int track_block_upload(xivo_hip_ctx* c, int B, const int* off, const long long* ids, const double* meas) {
  const int n = off[B];
  const int set = c->life_cur ^ 1;
  HIP_TRY(hipEventSynchronize(c->life_ev[set]));
  const size_t off_bytes = pad8(((size_t)B + 1) * sizeof(int));
  const size_t bytes = off_bytes + (size_t)n * (sizeof(long long) + 3 * sizeof(double));
  if (bytes > c->life_set_bytes) return XIVO_HIP_ERR_INVALID;
  char* h = c->life_pin[set];
  memcpy(h, off, ((size_t)B + 1) * sizeof(int));
  if (n > 0) {
    memcpy(h + off_bytes, ids, (size_t)n * sizeof(long long));
    memcpy(h + off_bytes + (size_t)n * sizeof(long long), meas, (size_t)n * 3 * sizeof(double));
  }
  HIP_TRY(hipMemcpyAsync(c->life_dev, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->life_ev[set], c->stream));
  c->life_cur = set; c->life_n = n;
  return XIVO_HIP_OK;
}
// the packed tracks of B filters in the device block -> a.off / a.ids / a.meas
void track_block_args(xivo_hip_ctx* c, int B, int n, LifeArgs& a) {
  char* d = c->life_dev;
  const size_t off_bytes = pad8(((size_t)B + 1) * sizeof(int));
  a.off = reinterpret_cast<const int*>(d);
  a.ids = reinterpret_cast<const long long*>(d + off_bytes);
  a.meas = reinterpret_cast<const double*>(d + off_bytes + (size_t)n * sizeof(long long));
}
// ---- the in-state book of either life cycle: ids [Bmax][ld], group_refs [Bmax][n_groups]
int book_set(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id, long long* d_ids, int ld, int* d_refs) {
  const int F = c->F, G = c->lay.n_groups;
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
  HIP_TRY(hipMemcpyAsync(d_ids + (size_t)b0 * ld, ids.data(), ids.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_refs + (size_t)b0 * G, refs.data(), refs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the vectors above are pageable staging
  return XIVO_HIP_OK;
}
int book_get(xivo_hip_ctx* c, int b0, int nb, const long long* d_ids, int ld, const int* d_refs, long long* feat_id,
             int* feat_ref, int* group_refs) {
  const int F = c->F, G = c->lay.n_groups;
  std::vector<long long> ids;
  long long* idp = feat_id;
  if (!idp && feat_ref) { ids.resize((size_t)nb * F); idp = ids.data(); }
  if (idp) {
    int rc = d2h_rows(c, idp, (size_t)F * sizeof(long long), d_ids + (size_t)b0 * ld, (size_t)ld * sizeof(long long),
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
    int rc = d2h_rows(c, group_refs, (size_t)G * sizeof(int), d_refs + (size_t)b0 * G, (size_t)G * sizeof(int),
                      (size_t)G * sizeof(int), nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

long long* life_strided_ids(xivo_hip_ctx* c) {
  return reinterpret_cast<long long*>(c->life_dev + pad8(((size_t)c->Bmax + 1) * sizeof(int)));
}
double* life_strided_meas(xivo_hip_ctx* c) {
  return reinterpret_cast<double*>(life_strided_ids(c) + (size_t)c->Bmax * c->life_opts.tracks_max);
}
}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_life_config(xivo_hip_ctx* c, const xivo_life_opts* o) {
  if (!c || !o || o->tracks_max < 0 || o->tracks_max > XIVO_LIFE_MAX_TRACKS) return XIVO_HIP_ERR_INVALID;
  if (o->tracks_max > 0) {
    if (c->fpool || !c->have_layout) return XIVO_HIP_ERR_INVALID;
    if (!isfinite(o->min_depth) || !isfinite(o->max_depth) || o->min_new_features < 0) return XIVO_HIP_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (!isfinite(o->var_xyz[i])) return XIVO_HIP_ERR_INVALID;
    if (c->lay.n_features > XIVO_LIFE_MAX_SLOTS || c->lay.n_groups > XIVO_LIFE_MAX_SLOTS || c->cam.model != XIVO_CAM_PINHOLE)
      return XIVO_HIP_ERR_UNSUPPORTED;
  }
  if (c->plife_on) return XIVO_HIP_OK;   // (tracks_max = 0; the track block is the pool life cycle's: nothing of this one to release)
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
  life_release(c);
  if (o->tracks_max == 0) return XIVO_HIP_OK;
  int rc = ensure_gate_buffers(c, 1);         // the resident feature list, so that the frame calls allocate nothing
  if (rc) return rc;
  const size_t B = c->Bmax, ld = c->lay.n_features, G = c->lay.n_groups;
  rc = c->mem.raw(&c->life_feat_id, B * ld);
  if (!rc) rc = c->mem.raw(&c->life_group_refs, B * G);
  if (!rc) rc = c->mem.zeroed(&c->life_stats, B);
  if (!rc) rc = track_block_alloc(c, o->tracks_max);   // (shared with the pool life cycle)
  // all bytes 0xff: every feature slot and every group slot reads -1 - free
  if (!rc && hipMemsetAsync(c->life_feat_id, 0xff, B * ld * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(c->life_group_refs, 0xff, B * G * sizeof(int), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { life_release(c); return rc; }
  c->life_ld = (int)ld; c->life_opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_life_set_book(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life_feat_id || c->life_B != 0 || c->F <= 0 || c->F > c->life_ld || (nb > 0 && !feat_id))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return book_set(c, b0, nb, feat_id, c->life_feat_id, c->life_ld, c->life_group_refs);
}

int xivo_hip_life_get_book(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life_feat_id || c->F <= 0 || c->F > c->life_ld) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return book_get(c, b0, nb, c->life_feat_id, c->life_ld, c->life_group_refs, feat_id, feat_ref, group_refs);
}

int xivo_hip_life_begin(xivo_hip_ctx* c, int B, int F, const int* off, const long long* ids, const double* meas) {
  if (!c || !c->life_feat_id || c->fpool || !c->have_layout || !c->poses || B <= 0 || B > c->Bmax || F <= 0 ||
      F > c->life_ld || 2 * F > c->Mmax || !off || c->life_B != 0)
    return XIVO_HIP_ERR_INVALID;
  if (!track_block_frame_ok(B, off, ids, meas, c->life_opts.tracks_max)) return XIVO_HIP_ERR_INVALID;
  const int n = off[B];
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by life_config: checks F only)
  if (rc) return rc;
  rc = track_block_upload(c, B, off, ids, meas);
  if (rc) return rc;
  c->life_strided = false; c->pcw_tracks_B = 0; c->pcw_fresh = false;   // (the upload overwrites what the producer left)
  c->F = F;   // the list length, as xivo_hip_edit_batch / xivo_hip_set_pixels set it (neither touches the staged rows or dx_ok)
  const LifeArgs a = life_args(c, B, n);
  {
    StageTimer st(c, ST_OTHER, 0.0, "life_begin_kernel");
    if (launch_life_begin(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->life_B = B;
  return XIVO_HIP_OK;
}

int xivo_hip_life_begin_tracks(xivo_hip_ctx* c, int B, int F) {
  if (!c || !c->life_feat_id || c->fpool || !c->have_layout || !c->poses || B <= 0 || B > c->Bmax || F <= 0 ||
      F > c->life_ld || 2 * F > c->Mmax || c->life_B != 0 || !c->pcw_cnt || !c->pcw_fresh || c->pcw_tracks_B != B)
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  int rc = ensure_gate_buffers(c, F);   // (allocated by life_config: checks F only)
  if (rc) return rc;
  c->life_strided = true; c->life_n = 0; c->pcw_fresh = false;
  c->F = F;
  const LifeArgs a = life_args(c, B, 0);
  {
    StageTimer st(c, ST_OTHER, 0.0, "life_begin_kernel");
    if (launch_life_begin(a, B, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->life_B = B;
  return XIVO_HIP_OK;
}

int xivo_hip_life_end(xivo_hip_ctx* c, int B) {
  if (!c || !c->life_feat_id || c->fpool || B <= 0 || B != c->life_B || !c->mask || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  LifeArgs a = life_args(c, B, c->life_n);
  // the inlier mask where the update left it (xivo_hip_get_gate): the layout-faithful gate strides by Fmax, the dense-row gate by F
  a.mask = c->mask; a.mask_ld = c->rows.gate_layout() == GateLayout::strided ? c->Fmax : c->F;
  a.status = c->status;
  const xivo_life_opts& o = c->life_opts;
  a.min_new_features = o.min_new_features; a.min_depth = o.min_depth; a.max_depth = o.max_depth;
  for (int i = 0; i < 3; ++i) a.var_xyz[i] = o.var_xyz[i];
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  a.fx = c->cam.fx; a.fy = c->cam.fy; a.cx = c->cam.cx; a.cy = c->cam.cy;
  c->life_B = 0;
  StageTimer st(c, ST_OTHER, 0.0, "life_end_kernel");
  return launch_life_end(a, B, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_life_stats(xivo_hip_ctx* c, int b0, int nb, xivo_life_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->life_stats || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, out, sizeof(xivo_life_stats), c->life_stats + b0, sizeof(xivo_life_stats), sizeof(xivo_life_stats), nb);
}

}  // extern "C"
