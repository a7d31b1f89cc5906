// C ABI, loop closure on the device (include/xivo_hip.h, xivo_hip_lcmap_*): the resident landmark map, the add and close calls
// around it, loading and reading whole maps, the counters; and loop closure inside the device life cycle
// (xivo_hip_lcmap_life_config): the keys beside the track block and the book, the add and close calls on the records and
// queries the device made itself. Host-side orchestration only (capi_internal.h); the kernels are
// lcmap_kernels.hip's, the rows are handed over as xivo_hip_close_loop_stack hands its rows over (capi_oos.hip).
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

void lcmap_release(xivo_hip_ctx* c) {   // (the stream must be idle; the staging blocks stay: they are no part of a configuration)
  lclife_release(c);   // the life cycle's records and queries are this map's
  LcMap& m = c->lcmap;
  c->mem.release(&m.entries, &m.count, &m.stats, &m.matches, &m.closing, &m.cov, &m.visit, &m.cov_stats);
  m.opts = xivo_lcmap_opts{};
  m.cov_opts = xivo_lcmap_cov_opts{}; m.t = 0;
}

LcMapBuffers map_buffers(xivo_hip_ctx* c) {
  const LcMap& m = c->lcmap;
  return LcMapBuffers{m.entries, m.count, m.stats, m.opts.map_max};
}
// (all null without xivo_hip_lcmap_cov_config: the kernels' first instantiation runs)
LcMapCovBuffers cov_buffers(xivo_hip_ctx* c) {
  const LcMap& m = c->lcmap;
  return LcMapCovBuffers{m.cov, m.visit, m.cov_stats, m.cov_opts.revisit_gap, m.t};
}

// a call's records (rec_bytes of them) and the offsets off [B + 1] of every filter's share, through the page-locked staging to
// the device block: *d_recs, *d_off point into it. Enqueues; the caller's memory is free when this returns.
int upload_call(xivo_hip_ctx* c, const void* recs, size_t rec_bytes, const std::vector<int>& off, const char** d_recs, const int** d_off) {
  LcMap& m = c->lcmap;
  const size_t b_r = (rec_bytes + 255) & ~(size_t)255, b_o = off.size() * sizeof(int), total = b_r + b_o;
  if (total > m.up_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));   // the old blocks may still be read
    const size_t cap = std::max(total, std::max((size_t)4096, 2 * m.up_cap));
    m.up.release(); m.up_cap = 0;
    if (int rc = m.up.alloc(cap)) return rc;
    if (int rc = c->mem.grow(&m.io, &m.io_cap, cap)) { m.up.release(); return rc; }
    m.up_cap = cap;
  }
  char* h = nullptr;
  if (int rc = m.up.stage(&h)) return rc;
  if (rec_bytes) memcpy(h, recs, rec_bytes);
  memcpy(h + b_r, off.data(), b_o);
  if (int rc = m.up.enqueue(m.io, total, c->stream)) return rc;
  *d_recs = m.io; *d_off = reinterpret_cast<const int*>(m.io + b_r);
  return XIVO_HIP_OK;
}

// what add and close check first
int call_status(xivo_hip_ctx* c, int B, int n, const void* recs) {
  if (!c || !c->lcmap.configured() || !c->have_layout || !c->poses || !c->groups || !c->feats || B <= 0 || B > c->Bmax || n < 0 || (n > 0 && !recs))
    return XIVO_HIP_ERR_INVALID;
  if (c->calib_on || c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
  return XIVO_HIP_OK;
}

// the add kernel over records that are on the device: a.recs and a.off, or a.cnt / a.row, are the caller's
int add_launch(xivo_hip_ctx* c, int B, LcMapAddArgs& a) {
  a.map = map_buffers(c); a.ext = cov_buffers(c);
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.Fmax = c->Fmax; a.F = c->F;
  a.lay = c->lay; a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  c->P.to(a.P, a.strideP, a.ldp);
  a.max_depth_var = c->lcmap.opts.max_depth_var; a.batch = B;
  StageTimer st(c, ST_OTHER, 0.0, "lcmap_add_kernel");
  HIP_TRY((hipError_t)launch_lcmap_add(a, c->stream));
  return XIVO_HIP_OK;
}

// match, rows, verify and the hand-over of the rows over queries that are on the device (a.queries and a.off, or a.cnt / a.row,
// are the caller's); n_closing_out as xivo_hip_lcmap_close takes it
int close_launch(xivo_hip_ctx* c, int B, LcMapCloseArgs& a, int* n_closing_out) {
  const xivo_lcmap_opts& o = c->lcmap.opts;
  const int M = 2 * o.lc_max, N = c->N;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_H = 0, o_inn = al((size_t)B * M * N * sizeof(double)), o_R = al(o_inn + (size_t)B * M * sizeof(double)),
               total = al(o_R + (size_t)B * M * sizeof(double));
  if (total > c->lc_cap) HIP_TRY(hipStreamSynchronize(c->stream));   // (growing frees the block an earlier call's kernels read)
  if (int rc = c->mem.grow(&c->lc_buf, &c->lc_cap, total)) return rc;
  char* base = c->lc_buf;
  HIP_TRY(hipMemsetAsync(base + o_H, 0, (size_t)B * M * N * sizeof(double), c->stream));   // H_.setZero(2n, N) (update.cpp:184)
  c->lcmap.t += 1;   // (a call that stages nothing below is a call all the same)
  a.map = map_buffers(c); a.ext = cov_buffers(c);
  a.poses = c->poses; a.groups = c->groups; a.lay = c->lay; a.cam = c->cam; a.cl = xivo_calib_layout{-1, -1, 0, 0};
  c->P.to(a.P, a.strideP, a.ldp);
  a.H = reinterpret_cast<double*>(base + o_H); a.strideH = (long)M * N; a.ldh = M;
  a.inn = reinterpret_cast<double*>(base + o_inn); a.diagR = reinterpret_cast<double*>(base + o_R); a.strideV = M;
  a.matches = c->lcmap.matches; a.closing = c->lcmap.closing;
  a.lc_max = o.lc_max; a.min_matches = o.min_matches; a.Rlc = o.Rlc; a.chi2 = o.chi2; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "lcmap_close_kernel");
    HIP_TRY((hipError_t)launch_lcmap_close(a, c->stream));
  }
  if (n_closing_out) {
    std::vector<int> closing((size_t)B);
    HIP_TRY(hipMemcpyAsync(closing.data(), c->lcmap.closing, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int k = 0;
    for (int v : closing) k += v != 0;
    *n_closing_out = k;
    if (k == 0) return XIVO_HIP_OK;   // nobody closes: the frame's staged rows stay as they were
  }
  return stage_measurements(c, 0, B, M, a.H, a.strideH, a.ldh, a.inn, a.strideV, a.diagR, a.strideV);
}

// xivo_hip_lcmap_add_resident / _close_resident: the option is on and a frame of B filters of the immediate life cycle is open
bool lclife_frame(const xivo_hip_ctx* c, int B) {
  return c && c->lclife.configured() && c->lcmap.configured() && c->life.configured() && B > 0 && B == track_block_frame(c);
}

}  // namespace

namespace xivo_hip::capi {

void lclife_release(xivo_hip_ctx* c) {
  LcLife& k = c->lclife;
  c->mem.release(&k.keys, &k.feat_key, &k.recs, &k.n_recs, &k.queries, &k.n_queries, &k.tracked, &k.rm, &k.status);
  k = LcLife{};   // (the page-locked staging of the keys goes with it)
}

int lclife_upload_keys(xivo_hip_ctx* c, int n, const long long* keys) {
  LcLife& k = c->lclife;
  if (n <= 0) return XIVO_HIP_OK;
  if (!keys) {   // all bytes 0xff: every key reads -1 (lclife_no_key)
    HIP_TRY(hipMemsetAsync(k.keys, 0xff, (size_t)n * sizeof(long long), c->stream));
    return XIVO_HIP_OK;
  }
  char* h = nullptr;
  if (int rc = k.up.stage(&h)) return rc;
  memcpy(h, keys, (size_t)n * sizeof(long long));   // (n <= Bmax * tracks_max: track_block_frame_ok)
  return k.up.enqueue(k.keys, (size_t)n * sizeof(long long), c->stream);
}

void lclife_args(xivo_hip_ctx* c, LifeArgs& a) {
  const LcLife& k = c->lclife;
  if (!k.configured() || !c->life.configured()) return;
  a.keys = k.keys; a.feat_key = k.feat_key; a.lc_recs = k.recs; a.lc_n_recs = k.n_recs; a.lc_tracked = k.tracked; a.lc_rm = k.rm;
}

}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_lcmap_life_config(xivo_hip_ctx* c, int on) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || (on != 0 && on != 1) || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  if (on) {
    if (!c->life_cycle_configured() || !c->lcmap.configured()) return XIVO_HIP_ERR_INVALID;
    if (c->plife.configured()) return XIVO_HIP_ERR_UNSUPPORTED;   // the pool book carries no keys
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  lclife_release(c);
  if (!on) return XIVO_HIP_OK;
  LcLife& k = c->lclife;
  const size_t B = (size_t)c->Bmax, ld = (size_t)c->book.ld, G = (size_t)c->lay.n_groups, nt = B * track_block_row(c);
  int rc = c->mem.raw(&k.keys, nt);
  if (!rc) rc = k.up.alloc(nt * sizeof(long long));
  if (!rc) rc = c->mem.raw(&k.feat_key, B * ld);
  if (!rc) rc = c->mem.zeroed(&k.recs, B * ld);
  if (!rc) rc = c->mem.zeroed(&k.n_recs, B);
  if (!rc) rc = c->mem.zeroed(&k.queries, B * ld);
  if (!rc) rc = c->mem.zeroed(&k.n_queries, B);
  if (!rc) rc = c->mem.zeroed(&k.tracked, B * ld);
  if (!rc) rc = c->mem.zeroed(&k.rm, B * (2 + ld + G));
  if (!rc) rc = c->mem.zeroed(&k.status, B);
  // all bytes 0xff: every track and every slot - the features in the state now among them - has the key -1
  if (!rc && hipMemsetAsync(k.keys, 0xff, nt * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipMemsetAsync(k.feat_key, 0xff, B * ld * sizeof(long long), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc) { lclife_release(c); return rc; }
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_add_resident(xivo_hip_ctx* c, int B) {
  if (!lclife_frame(c, B) || c->lclife.stage != LcLife::kBegun) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (int rc = call_status(c, B, 0, nullptr)) return rc;
  LcMapAddArgs a{};
  a.recs = c->lclife.recs; a.cnt = c->lclife.n_recs; a.row = c->book.ld;
  if (int rc = add_launch(c, B, a)) return rc;
  LifeArgs la = life_args_common(c, B);
  StageTimer st(c, ST_OTHER, 0.0, "life_lc_apply_kernel");
  if (launch_life_lc_apply(la, B, c->stream)) return XIVO_HIP_ERR_HIP;
  c->lclife.stage = LcLife::kAdded;
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_close_resident(xivo_hip_ctx* c, int B, int* n_closing_out) {
  if (!lclife_frame(c, B) || c->lclife.stage != LcLife::kAdded || !c->mask || c->F <= 0) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (int rc = call_status(c, B, 0, nullptr)) return rc;
  LcLife& k = c->lclife;
  LcLifeQueryArgs q{};
  LifeArgs la = life_args_common(c, B);
  life_args_update(c, la);   // (the mask and its row stride as xivo_hip_life_end reads them)
  q.feat_id = c->book.feat_id; q.feat_key = k.feat_key; q.slot_ld = c->book.ld; q.tracked = k.tracked;
  q.mask = la.mask; q.mask_ld = la.mask_ld; q.feats = c->feats; q.Fmax = c->Fmax; q.F = c->F;
  q.status = c->status; q.status_out = k.status; q.queries = k.queries; q.n_queries = k.n_queries; q.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "lclife_query_kernel");
    HIP_TRY((hipError_t)launch_lclife_queries(q, c->stream));
  }
  k.stage = LcLife::kClosed;   // (the status is kept from here on, whatever becomes of the calls below)
  LcMapCloseArgs a{};
  a.queries = k.queries; a.cnt = k.n_queries; a.row = c->book.ld;
  return close_launch(c, B, a, n_closing_out);
}

int xivo_hip_lcmap_life_get_keys(xivo_hip_ctx* c, int b0, int nb, long long* feat_key, long long* ent_key) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lclife.configured() || ent_key || c->F <= 0 || c->F > c->book.ld) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (feat_key) {
    const size_t w = (size_t)c->F * sizeof(long long), ld = (size_t)c->book.ld;
    if (int rc = d2h_rows(c, feat_key, w, c->lclife.feat_key + (size_t)b0 * ld, ld * sizeof(long long), w, nb)) return rc;
  }
  return hipStreamSynchronize(c->stream) == hipSuccess ? XIVO_HIP_OK : XIVO_HIP_ERR_HIP;
}

int xivo_hip_lcmap_life_get_track_keys(xivo_hip_ctx* c, int b0, int nb, long long* keys) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lclife.configured() || !c->world.configured() || b0 + nb > c->world.tracks_B || (nb > 0 && !keys))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t ld = (size_t)track_block_row(c);
  std::vector<int> n((size_t)nb);
  if (int rc = d2h_rows(c, n.data(), sizeof(int), c->world.track_counts() + b0, sizeof(int), sizeof(int), nb)) return rc;
  if (int rc = d2h_rows(c, keys, ld * sizeof(long long), c->lclife.keys + (size_t)b0 * ld, ld * sizeof(long long), ld * sizeof(long long), nb)) return rc;
  // behind cnt[b] a row holds whatever an earlier frame left: blanked, as xivo_hip_pcw_get_tracks blanks the ids
  for (int b = 0; b < nb; ++b) std::fill(keys + (size_t)b * ld + n[(size_t)b], keys + (size_t)(b + 1) * ld, -1LL);
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_config(xivo_hip_ctx* c, const xivo_lcmap_opts* o) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !o || o->struct_size != (int)sizeof(xivo_lcmap_opts) || o->map_max < 0) return XIVO_HIP_ERR_INVALID;
  if (o->map_max > 0) {
    if (o->map_max > XIVO_LCMAP_MAX_ENTRIES || o->lc_max > XIVO_LCMAP_MAX_MATCHES || c->calib_on || c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
    if (!c->have_layout || o->lc_max < 1 || 2 * o->lc_max > c->Mmax || !(o->Rlc > 0.0) || !std::isfinite(o->Rlc) || o->min_matches < 1 ||
        !(o->chi2 >= 0.0) || !(o->max_depth_var >= 0.0))
      return XIVO_HIP_ERR_INVALID;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  lcmap_release(c);
  if (o->map_max == 0) return XIVO_HIP_OK;
  LcMap& m = c->lcmap;
  const size_t B = (size_t)c->Bmax, nm = B * o->lc_max;
  int rc = c->mem.zeroed(&m.entries, B * o->map_max);
  if (!rc) rc = c->mem.zeroed(&m.count, B);
  if (!rc) rc = c->mem.zeroed(&m.stats, B);
  if (!rc) rc = c->mem.zeroed(&m.matches, nm);
  if (!rc) rc = c->mem.zeroed(&m.closing, B);
  if (!rc) {   // no close call yet: every list position is empty
    std::vector<xivo_lcmap_match> empty(nm);
    for (xivo_lcmap_match& e : empty) { memset(&e, 0, sizeof(e)); e.entry = -1; }
    if (hipMemcpy(m.matches, empty.data(), nm * sizeof(xivo_lcmap_match), hipMemcpyHostToDevice) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  }
  if (rc) { lcmap_release(c); return rc; }
  m.opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_add(xivo_hip_ctx* c, int B, int n, const xivo_lcmap_add_rec* recs) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (int rc = call_status(c, B, n, recs)) return rc;
  if (n == 0) return XIVO_HIP_OK;
  std::vector<int> off((size_t)B + 1, 0);
  for (int i = 0; i < n; ++i) {
    const xivo_lcmap_add_rec& r = recs[i];
    // (a position outside the resident list is an address, not a free slot)
    if (r.b < 0 || r.b >= B || (i > 0 && r.b < recs[i - 1].b) || r.feat < 0 || r.feat >= c->F) return XIVO_HIP_ERR_INVALID;
    off[(size_t)r.b + 1] += 1;
  }
  for (int b = 0; b < B; ++b) off[(size_t)b + 1] += off[b];
  LcMapAddArgs a{};
  const char* d_recs = nullptr;
  if (int rc = upload_call(c, recs, (size_t)n * sizeof(xivo_lcmap_add_rec), off, &d_recs, &a.off)) return rc;
  a.recs = reinterpret_cast<const xivo_lcmap_add_rec*>(d_recs);
  return add_launch(c, B, a);
}

int xivo_hip_lcmap_close(xivo_hip_ctx* c, int B, int n, const xivo_lcmap_query* queries, int* n_closing_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (int rc = call_status(c, B, n, queries)) return rc;
  std::vector<int> off((size_t)B + 1, 0);
  for (int i = 0; i < n; ++i) {
    const xivo_lcmap_query& q = queries[i];
    if (q.b < 0 || q.b >= B || (i > 0 && q.b < queries[i - 1].b) || q.group_sind < -1 || q.group_sind >= c->lay.n_groups) return XIVO_HIP_ERR_INVALID;
    off[(size_t)q.b + 1] += 1;
  }
  for (int b = 0; b < B; ++b) off[(size_t)b + 1] += off[b];
  LcMapCloseArgs a{};
  const char* d_q = nullptr;
  if (int rc = upload_call(c, queries, (size_t)n * sizeof(xivo_lcmap_query), off, &d_q, &a.off)) return rc;
  a.queries = reinterpret_cast<const xivo_lcmap_query*>(d_q);
  return close_launch(c, B, a, n_closing_out);
}

int xivo_hip_lcmap_set(xivo_hip_ctx* c, int b0, int nb, const xivo_lcmap_entry* entries, const int* count) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.configured() || (nb > 0 && (!entries || !count))) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t mm = (size_t)c->lcmap.opts.map_max;
  std::vector<long long> keys;
  for (int b = 0; b < nb; ++b) {
    if (count[b] < 0 || (size_t)count[b] > mm) return XIVO_HIP_ERR_INVALID;
    keys.clear();
    for (int i = 0; i < count[b]; ++i) keys.push_back(entries[b * mm + i].key);
    std::sort(keys.begin(), keys.end());
    if (!keys.empty() && (keys.front() < 0 || std::adjacent_find(keys.begin(), keys.end()) != keys.end())) return XIVO_HIP_ERR_INVALID;
  }
  HIP_TRY(hipMemcpyAsync(c->lcmap.entries + b0 * mm, entries, nb * mm * sizeof(xivo_lcmap_entry), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lcmap.count + b0, count, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  // a loaded map: exact points until xivo_hip_lcmap_set_cov says otherwise, never seen
  if (c->lcmap.cov) HIP_TRY(hipMemsetAsync(c->lcmap.cov + b0 * mm * 6, 0, nb * mm * 6 * sizeof(double), c->stream));
  if (c->lcmap.visit) HIP_TRY(hipMemsetAsync(c->lcmap.visit + b0 * mm * 2, 0, nb * mm * 2 * sizeof(int), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // entries / count are borrowed host memory
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_get(xivo_hip_ctx* c, int b0, int nb, xivo_lcmap_entry* entries, int* count) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.configured()) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t mm = (size_t)c->lcmap.opts.map_max;
  if (entries) HIP_TRY(hipMemcpyAsync(entries, c->lcmap.entries + b0 * mm, nb * mm * sizeof(xivo_lcmap_entry), hipMemcpyDeviceToHost, c->stream));
  if (count) HIP_TRY(hipMemcpyAsync(count, c->lcmap.count + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_get_matches(xivo_hip_ctx* c, int b0, int nb, xivo_lcmap_match* matches) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.configured() || (nb > 0 && !matches)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t lm = (size_t)c->lcmap.opts.lc_max;
  HIP_TRY(hipMemcpyAsync(matches, c->lcmap.matches + b0 * lm, nb * lm * sizeof(xivo_lcmap_match), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_get_stats(xivo_hip_ctx* c, int b0, int nb, xivo_lcmap_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.configured() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(out, c->lcmap.stats + b0, (size_t)nb * sizeof(xivo_lcmap_stats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_cov_config(xivo_hip_ctx* c, const xivo_lcmap_cov_opts* o) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->lcmap.configured() || !o || o->struct_size != (int)sizeof(xivo_lcmap_cov_opts) || (o->point_cov != 0 && o->point_cov != 1) ||
      o->revisit_gap < 0)
    return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipStreamSynchronize(c->stream));
  LcMap& m = c->lcmap;
  c->mem.release(&m.cov, &m.visit, &m.cov_stats);
  m.cov_opts = xivo_lcmap_cov_opts{}; m.t = 0;
  if (!o->point_cov && o->revisit_gap == 0) return XIVO_HIP_OK;
  const size_t B = (size_t)c->Bmax, ne = B * m.opts.map_max;
  int rc = c->mem.zeroed(&m.cov_stats, B);
  if (!rc && o->point_cov) rc = c->mem.zeroed(&m.cov, ne * 6);
  if (!rc && o->revisit_gap > 0) rc = c->mem.zeroed(&m.visit, ne * 2);
  if (rc) { c->mem.release(&m.cov, &m.visit, &m.cov_stats); return rc; }
  m.cov_opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_set_cov(xivo_hip_ctx* c, int b0, int nb, const double* cov) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.cov || (nb > 0 && !cov)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t per = (size_t)c->lcmap.opts.map_max * 6, n = (size_t)nb * per;
  for (size_t i = 0; i < n; ++i) {
    const size_t k = i % 6;
    if (!std::isfinite(cov[i]) || ((k == 0 || k == 3 || k == 5) && cov[i] < 0.0)) return XIVO_HIP_ERR_INVALID;
  }
  HIP_TRY(hipMemcpyAsync(c->lcmap.cov + b0 * per, cov, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // cov is borrowed host memory
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_get_cov(xivo_hip_ctx* c, int b0, int nb, double* cov) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.cov || (nb > 0 && !cov)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t per = (size_t)c->lcmap.opts.map_max * 6;
  HIP_TRY(hipMemcpyAsync(cov, c->lcmap.cov + b0 * per, (size_t)nb * per * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_lcmap_get_cov_stats(xivo_hip_ctx* c, int b0, int nb, xivo_lcmap_cov_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->lcmap.cov_stats || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(out, c->lcmap.cov_stats + b0, (size_t)nb * sizeof(xivo_lcmap_cov_stats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
