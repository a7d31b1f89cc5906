// C ABI, loop closure on the device (include/xivo_hip.h, xivo_hip_lcmap_*): the resident landmark map, the add and close calls
// around it, loading and reading whole maps, the counters. Host-side orchestration only (capi_internal.h); the kernels are
// lcmap_kernels.hip's, the rows are handed over as xivo_hip_close_loop_stack hands its rows over (capi_oos.hip).
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

void lcmap_release(xivo_hip_ctx* c) {   // (the stream must be idle; the staging blocks stay: they are no part of a configuration)
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

}  // namespace

extern "C" {

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
  a.map = map_buffers(c); a.ext = cov_buffers(c); a.recs = reinterpret_cast<const xivo_lcmap_add_rec*>(d_recs);
  a.poses = c->poses; a.groups = c->groups; a.feats = c->feats; a.Fmax = c->Fmax; a.F = c->F;
  a.lay = c->lay; a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  c->P.to(a.P, a.strideP, a.ldp);
  a.max_depth_var = c->lcmap.opts.max_depth_var; a.batch = B;
  StageTimer st(c, ST_OTHER, 0.0, "lcmap_add_kernel");
  HIP_TRY((hipError_t)launch_lcmap_add(a, c->stream));
  return XIVO_HIP_OK;
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
  const xivo_lcmap_opts& o = c->lcmap.opts;
  const int M = 2 * o.lc_max, N = c->N;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_H = 0, o_inn = al((size_t)B * M * N * sizeof(double)), o_R = al(o_inn + (size_t)B * M * sizeof(double)),
               total = al(o_R + (size_t)B * M * sizeof(double));
  if (total > c->lc_cap) HIP_TRY(hipStreamSynchronize(c->stream));   // (growing frees the block an earlier call's kernels read)
  if (int rc = c->mem.grow(&c->lc_buf, &c->lc_cap, total)) return rc;
  LcMapCloseArgs a{};
  const char* d_q = nullptr;
  if (int rc = upload_call(c, queries, (size_t)n * sizeof(xivo_lcmap_query), off, &d_q, &a.off)) return rc;
  char* base = c->lc_buf;
  HIP_TRY(hipMemsetAsync(base + o_H, 0, (size_t)B * M * N * sizeof(double), c->stream));   // H_.setZero(2n, N) (update.cpp:184)
  c->lcmap.t += 1;   // (a call that stages nothing below is a call all the same)
  a.map = map_buffers(c); a.ext = cov_buffers(c); a.queries = reinterpret_cast<const xivo_lcmap_query*>(d_q);
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
