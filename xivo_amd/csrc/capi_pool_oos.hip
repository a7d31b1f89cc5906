// C ABI, MSCKF update from tracks that end outside the state (include/xivo_hip.h, xivo_hip_pool_oos_*): the frame's OOS list from
// the dropped pool entries, its fixed row block behind the in-state rows, the chi-square gate of the projected rows. Host-side
// orchestration only (capi_internal.h); the rows are oos_kernel's, appended as xivo_hip_oos_project_ex appends them (capi_oos.hip).
#include <algorithm>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace xivo_hip::capi {
void pool_oos_release(xivo_hip_ctx* c) {
  c->mem.release(&c->pool_oos.gamma, &c->pool_oos.stats, &c->pool_oos.anc_born, &c->pool_oos.hist_cnt);
  c->mem.release(&c->pool_oos.hist_anchor, &c->pool_oos.hist_born, &c->pool_oos.hist_xp);
  c->pool_oos = PoolOos{};
}

namespace {
PoolOosLifeArgs life_args(xivo_hip_ctx* c, int B) {
  const xivo_pool_oos_opts& o = c->pool_oos.opts;
  PoolOosLifeArgs a{};
  a.pool = c->pool.entries; a.anchors = c->pool.anchors; a.pool_max = c->pool.pool_max(); a.anchor_max = c->pool.anchor_max();
  a.poses = c->poses; a.groups = c->groups; a.n_groups = c->lay.n_groups;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.min_depth = c->pool.opts.min_depth; a.max_depth = c->pool.opts.max_depth;
  a.ent_id = c->plife.ent_id; a.ent_born = c->plife.ent_born; a.anc_used = c->plife.anc_used; a.anc_life = c->plife.anc_life;
  a.xp = c->plife.xp;
  a.anc_born = c->pool_oos.anc_born; a.hist_cnt = c->pool_oos.hist_cnt; a.hist_anchor = c->pool_oos.hist_anchor;
  a.hist_born = c->pool_oos.hist_born; a.hist_xp = c->pool_oos.hist_xp;
  a.oos_max = o.oos_max; a.max_obs = o.max_obs; a.min_obs = o.min_obs;
  a.list = c->resident_oos.feats; a.stats = c->pool_oos.stats; a.batch = B;
  return a;
}
}  // namespace

int pool_oos_life_select(xivo_hip_ctx* c, int B) {
  if (!c->pool_oos.configured()) return XIVO_HIP_OK;
  // (the resident list holds Bmax x oos_max features since the configuration: its block only ever grows)
  StageTimer st(c, ST_OTHER, 0.0, "pool_oos_select_kernel");
  HIP_TRY((hipError_t)launch_pool_oos_select(life_args(c, B), c->stream));
  c->resident_oos.nb = B; c->resident_oos.n = c->pool_oos.opts.oos_max; c->resident_oos.whole = 0;
  c->pool_oos.B = B; c->pool_oos.projected = false;
  return XIVO_HIP_OK;
}

int pool_oos_life_record(xivo_hip_ctx* c, int B, int frame) {
  if (!c->pool_oos.configured()) return XIVO_HIP_OK;
  PoolOosLifeArgs a = life_args(c, B);
  a.frame = frame;
  StageTimer st(c, ST_OTHER, 0.0, "pool_oos_record_kernel");
  HIP_TRY((hipError_t)launch_pool_oos_record(a, c->stream));
  return XIVO_HIP_OK;
}
}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_pool_oos_config(xivo_hip_ctx* c, const xivo_pool_oos_opts* o) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !o || o->struct_size != (int)sizeof(xivo_pool_oos_opts) || !c->pool.configured() || !c->have_layout) return XIVO_HIP_ERR_INVALID;
  if (o->oos_max < 0) return XIVO_HIP_ERR_INVALID;
  if (o->oos_max > 0) {
    if (o->max_obs < 2 || o->max_obs > XIVO_OOS_MAX_OBS || o->min_obs < 2 || o->min_obs > o->max_obs || !(o->Roos > 0.0)) return XIVO_HIP_ERR_INVALID;
    for (int d = 0; d < 32; ++d)
      if (!(o->chi2[d] >= 0.0)) return XIVO_HIP_ERR_INVALID;
    // one wave's lanes fill the list positions (pool_oos_collect_kernel / pool_oos_select_kernel)
    if (o->oos_max > 64) return XIVO_HIP_ERR_UNSUPPORTED;
    // the device life cycle's rings start empty with its books: only before its first frame
    if (c->plife.configured() && c->plife.frame != 0) return XIVO_HIP_ERR_INVALID;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  pool_oos_release(c);
  if (o->oos_max == 0) return XIVO_HIP_OK;
  const size_t nl = (size_t)c->Bmax * o->oos_max;
  int rc = c->mem.zeroed(&c->pool_oos.gamma, nl);
  if (!rc) rc = c->mem.zeroed(&c->pool_oos.stats, (size_t)c->Bmax);
  if (!rc && nl > c->resident_oos.cap) rc = c->mem.grow(&c->resident_oos.feats, &c->resident_oos.cap, nl);
  if (!rc && c->plife.configured()) {
    const size_t ne = (size_t)c->Bmax * c->pool.pool_max(), mo = (size_t)o->max_obs;
    rc = c->mem.zeroed(&c->pool_oos.anc_born, (size_t)c->Bmax * c->pool.anchor_max());
    if (!rc) rc = c->mem.zeroed(&c->pool_oos.hist_cnt, ne);
    if (!rc) rc = c->mem.zeroed(&c->pool_oos.hist_anchor, ne * mo);
    if (!rc) rc = c->mem.zeroed(&c->pool_oos.hist_born, ne * mo);
    if (!rc) rc = c->mem.zeroed(&c->pool_oos.hist_xp, ne * mo * 2);
  }
  // (every byte of the list defined, the structs' padding included: the two life cycles' lists compare byte for byte)
  if (!rc && hipMemsetAsync(c->resident_oos.feats, 0, c->resident_oos.cap * sizeof(xivo_oos_in), c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (!rc && !c->resident_oos.rows) rc = c->mem.zeroed(&c->resident_oos.rows, (size_t)c->Bmax);
  if (rc) { pool_oos_release(c); return rc; }
  c->pool_oos.opts = *o;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_rows(xivo_hip_ctx* c) { return c && c->pool_oos.configured() ? c->pool_oos.rows() : 0; }

int xivo_hip_pool_oos_collect(xivo_hip_ctx* c, int B, int n, const xivo_pool_oos_cand* cands) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->pool_oos.configured() || !c->pool.configured() || c->plife.configured() || !c->poses || B <= 0 || B > c->Bmax || n < 0 ||
      (n > 0 && !cands))
    return XIVO_HIP_ERR_INVALID;
  const xivo_pool_oos_opts& o = c->pool_oos.opts;
  std::vector<int> off((size_t)B + 1, 0);
  for (int i = 0; i < n; ++i) {
    const xivo_pool_oos_cand& r = cands[i];
    if (r.b < 0 || r.b >= B || r.entry < 0 || r.entry >= c->pool.pool_max() || r.n_obs < 0 || r.n_obs > o.max_obs) return XIVO_HIP_ERR_INVALID;
    if (i > 0 && (r.b < cands[i - 1].b || (r.b == cands[i - 1].b && r.entry <= cands[i - 1].entry))) return XIVO_HIP_ERR_INVALID;
    off[(size_t)r.b + 1] += 1;
  }
  for (int b = 0; b < B; ++b) off[(size_t)b + 1] += off[b];
  const size_t b_c = ((size_t)n * sizeof(xivo_pool_oos_cand) + 255) & ~(size_t)255, b_o = off.size() * sizeof(int);
  int rc = c->mem.grow(&c->pool.io, &c->pool.io_cap, b_c + b_o);
  if (rc) return rc;
  // (a list of more features per filter may have replaced the resident one since the configuration)
  if (c->resident_oos.cap < (size_t)c->Bmax * o.oos_max) return XIVO_HIP_ERR_INVALID;
  char* io = c->pool.io;
  if (n > 0) HIP_TRY(hipMemcpyAsync(io, cands, (size_t)n * sizeof(xivo_pool_oos_cand), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(io + b_c, off.data(), b_o, hipMemcpyHostToDevice, c->stream));
  PoolOosCollectArgs a{};
  a.pool = c->pool.entries; a.anchors = c->pool.anchors; a.pool_max = c->pool.pool_max(); a.anchor_max = c->pool.anchor_max();
  a.poses = c->poses; a.groups = c->groups; a.n_groups = c->lay.n_groups;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.min_depth = c->pool.opts.min_depth; a.max_depth = c->pool.opts.max_depth;
  a.cands = (const xivo_pool_oos_cand*)io; a.off = (const int*)(io + b_c);
  a.oos_max = o.oos_max; a.max_obs = o.max_obs; a.min_obs = o.min_obs;
  a.list = c->resident_oos.feats; a.stats = c->pool_oos.stats; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_oos_collect_kernel");
    HIP_TRY((hipError_t)launch_pool_oos_collect(a, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // cands / off are borrowed host memory
  c->resident_oos.nb = B; c->resident_oos.n = o.oos_max; c->resident_oos.whole = 0;
  c->pool_oos.B = B; c->pool_oos.projected = false;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_project(xivo_hip_ctx* c, int B) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->pool_oos.configured() || !c->have_layout || B <= 0 || B != c->pool_oos.B || c->rows.rows() <= 0 || c->rows.oos_row0() >= 0 ||
      !c->resident_oos.holds(B, c->pool_oos.opts.oos_max, 0))
    return XIVO_HIP_ERR_INVALID;
  const xivo_pool_oos_opts& o = c->pool_oos.opts;
  const int M = c->rows.rows(), rows = c->pool_oos.rows();
  // the gate below reads and clears dense rows without a transposed copy: the mixed stacking only
  if (c->calib_on || c->rows.dense_alive() || c->rows.dense_from_compressed() || (c->flags & XIVO_HIP_FLAG_DENSE_H) || M % 2 != 0 ||
      M + round_up16(rows + 16) > c->Mpmax || c->Np > 512)
    return XIVO_HIP_ERR_UNSUPPORTED;
  bool mixed = false;
  if (int rc = oos_rows_begin(c, 0, B, rows, &mixed)) return rc;
  if (!mixed) return XIVO_HIP_ERR_UNSUPPORTED;
  HIP_TRY((hipError_t)launch_oos_block_init(meas_buffers(c), M, rows, o.Roos, B, c->stream));
  if (int rc = oos_rows_launch(c, B, o.oos_max, M, o.Roos, 0, mixed)) return rc;
  c->dx_clear();
  c->rows.oos_appended(rows, o.Roos, mixed, 0, B);
  c->pool_oos.projected = true;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_gate(xivo_hip_ctx* c, int B) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->pool_oos.configured() || !c->pool_oos.projected || B != c->pool_oos.B || c->rows.mixed_row0() < 0 || c->rows.ht_alive() ||
      c->rows.oos_max_rows() != c->pool_oos.rows() || !c->resident_oos.holds(B, c->pool_oos.opts.oos_max, 0))
    return XIVO_HIP_ERR_INVALID;
  const xivo_pool_oos_opts& o = c->pool_oos.opts;
  OosGateArgs a{};
  a.feats = c->resident_oos.feats; a.n_oos = o.oos_max; a.lay = c->lay;
  c->H.to(a.H, a.strideH, a.ldh); c->inn.to(a.inn, a.strideInn); c->P.to(a.P, a.strideP, a.ldp);
  a.row0 = c->rows.oos_row0(); a.Mp = c->Mpmax; a.Roos = o.Roos;
  std::copy(o.chi2, o.chi2 + 32, a.chi2);
  a.gamma = c->pool_oos.gamma;
  a.gated = &c->pool_oos.stats[0].oos_gated; a.gated_stride = (int)(sizeof(xivo_pool_oos_stats) / sizeof(long long)); a.batch = B;
  c->dx_clear();
  c->pool_oos.projected = false;   // one gate per projection
  StageTimer st(c, ST_GATE, 0.0, "oos_gate_kernel");
  HIP_TRY((hipError_t)launch_oos_gate(a, c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_get_rings(xivo_hip_ctx* c, int b0, int nb, int* anc_born, int* hist_cnt, int* hist_anchor, int* hist_born,
                                double* hist_xp) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->pool_oos.configured() || !c->pool_oos.hist_cnt) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t pm = c->pool.pool_max(), am = c->pool.anchor_max(), mo = c->pool_oos.opts.max_obs;
  const PoolOos& p = c->pool_oos;
  if (anc_born) HIP_TRY(hipMemcpyAsync(anc_born, p.anc_born + b0 * am, nb * am * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (hist_cnt) HIP_TRY(hipMemcpyAsync(hist_cnt, p.hist_cnt + b0 * pm, nb * pm * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (hist_anchor) HIP_TRY(hipMemcpyAsync(hist_anchor, p.hist_anchor + b0 * pm * mo, nb * pm * mo * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (hist_born) HIP_TRY(hipMemcpyAsync(hist_born, p.hist_born + b0 * pm * mo, nb * pm * mo * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (hist_xp) HIP_TRY(hipMemcpyAsync(hist_xp, p.hist_xp + b0 * pm * mo * 2, nb * pm * mo * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_get(xivo_hip_ctx* c, int b0, int nb, xivo_oos_in* list, double* gamma) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->pool_oos.configured() || c->resident_oos.n != c->pool_oos.opts.oos_max || b0 + nb > c->pool_oos.B)
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t n = (size_t)c->pool_oos.opts.oos_max;
  if (list) HIP_TRY(hipMemcpyAsync(list, c->resident_oos.feats + b0 * n, nb * n * sizeof(xivo_oos_in), hipMemcpyDeviceToHost, c->stream));
  if (gamma) HIP_TRY(hipMemcpyAsync(gamma, c->pool_oos.gamma + b0 * n, nb * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_oos_get_stats(xivo_hip_ctx* c, int b0, int nb, xivo_pool_oos_stats* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->pool_oos.configured() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(out, c->pool_oos.stats + b0, (size_t)nb * sizeof(xivo_pool_oos_stats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
