// C ABI, features outside the state (include/xivo_hip.h): the depth sub-filter, the candidate order, the feature pool and the depth
// initialisation of new tracks (triangulation, AdaptInitialDepth). Host-side orchestration only (capi_internal.h); the pool's host
// mirrors are PoolMirror (pool_mirror.h).
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace xivo_hip::capi {
// one pool step of filters [0, B) on the context's pool: everything but where the pixels come from and the results go (xp, order,
// n, live) - xivo_hip_pool_step points them at its per-call staging, xivo_hip_pool_life_begin at its resident buffers
PoolStepArgs pool_step_args(xivo_hip_ctx* c, int B, int strict) {
  PoolStepArgs a{};
  a.pool = c->pool.entries; a.anchors = c->pool.anchors; a.pool_max = c->pool.pool_max(); a.anchor_max = c->pool.anchor_max();
  a.poses = c->poses; a.groups = c->groups; a.n_groups = c->lay.n_groups;
  a.cam = c->cam; a.calib = c->calib_on ? c->calib : nullptr; a.cam_dim = c->calib_on ? c->cl.cam_dim : 0;
  a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  a.o = c->pool.opts; a.remove_outlier = c->pool.remove_outlier; a.strict = strict ? 1 : 0; a.batch = B;
  a.tri = c->pool.tri; a.tri_good = c->pool.tri_counts; a.tri_bad = c->pool.tri_counts + c->Bmax;
  return a;
}
}  // namespace xivo_hip::capi

extern "C" {

static int ensure_pool_io(xivo_hip_ctx* c, size_t bytes) { return c->mem.grow(&c->pool.io, &c->pool.io_cap, bytes); }

int xivo_hip_subfilter_update(xivo_hip_ctx* c, int b0, int nb, int n, xivo_subfilter_feat* feats,
                              const xivo_subfilter_opts* opts) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->have_layout || !c->poses || n <= 0 || !feats || !opts) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  for (size_t i = 0; i < (size_t)nb * n; ++i)
    if (feats[i].ref_sind < 0 || feats[i].ref_sind >= c->lay.n_groups) return XIVO_HIP_ERR_INVALID;
  const size_t bytes = (size_t)nb * n * sizeof(xivo_subfilter_feat);
  if (int rc = c->mem.grow(&c->sub, &c->sub_cap, (size_t)nb * n)) return rc;
  HIP_TRY(hipMemcpyAsync(c->sub, feats, bytes, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "subfilter_kernel");
    if (launch_subfilter(c->sub, n, c->poses + b0, c->groups + (size_t)b0 * c->lay.n_groups, c->lay.n_groups, c->cam,
                         *opts, nb, c->stream, c->calib_on ? c->calib + b0 : nullptr, c->calib_on ? c->cl.cam_dim : 0,
                         (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0))
      return XIVO_HIP_ERR_HIP;
  }
  HIP_TRY(hipMemcpyAsync(feats, c->sub, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

// Criteria::CandidateComparison (src/options.cpp:34-61) and the selection order of SelectAndAddNewFeatures /
// AddFeaturesToState-style loops (src/manager.cpp:364-376,417-421): host arithmetic on the array
// xivo_hip_subfilter_update returned - no device work.
int xivo_hip_candidate_order(const xivo_subfilter_feat* feats, int nb, int n, int strict, int score_type, int* order_out,
                             int* n_out, double* score_out) {
  if (!feats || nb < 0 || n <= 0 || !order_out || !n_out || score_type < 0 || score_type > 2) return XIVO_HIP_ERR_INVALID;
  for (int b = 0; b < nb; ++b) {
    const xivo_subfilter_feat* f = feats + (size_t)b * n;
    std::vector<int> idx;
    for (int i = 0; i < n; ++i) {
      if (score_out) {
        const double dn = sqrt(f[i].P[0] * f[i].P[0] + f[i].P[4] * f[i].P[4] + f[i].P[8] * f[i].P[8]);   // P().diagonal().norm()
        score_out[(size_t)b * n + i] = score_type == 0 ? -1.0 * f[i].P[8] : (score_type == 1 ? -1.0 * dn : -1.0 * (dn + f[i].outlier_counter));
      }
      if (f[i].candidate & (strict ? 2 : 1)) idx.push_back(i);
    }
    // as coded, the comparison ignores the score it has just computed from comparison_score_type and orders by
    // status, then Feature::score() = -P(2,2) (options.cpp:60); FeatureStatus READY = 2 > INITIALIZING = 1 (core.h:190-199).
    // std::sort leaves the order of equivalent elements unspecified: here ties keep the list order.
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int c2) {
      const int s1 = f[a].status == XIVO_FEAT_READY ? 2 : 1, s2 = f[c2].status == XIVO_FEAT_READY ? 2 : 1;
      return (s1 > s2) || (s1 == s2 && -f[a].P[8] > -f[c2].P[8]);
    });
    n_out[b] = (int)idx.size();
    for (int i = 0; i < n; ++i) order_out[(size_t)b * n + i] = i < (int)idx.size() ? idx[i] : -1;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_pool_config(xivo_hip_ctx* c, int pool_max, int anchor_max, const xivo_subfilter_opts* opts,
                         double remove_outlier_counter) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || pool_max < 1 || anchor_max < 1 || !opts) return XIVO_HIP_ERR_INVALID;
  if (pool_max > XIVO_POOL_MAX_ENTRIES) return XIVO_HIP_ERR_UNSUPPORTED;
  HIP_TRY(hipStreamSynchronize(c->stream));
  pool_life_release(c);   // the device pool life cycle's books describe the pool given back here
  lclife_release(c);      // (a context with a pool runs no immediate life cycle: its keys go too)
  pool_oos_release(c);    // ... and so do the OOS list and counters of its dropped entries
  c->mem.release(&c->pool.entries, &c->pool.anchors, &c->pool.tri_counts, &c->pool.init_z);
  c->pool.reset();   // (the mirrors, the triangulation and adaptive-depth options with it)
  const size_t ne = (size_t)c->Bmax * pool_max, na = (size_t)c->Bmax * anchor_max;
  int rc = c->mem.raw(&c->pool.entries, ne);
  if (!rc) rc = c->mem.raw(&c->pool.anchors, na);
  if (!rc) rc = c->mem.raw(&c->pool.tri_counts, 2 * (size_t)c->Bmax);
  if (!rc) rc = c->mem.raw(&c->pool.init_z, (size_t)c->Bmax);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->pool.tri_counts, 0, 2 * (size_t)c->Bmax * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->pool.init_z, 0, (size_t)c->Bmax * sizeof(double), c->stream));
  // all bytes 0xff: every entry's anchor (ref_sind) and every anchor's slot read -1 - free / unlinked
  HIP_TRY(hipMemsetAsync(c->pool.entries, 0xff, ne * sizeof(xivo_subfilter_feat), c->stream));
  HIP_TRY(hipMemsetAsync(c->pool.anchors, 0xff, na * sizeof(PoolAnchor), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pool.mirror.configure(c->Bmax, pool_max, anchor_max);   // every entry free, no anchor created
  c->pool.opts = *opts; c->pool.remove_outlier = remove_outlier_counter;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_anchor(xivo_hip_ctx* c, int b0, int nb, const int* slot) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->pool.configured() || c->plife.configured() || !c->poses || (nb > 0 && !slot)) return XIVO_HIP_ERR_INVALID;
  for (int b = 0; b < nb; ++b) {
    if (slot[b] < -1 || slot[b] >= c->pool.anchor_max()) return XIVO_HIP_ERR_INVALID;
    if (slot[b] >= 0 && c->pool.mirror.anchor_linked(b0 + b, slot[b])) return XIVO_HIP_ERR_INVALID;
  }
  if (nb == 0) return XIVO_HIP_OK;
  int rc = ensure_pool_io(c, (size_t)nb * sizeof(int));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->pool.io, slot, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_anchor_kernel");
    HIP_TRY((hipError_t)launch_pool_anchor(c->pool.anchors + (size_t)b0 * c->pool.anchor_max(), c->pool.anchor_max(), c->poses + b0,
                                           (const int*)c->pool.io, nb, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // slot is borrowed host memory
  for (int b = 0; b < nb; ++b)
    if (slot[b] >= 0) c->pool.mirror.anchor_created(b0 + b, slot[b]);
  return XIVO_HIP_OK;
}

int xivo_hip_pool_add(xivo_hip_ctx* c, int n, const xivo_pool_new* recs) { return xivo_hip_pool_add_ex(c, n, recs, 0u); }

int xivo_hip_pool_add_ex(xivo_hip_ctx* c, int n, const xivo_pool_new* recs, unsigned options) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->pool.configured() || c->plife.configured() || !c->have_layout || n < 0 || (n > 0 && !recs)) return XIVO_HIP_ERR_INVALID;
  if ((options & ~XIVO_POOL_ADD_ADAPTIVE_Z) != 0u) return XIVO_HIP_ERR_INVALID;
  const bool adaptive = (options & XIVO_POOL_ADD_ADAPTIVE_Z) != 0u;
  if (adaptive && !c->pool.adapt_on) return XIVO_HIP_ERR_INVALID;
  std::vector<long> keys((size_t)n);
  for (int i = 0; i < n; ++i) {
    const xivo_pool_new& r = recs[i];
    if (r.b < 0 || r.b >= c->Bmax || r.entry < 0 || r.entry >= c->pool.pool_max() || r.anchor < 0 || r.anchor >= c->pool.anchor_max() ||
        !c->pool.mirror.anchor_exists(r.b, r.anchor) || (!adaptive && !(r.z0 > 0.0)))
      return XIVO_HIP_ERR_INVALID;
    keys[i] = (long)r.b * c->pool.pool_max() + r.entry;
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return XIVO_HIP_ERR_INVALID;   // one record per entry
  if (n == 0) return XIVO_HIP_OK;
  int rc = ensure_pool_io(c, (size_t)n * sizeof(xivo_pool_new));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->pool.io, recs, (size_t)n * sizeof(xivo_pool_new), hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_add_kernel");
    HIP_TRY((hipError_t)launch_pool_add(c->pool.entries, c->pool.pool_max(), (const xivo_pool_new*)c->pool.io, n, c->cam,
                                        c->calib_on ? c->calib : nullptr, c->calib_on ? c->cl.cam_dim : 0,
                                        (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0, c->stream, adaptive ? c->pool.init_z : nullptr));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // recs is borrowed host memory
  for (int i = 0; i < n; ++i) c->pool.mirror.entry_added(recs[i].b, recs[i].entry, recs[i].anchor);
  return XIVO_HIP_OK;
}

int xivo_hip_pool_step(xivo_hip_ctx* c, int B, const double* xp, int strict, int* order_out, int* n_out,
                       unsigned char* live_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->pool.configured() || c->plife.configured() || !c->have_layout || !c->poses || B <= 0 || B > c->Bmax || !xp || !order_out || !n_out ||
      !live_out)
    return XIVO_HIP_ERR_INVALID;
  const size_t ne = (size_t)B * c->pool.pool_max();
  const size_t b_xp = ne * 2 * sizeof(double), b_ord = ne * sizeof(int), b_n = (size_t)B * sizeof(int);
  int rc = ensure_pool_io(c, b_xp + b_ord + b_n + ne);
  if (rc) return rc;
  char* io = c->pool.io;
  PoolStepArgs a = pool_step_args(c, B, strict);
  a.xp = (const double*)io; a.order = (int*)(io + b_xp); a.n = (int*)(io + b_xp + b_ord);
  a.live = (unsigned char*)(io + b_xp + b_ord + b_n);
  HIP_TRY(hipMemcpyAsync(io, xp, b_xp, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "pool_step_kernel");
    HIP_TRY((hipError_t)launch_pool_step(a, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(order_out, a.order, b_ord, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(n_out, a.n, b_n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(live_out, a.live, ne, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pool.mirror.entries_dead(live_out, B);
  return XIVO_HIP_OK;
}

int xivo_hip_pool_get(xivo_hip_ctx* c, int b0, int nb, xivo_subfilter_feat* entries, xivo_group_in* anchor_poses,
                      int* anchor_slots) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !c->pool.configured()) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (entries)
    HIP_TRY(hipMemcpyAsync(entries, c->pool.entries + (size_t)b0 * c->pool.pool_max(), (size_t)nb * c->pool.pool_max() * sizeof(xivo_subfilter_feat),
                           hipMemcpyDeviceToHost, c->stream));
  std::vector<PoolAnchor> anc;
  if (anchor_poses || anchor_slots) {
    anc.resize((size_t)nb * c->pool.anchor_max());
    HIP_TRY(hipMemcpyAsync(anc.data(), c->pool.anchors + (size_t)b0 * c->pool.anchor_max(), anc.size() * sizeof(PoolAnchor),
                           hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < anc.size(); ++i) {
    if (anchor_poses) anchor_poses[i] = anc[i].g;
    if (anchor_slots) anchor_slots[i] = anc[i].slot;
  }
  return XIVO_HIP_OK;
}

// ---- depth initialisation of new tracks: triangulation and AdaptInitialDepth
static bool tri_opts_ok(const xivo_triangulate_opts* o) {
  return o->struct_size == (int)sizeof(xivo_triangulate_opts) && o->method >= XIVO_TRI_OFF && o->method <= XIVO_TRI_LINF;
}

int xivo_hip_triangulate(xivo_hip_ctx* c, int n, const xivo_tri_in* in, xivo_tri_out* out, const xivo_triangulate_opts* o) {
  if (!c || n < 0 || !o || (n > 0 && (!in || !out)) || !tri_opts_ok(o) || o->method == XIVO_TRI_OFF) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (n == 0) return XIVO_HIP_OK;
  const size_t bi = (size_t)n * sizeof(xivo_tri_in), bo = (size_t)n * sizeof(xivo_tri_out);
  int rc = ensure_pool_io(c, bi + bo);
  if (rc) return rc;
  char* io = c->pool.io;
  HIP_TRY(hipMemcpyAsync(io, in, bi, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "triangulate_kernel");
    HIP_TRY((hipError_t)launch_triangulate((const xivo_tri_in*)io, (xivo_tri_out*)(io + bi), n, *o, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(out, io + bi, bo, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_triangulation(xivo_hip_ctx* c, const xivo_triangulate_opts* o) {
  if (!c || !c->pool.configured() || (o && !tri_opts_ok(o))) return XIVO_HIP_ERR_INVALID;
  c->pool.tri = o ? *o : xivo_triangulate_opts{};
  return XIVO_HIP_OK;
}

int xivo_hip_pool_tri_counts(xivo_hip_ctx* c, int b0, int nb, int* good_out, int* bad_out) {
  if (bad_range(c, b0, nb) || !c->pool.tri_counts) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (nb == 0) return XIVO_HIP_OK;
  if (good_out)
    HIP_TRY(hipMemcpyAsync(good_out, c->pool.tri_counts + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (bad_out)
    HIP_TRY(hipMemcpyAsync(bad_out, c->pool.tri_counts + c->Bmax + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_adapt_depth_config(xivo_hip_ctx* c, const xivo_adapt_depth_opts* o) {
  if (!c || !c->pool.init_z || !o || o->struct_size != (int)sizeof(xivo_adapt_depth_opts) || !(o->initial_z > 0.0) ||
      !(o->median_weight >= 0.0 && o->median_weight <= 1.0))
    return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  std::vector<double> z((size_t)c->Bmax, o->initial_z);
  HIP_TRY(hipMemcpyAsync(c->pool.init_z, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pool.adapt = *o; c->pool.adapt_on = true;
  return XIVO_HIP_OK;
}

int xivo_hip_pool_adapt_depth(xivo_hip_ctx* c, int B, double* init_z_out) {
  if (!c || !c->pool.configured() || !c->pool.adapt_on || B <= 0 || B > c->Bmax) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (adapt_depth_lds(c->feats ? c->F : 0, c->pool.pool_max()) > 60 * 1024) return XIVO_HIP_ERR_UNSUPPORTED;
  int rc = ensure_pool_io(c, (size_t)B * sizeof(double));
  if (rc) return rc;
  AdaptDepthArgs a{};
  a.feats = c->feats; a.F = c->feats ? c->F : 0; a.Fmax = c->Fmax;
  a.pool = c->pool.entries; a.pool_max = c->pool.pool_max();
  a.init_z = c->pool.init_z; a.init_z_out = (double*)c->pool.io;
  a.beta = c->pool.adapt.median_weight; a.min_z = c->pool.adapt.min_z; a.max_z = c->pool.adapt.max_z;
  a.min_lifetime = c->pool.adapt.min_feature_lifetime; a.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0; a.batch = B;
  {
    StageTimer st(c, ST_OTHER, 0.0, "adapt_depth_kernel");
    HIP_TRY((hipError_t)launch_adapt_depth(a, c->stream));
  }
  if (init_z_out) HIP_TRY(hipMemcpyAsync(init_z_out, a.init_z_out, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_pool_get_init_z(xivo_hip_ctx* c, int b0, int nb, double* init_z_out) {
  if (bad_range(c, b0, nb) || !c->pool.init_z || !c->pool.adapt_on || (nb > 0 && !init_z_out)) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(init_z_out, c->pool.init_z + b0, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}
}  // extern "C"
