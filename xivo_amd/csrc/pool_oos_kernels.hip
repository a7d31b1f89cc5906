// The OOS / MSCKF list of a frame from pool entries whose track ended (gfx950), driven by capi_pool_oos.hip.
//
//  pool_oos_collect_kernel   which dropped entries are used (plife_oos_decide, pool_lifecycle_device.h) and the xivo_oos_in of
//                            each: Xs = Feature::Xs(gbc) (src/feature.cpp:107-118) of the resident entry and its anchor's pose,
//                            the valid observations oldest first - from the records the host life cycle hands over
//  pool_oos_select_kernel    the same list in the device pool life cycle, between its begin kernel and the pool step: the
//                            dropped entries are the resident live ones whose step pixel is NaN, their observations come from
//                            the rings in HBM (plife_valid_obs)
//  pool_oos_record_kernel    behind the device life cycle's end kernel: the anchor created in the frame observes every live entry
//                            (plife_hist_reset / plife_hist_append)
// One wave per filter. The device life cycle's select looks at every pool entry: one lane per entry for what is independent
// (dropped, READY, depth, valid observations), lane 0 only for the ordered pick, one lane per list position to write it. The
// host path's collect does the same over the records it is handed. Both producers write a list position through pool_oos_write_obs / pool_oos_write_xs, so the two
// life cycles leave the same bytes. The rows themselves are oos_kernel's (glevel_kernels.hip).
#include "ekf_kernels.h"
#include "geometry_device.h"
#include "pool_lifecycle_device.h"

namespace xivo_hip {

namespace {

// observation q of a list position (k counts the ones written); the tail behind the last one is cleared by pool_oos_close_obs
__device__ __forceinline__ void pool_oos_write_obs(xivo_oos_in& out, int& k, int g, double u, double v) {
  out.group_sind[k] = g; out.xp[k][0] = u; out.xp[k][1] = v;
  ++k;
}
__device__ __forceinline__ void pool_oos_close_obs(xivo_oos_in& out, int k) {
  out.n_obs = k;
  for (int q = k; q < XIVO_OOS_MAX_OBS; ++q) { out.group_sind[q] = 0; out.xp[q][0] = 0.0; out.xp[q][1] = 0.0; }
}
// Xs(gbc) = ref_->gsb() * gbc * Xc (feature.cpp:112-113), in lc_rows_kernel's order, of resident entry f: its anchor's pose is
// the slot's resident pose while linked, else the frozen one (as the sub-filter step reads it)
__device__ __forceinline__ void pool_oos_write_xs(xivo_oos_in& out, const xivo_subfilter_feat& f, const PoolAnchor* anchors,
                                                  const xivo_group_in* groups, int n_groups, const xivo_pose_in& pose, int invdepth) {
  const PoolAnchor& A = anchors[f.ref_sind];
  const xivo_group_in& G = (A.slot >= 0 && A.slot < n_groups) ? groups[A.slot] : A.g;
  M3 dXc_dx;
  const V3 Xc = feature_unproject(f.x, invdepth, dXc_dx);
  V3 Xb = m3_mulv(m3_from_colmajor(pose.Rbc), Xc);
#pragma unroll
  for (int i = 0; i < 3; ++i) Xb.v[i] += pose.Tbc[i];
  const V3 Xs = m3_mulv(m3_from_colmajor(G.Rsb), Xb);
#pragma unroll
  for (int i = 0; i < 3; ++i) out.Xs[i] = Xs.v[i] + G.Tsb[i];
}

__global__ __launch_bounds__(64) void pool_oos_collect_kernel(PoolOosCollectArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sPick[64];   // record index of list position q (oos_max <= 64)
  __shared__ int sUsed;
  __shared__ signed char sCase[XIVO_POOL_MAX_ENTRIES];   // per record (distinct entries: at most pool_max): 0 not eligible, 1 eligible, 2 short
  const int c0 = a.off[filt], c1 = a.off[filt + 1];
  const int nrec = c1 - c0 < XIVO_POOL_MAX_ENTRIES ? c1 - c0 : XIVO_POOL_MAX_ENTRIES;
  // one lane per record for what is independent (live, READY, depth, observations inside the layout: plife_oos_decide with
  // nothing used yet and room for one), lane 0 for the ordered pick
  for (int i = lane; i < nrec; i += 64) {
    const xivo_pool_oos_cand& r = a.cands[c0 + i];
    int cs = 0;
    if (r.entry >= 0 && r.entry < a.pool_max) {
      const xivo_subfilter_feat& f = a.pool[(long)filt * a.pool_max + r.entry];
      if (f.ref_sind >= 0 && f.ref_sind < a.anchor_max) {                  // a live entry
        const double z = feature_depth(f.x[2], a.invdepth);
        int k = 0;                                                         // observations inside the layout
        for (int q = 0; q < r.n_obs && q < a.max_obs; ++q) k += (r.group_sind[q] >= 0 && r.group_sind[q] < a.n_groups) ? 1 : 0;
        const int d = plife_oos_decide(f.status == XIVO_FEAT_READY, z > a.min_depth && z < a.max_depth, k, a.min_obs, 0, 1);
        cs = d == PLIFE_OOS_USED ? 1 : (d == PLIFE_OOS_SHORT ? 2 : 0);
      }
    }
    sCase[i] = (signed char)cs;
  }
  __syncthreads();
  if (lane == 0) {
    int used = 0;
    long long n_short = 0, n_surplus = 0;
    for (int i = 0; i < nrec; ++i) {
      if (sCase[i] == 2) ++n_short;
      else if (sCase[i] == 1) { if (used < a.oos_max) sPick[used++] = c0 + i; else ++n_surplus; }
    }
    sUsed = used;
    xivo_pool_oos_stats& st = a.stats[filt];
    st.oos_used += used; st.oos_short += n_short; st.oos_surplus += n_surplus;
  }
  __syncthreads();
  if (lane >= a.oos_max) return;
  xivo_oos_in& out = a.list[(long)filt * a.oos_max + lane];
  if (lane >= sUsed) { out.n_obs = 0; return; }
  const xivo_pool_oos_cand& r = a.cands[sPick[lane]];
  const xivo_subfilter_feat& f = a.pool[(long)filt * a.pool_max + r.entry];
  pool_oos_write_xs(out, f, a.anchors + (long)filt * a.anchor_max, a.groups + (long)filt * a.n_groups, a.n_groups, a.poses[filt],
                    a.invdepth);
  int k = 0;
  for (int q = 0; q < r.n_obs && q < a.max_obs; ++q) {
    const int g = r.group_sind[q];
    if (g < 0 || g >= a.n_groups) continue;                                // a bad slot drops that observation
    pool_oos_write_obs(out, k, g, r.xp[q][0], r.xp[q][1]);
  }
  pool_oos_close_obs(out, k);
}

__global__ __launch_bounds__(64) void pool_oos_select_kernel(PoolOosLifeArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sLink[XIVO_POOL_LIFE_MAX_ANCHORS];
  __shared__ int sPick[64];   // entry of list position q
  __shared__ int sUsed;
  __shared__ signed char sCase[XIVO_POOL_MAX_ENTRIES];   // per entry: -1 not dropped, 0 not eligible, 1 eligible, 2 short
  const int pm = a.pool_max, am = a.anchor_max, mo = a.max_obs;
  const xivo_subfilter_feat* pool = a.pool + (long)filt * pm;
  const PoolAnchor* anchors = a.anchors + (long)filt * am;
  xivo_oos_in* list = a.list + (long)filt * a.oos_max;
  const int* cnt = a.hist_cnt + (long)filt * pm;
  const int* ha = a.hist_anchor + (long)filt * pm * mo;
  const int* hb = a.hist_born + (long)filt * pm * mo;
  const double* hx = a.hist_xp + (long)filt * pm * mo * 2;
  const int* aused = a.anc_used + (long)filt * am;
  const int* aborn = a.anc_born + (long)filt * am;
  for (int t = lane; t < am; t += 64) sLink[t] = anchors[t].slot;   // (after the begin kernel's removals: the groups that left are unlinked)
  __syncthreads();
  // what is independent per entry, one lane each: dropped, READY, depth, the number of valid observations (the rule's outcome
  // but for its place in the order: plife_oos_decide with nothing used yet and room for one)
  int slot[XIVO_OOS_MAX_OBS], grp[XIVO_OOS_MAX_OBS];
  for (int e = lane; e < pm; e += 64) {
    const xivo_subfilter_feat& f = pool[e];
    const double u = a.xp[2 * ((long)filt * pm + e)];
    int c = -1;
    // live in the resident pool and without a pixel for the step: the tracker dropped it this frame
    if (f.ref_sind >= 0 && f.ref_sind < am && u != u) {
      const int k = plife_valid_obs(cnt, ha, hb, e, mo, aused, aborn, sLink, am, a.n_groups, slot, grp);
      const double z = feature_depth(f.x[2], a.invdepth);
      const int d = plife_oos_decide(f.status == XIVO_FEAT_READY, z > a.min_depth && z < a.max_depth, k, a.min_obs, 0, 1);
      c = d == PLIFE_OOS_USED ? 1 : (d == PLIFE_OOS_SHORT ? 2 : 0);
    }
    sCase[e] = (signed char)c;
  }
  __syncthreads();
  if (lane == 0) {   // the order: ascending entry, the first oos_max eligible ones are used, the others surplus
    int used = 0;
    long long n_short = 0, n_surplus = 0;
    for (int e = 0; e < pm; ++e) {
      if (sCase[e] == 2) ++n_short;
      else if (sCase[e] == 1) { if (used < a.oos_max) sPick[used++] = e; else ++n_surplus; }
    }
    sUsed = used;
    xivo_pool_oos_stats& st = a.stats[filt];
    st.oos_used += used; st.oos_short += n_short; st.oos_surplus += n_surplus;
  }
  __syncthreads();
  if (lane >= a.oos_max) return;
  xivo_oos_in& out = list[lane];
  if (lane >= sUsed) { out.n_obs = 0; return; }
  const int e = sPick[lane];       // one lane per list position: its observations from the ring, oldest first, then Xs
  const int k = plife_valid_obs(cnt, ha, hb, e, mo, aused, aborn, sLink, am, a.n_groups, slot, grp);
  int kk = 0;
  for (int q = 0; q < k; ++q) pool_oos_write_obs(out, kk, grp[q], hx[2 * (e * mo + slot[q])], hx[2 * (e * mo + slot[q]) + 1]);
  pool_oos_close_obs(out, kk);
  pool_oos_write_xs(out, pool[e], anchors, a.groups + (long)filt * a.n_groups, a.n_groups, a.poses[filt], a.invdepth);
}

// one workgroup per filter. The anchor the end kernel created in this frame is the one used anchor of life 0 (every older one was
// ticked by the begin kernel, and a new one cannot expire in its own frame); entries born in this frame start an empty ring.
__global__ __launch_bounds__(64) void pool_oos_record_kernel(PoolOosLifeArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sNew;
  const int pm = a.pool_max, am = a.anchor_max, mo = a.max_obs;
  if (lane == 0) sNew = -1;
  __syncthreads();
  for (int t = lane; t < am; t += 64)
    if (a.anc_used[(long)filt * am + t] && a.anc_life[(long)filt * am + t] == 0) sNew = t;
  __syncthreads();
  const int an = sNew;
  if (an < 0) return;                                   // a frame that creates no anchor records nothing
  if (lane == 0) a.anc_born[(long)filt * am + an] = a.frame;
  int* cnt = a.hist_cnt + (long)filt * pm;
  int* ha = a.hist_anchor + (long)filt * pm * mo;
  int* hb = a.hist_born + (long)filt * pm * mo;
  double* hx = a.hist_xp + (long)filt * pm * mo * 2;
  for (int e = lane; e < pm; e += 64) {
    if (a.ent_id[(long)filt * pm + e] < 0) continue;
    if (a.ent_born[(long)filt * pm + e] == a.frame) plife_hist_reset(cnt, e);
    const xivo_subfilter_feat& f = a.pool[(long)filt * pm + e];   // (xp: the frame's pixel - the step's, or the new entry's first)
    const int s = plife_hist_append(cnt, ha, hb, e, mo, an, a.frame);
    hx[2 * (e * mo + s)] = f.xp[0]; hx[2 * (e * mo + s) + 1] = f.xp[1];
  }
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_pool_oos_select(const PoolOosLifeArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(pool_oos_select_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_pool_oos_record(const PoolOosLifeArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(pool_oos_record_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_pool_oos_collect(const PoolOosCollectArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(pool_oos_collect_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
