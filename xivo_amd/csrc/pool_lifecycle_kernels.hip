// The per-frame feature life cycle of the "subfilter" mode on the device (gfx950): what SequenceRunner._frame_subfilter
// (xivo_amd/sequence.py) decides per filter on the host around xivo_hip_pool_step and sends down as xivo_edit_op lists, pixel
// arrays, anchor slots and xivo_pool_new records. One workgroup of 256 threads per filter; the filter's books, the frame's
// track ids and the per-slot, per-entry and per-anchor tables in static LDS. The in-state half (book, track ids, association,
// removals, pixels) is instate_book_device.h's, shared with lifecycle_kernels.hip; this file keeps what is about entries and anchors.
//
//  pool_life_begin_kernel  before the step: Group::IncrementLifetime (src/manager.cpp:36-41), association of tracks with feature
//                          slots and pool entries, tracker-dropped features leave the state with the groups they leave empty
//                          (ProcessTracks, :152-169), tracker-dropped entries leave the pool, the step's pixels (:171-250)
//  (pool_tri_kernel / pool_step_kernel of pool_kernels.hip run here, on device buffers)
//  pool_life_admit_kernel  entries the step did not leave live are freed (:236-240), the walk over the step's order
//                          (SelectAndAddNewFeatures / ZeroGaugeXYAddFeatures, :332-450), the frame's pixels of the in-state features
//  (the update and AbsorbError run here)
//  pool_life_end_kernel    gate-rejected features leave (src/update.cpp:105-113), empty groups are discarded, new tracks get an
//                          anchor from the updated pose and pool entries (Group::Create + InitializeJustCreatedTracks,
//                          :121-126, :575-600), EnforceMaxGroupLifetime (:282-304)
// (paths relative to the reference tree). The decisions are the functions of pool_lifecycle_device.h / lifecycle_device.h; the
// P edits are the functions of edit_device.h that edit_batch_kernel calls, in the order the host's op lists have; a new anchor
// and a new entry are written by the functions of pool_device.h that pool_anchor_kernel / pool_add_kernel call. So P, the
// scene, the pool and the anchors come out bit for bit as from the host life cycle. Nothing crosses workgroups: no atomics on
// global memory, the counters and the books belong to the filter's own workgroup (LDS atomics only). The tracks are read
// through life_track_begin / life_track_count (lifecycle_tracks_device.h) alone.
#include "ekf_kernels.h"
#include "geometry_device.h"
#include "instate_book_device.h"
#include "pool_device.h"
#include "pool_lifecycle_device.h"

namespace xivo_hip {

namespace {

constexpr int kTracks = XIVO_LIFE_MAX_TRACKS, kSlots = XIVO_LIFE_MAX_SLOTS, kEntries = XIVO_POOL_MAX_ENTRIES,
              kAnchors = XIVO_POOL_LIFE_MAX_ANCHORS;

// the LDS plan of the three kernels: the in-state book (16 KiB of ids, 2 + 5 x 1 KiB per-slot tables), 8 KiB of per-track
// flags, 4 + 5 x 2 KiB per-entry tables, 3 x 1 KiB per-anchor tables, 3 x 2 KiB of walk ops = 54 KiB
struct PoolLifeLds {
  InstateBook k;               // (ids: begin, end)
  long long eid[kEntries];     // pool book: track id by entry
  int fresh[kTracks];          // end: the track is new
  int eborn[kEntries];
  int eanc[kEntries];          // anchor by entry (the resident ref_sind of a held entry)
  int etrack[kEntries];        // entry -> track of the frame that feeds it (-1: none)
  int efree[kEntries], pick[kEntries];   // end: free entries ascending, new tracks by rank
  int aused[kAnchors], alife[kAnchors];  // pool book
  int alink[kAnchors];         // group slot by anchor (the resident slot)
  int op_kind[2 * kSlots], op_i0[2 * kSlots], op_i1[2 * kSlots];   // admit: the walk's ops
  int n_ops, n_dead, n_new, a_new, n_take, n_expired;
};

// the books and the ids of the filter's n tracks come in (n = 0: a kernel that does not look at the ids)
__device__ __forceinline__ void plife_load(const PoolLifeArgs& a, PoolLifeLds& s, int b, int n, int tid) {
  const int pm = a.pool_max, am = a.anchor_max;
  book_load(a.life, s.k, b, tid);
  for (int e = tid; e < pm; e += 256) {
    const long long id = a.ent_id[(long)b * pm + e];
    const int anc = a.pool[(long)b * pm + e].ref_sind;
    s.eid[e] = id;
    s.eborn[e] = a.ent_born[(long)b * pm + e];
    s.eanc[e] = (id >= 0 && anc >= 0 && anc < am) ? anc : -1;
    s.etrack[e] = -1;
  }
  for (int t = tid; t < am; t += 256) {
    s.aused[t] = a.anc_used[(long)b * am + t];
    s.alife[t] = a.anc_life[(long)b * am + t];
    s.alink[t] = a.anchors[(long)b * am + t].slot;
  }
  book_load_ids(a.life, s.k, b, n, tid);
}

// the books go back (the entry's anchor and the anchor's link are resident in the pool and the anchor table themselves)
__device__ __forceinline__ void plife_store(const PoolLifeArgs& a, const PoolLifeLds& s, int b, int tid) {
  const int pm = a.pool_max, am = a.anchor_max;
  book_store(a.life, s.k, b, tid);
  for (int e = tid; e < pm; e += 256) { a.ent_id[(long)b * pm + e] = s.eid[e]; a.ent_born[(long)b * pm + e] = s.eborn[e]; }
  for (int t = tid; t < am; t += 256) { a.anc_used[(long)b * am + t] = s.aused[t]; a.anc_life[(long)b * am + t] = s.alife[t]; }
}

// thread 0: groups left empty go to rm_group and their anchors are unlinked
__device__ __forceinline__ void plife_discard_groups(PoolLifeLds& s, int G, int am) {
  book_discard_empty_groups(s.k, G);
  for (int q = 0; q < s.k.n_rm_group; ++q)
    for (int t = 0; t < am; ++t) plife_unlink(s.alink, t, s.k.rm_group[q]);
}

__device__ __forceinline__ void plife_apply_removals(const PoolLifeArgs& a, const PoolLifeLds& s, int b, int tid) {
  book_apply_removals(a.life, s.k, b, a.anchors + (long)b * a.anchor_max, a.anchor_max, tid);
}

__global__ __launch_bounds__(256) void pool_life_begin_kernel(PoolLifeArgs a) {
  __shared__ PoolLifeLds s;
  const LifeArgs& l = a.life;
  const int b = blockIdx.x, tid = threadIdx.x, F = l.F, G = l.lay.n_groups, pm = a.pool_max, am = a.anchor_max;
  const int k0 = life_track_begin(l, b), n = life_track_count(l, b);
  plife_load(a, s, b, n, tid);
  __syncthreads();
  for (int t = tid; t < am; t += 256) s.alife[t] = plife_anchor_tick(s.aused[t], s.alife[t]);
  // association: one thread per track scans the in-state ids, then the pool's; of a repeated id the last occurrence feeds
  book_associate(s.k, F, n, tid);
  for (int k = tid; k < n; k += 256)
    for (int e = 0; e < pm; ++e)
      if (plife_entry_holds(s.eid, e, s.k.ids[k])) atomicMax(&s.etrack[e], k);
  __syncthreads();
  if (tid == 0) {   // ProcessTracks (src/manager.cpp:152-169)
    book_drop_where(s.k, F, [&](int j) { return s.k.slot_track[j] < 0; });
    plife_discard_groups(s, G, am);
    a.stats[b].dropped += s.k.n_rm_feat;
  }
  // the pool's side (:171-250): an entry without a track is freed; the step frees the resident entry on the NaN it gets
  for (int e = tid; e < pm; e += 256) {
    const bool leaves = plife_entry_leaves(s.eid, s.eanc, e, s.etrack[e]);
    double u = __longlong_as_double(0x7ff8000000000000LL), v = u;
    if (!leaves) { const double* m = l.meas + 3 * (long)(k0 + s.etrack[e]); u = m[0]; v = m[1]; }
    a.xp[2 * ((long)b * pm + e)] = u; a.xp[2 * ((long)b * pm + e) + 1] = v;
    a.ent_track[(long)b * pm + e] = leaves ? -1 : s.etrack[e];
  }
  __syncthreads();
  for (int j = tid; j < F; j += 256) a.slot_track[(long)b * l.slot_ld + j] = s.k.fid[j] >= 0 ? s.k.slot_track[j] : -1;
  plife_apply_removals(a, s, b, tid);
  plife_store(a, s, b, tid);
}

__global__ __launch_bounds__(256) void pool_life_admit_kernel(PoolLifeArgs a) {
  __shared__ PoolLifeLds s;
  const LifeArgs& l = a.life;
  const int b = blockIdx.x, tid = threadIdx.x, F = l.F, G = l.lay.n_groups, pm = a.pool_max, am = a.anchor_max;
  double* P = l.P + (long)b * l.strideP;
  xivo_feat_in* feats = l.feats + (long)b * l.Fmax;
  plife_load(a, s, b, 0, tid);
  if (tid == 0) s.n_dead = 0;
  __syncthreads();
  for (int j = tid; j < F; j += 256) s.k.slot_track[j] = a.slot_track[(long)b * l.slot_ld + j];
  for (int e = tid; e < pm; e += 256) {
    s.etrack[e] = a.ent_track[(long)b * pm + e];
    if (plife_free_if_dead(s.eid, s.eanc, e, a.live[(long)b * pm + e])) atomicAdd(&s.n_dead, 1);   // (:236-240)
  }
  __syncthreads();
  if (tid == 0) {   // the walk is serial by its nature: every step depends on the slots the one before took
    int n_adm = 0, n_gadd = 0, n_in = 0;
    long long steps = 0;
    int n = a.n[b];
    n = n < 0 ? 0 : (n > pm ? pm : n);
    s.n_ops = plife_walk(a.order + (long)b * pm, n, a.frame, s.k.fid, s.k.fref, s.k.gref, F, G, s.eid, s.eanc, s.eborn, s.etrack, pm,
                         s.alink, am, s.k.slot_track, s.op_kind, s.op_i0, s.op_i1, &n_adm, &n_gadd, &steps);
    for (int j = 0; j < F; ++j) n_in += s.k.fid[j] >= 0 ? 1 : 0;
    xivo_pool_life_stats& st = a.stats[b];
    st.pool_outliers += s.n_dead;
    st.admitted += n_adm; st.groups_added += n_gadd; st.admit_steps += steps;
    st.updates += n_in > 0 ? 1 : 0;
  }
  __syncthreads();
  for (int o = 0; o < s.n_ops; ++o) {   // (uniform over the workgroup)
    if (s.op_kind[o] == PLIFE_OP_ADD_GROUP_ANCHOR)
      edit_add_group_anchor(P, l.ldp, l.Np, l.lay, l.groups + (long)b * G, a.anchors[(long)b * am + s.op_i1[o]], s.op_i0[o], tid);
    else
      edit_admit_pool(P, l.ldp, l.Np, l.lay, feats, a.pool[(long)b * pm + s.op_i1[o]], a.anchors + (long)b * am, s.op_i0[o],
                      s.op_i0[o], tid);
  }
  book_take_pixels(l, s.k, b, tid);   // every in-state feature, those just admitted included
  plife_store(a, s, b, tid);
}

__global__ __launch_bounds__(256) void pool_life_end_kernel(PoolLifeArgs a) {
  __shared__ PoolLifeLds s;
  const LifeArgs& l = a.life;
  const int b = blockIdx.x, tid = threadIdx.x, F = l.F, G = l.lay.n_groups, pm = a.pool_max, am = a.anchor_max;
  const int k0 = life_track_begin(l, b), n = life_track_count(l, b);
  plife_load(a, s, b, n, tid);
  __syncthreads();
  if (tid == 0) {
    // gate-rejected features leave (src/update.cpp:105-113); their tracks are new tracks again
    book_drop_where(s.k, F, [&](int j) { return !l.mask[(long)b * l.mask_ld + j]; });
    plife_discard_groups(s, G, am);
    s.n_new = 0; s.a_new = -1; s.n_take = 0; s.n_expired = 0;
    xivo_pool_life_stats& st = a.stats[b];
    st.rejected += s.k.n_rm_feat;
    st.not_spd += (l.status && l.status[b]) ? 1 : 0;
  }
  __syncthreads();
  plife_apply_removals(a, s, b, tid);
  // new tracks: in neither the state nor the pool, the first occurrence of their id
  for (int k = tid; k < n; k += 256) s.fresh[k] = plife_is_unheld(s.k.fid, F, s.eid, pm, s.k.ids[k]) ? 1 : 0;
  __syncthreads();
  for (int k = tid; k < n; k += 256)   // (an earlier occurrence is unheld exactly when this one is: same id)
    if (s.fresh[k] && !plife_first_occurrence(s.k.ids, k)) s.fresh[k] = 2;
  __syncthreads();
  for (int k = tid; k < n; k += 256) s.fresh[k] = s.fresh[k] == 1 ? 1 : 0;
  __syncthreads();
  // their order by rank counting; only the first pool_max can find an entry
  for (int k = tid; k < n; k += 256) {
    if (!s.fresh[k]) continue;
    atomicAdd(&s.n_new, 1);
    const int r = life_rank(s.k.ids, s.fresh, n, k);
    if (r < pm) s.pick[r] = k;
  }
  __syncthreads();
  if (tid == 0 && s.n_new > 0) {
    const int an = plife_free_anchor(s.aused, am);
    const int n_free = plife_free_entries(s.eid, pm, s.efree);
    xivo_pool_life_stats& st = a.stats[b];
    st.pool_dropped += plife_surplus(s.n_new, n_free, an);
    if (an >= 0) {
      plife_create_anchor(s.aused, s.alife, s.alink, an);
      const int n_take = n_free < s.n_new ? n_free : s.n_new;
      for (int q = 0; q < n_take; ++q) plife_take_entry(s.eid, s.eanc, s.eborn, s.efree[q], s.k.ids[s.pick[q]], an, a.frame);
      s.a_new = an; s.n_take = n_take;
      st.anchors_created += 1; st.pool_added += n_take;
    }
  }
  __syncthreads();
  if (s.a_new >= 0) {   // (uniform over the workgroup)
    // Group::Create(X_.Rsb, X_.Tsb) from the updated pose, then Feature::Initialize of every new entry
    if (tid == 0) pool_create_anchor(a.anchors[(long)b * am + s.a_new], l.poses[b]);
    const xivo_cam cam = filter_cam(a.cam, a.calib, a.cam_dim, b);
    const double z0 = a.init_z ? a.init_z[b] : a.initial_z;
    for (int q = tid; q < s.n_take; q += 256)
      pool_init_entry(a.pool[(long)b * pm + s.efree[q]], cam, l.meas + 3 * (long)(k0 + s.pick[q]), z0, a.std_xyz, s.a_new,
                      l.invdepth);
  }
  // EnforceMaxGroupLifetime (:282-304)
  for (int t = tid; t < am; t += 256)
    if (plife_expire_anchor(s.aused, s.alife, s.alink, t, a.max_group_lifetime, s.eid, s.eanc, pm)) atomicAdd(&s.n_expired, 1);
  __syncthreads();
  if (tid == 0) a.stats[b].anchors_freed += s.n_expired;
  plife_store(a, s, b, tid);
}

}  // namespace

int launch_pool_life_begin(const PoolLifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(pool_life_begin_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_pool_life_admit(const PoolLifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(pool_life_admit_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_pool_life_end(const PoolLifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(pool_life_end_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace xivo_hip
