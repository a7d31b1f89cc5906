// The per-frame feature life cycle on the device (gfx950), "immediate" mode: what SequenceRunner.frame (xivo_amd/sequence.py)
// and BatchEstimator::VisualMeasPointCloud (xivo_amd/host/batch_estimator.cpp) decide per filter on the host and send down as
// xivo_edit_op lists. One workgroup of 256 threads per filter, the filter's book and the frame's track ids in LDS (InstateBook,
// instate_book_device.h: the in-state half this file shares with pool_lifecycle_kernels.hip).
//
//  life_begin_kernel   before the update: association of tracks and slots, new pixels, tracker-dropped features leave
//                      (ProcessTracks, src/manager.cpp:152-169; RemoveFeatureFromState, src/estimator.cpp:762-783), groups left
//                      empty leave with them (RemoveGroupFromState, src/estimator.cpp:745-759)
//  life_end_kernel     after AbsorbError: gate-rejected features leave (src/update.cpp:105-113), empty groups are discarded,
//                      candidates are ordered and the first enter with a new group (SelectAndAddNewFeatures,
//                      src/manager.cpp:332-450; AddGroupToState, src/estimator.cpp:801-816; AddFeatureToState :820-846 +
//                      Feature::Initialize, src/feature.cpp:144-150, FillCovarianceBlock :753-760)
// (paths relative to the reference tree). The decisions are the functions of lifecycle_device.h; the P edits are the functions
// of edit_device.h that edit_batch_kernel's cases call, in the order the host's op lists have, so P and the scene come out bit for bit as from the
// op lists - up to log z, where libm and the device library may differ in the last place. Nothing crosses workgroups: no
// atomics on global memory, the counters and the book belong to the filter's own workgroup (LDS atomics only).
// The frame's tracks are read in one of two forms (LifeArgs, ekf_kernels.h): packed behind offsets as the host uploads them, or
// one row per filter with a count as pcw_tracks_kernel (pcw_kernels.hip) leaves them; life_track_begin / life_track_count
// (lifecycle_tracks_device.h) are the only place that tells them apart.
// Loop closure inside the life cycle (xivo_hip_lcmap_life_config: LifeArgs::feat_key is then not null; the rules are
// lcmap_life_device.h's): the begin kernel decides and does not edit - the leaving slots become the frame's add records, with
// the key the book held, and the removals wait in LifeArgs::lc_rm until the map has read the leaving features from the state as
// it was; life_lc_apply_kernel then makes them, with book_apply_removals as the begin kernel does otherwise. The end kernel
// hands a new feature its track's key and frees the key of a rejected one (no record: DestroyFeatures). feat_key is read and
// written in global memory by thread 0 alone: the LDS plan stays what it was.
#include "ekf_kernels.h"
#include "instate_book_device.h"
#include "lcmap_life_device.h"

namespace xivo_hip {

namespace {

constexpr int kTracks = XIVO_LIFE_MAX_TRACKS, kSlots = XIVO_LIFE_MAX_SLOTS;

// the LDS plan of both kernels: the in-state book (16 KiB of ids, 2 KiB + 5 x 1 KiB per-slot tables), 8 KiB of per-track flags,
// 2 x 1 KiB per-slot tables = 33 KiB
struct LifeLds {
  InstateBook k;
  int cand[kTracks];           // life_end: the track is a candidate
  int free_slots[kSlots], pick[kSlots];
  int g_new, n_free, open, n_cand;
};

__global__ __launch_bounds__(256) void life_begin_kernel(LifeArgs a) {
  __shared__ LifeLds s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = life_track_count(a, b);
  book_load(a, s.k, b, tid);
  book_load_ids(a, s.k, b, n, tid);
  __syncthreads();
  book_associate(s.k, a.F, n, tid);
  __syncthreads();
  book_take_pixels(a, s.k, b, tid);
  if (a.feat_key) {   // (uniform; before thread 0 frees the slots that leave: fid of a tracked slot is not written)
    const int k0 = life_track_begin(a, b);
    for (int j = tid; j < a.F; j += 256) {
      const int k = s.k.slot_track[j];
      const double u = k >= 0 ? a.meas[3 * (long)(k0 + k)] : 0.0;
      a.lc_tracked[(long)b * a.slot_ld + j] = k >= 0 && lclife_tracked(s.k.fid[j], k, u != u) ? 1 : 0;
    }
  }
  if (tid == 0) {   // ProcessTracks (src/manager.cpp:152-169)
    const int n_in = book_drop_where(s.k, a.F, [&](int j) { return lclife_leaves(s.k.fid[j], s.k.slot_track[j]) != 0; });
    book_discard_empty_groups(s.k, a.lay.n_groups);
    xivo_life_stats& st = a.stats[b];
    st.dropped += s.k.n_rm_feat;
    st.updates += n_in > 0 ? 1 : 0;
  }
  __syncthreads();
  if (a.feat_key) {   // (uniform) decide only: the records and the removals go to the add call
    if (tid == 0) {
      long long* key = a.feat_key + (long)b * a.slot_ld;
      int* rm = a.lc_rm + (long)b * (2 + a.slot_ld + a.lay.n_groups);
      for (int q = 0; q < s.k.n_rm_feat; ++q) {   // (rm_feat is in ascending slot order)
        const int j = s.k.rm_feat[q];
        xivo_lcmap_add_rec& r = a.lc_recs[lclife_list_pos(b, a.slot_ld, q)];
        r.b = b; r.feat = j; r.key = key[j];
        key[j] = lclife_no_key();
        rm[2 + q] = j;
      }
      for (int q = 0; q < s.k.n_rm_group; ++q) rm[2 + a.slot_ld + q] = s.k.rm_group[q];
      rm[0] = s.k.n_rm_feat; rm[1] = s.k.n_rm_group;
      a.lc_n_recs[b] = s.k.n_rm_feat;
    }
    book_store(a, s.k, b, tid);
    return;
  }
  book_apply_removals(a, s.k, b, nullptr, 0, tid);
  book_store(a, s.k, b, tid);
}

// the removals a deciding begin kernel left in lc_rm, behind the map's add kernel: the begin kernel's own last step
__global__ __launch_bounds__(256) void life_lc_apply_kernel(LifeArgs a) {
  __shared__ InstateBook s;
  const int b = blockIdx.x, tid = threadIdx.x, G = a.lay.n_groups;
  const int* rm = a.lc_rm + (long)b * (2 + a.slot_ld + G);
  const int n_feat = min(max(rm[0], 0), min(a.F, kSlots)), n_group = min(max(rm[1], 0), min(G, kSlots));
  for (int q = tid; q < n_feat; q += 256) s.rm_feat[q] = rm[2 + q];
  for (int q = tid; q < n_group; q += 256) s.rm_group[q] = rm[2 + a.slot_ld + q];
  if (tid == 0) { s.n_rm_feat = n_feat; s.n_rm_group = n_group; }
  __syncthreads();
  book_apply_removals(a, s, b, nullptr, 0, tid);
}

// Feature::Initialize (src/feature.cpp:144-150) of a point-cloud track: no product is followed by a sum here, and contraction
// stays off so that none appears
__device__ __forceinline__ void life_init_feature(const LifeArgs& a, const double* m, double* x) {
#pragma clang fp contract(off)
  x[0] = (m[0] - a.cx) / a.fx;
  x[1] = (m[1] - a.cy) / a.fy;
  x[2] = a.invdepth ? 1.0 / m[2] : log(m[2]);
}

__global__ __launch_bounds__(256) void life_end_kernel(LifeArgs a) {
  __shared__ LifeLds s;
  const int b = blockIdx.x, tid = threadIdx.x, F = a.F, G = a.lay.n_groups;
  double* P = a.P + (long)b * a.strideP;
  xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  const int k0 = life_track_begin(a, b), n = life_track_count(a, b);
  book_load(a, s.k, b, tid);
  book_load_ids(a, s.k, b, n, tid);
  __syncthreads();
  if (tid == 0) {
    // gate-rejected features leave (src/update.cpp:105-113); their tracks are candidates again
    const int n_in = book_drop_where(s.k, F, [&](int j) { return !a.mask[(long)b * a.mask_ld + j]; });
    book_discard_empty_groups(s.k, G);
    if (a.feat_key)   // a rejected feature's key goes with it and makes no record (DestroyFeatures)
      for (int q = 0; q < s.k.n_rm_feat; ++q) a.feat_key[(long)b * a.slot_ld + s.k.rm_feat[q]] = lclife_no_key();
    s.g_new = life_free_group(s.k.gref, G);
    s.n_free = life_free_slots(s.k.fid, F, s.free_slots);
    s.open = life_admission_open(s.g_new, s.n_free, n_in, a.min_new_features) ? 1 : 0;
    s.n_cand = 0;
    xivo_life_stats& st = a.stats[b];
    st.rejected += s.k.n_rm_feat;
    st.not_spd += (a.status && a.status[b]) ? 1 : 0;
  }
  __syncthreads();
  book_apply_removals(a, s.k, b, nullptr, 0, tid);
  if (s.open) {   // (uniform over the workgroup)
    for (int k = tid; k < n; k += 256)
      s.cand[k] = life_is_candidate(life_in_state(s.k.fid, F, s.k.ids[k]), a.meas[3 * (long)(k0 + k) + 2], a.min_depth, a.max_depth) ? 1 : 0;
    __syncthreads();
    // candidate order by rank counting; only the first n_free are needed
    for (int k = tid; k < n; k += 256) {
      if (!s.cand[k]) continue;
      atomicAdd(&s.n_cand, 1);
      const int r = life_rank(s.k.ids, s.cand, n, k);
      if (r < s.n_free) s.pick[r] = k;
    }
    __syncthreads();
    if (s.n_cand > 0) {
      const int g = s.g_new, n_new = min(s.n_free, s.n_cand);
      // XIVO_EDIT_ADD_GROUP from the current pose, then XIVO_EDIT_ADD_FEATURE of every new feature with P_ = diag(var_xyz)
      edit_add_group(P, a.ldp, a.Np, a.lay, a.groups + (long)b * G, a.poses[b].Rsb, a.poses[b].Tsb, g, tid);
      for (int q = 0; q < n_new; ++q) {
        const int j = s.free_slots[q];
        const double* m = a.meas + 3 * (long)(k0 + s.pick[q]);
        double x[3] = {0.0, 0.0, 0.0};
        if (tid == 0) life_init_feature(a, m, x);
        edit_add_feature(P, a.ldp, a.Np, a.lay, feats[j], x, m, j, g, tid % 4 == 0 && tid < 9 ? (a.tune_var ? a.tune_var[3 * (long)b + tid / 4] : a.var_xyz[tid / 4]) : 0.0, tid);
      }
      if (tid == 0) {
        for (int q = 0; q < n_new; ++q) { s.k.fid[s.free_slots[q]] = s.k.ids[s.pick[q]]; }
        if (a.feat_key)   // the new feature takes its track's key
          for (int q = 0; q < n_new; ++q) a.feat_key[(long)b * a.slot_ld + s.free_slots[q]] = a.keys[k0 + s.pick[q]];
        s.k.gref[g] = n_new;
        xivo_life_stats& st = a.stats[b];
        st.admitted += n_new;
        st.groups_added += 1;
      }
      __syncthreads();
    }
  }
  book_store(a, s.k, b, tid);
}

}  // namespace

int launch_life_begin(const LifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(life_begin_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_life_lc_apply(const LifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(life_lc_apply_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_life_end(const LifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(life_end_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace xivo_hip
