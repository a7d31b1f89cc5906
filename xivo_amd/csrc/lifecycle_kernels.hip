// The per-frame feature life cycle on the device (gfx950), "immediate" mode: what SequenceRunner.frame (xivo_amd/sequence.py)
// and BatchEstimator::VisualMeasPointCloud (xivo_amd/host/batch_estimator.cpp) decide per filter on the host and send down as
// xivo_edit_op lists. One workgroup of 256 threads per filter, the filter's book and the frame's track ids in LDS.
//
//  life_begin_kernel   before the update: association of tracks and slots, new pixels, tracker-dropped features leave
//                      (ProcessTracks, src/manager.cpp:152-169; RemoveFeatureFromState, src/estimator.cpp:762-783), groups left
//                      empty leave with them (RemoveGroupFromState, src/estimator.cpp:745-759)
//  life_end_kernel     after AbsorbError: gate-rejected features leave (src/update.cpp:105-113), empty groups are discarded,
//                      candidates are ordered and the first enter with a new group (SelectAndAddNewFeatures,
//                      src/manager.cpp:332-450; AddGroupToState, src/estimator.cpp:801-816; AddFeatureToState :820-846 +
//                      Feature::Initialize, src/feature.cpp:144-150, FillCovarianceBlock :753-760)
// (paths relative to the reference tree). The decisions are the functions of lifecycle_device.h; the P edits are those of
// edit_batch_kernel (edit_device.h) in the order the host's op lists have, so P and the scene come out bit for bit as from the
// op lists - up to log z, where libm and the device library may differ in the last place. Nothing crosses workgroups: no
// atomics on global memory, the counters and the book belong to the filter's own workgroup (LDS atomics only).
// The frame's tracks are read in one of two forms (LifeArgs, ekf_kernels.h): packed behind offsets as the host uploads them, or
// one row per filter with a count as pcw_tracks_kernel (pcw_kernels.hip) leaves them; life_track_begin / life_track_count
// (lifecycle_tracks_device.h) are the only place that tells them apart.
#include "edit_device.h"
#include "ekf_kernels.h"
#include "lifecycle_device.h"
#include "lifecycle_tracks_device.h"

namespace xivo_hip {

namespace {

constexpr int kTracks = XIVO_LIFE_MAX_TRACKS, kSlots = XIVO_LIFE_MAX_SLOTS;

// the LDS plan of both kernels: 16 KiB of ids, 8 KiB of per-track flags, 2 KiB + 7 x 1 KiB per-slot tables = 33 KiB
struct LifeLds {
  long long ids[kTracks];      // the filter's track ids
  int cand[kTracks];           // life_end: the track is a candidate
  long long fid[kSlots];       // book: track id by feature slot
  int fref[kSlots];            // reference group by feature slot (the resident ref_sind)
  int slot_track[kSlots];      // slot -> track of the frame that feeds it (-1: none)
  int gref[kSlots];            // book: references by group slot
  int rm_feat[kSlots], rm_group[kSlots], free_slots[kSlots], pick[kSlots];
  int n_rm_feat, n_rm_group, g_new, n_free, open, n_cand;
};

__device__ __forceinline__ void life_load(const LifeArgs& a, LifeLds& s, int b, int n, int tid) {
  const int F = a.F, G = a.lay.n_groups;
  const long long* book_id = a.feat_id + (long)b * a.slot_ld;
  const xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  for (int j = tid; j < F; j += 256) {
    const long long id = book_id[j];
    const int ref = feats[j].ref_sind;
    s.fid[j] = id;
    s.fref[j] = (id >= 0 && ref >= 0 && ref < G) ? ref : -1;
    s.slot_track[j] = -1;
  }
  for (int g = tid; g < G; g += 256) s.gref[g] = a.group_refs[(long)b * G + g];
  const int k0 = life_track_begin(a, b);
  for (int k = tid; k < n; k += 256) s.ids[k] = a.ids[k0 + k];
}

__device__ __forceinline__ void life_store(const LifeArgs& a, const LifeLds& s, int b, int tid) {
  const int F = a.F, G = a.lay.n_groups;
  for (int j = tid; j < F; j += 256) a.feat_id[(long)b * a.slot_ld + j] = s.fid[j];
  for (int g = tid; g < G; g += 256) a.group_refs[(long)b * G + g] = s.gref[g];
}

// the op list's XIVO_EDIT_REMOVE_FEATURE of every slot in rm_feat, then XIVO_EDIT_REMOVE_GROUP of every slot in rm_group
__device__ __forceinline__ void life_apply_removals(const LifeArgs& a, const LifeLds& s, double* P, xivo_feat_in* feats, int tid) {
  for (int q = 0; q < s.n_rm_feat; ++q) {
    const int j = s.rm_feat[q];
    const int sind = feats[j].sind;
    __syncthreads();
    if (sind >= 0) {
      if (sind < a.lay.n_features) edit_zero_rc(P, a.ldp, a.Np, a.lay.feature_begin + 3 * sind, 3, tid);
      if (tid == 0) feats[j].sind = -1;
      __syncthreads();
    }
  }
  for (int q = 0; q < s.n_rm_group; ++q) edit_zero_rc(P, a.ldp, a.Np, a.lay.group_begin + 6 * s.rm_group[q], 6, tid);
}

__global__ __launch_bounds__(256) void life_begin_kernel(LifeArgs a) {
  __shared__ LifeLds s;
  const int b = blockIdx.x, tid = threadIdx.x, F = a.F, G = a.lay.n_groups;
  double* P = a.P + (long)b * a.strideP;
  xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  const int k0 = life_track_begin(a, b), n = life_track_count(a, b);
  life_load(a, s, b, n, tid);
  __syncthreads();
  // association: one thread per track scans the in-state ids; of a repeated id the last occurrence feeds the slot
  for (int k = tid; k < n; k += 256) {
    const long long id = s.ids[k];
    for (int j = 0; j < F; ++j)
      if (life_slot_holds(s.fid, j, id)) atomicMax(&s.slot_track[j], k);
  }
  __syncthreads();
  // tracked features take their new pixel (xivo_hip_set_pixels: a NaN pair leaves the entry as it is)
  for (int j = tid; j < F; j += 256) {
    if (s.slot_track[j] < 0) continue;   // (only slot_track: thread 0 below writes fid of the slots that have none)
    const double* m = a.meas + 3 * (long)(k0 + s.slot_track[j]);
    const double u = m[0], v = m[1];
    if (u != u || v != v) continue;
    feats[j].xp[0] = u; feats[j].xp[1] = v;
  }
  if (tid == 0) {   // ProcessTracks (src/manager.cpp:152-169): a few dozen slots, serial
    int n_rm = 0, n_in = 0;
    for (int j = 0; j < F; ++j) {
      if (s.fid[j] < 0) continue;
      if (s.slot_track[j] < 0) { s.rm_feat[n_rm++] = j; life_drop_feature(s.fid, s.fref, s.gref, j); }
      else ++n_in;
    }
    s.n_rm_feat = n_rm;
    s.n_rm_group = life_discard_empty_groups(s.gref, G, s.rm_group);
    xivo_life_stats& st = a.stats[b];
    st.dropped += n_rm;
    st.updates += n_in > 0 ? 1 : 0;
  }
  __syncthreads();
  life_apply_removals(a, s, P, feats, tid);
  life_store(a, s, b, tid);
}

// Feature::Initialize (src/feature.cpp:144-150) of a point-cloud track: no product is followed by a sum here, and contraction
// stays off so that none appears
__device__ __forceinline__ void life_init_feature(const LifeArgs& a, xivo_feat_in& f, const double* m, int slot, int g) {
#pragma clang fp contract(off)
  const double u = m[0], v = m[1], z = m[2];
  f.x[0] = (u - a.cx) / a.fx;
  f.x[1] = (v - a.cy) / a.fy;
  f.x[2] = a.invdepth ? 1.0 / z : log(z);
  f.xp[0] = u; f.xp[1] = v;
  f.sind = slot; f.ref_sind = g;
}

__global__ __launch_bounds__(256) void life_end_kernel(LifeArgs a) {
  __shared__ LifeLds s;
  const int b = blockIdx.x, tid = threadIdx.x, F = a.F, G = a.lay.n_groups;
  double* P = a.P + (long)b * a.strideP;
  xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  xivo_group_in* groups = a.groups + (long)b * G;
  const int k0 = life_track_begin(a, b), n = life_track_count(a, b);
  life_load(a, s, b, n, tid);
  __syncthreads();
  if (tid == 0) {
    // gate-rejected features leave (src/update.cpp:105-113); their tracks are candidates again
    int n_rm = 0, n_in = 0;
    for (int j = 0; j < F; ++j) {
      if (s.fid[j] < 0) continue;
      if (!a.mask[(long)b * a.mask_ld + j]) { s.rm_feat[n_rm++] = j; life_drop_feature(s.fid, s.fref, s.gref, j); }
      else ++n_in;
    }
    s.n_rm_feat = n_rm;
    s.n_rm_group = life_discard_empty_groups(s.gref, G, s.rm_group);
    s.g_new = life_free_group(s.gref, G);
    s.n_free = life_free_slots(s.fid, F, s.free_slots);
    s.open = life_admission_open(s.g_new, s.n_free, n_in, a.min_new_features) ? 1 : 0;
    s.n_cand = 0;
    xivo_life_stats& st = a.stats[b];
    st.rejected += n_rm;
    st.not_spd += (a.status && a.status[b]) ? 1 : 0;
  }
  __syncthreads();
  life_apply_removals(a, s, P, feats, tid);
  if (s.open) {   // (uniform over the workgroup)
    for (int k = tid; k < n; k += 256)
      s.cand[k] = life_is_candidate(life_in_state(s.fid, F, s.ids[k]), a.meas[3 * (long)(k0 + k) + 2], a.min_depth, a.max_depth) ? 1 : 0;
    __syncthreads();
    // candidate order by rank counting; only the first n_free are needed
    for (int k = tid; k < n; k += 256) {
      if (!s.cand[k]) continue;
      atomicAdd(&s.n_cand, 1);
      const int r = life_rank(s.ids, s.cand, n, k);
      if (r < s.n_free) s.pick[r] = k;
    }
    __syncthreads();
    if (s.n_cand > 0) {
      const int g = s.g_new, n_new = min(s.n_free, s.n_cand);
      const xivo_pose_in& X = a.poses[b];
      // XIVO_EDIT_ADD_GROUP: Estimator::AddGroupToState (src/estimator.cpp:801-816) from the current pose
      if (tid < 9) groups[g].Rsb[tid] = X.Rsb[tid];
      else if (tid < 12) groups[g].Tsb[tid - 9] = X.Tsb[tid - 9];
      const int goff = a.lay.group_begin + 6 * g;
      edit_copy_rc(P, a.ldp, a.Np, goff, 0, 3, tid);       // Index::Wsb
      edit_copy_rc(P, a.ldp, a.Np, goff + 3, 3, 3, tid);   // Index::Tsb
      // XIVO_EDIT_ADD_FEATURE of every new feature: AddFeatureToState (:820-846) + FillCovarianceBlock (src/feature.cpp:753-760)
      for (int q = 0; q < n_new; ++q) {
        const int j = s.free_slots[q], k = s.pick[q];
        if (tid == 0) life_init_feature(a, feats[j], a.meas + 3 * (long)(k0 + k), j, g);
        const int foff = a.lay.feature_begin + 3 * j;
        edit_zero_rc(P, a.ldp, a.Np, foff, 3, tid);
        if (tid < 3) P[(foff + tid) + (long)(foff + tid) * a.ldp] = a.var_xyz[tid];
        __syncthreads();
      }
      if (tid == 0) {
        for (int q = 0; q < n_new; ++q) { s.fid[s.free_slots[q]] = s.ids[s.pick[q]]; }
        s.gref[g] = n_new;
        xivo_life_stats& st = a.stats[b];
        st.admitted += n_new;
        st.groups_added += 1;
      }
      __syncthreads();
    }
  }
  life_store(a, s, b, tid);
}

}  // namespace

int launch_life_begin(const LifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(life_begin_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
int launch_life_end(const LifeArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(life_end_kernel, dim3(batch), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace xivo_hip
