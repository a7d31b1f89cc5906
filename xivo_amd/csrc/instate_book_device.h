// The in-state half of a device life cycle's workgroup: one filter's slot book and the frame's track ids in LDS, and the steps
// both life cycles take on them - load, association of tracks and slots, "these features leave", the P edits that go with it,
// the tracked features' new pixels, store. Device-only plumbing of lifecycle_kernels.hip and pool_lifecycle_kernels.hip (which
// embed the struct in their LDS plans); the decisions are lifecycle_device.h's, the P edits edit_device.h's, the tracks are read
// through lifecycle_tracks_device.h. All 256 threads make every call but book_drop_where / book_discard_empty_groups, which
// are thread 0's.
#pragma once
#include "edit_device.h"
#include "ekf_kernels.h"
#include "lifecycle_device.h"
#include "lifecycle_tracks_device.h"

namespace xivo_hip {

// 16 KiB of ids, 2 KiB + 5 x 1 KiB per-slot tables
struct InstateBook {
  long long ids[XIVO_LIFE_MAX_TRACKS];   // the filter's track ids
  long long fid[XIVO_LIFE_MAX_SLOTS];    // book: track id by feature slot
  int fref[XIVO_LIFE_MAX_SLOTS];         // reference group by feature slot (the resident ref_sind)
  int slot_track[XIVO_LIFE_MAX_SLOTS];   // slot -> track of the frame that feeds it (-1: none)
  int gref[XIVO_LIFE_MAX_SLOTS];         // book: references by group slot
  int rm_feat[XIVO_LIFE_MAX_SLOTS], rm_group[XIVO_LIFE_MAX_SLOTS];   // who leaves, in op-list order
  int n_rm_feat, n_rm_group;
};

// the book of filter b
__device__ __forceinline__ void book_load(const LifeArgs& a, InstateBook& s, int b, int tid) {
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
}
// the ids of its n tracks (a kernel that does not look at them leaves this out)
__device__ __forceinline__ void book_load_ids(const LifeArgs& a, InstateBook& s, int b, int n, int tid) {
  const int k0 = life_track_begin(a, b);
  for (int k = tid; k < n; k += 256) s.ids[k] = a.ids[k0 + k];
}

__device__ __forceinline__ void book_store(const LifeArgs& a, const InstateBook& s, int b, int tid) {
  const int F = a.F, G = a.lay.n_groups;
  for (int j = tid; j < F; j += 256) a.feat_id[(long)b * a.slot_ld + j] = s.fid[j];
  for (int g = tid; g < G; g += 256) a.group_refs[(long)b * G + g] = s.gref[g];
}

// association, the slots' side: one thread per track scans the in-state ids; of a repeated id the last occurrence feeds the slot
__device__ __forceinline__ void book_associate(InstateBook& s, int F, int n, int tid) {
  for (int k = tid; k < n; k += 256) {
    const long long id = s.ids[k];
    for (int j = 0; j < F; ++j)
      if (life_slot_holds(s.fid, j, id)) atomicMax(&s.slot_track[j], k);
  }
}

// thread 0: every held slot j with leaves(j) leaves the book and goes to rm_feat (a few dozen slots, serial); returns how many stay
template <class Pred>
__device__ __forceinline__ int book_drop_where(InstateBook& s, int F, Pred leaves) {
  int n_rm = 0, n_in = 0;
  for (int j = 0; j < F; ++j) {
    if (s.fid[j] < 0) continue;
    if (leaves(j)) { s.rm_feat[n_rm++] = j; life_drop_feature(s.fid, s.fref, s.gref, j); }
    else ++n_in;
  }
  s.n_rm_feat = n_rm;
  return n_in;
}
// thread 0: the groups left empty go to rm_group
__device__ __forceinline__ void book_discard_empty_groups(InstateBook& s, int G) {
  s.n_rm_group = life_discard_empty_groups(s.gref, G, s.rm_group);
}

// the op list's XIVO_EDIT_REMOVE_FEATURE of every slot in rm_feat, then XIVO_EDIT_REMOVE_GROUP of every slot in rm_group
// (`anchors`: the filter's own, anchor_max = 0 and null without a pool)
__device__ __forceinline__ void book_apply_removals(const LifeArgs& a, const InstateBook& s, int b, PoolAnchor* anchors, int anchor_max,
                                                    int tid) {
  double* P = a.P + (long)b * a.strideP;
  xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  for (int q = 0; q < s.n_rm_feat; ++q) edit_remove_feature(P, a.ldp, a.Np, a.lay, feats, s.rm_feat[q], tid);
  for (int q = 0; q < s.n_rm_group; ++q)
    edit_remove_group(P, a.ldp, a.Np, a.lay, a.groups + (long)b * a.lay.n_groups, anchors, anchor_max, s.rm_group[q], tid);
}

// tracked features take their new pixel (xivo_hip_set_pixels: a NaN pair leaves the entry as it is). slot_track is looked at
// first: thread 0 may be dropping the slots that have none (book_drop_where) at the same time, and writes fid of those alone
__device__ __forceinline__ void book_take_pixels(const LifeArgs& a, const InstateBook& s, int b, int tid) {
  xivo_feat_in* feats = a.feats + (long)b * a.Fmax;
  const int k0 = life_track_begin(a, b);
  for (int j = tid; j < a.F; j += 256) {
    if (s.slot_track[j] < 0 || s.fid[j] < 0) continue;
    const double* m = a.meas + 3 * (long)(k0 + s.slot_track[j]);
    const double u = m[0], v = m[1];
    if (u != u || v != v) continue;
    feats[j].xp[0] = u; feats[j].xp[1] = v;
  }
}

}  // namespace xivo_hip
