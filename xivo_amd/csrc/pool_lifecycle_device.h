// The decisions of the per-frame feature life cycle in the "subfilter" mode (the reference's own: a new track lives in the
// out-of-state pool first) as plain functions over ONE filter's books and the frame's track arrays. Integer logic and
// comparisons only - no arithmetic of the filter. Host and device: the kernels of pool_lifecycle_kernels.hip call these
// functions, and a host compiler takes the header with lifecycle_device.h alone (tests/pool_lifecycle_driver.cpp replays
// scripted frames through them without a GPU).
//
// Every rule restates SequenceRunner._frame_subfilter (xivo_amd/sequence.py; cited below by its comment markers, which do not
// move when the file grows), which follows Estimator::UpdateStep of the
// reference (src/manager.cpp:18-130); anchors play the role of the reference's groups that are not in the state.
//
// The in-state book (feat_id, feat_ref, group_refs) is lifecycle_device.h's. The pool book of a filter:
//   ent_id[pool_max]     track id held by pool entry e, -1: free
//   ent_born[pool_max]   the frame counter at which the entry was created
//   anc_used[anchor_max] the anchor exists
//   anc_life[anchor_max] Group::lifetime: frames since the anchor was created
// An entry's anchor (ent_anchor below) is the resident pool[e].ref_sind and an anchor's link (anc_link) the resident
// anchors[a].slot: the kernels keep working copies of both, nothing resident duplicates them.
#pragma once

#include "lifecycle_device.h"

// anchors per filter the kernels' LDS plan holds (pool_lifecycle_kernels.hip); a larger anchor table is refused. (Also in
// include/xivo_hip.h, which this header must not need.)
#ifndef XIVO_POOL_LIFE_MAX_ANCHORS
#define XIVO_POOL_LIFE_MAX_ANCHORS 256
#endif

namespace xivo_hip {

// what the walk over the step's candidate order decides, in op-list order (XIVO_EDIT_ADD_GROUP_ANCHOR / XIVO_EDIT_ADMIT_POOL)
enum { PLIFE_OP_ADD_GROUP_ANCHOR = 0, PLIFE_OP_ADMIT_POOL = 1 };

// ---- anchor lifetime: Group::IncrementLifetime (src/manager.cpp:36-41; _frame_subfilter at "Group::IncrementLifetime")
// a used anchor's life is incremented, an unused anchor's life is 0
XIVO_LIFE_HD int plife_anchor_tick(int used, int life) { return used ? life + 1 : 0; }

// ---- association of tracks and pool entries (_frame_subfilter's position table `pos`)
// the rules of the feature slots hold for the entries: a free entry holds -1 and matches nothing, of a repeated id the last
// occurrence supplies the pixel. plife_track_of_entry is the serial form (host code); the begin kernel reaches the same k
// with one thread per track and an LDS maximum per entry over plife_entry_holds.
XIVO_LIFE_HD bool plife_entry_holds(const long long* ent_id, int e, long long id) { return life_slot_holds(ent_id, e, id); }
XIVO_LIFE_HD bool plife_in_pool(const long long* ent_id, int pool_max, long long id) { return life_in_state(ent_id, pool_max, id); }
XIVO_LIFE_HD int plife_track_of_entry(const long long* ent_id, int e, const long long* ids, int n) {
  return life_track_of_slot(ent_id, e, ids, n);
}

// ---- leaving the pool: _PoolBook.free_entry (sequence.py)
XIVO_LIFE_HD void plife_free_entry(long long* ent_id, int* ent_anchor, int e) { ent_id[e] = -1; ent_anchor[e] = -1; }

// ---- a group slot leaves the state: _PoolBook.unlink_slot (sequence.py; XIVO_EDIT_REMOVE_GROUP freezes the anchor at
// the group's pose on the device). true when anchor a was linked to slot g and is unlinked now.
XIVO_LIFE_HD bool plife_unlink(int* anc_link, int a, int g) {
  if (anc_link[a] != g) return false;
  anc_link[a] = -1;
  return true;
}

// ---- ProcessTracks, the pool's side (src/manager.cpp:171-250; _frame_subfilter at "--- ProcessTracks", the loop over ent_id):
// an entry without a track is freed, every other entry's pixel goes to the step. true: entry e is free (before or now) and the
// step gets NaN for it.
XIVO_LIFE_HD bool plife_entry_leaves(long long* ent_id, int* ent_anchor, int e, int track) {
  if (ent_id[e] < 0) return true;
  if (track >= 0) return false;
  plife_free_entry(ent_id, ent_anchor, e);
  return true;
}

// ---- after the step: an entry the step did not leave live is freed - sub-filter outlier (src/manager.cpp:236-240;
// _frame_subfilter at "sub-filter outlier"). true when a held entry was freed.
XIVO_LIFE_HD bool plife_free_if_dead(long long* ent_id, int* ent_anchor, int e, int live) {
  if (ent_id[e] < 0 || live) return false;
  plife_free_entry(ent_id, ent_anchor, e);
  return true;
}

// ---- SelectAndAddNewFeatures / ZeroGaugeXYAddFeatures (src/manager.cpp:332-450; _frame_subfilter at
// "--- SelectAndAddNewFeatures"): the walk over the step's
// order[0..n). Free feature slots and free group slots are taken in ascending order. The walk stops when no feature slot is
// free; an entry whose anchor is unlinked takes the lowest free group slot (ADD_GROUP_ANCHOR); without a free group slot that
// entry is skipped and the walk goes on (src/manager.cpp:437-441) - a later entry whose anchor is linked is still admitted;
// admission is ADMIT_POOL into the lowest free feature slot, after which the entry is freed. slot_track[j] of an admitted slot
// becomes the entry's track. Ops (kind, i0, i1): ADD_GROUP_ANCHOR (g, a), ADMIT_POOL (j, e); at most F + n_groups of them.
// admit_steps accumulates frame - ent_born of every admitted entry. Returns the number of ops; *n_admitted, *n_groups_added.
XIVO_LIFE_HD int plife_walk(const int* order, int n, int frame, long long* feat_id, int* feat_ref, int* group_refs, int F,
                            int n_groups, long long* ent_id, int* ent_anchor, const int* ent_born, const int* ent_track,
                            int pool_max, int* anc_link, int anchor_max, int* slot_track, int* op_kind, int* op_i0, int* op_i1,
                            int* n_admitted, int* n_groups_added, long long* admit_steps) {
  int n_ops = 0, j = 0, g = 0, adm = 0, gadd = 0;
  for (int q = 0; q < n; ++q) {
    while (j < F && feat_id[j] >= 0) ++j;                    // the lowest free feature slot
    if (j >= F) break;
    const int e = order[q];
    if (e < 0 || e >= pool_max || ent_id[e] < 0) continue;   // (the step orders live entries only)
    const int a = ent_anchor[e];
    if (a < 0 || a >= anchor_max) continue;
    if (anc_link[a] < 0) {
      while (g < n_groups && group_refs[g] >= 0) ++g;        // the lowest free group slot
      if (g >= n_groups) continue;                           // its group would need a free slot: the entry waits
      op_kind[n_ops] = PLIFE_OP_ADD_GROUP_ANCHOR; op_i0[n_ops] = g; op_i1[n_ops] = a; ++n_ops;
      anc_link[a] = g; group_refs[g] = 0; ++gadd;
    }
    const int gs = anc_link[a];
    op_kind[n_ops] = PLIFE_OP_ADMIT_POOL; op_i0[n_ops] = j; op_i1[n_ops] = e; ++n_ops;
    feat_id[j] = ent_id[e]; feat_ref[j] = gs; group_refs[gs] += 1;
    slot_track[j] = ent_track[e];
    *admit_steps += frame - ent_born[e];
    plife_free_entry(ent_id, ent_anchor, e);
    ++adm;
  }
  *n_admitted = adm; *n_groups_added = gadd;
  return n_ops;
}

// ---- new tracks: InitializeJustCreatedTracks (src/manager.cpp:121-126, :575-600; _frame_subfilter at "--- Group::Create", the
// list `new`)
// a track is new when its id is in neither the state nor the pool - after the frame's rejections - and no earlier track of the
// frame carries the same id: of a repeated id among the new tracks only the first in (id, position) order takes part, the
// others are ignored and counted nowhere (the host life cycle has no rule for them: it fails). Two steps so that the kernel
// can evaluate the first for all tracks before it scans for the earlier occurrence.
XIVO_LIFE_HD bool plife_is_unheld(const long long* feat_id, int F, const long long* ent_id, int pool_max, long long id) {
  return id >= 0 && !life_in_state(feat_id, F, id) && !plife_in_pool(ent_id, pool_max, id);
}
XIVO_LIFE_HD bool plife_first_occurrence(const long long* ids, int k) {
  for (int q = 0; q < k; ++q)
    if (ids[q] == ids[k]) return false;
  return true;
}
// new tracks are ordered by ascending id, ties by position: life_before / life_rank of lifecycle_device.h

// ---- where new tracks go (_frame_subfilter, afree / efree): the lowest free anchor (-1: none - all new tracks are dropped), the
// free entries in ascending order
XIVO_LIFE_HD int plife_free_anchor(const int* anc_used, int anchor_max) {
  for (int a = 0; a < anchor_max; ++a)
    if (!anc_used[a]) return a;
  return -1;
}
XIVO_LIFE_HD int plife_free_entries(const long long* ent_id, int pool_max, int* free_entries) {
  return life_free_slots(ent_id, pool_max, free_entries);
}
// the anchor is created unlinked with life 0 (Group::Create, src/group.cpp:17-24; _frame_subfilter, `a = afree[0]`)
XIVO_LIFE_HD void plife_create_anchor(int* anc_used, int* anc_life, int* anc_link, int a) {
  anc_used[a] = 1; anc_life[a] = 0; anc_link[a] = -1;
}
// new track of id `id` takes entry e of anchor a in frame `frame` (_frame_subfilter, the loop over zip(efree, new))
XIVO_LIFE_HD void plife_take_entry(long long* ent_id, int* ent_anchor, int* ent_born, int e, long long id, int a, int frame) {
  ent_id[e] = id; ent_anchor[e] = a; ent_born[e] = frame;
}
// how many of n_new new tracks find no entry (n_pool_dropped, _frame_subfilter)
XIVO_LIFE_HD int plife_surplus(int n_new, int n_free_entries, int anchor) {
  return anchor < 0 ? n_new : (n_new > n_free_entries ? n_new - n_free_entries : 0);
}

// ---- EnforceMaxGroupLifetime (src/manager.cpp:282-304; _frame_subfilter at "--- EnforceMaxGroupLifetime"): a used, unlinked
// anchor with life > max_group_lifetime that no live entry references is freed. true when anchor a was freed.
XIVO_LIFE_HD bool plife_expire_anchor(int* anc_used, const int* anc_life, const int* anc_link, int a, int max_group_lifetime,
                                      const long long* ent_id, const int* ent_anchor, int pool_max) {
  if (!anc_used[a] || anc_link[a] >= 0 || !(anc_life[a] > max_group_lifetime)) return false;
  for (int e = 0; e < pool_max; ++e)
    if (ent_id[e] >= 0 && ent_anchor[e] == a) return false;
  anc_used[a] = 0;
  return true;
}

// ---- OOS / MSCKF use of entries that leave the pool (SequenceConfig.use_oos; _frame_subfilter at "--- OOS selection" and
// "--- OOS history"). Two more arrays of the pool book and the observation ring of every entry:
//   anc_born[anchor_max]           the frame counter at which the anchor was created (tells a re-used anchor index apart)
//   hist_cnt[pool_max]             observations appended since the entry was taken (not capped: slot = count % max_obs)
//   hist_anchor / hist_born [pool_max][max_obs]   the observing anchor and its creation frame; the pixels sit beside them
// An observation is appended at the end of a frame that created an anchor, for every live entry that had a track in that frame
// (the reference's graph edge "feature seen from the group created this frame", src/manager.cpp:121-126). A history reference
// does not keep an anchor alive.

// what the walk over the dropped entries decides for one of them
enum { PLIFE_OOS_NONE = 0, PLIFE_OOS_USED = 1, PLIFE_OOS_SHORT = 2, PLIFE_OOS_SURPLUS = 3 };

// a new entry starts with an empty ring (with plife_take_entry)
XIVO_LIFE_HD void plife_hist_reset(int* hist_cnt, int e) { hist_cnt[e] = 0; }
// append (anchor a, created in `frame`) to entry e's ring; returns the ring slot the caller stores the pixel in. The oldest
// observation is overwritten once the ring is full.
XIVO_LIFE_HD int plife_hist_append(int* hist_cnt, int* hist_anchor, int* hist_born, int e, int max_obs, int a, int frame) {
  const int s = hist_cnt[e] % max_obs;
  hist_anchor[e * max_obs + s] = a; hist_born[e * max_obs + s] = frame;
  hist_cnt[e] += 1;
  return s;
}
// observations the ring holds, and the slot of the q-th oldest of them
XIVO_LIFE_HD int plife_hist_len(int cnt, int max_obs) { return cnt < max_obs ? cnt : max_obs; }
XIVO_LIFE_HD int plife_hist_slot(int cnt, int max_obs, int q) { return cnt <= max_obs ? q : (cnt + q) % max_obs; }
// an observation counts when its anchor still exists with the same creation frame and is linked to a group slot now; returns
// that slot, -1: the observation does not count
XIVO_LIFE_HD int plife_obs_group(int a, int born, const int* anc_used, const int* anc_born, const int* anc_link, int anchor_max,
                                 int n_groups) {
  if (a < 0 || a >= anchor_max || !anc_used[a] || anc_born[a] != born) return -1;
  const int g = anc_link[a];
  return g >= 0 && g < n_groups ? g : -1;
}
// the valid observations of entry e, oldest first: slot_out / group_out [max_obs]; returns their number
XIVO_LIFE_HD int plife_valid_obs(const int* hist_cnt, const int* hist_anchor, const int* hist_born, int e, int max_obs,
                                 const int* anc_used, const int* anc_born, const int* anc_link, int anchor_max, int n_groups,
                                 int* slot_out, int* group_out) {
  const int len = plife_hist_len(hist_cnt[e], max_obs);
  int k = 0;
  for (int q = 0; q < len; ++q) {
    const int s = plife_hist_slot(hist_cnt[e], max_obs, q);
    const int g = plife_obs_group(hist_anchor[e * max_obs + s], hist_born[e * max_obs + s], anc_used, anc_born, anc_link,
                                  anchor_max, n_groups);
    if (g >= 0) { slot_out[k] = s; group_out[k] = g; ++k; }
  }
  return k;
}
// a live entry without a track this frame is looked at, in ascending entry index, before the pool step frees anything
XIVO_LIFE_HD bool plife_oos_dropped(const long long* ent_id, int e, int track) { return ent_id[e] >= 0 && track < 0; }
// ... and used when it is READY, has at least min_obs valid observations, its depth lies inside (min_depth, max_depth) - the
// caller's comparison - and fewer than oos_max entries of the filter were used before it. READY with fewer observations counts
// as short, eligible beyond oos_max as surplus.
XIVO_LIFE_HD int plife_oos_decide(bool ready, bool depth_ok, int k, int min_obs, int n_used, int oos_max) {
  if (!ready) return PLIFE_OOS_NONE;
  if (k < min_obs) return PLIFE_OOS_SHORT;
  if (!depth_ok) return PLIFE_OOS_NONE;
  return n_used < oos_max ? PLIFE_OOS_USED : PLIFE_OOS_SURPLUS;
}
// rows of the fixed block every frame appends behind the in-state rows: oos_max features of at most 2 max_obs - 3 rows
XIVO_LIFE_HD int plife_oos_rows(int oos_max, int max_obs) { return oos_max * (2 * max_obs - 3); }

}  // namespace xivo_hip
