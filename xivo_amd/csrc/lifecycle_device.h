// The decisions of the per-frame feature life cycle ("immediate" mode) as plain functions over ONE filter's slot book and the
// frame's track arrays: who is tracked, who leaves, which groups go with them, whether new features are admitted, which
// candidates and into which slots. Integer logic and comparisons only - no arithmetic of the filter. Host and device: the
// kernels of lifecycle_kernels.hip call these functions, and a host compiler takes the header alone
// (tests/lifecycle_driver.cpp replays scripted frames through them without a GPU).
//
// Every rule restates SequenceRunner.frame (xivo_amd/sequence.py) and BatchEstimator::VisualMeasPointCloud
// (xivo_amd/host/batch_estimator.cpp), which follow the reference:
//   tracker-dropped features leave            ProcessTracks                 src/manager.cpp:152-169
//   gate-rejected features leave              Estimator::Update             src/update.cpp:105-113
//   a group leaves with its last feature      DiscardAffectedGroups, simplified; RemoveGroupFromState src/estimator.cpp:745-759
//   new features enter with a new group       SelectAndAddNewFeatures       src/manager.cpp:332-450, AddGroupToState
//                                             src/estimator.cpp:801-816, AddFeatureToState :820-846
// The book of a filter: feat_id[F] (track id held by feature slot j, -1: free; list position j is slot j), feat_ref[F] (group
// slot the feature is anchored to, -1: free) and group_refs[n_groups] (-1: free group slot, else the number of in-state features
// anchored there).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_LIFE_HD __host__ __device__ __forceinline__
#else
#define XIVO_LIFE_HD inline
#endif

namespace xivo_hip {

// ---- association
// true when feature slot j holds track `id` (a free slot holds -1 and matches nothing: track ids are >= 0)
XIVO_LIFE_HD bool life_slot_holds(const long long* feat_id, int j, long long id) { return id >= 0 && feat_id[j] == id; }
// whether any slot holds `id` - "the track is in the state" (id2slot of the host books)
XIVO_LIFE_HD bool life_in_state(const long long* feat_id, int F, long long id) {
  for (int j = 0; j < F; ++j)
    if (life_slot_holds(feat_id, j, id)) return true;
  return false;
}
// the track that feeds slot j: the LAST position k < n with ids[k] == feat_id[j] (a repeated id: the last occurrence supplies
// the pixel, as the host's position table does), -1: the tracker dropped the feature. One slot's serial form, for host code
// (tests/lifecycle_driver.cpp); life_begin_kernel reaches the same k with one thread per track and an LDS maximum per slot
// over life_slot_holds, which only a GPU test can check.
XIVO_LIFE_HD int life_track_of_slot(const long long* feat_id, int j, const long long* ids, int n) {
  int k_last = -1;
  for (int k = 0; k < n; ++k)
    if (life_slot_holds(feat_id, j, ids[k])) k_last = k;
  return k_last;
}

// ---- leaving the state
// slot j leaves (drop_feature of the host books): its group loses one reference
XIVO_LIFE_HD void life_drop_feature(long long* feat_id, int* feat_ref, int* group_refs, int j) {
  if (feat_ref[j] >= 0) group_refs[feat_ref[j]] -= 1;
  feat_id[j] = -1; feat_ref[j] = -1;
}
// groups left without a feature are discarded, ascending slot order: removed[0..return) lists them, their slots become free
XIVO_LIFE_HD int life_discard_empty_groups(int* group_refs, int n_groups, int* removed) {
  int n = 0;
  for (int g = 0; g < n_groups; ++g)
    if (group_refs[g] == 0) { removed[n++] = g; group_refs[g] = -1; }
  return n;
}

// ---- free slots
XIVO_LIFE_HD int life_free_group(const int* group_refs, int n_groups) {   // the lowest free group slot, -1: none
  for (int g = 0; g < n_groups; ++g)
    if (group_refs[g] < 0) return g;
  return -1;
}
// free feature slots in ascending order into free_slots[0..return)
XIVO_LIFE_HD int life_free_slots(const long long* feat_id, int F, int* free_slots) {
  int n = 0;
  for (int j = 0; j < F; ++j)
    if (feat_id[j] < 0) free_slots[n++] = j;
  return n;
}

// ---- admission
// skipped without a free group slot g, or with fewer than min_new_features free slots while the state is not empty
XIVO_LIFE_HD bool life_admission_open(int g, int n_free, int n_instate, int min_new_features) {
  return g >= 0 && !(n_free < min_new_features && n_instate > 0);
}
// a candidate: a track not in the state whose depth lies strictly inside (min_depth, max_depth); NaN is no candidate
XIVO_LIFE_HD bool life_is_candidate(bool in_state, double depth, double min_depth, double max_depth) {
  return !in_state && min_depth < depth && depth < max_depth;
}
// candidate order: ascending id, ties by position in the frame (the host's stable sort)
XIVO_LIFE_HD bool life_before(long long id_a, int k_a, long long id_b, int k_b) {
  return id_a < id_b || (id_a == id_b && k_a < k_b);
}
// rank of candidate k among the n tracks of the frame: the candidates ordered before it (rank counting - only the ranks below
// the number of free slots are ever used). cand[k'] != 0 marks a candidate.
template <class Flag>
XIVO_LIFE_HD int life_rank(const long long* ids, const Flag* cand, int n, int k) {
  int r = 0;
  const long long id = ids[k];
  for (int q = 0; q < n; ++q)
    if (cand[q] && life_before(ids[q], q, id, k)) ++r;
  return r;
}

}  // namespace xivo_hip
