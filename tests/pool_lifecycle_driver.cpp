// Host driver of xivo_amd/csrc/pool_lifecycle_device.h (tests/test_pool_lifecycle_cpu.py): replays a scripted run of the
// "subfilter" life cycle - per frame and filter the tracks (ids), what the pool step answered (live flags, the candidate order)
// and the gating outcome per slot - through the decision functions the pool life cycle kernels call, composed in the kernels'
// order, and prints the decisions as the equivalent op sequences, pixel sources, anchor / entry creations, and the books and
// counters after each frame. Compiled with a host compiler against the two headers alone. The entry's anchor and the anchor's
// link, which are resident on the device, are plain arrays here.
//
// stdin:  F G pool_max anchor_max max_group_lifetime B T
//         then T frames x B filters:  n / n ids / pool_max live flags / n_order / n_order entries / F mask values
// stdout: per frame  "P b kind i0 i1 i2"  ops before the step          "X b e k"  entry e's pixel comes from track k
//                    "Q b kind i0 i1 i2"  ops of the walk               "T b j k"  slot j's pixel comes from track k
//                    "R b kind i0 i1 i2"  ops after the update          "A b a"    anchor a is created
//                    "N b e a k"          track k takes entry e of anchor a
//                    "B b | feat_id | feat_ref | group_refs | ent_id | ent_anchor | ent_born | anc_used | anc_life | anc_link"
//                    "C b updates rejected dropped admitted groups_added pool_added pool_dropped pool_outliers anchors_created
//                         anchors_freed admit_steps"   (accumulated), then "E"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pool_lifecycle_device.h"

using namespace xivo_hip;

namespace {
enum { REMOVE_GROUP = 4, REMOVE_FEATURE = 6, ADD_GROUP_ANCHOR = 8, ADMIT_POOL = 9 };   // XIVO_EDIT_* of include/xivo_hip.h

struct Books {
  std::vector<long long> feat_id, ent_id;
  std::vector<int> feat_ref, group_refs, ent_anchor, ent_born, anc_used, anc_life, anc_link;
  long long updates = 0, rejected = 0, dropped = 0, admitted = 0, groups_added = 0, pool_added = 0, pool_dropped = 0,
            pool_outliers = 0, anchors_created = 0, anchors_freed = 0, admit_steps = 0;
};

int read_int() {
  int v;
  if (scanf("%d", &v) != 1) exit(2);
  return v;
}

// the removals of one stage: slots in rm leave the book, groups left empty leave with them and their anchors are unlinked
void removals(Books& bk, const std::vector<int>& rm, int G, int am, int b, char tag) {
  std::vector<int> removed(G);
  for (int j : rm) {
    printf("%c %d %d %d 0 0\n", tag, b, REMOVE_FEATURE, j);
    life_drop_feature(bk.feat_id.data(), bk.feat_ref.data(), bk.group_refs.data(), j);
  }
  const int n_rg = life_discard_empty_groups(bk.group_refs.data(), G, removed.data());
  for (int q = 0; q < n_rg; ++q) {
    printf("%c %d %d %d 0 0\n", tag, b, REMOVE_GROUP, removed[q]);
    for (int a = 0; a < am; ++a) plife_unlink(bk.anc_link.data(), a, removed[q]);
  }
}
}  // namespace

int main() {
  const int F = read_int(), G = read_int(), pm = read_int(), am = read_int(), max_life = read_int(), B = read_int(), T = read_int();
  if (am > XIVO_POOL_LIFE_MAX_ANCHORS) return 3;
  std::vector<Books> books(B);
  for (auto& bk : books) {
    bk.feat_id.assign(F, -1); bk.feat_ref.assign(F, -1); bk.group_refs.assign(G, -1);
    bk.ent_id.assign(pm, -1); bk.ent_anchor.assign(pm, -1); bk.ent_born.assign(pm, 0);
    bk.anc_used.assign(am, 0); bk.anc_life.assign(am, 0); bk.anc_link.assign(am, -1);
  }
  std::vector<int> op_kind(F + G), op_i0(F + G), op_i1(F + G), efree(pm);
  for (int frame = 1; frame <= T; ++frame) {
    for (int b = 0; b < B; ++b) {
      Books& bk = books[b];
      const int n = read_int();
      std::vector<long long> ids(n);
      for (int k = 0; k < n; ++k) if (scanf("%lld", &ids[k]) != 1) return 2;
      std::vector<int> live(pm), order, mask(F);
      for (int e = 0; e < pm; ++e) live[e] = read_int();
      order.resize(read_int());
      for (int& e : order) e = read_int();
      for (int j = 0; j < F; ++j) mask[j] = read_int();

      // ---- pool_life_begin_kernel
      for (int a = 0; a < am; ++a) bk.anc_life[a] = plife_anchor_tick(bk.anc_used[a], bk.anc_life[a]);
      std::vector<int> slot_track(F, -1), ent_track(pm, -1), rm;
      for (int j = 0; j < F; ++j) slot_track[j] = life_track_of_slot(bk.feat_id.data(), j, ids.data(), n);
      for (int e = 0; e < pm; ++e) ent_track[e] = plife_track_of_entry(bk.ent_id.data(), e, ids.data(), n);
      for (int j = 0; j < F; ++j)
        if (bk.feat_id[j] >= 0 && slot_track[j] < 0) rm.push_back(j);
      bk.dropped += (long long)rm.size();
      removals(bk, rm, G, am, b, 'P');
      for (int e = 0; e < pm; ++e) {
        if (plife_entry_leaves(bk.ent_id.data(), bk.ent_anchor.data(), e, ent_track[e])) ent_track[e] = -1;
        else printf("X %d %d %d\n", b, e, ent_track[e]);
      }
      // ---- (the step runs here: live / order are its answer)  pool_life_admit_kernel
      for (int e = 0; e < pm; ++e)
        if (plife_free_if_dead(bk.ent_id.data(), bk.ent_anchor.data(), e, live[e])) bk.pool_outliers += 1;
      int n_adm = 0, n_gadd = 0;
      const int n_ops = plife_walk(order.data(), (int)order.size(), frame, bk.feat_id.data(), bk.feat_ref.data(), bk.group_refs.data(),
                                   F, G, bk.ent_id.data(), bk.ent_anchor.data(), bk.ent_born.data(), ent_track.data(), pm,
                                   bk.anc_link.data(), am, slot_track.data(), op_kind.data(), op_i0.data(), op_i1.data(), &n_adm,
                                   &n_gadd, &bk.admit_steps);
      for (int o = 0; o < n_ops; ++o) {
        if (op_kind[o] == PLIFE_OP_ADD_GROUP_ANCHOR) printf("Q %d %d %d %d 0\n", b, ADD_GROUP_ANCHOR, op_i0[o], op_i1[o]);
        else printf("Q %d %d %d %d %d\n", b, ADMIT_POOL, op_i0[o], op_i0[o], op_i1[o]);
      }
      bk.admitted += n_adm; bk.groups_added += n_gadd;
      int n_in = 0;
      for (int j = 0; j < F; ++j) {
        if (bk.feat_id[j] < 0) continue;
        ++n_in;
        if (slot_track[j] >= 0) printf("T %d %d %d\n", b, j, slot_track[j]);
      }
      bk.updates += n_in > 0 ? 1 : 0;
      // ---- (the update runs here: mask is its answer)  pool_life_end_kernel
      rm.clear();
      for (int j = 0; j < F; ++j)
        if (bk.feat_id[j] >= 0 && !mask[j]) rm.push_back(j);
      bk.rejected += (long long)rm.size();
      removals(bk, rm, G, am, b, 'R');
      std::vector<int> fresh(n, 0), pick(pm, -1);
      int n_new = 0;
      for (int k = 0; k < n; ++k)
        fresh[k] = plife_is_unheld(bk.feat_id.data(), F, bk.ent_id.data(), pm, ids[k]) && plife_first_occurrence(ids.data(), k) ? 1 : 0;
      for (int k = 0; k < n; ++k) {
        if (!fresh[k]) continue;
        ++n_new;
        const int r = life_rank(ids.data(), fresh.data(), n, k);
        if (r < pm) pick[r] = k;
      }
      if (n_new > 0) {
        const int an = plife_free_anchor(bk.anc_used.data(), am);
        const int n_free = plife_free_entries(bk.ent_id.data(), pm, efree.data());
        bk.pool_dropped += plife_surplus(n_new, n_free, an);
        if (an >= 0) {
          plife_create_anchor(bk.anc_used.data(), bk.anc_life.data(), bk.anc_link.data(), an);
          printf("A %d %d\n", b, an);
          const int n_take = n_free < n_new ? n_free : n_new;
          for (int q = 0; q < n_take; ++q) {
            plife_take_entry(bk.ent_id.data(), bk.ent_anchor.data(), bk.ent_born.data(), efree[q], ids[pick[q]], an, frame);
            printf("N %d %d %d %d\n", b, efree[q], an, pick[q]);
          }
          bk.anchors_created += 1; bk.pool_added += n_take;
        }
      }
      for (int a = 0; a < am; ++a)
        if (plife_expire_anchor(bk.anc_used.data(), bk.anc_life.data(), bk.anc_link.data(), a, max_life, bk.ent_id.data(),
                                bk.ent_anchor.data(), pm))
          bk.anchors_freed += 1;
    }
    for (int b = 0; b < B; ++b) {
      const Books& bk = books[b];
      printf("B %d |", b);
      for (long long v : bk.feat_id) printf(" %lld", v);
      printf(" |");
      for (int v : bk.feat_ref) printf(" %d", v);
      printf(" |");
      for (int v : bk.group_refs) printf(" %d", v);
      printf(" |");
      for (long long v : bk.ent_id) printf(" %lld", v);
      printf(" |");
      for (int v : bk.ent_anchor) printf(" %d", v);
      printf(" |");
      for (int e = 0; e < pm; ++e) printf(" %d", bk.ent_id[e] >= 0 ? bk.ent_born[e] : 0);
      printf(" |");
      for (int v : bk.anc_used) printf(" %d", v);
      printf(" |");
      for (int v : bk.anc_life) printf(" %d", v);
      printf(" |");
      for (int v : bk.anc_link) printf(" %d", v);
      printf("\nC %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", b, bk.updates, bk.rejected, bk.dropped, bk.admitted,
             bk.groups_added, bk.pool_added, bk.pool_dropped, bk.pool_outliers, bk.anchors_created, bk.anchors_freed, bk.admit_steps);
    }
    printf("E\n");
  }
  return 0;
}
