// Host driver of xivo_amd/csrc/lifecycle_device.h (tests/test_lifecycle_cpu.py): replays a scripted run - per frame and filter
// the tracks (id, depth) and the gating outcome per slot - through the decision functions the life cycle kernels call, composed
// in the kernels' order, and prints the decisions as the equivalent op sequence and the book after each frame. Compiled with a
// host compiler against the header alone.
//
// stdin:  F G min_new_features min_depth max_depth B T          (doubles as hex floats)
//         then T frames x B filters:  n / n lines "id depth" / one line of F mask values (0 / 1)
// stdout: per frame  "T b j k"       slot j of filter b is fed by track k of the frame
//                    "P b kind i0 i1 i2"   ops before the update     "Q b kind i0 i1 i2"   ops after it
//                    "B b | feat_id.. | feat_ref.. | group_refs.."  the book after the frame, then "E"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lifecycle_device.h"

using namespace xivo_hip;

namespace {
enum { ADD_GROUP = 3, REMOVE_GROUP = 4, ADD_FEATURE = 5, REMOVE_FEATURE = 6 };   // XIVO_EDIT_* of include/xivo_hip.h

struct Book {
  std::vector<long long> feat_id;
  std::vector<int> feat_ref, group_refs;
};

double read_double() {
  char buf[128];
  if (scanf("%127s", buf) != 1) exit(2);
  return strtod(buf, nullptr);
}
}  // namespace

int main() {
  int F, G, min_new, B, T;
  if (scanf("%d %d %d", &F, &G, &min_new) != 3) return 2;
  const double min_depth = read_double(), max_depth = read_double();
  if (scanf("%d %d", &B, &T) != 2) return 2;
  std::vector<Book> books(B);
  for (auto& bk : books) { bk.feat_id.assign(F, -1); bk.feat_ref.assign(F, -1); bk.group_refs.assign(G, -1); }
  std::vector<int> removed(G), free_slots(F), pick(F), mask(F);
  for (int t = 0; t < T; ++t) {
    std::vector<std::vector<long long>> ids(B);
    std::vector<std::vector<double>> depth(B);
    std::vector<std::vector<int>> masks(B);
    for (int b = 0; b < B; ++b) {
      int n;
      if (scanf("%d", &n) != 1) return 2;
      ids[b].resize(n); depth[b].resize(n);
      for (int k = 0; k < n; ++k) {
        if (scanf("%lld", &ids[b][k]) != 1) return 2;
        depth[b][k] = read_double();
      }
      masks[b].resize(F);
      for (int j = 0; j < F; ++j) if (scanf("%d", &masks[b][j]) != 1) return 2;
    }
    // ---- life_begin_kernel
    for (int b = 0; b < B; ++b) {
      Book& bk = books[b];
      const int n = (int)ids[b].size();
      std::vector<int> slot_track(F, -1);
      for (int j = 0; j < F; ++j) slot_track[j] = life_track_of_slot(bk.feat_id.data(), j, ids[b].data(), n);
      for (int j = 0; j < F; ++j) {
        if (bk.feat_id[j] < 0) continue;
        if (slot_track[j] >= 0) { printf("T %d %d %d\n", b, j, slot_track[j]); continue; }
        printf("P %d %d %d 0 0\n", b, REMOVE_FEATURE, j);
        life_drop_feature(bk.feat_id.data(), bk.feat_ref.data(), bk.group_refs.data(), j);
      }
      const int n_rg = life_discard_empty_groups(bk.group_refs.data(), G, removed.data());
      for (int q = 0; q < n_rg; ++q) printf("P %d %d %d 0 0\n", b, REMOVE_GROUP, removed[q]);
    }
    // ---- life_end_kernel
    for (int b = 0; b < B; ++b) {
      Book& bk = books[b];
      const int n = (int)ids[b].size();
      int n_in = 0;
      for (int j = 0; j < F; ++j) {
        if (bk.feat_id[j] < 0) continue;
        if (!masks[b][j]) {
          printf("Q %d %d %d 0 0\n", b, REMOVE_FEATURE, j);
          life_drop_feature(bk.feat_id.data(), bk.feat_ref.data(), bk.group_refs.data(), j);
        } else ++n_in;
      }
      const int n_rg = life_discard_empty_groups(bk.group_refs.data(), G, removed.data());
      for (int q = 0; q < n_rg; ++q) printf("Q %d %d %d 0 0\n", b, REMOVE_GROUP, removed[q]);
      const int g = life_free_group(bk.group_refs.data(), G);
      const int n_free = life_free_slots(bk.feat_id.data(), F, free_slots.data());
      if (!life_admission_open(g, n_free, n_in, min_new)) continue;
      std::vector<int> cand(n);
      int n_cand = 0;
      for (int k = 0; k < n; ++k) {
        cand[k] = life_is_candidate(life_in_state(bk.feat_id.data(), F, ids[b][k]), depth[b][k], min_depth, max_depth) ? 1 : 0;
        n_cand += cand[k];
      }
      for (int k = 0; k < n; ++k) {
        if (!cand[k]) continue;
        const int r = life_rank(ids[b].data(), cand.data(), n, k);
        if (r < n_free) pick[r] = k;
      }
      if (n_cand == 0) continue;
      printf("Q %d %d %d 0 0\n", b, ADD_GROUP, g);
      const int n_new = n_free < n_cand ? n_free : n_cand;
      for (int q = 0; q < n_new; ++q) {
        const int j = free_slots[q];
        printf("Q %d %d %d %d %d\n", b, ADD_FEATURE, j, j, g);
        bk.feat_id[j] = ids[b][pick[q]]; bk.feat_ref[j] = g;
      }
      bk.group_refs[g] = n_new;
    }
    for (int b = 0; b < B; ++b) {
      const Book& bk = books[b];
      printf("B %d |", b);
      for (int j = 0; j < F; ++j) printf(" %lld", bk.feat_id[j]);
      printf(" |");
      for (int j = 0; j < F; ++j) printf(" %d", bk.feat_ref[j]);
      printf(" |");
      for (int g = 0; g < G; ++g) printf(" %d", bk.group_refs[g]);
      printf("\n");
    }
    printf("E\n");
  }
  return 0;
}
