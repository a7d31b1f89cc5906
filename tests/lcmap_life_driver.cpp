// Host driver of the rules of loop closure inside the device life cycle (xivo_amd/csrc/lcmap_life_device.h): a stand-alone
// program built from that header alone (plus include/xivo_hip.h for the sizes of the two ABI structs the lists hold) with a host
// compiler, plain and under AddressSanitizer / UBSan (tests/test_lcmap_life_cpu.py). It walks hand-made books the way the begin
// kernel and the query kernel do - slots in ascending order, a yielding slot ranked by the yielding slots before it - and prints
// every record and query with its list position; the test holds the lines against SequenceRunner._lc_add / _lc_close.
//
// stdin:  B row F, then per filter F slots of  feat_id slot_track u_is_nan mask key
// stdout: "S" and the sizeof of xivo_lcmap_add_rec, xivo_lcmap_query; per filter
//   "r n  slot key pos ..."   the add records of the begin call
//   "q n  slot key pos ..."   the queries of the close call, on the book the begin call left
//   "k key ..."               feat_key after the begin call
// and last "c ..." the counts lclife_list_count lets through at its bounds.
#include <cstdio>
#include <vector>

#include "../include/xivo_hip.h"
#include "lcmap_life_device.h"

using namespace xivo_hip;

int main() {
  printf("S %zu %zu\n", sizeof(xivo_lcmap_add_rec), sizeof(xivo_lcmap_query));
  int B, row, F;
  if (scanf("%d %d %d", &B, &row, &F) != 3 || B < 0 || F < 0 || F > row) return 2;
  // exactly B rows of `row` positions: a position outside a filter's row, or the lists, is the sanitizer's
  std::vector<xivo_lcmap_add_rec> recs((size_t)B * row);
  std::vector<xivo_lcmap_query> queries((size_t)B * row);
  for (int b = 0; b < B; ++b) {
    std::vector<long long> fid((size_t)F), key((size_t)F);
    std::vector<int> st((size_t)F), nan((size_t)F), mask((size_t)F), tracked((size_t)F);
    for (int j = 0; j < F; ++j)
      if (scanf("%lld %d %d %d %lld", &fid[j], &st[j], &nan[j], &mask[j], &key[j]) != 5) return 2;
    int n_rec = 0;
    for (int j = 0; j < F; ++j) {   // the begin call
      tracked[j] = lclife_tracked(fid[j], st[j], nan[j]);
      if (!lclife_leaves(fid[j], st[j])) continue;
      xivo_lcmap_add_rec& r = recs[(size_t)lclife_list_pos(b, row, n_rec++)];
      r.b = b; r.feat = j; r.key = key[j];
      fid[j] = -1; key[j] = lclife_no_key();
    }
    printf("r %d", n_rec);
    for (int i = 0; i < n_rec; ++i) {
      const long pos = lclife_list_pos(b, row, i);
      printf("  %d %lld %ld", recs[(size_t)pos].feat, recs[(size_t)pos].key, pos);
    }
    int n_q = 0;
    std::vector<int> q_slot;
    for (int j = 0; j < F; ++j) {   // the close call
      if (!lclife_queries(fid[j], mask[j], tracked[j])) continue;
      xivo_lcmap_query& q = queries[(size_t)lclife_list_pos(b, row, n_q++)];
      q.b = b; q.group_sind = -1; q.key = key[j];
      q_slot.push_back(j);
    }
    printf("\nq %d", n_q);
    for (int i = 0; i < n_q; ++i) {
      const long pos = lclife_list_pos(b, row, i);
      printf("  %d %lld %ld", q_slot[(size_t)i], queries[(size_t)pos].key, pos);
    }
    printf("\nk");
    for (int j = 0; j < F; ++j) printf(" %lld", key[j]);
    printf("\n");
  }
  printf("c %d %d %d %d\n", lclife_list_count(-1, 8), lclife_list_count(0, 8), lclife_list_count(8, 8), lclife_list_count(9, 8));
  return 0;
}
