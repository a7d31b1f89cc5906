// Host driver of the landmark map's integer rules (xivo_amd/csrc/lcmap_device.h): a stand-alone program built from that header
// alone (plus include/xivo_hip.h for the sizes of the ABI structs) with a host compiler, plain and under AddressSanitizer /
// UBSan (tests/test_lcmap_cpu.py). It keeps one filter's map the way the kernels do - the records of an add call in order,
// the queries of a close call ranked by the matching ones before them - and prints every decision; the test holds the lines
// against tests/lcmap_restate.py.
//
// stdin:  map_max lc_max min_matches n_ops, then per op
//   A n  (key in_state poor) x n      -> "a d..." the outcome of every record, "c count"
//   Q n  key x n  kept x lc_max       -> "s slot..." (-1: no match, -2: surplus), "l entry..." the list, "f frame neutral x lc_max"
// stdout starts with "S" and the sizeof of xivo_lcmap_opts, _entry, _add_rec, _query, _match, _stats, and ends with the
// floating-point rules at their ties ("p", "k") and lcmap_kept on gammas that are not finite ("n").
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/xivo_hip.h"
#include "lcmap_device.h"

using namespace xivo_hip;

int main() {
  printf("S %zu %zu %zu %zu %zu %zu\n", sizeof(xivo_lcmap_opts), sizeof(xivo_lcmap_entry), sizeof(xivo_lcmap_add_rec),
         sizeof(xivo_lcmap_query), sizeof(xivo_lcmap_match), sizeof(xivo_lcmap_stats));
  int map_max, lc_max, min_matches, n_ops;
  if (scanf("%d %d %d %d", &map_max, &lc_max, &min_matches, &n_ops) != 4) return 2;
  std::vector<xivo_lcmap_entry> map((size_t)map_max);   // exactly map_max entries: a write past `full` is the sanitizer's
  const long stride = sizeof(xivo_lcmap_entry) / sizeof(long long);
  int count = 0;
  for (int op = 0; op < n_ops; ++op) {
    char kind; int n;
    if (scanf(" %c %d", &kind, &n) != 2) return 2;
    if (kind == 'A') {
      printf("a");
      for (int i = 0; i < n; ++i) {
        long long key; int in_state, poor;
        if (scanf("%lld %d %d", &key, &in_state, &poor) != 3) return 2;
        // (the kernel's reading of a record: a negative key is never in the state's sense)
        const int ok = in_state && key >= 0;
        const int dup = ok && !poor && lcmap_find(&map.data()->key, stride, count, key) >= 0;
        const int d = lcmap_add_decide(ok, poor, dup, count, map_max);
        if (d == LCMAP_ADD_ACCEPT) { map[(size_t)count].key = key; ++count; }
        printf(" %d", d);
      }
      printf("\nc %d\n", count);
    } else if (kind == 'Q') {
      std::vector<int> list((size_t)lc_max, -1), flag((size_t)n), ent((size_t)n), kept((size_t)lc_max);
      for (int i = 0; i < n; ++i) {
        long long key;
        if (scanf("%lld", &key) != 1) return 2;
        ent[(size_t)i] = lcmap_find(map_max > 0 ? &map.data()->key : nullptr, stride, count, key);
        flag[(size_t)i] = ent[(size_t)i] >= 0;
      }
      for (int m = 0; m < lc_max; ++m)
        if (scanf("%d", &kept[(size_t)m]) != 1) return 2;
      printf("s");
      int total = 0;
      for (int i = 0; i < n; ++i) {
        int rank = 0;                                     // the matching queries before this one
        for (int j = 0; j < i; ++j) rank += flag[(size_t)j];
        int slot = -1;
        if (flag[(size_t)i]) {
          slot = lcmap_match_slot(rank, lc_max);
          if (slot >= 0) list[(size_t)slot] = ent[(size_t)i]; else slot = -2;
          ++total;
        }
        printf(" %d", slot);
      }
      printf("\nl");
      for (int m = 0; m < lc_max; ++m) printf(" %d", list[(size_t)m]);
      const int n_matched = total < lc_max ? total : lc_max;
      int n_kept = 0;
      for (int m = 0; m < n_matched; ++m) n_kept += kept[(size_t)m] != 0;
      const int frame = lcmap_frame_decide(n_matched, n_kept, min_matches);
      printf("\nf %d", frame);
      for (int m = 0; m < lc_max; ++m) printf(" %d", lcmap_pair_neutral(frame, m, n_matched, m < n_matched && kept[(size_t)m]));
      printf("\n");
    } else {
      return 2;
    }
  }
  // the two floating-point rules at their ties
  printf("p %d %d %d %d\n", lcmap_poor(1.0, 1.0), lcmap_poor(1.0000000000000002, 1.0), lcmap_poor(5.0, 0.0), lcmap_poor(0.5, 1.0));
  printf("k %d %d %d %d\n", lcmap_kept(1, 5.0, 5.0), lcmap_kept(1, 5.000000000000001, 5.0), lcmap_kept(1, 1e9, 0.0), lcmap_kept(0, 0.0, 5.0));
  // a gamma that is not finite is never kept, with a gate or without one; the largest finite one is, without a gate
  const double qnan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  printf("n %d %d %d %d %d %d %d\n", lcmap_kept(1, qnan, 5.99), lcmap_kept(1, qnan, 0.0), lcmap_kept(1, inf, 5.99), lcmap_kept(1, inf, 0.0),
         lcmap_kept(1, -inf, 5.99), lcmap_kept(1, -qnan, 0.0), lcmap_kept(1, std::numeric_limits<double>::max(), 0.0));
  return 0;
}
