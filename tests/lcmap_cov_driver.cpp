// Host driver of the landmark map's visit rule (xivo_amd/csrc/lcmap_device.h: lcmap_used_now, lcmap_resting,
// lcmap_frame_decide_visit, lcmap_pair_neutral_visit, lcmap_used_next): a stand-alone program built from that header alone
// (plus include/xivo_hip.h for the sizes of the two new ABI structs) with a host compiler, plain and under AddressSanitizer /
// UBSan (tests/test_lcmap_cov_cpu.py). It keeps one filter's map and its visit records the way lcmap_close_kernel does -
// every list position reads the records from before the call, the records of the matched entries are written after the
// frame's decision, a key at several positions is used if any of them used it - and prints every decision; the test holds
// the lines against tests/lcmap_cov_restate.py.
//
// stdin:  map_max lc_max min_matches gap n_ops, then per op
//   A n  key x n                      -> "c count"  (a key stored already, a negative key or a full map: nothing)
//   Q n  key x n  kept x lc_max       -> "l entry..." the list, "r resting..." per position, "f frame neutral x lc_max",
//                                        "v (last_seen used) x count" the visit records after the call
//   C 0  c00 c01 c02 c11 c12 c22  a0 a1 a2  b0 b1 b2 (hex floats)  -> "q lcmap_quad3(C, a, b)" as a hex float
// stdout starts with "S" and the sizeof of xivo_lcmap_cov_opts, _cov_stats, and ends with "g mismatches tried": the rules
// with gap = 0 against lcmap_frame_decide / lcmap_pair_neutral on every input of a small grid, and "n": what the visit rule
// makes of a gamma that is not finite.
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/xivo_hip.h"
#include "lcmap_device.h"

using namespace xivo_hip;

int main() {
  printf("S %zu %zu\n", sizeof(xivo_lcmap_cov_opts), sizeof(xivo_lcmap_cov_stats));
  int map_max, lc_max, min_matches, gap, n_ops;
  if (scanf("%d %d %d %d %d", &map_max, &lc_max, &min_matches, &gap, &n_ops) != 5) return 2;
  std::vector<long long> keys((size_t)map_max);          // exactly map_max of each: a write past the map is the sanitizer's
  std::vector<int> last_seen((size_t)map_max, 0), used((size_t)map_max, 0);
  int count = 0, t = 0;
  for (int op = 0; op < n_ops; ++op) {
    char kind; int n;
    if (scanf(" %c %d", &kind, &n) != 2) return 2;
    if (kind == 'A') {
      for (int i = 0; i < n; ++i) {
        long long key;
        if (scanf("%lld", &key) != 1) return 2;
        const int dup = lcmap_find(keys.data(), 1, count, key) >= 0;
        if (lcmap_add_decide(key >= 0, 0, dup, count, map_max) == LCMAP_ADD_ACCEPT) { keys[(size_t)count] = key; ++count; }
      }
      printf("c %d\n", count);
    } else if (kind == 'Q') {
      ++t;
      std::vector<int> list((size_t)lc_max, -1), kept((size_t)lc_max), used_now((size_t)lc_max, 0), resting((size_t)lc_max, 0);
      int rank = 0;
      for (int i = 0; i < n; ++i) {
        long long key;
        if (scanf("%lld", &key) != 1) return 2;
        const int e = lcmap_find(map_max > 0 ? keys.data() : nullptr, 1, count, key);
        if (e < 0) continue;
        const int slot = lcmap_match_slot(rank++, lc_max);
        if (slot >= 0) list[(size_t)slot] = e;
      }
      for (int m = 0; m < lc_max; ++m)
        if (scanf("%d", &kept[(size_t)m]) != 1) return 2;
      const int n_matched = rank < lc_max ? rank : lc_max;
      int n_kept = 0, n_fresh = 0;
      for (int m = 0; m < n_matched; ++m) {               // (the records from before the call)
        const size_t e = (size_t)list[(size_t)m];
        used_now[(size_t)m] = lcmap_used_now(last_seen[e], used[e], t, gap);
        resting[(size_t)m] = lcmap_resting(gap, used_now[(size_t)m]);
        kept[(size_t)m] = kept[(size_t)m] != 0;
        n_kept += kept[(size_t)m]; n_fresh += kept[(size_t)m] && !resting[(size_t)m];
      }
      const int frame = lcmap_frame_decide_visit(n_matched, n_kept, n_fresh, min_matches);
      printf("l");
      for (int m = 0; m < lc_max; ++m) printf(" %d", list[(size_t)m]);
      printf("\nr");
      for (int m = 0; m < lc_max; ++m) printf(" %d", resting[(size_t)m]);
      printf("\nf %d", frame);
      for (int m = 0; m < lc_max; ++m)
        printf(" %d", lcmap_pair_neutral_visit(frame, m, n_matched, m < n_matched && kept[(size_t)m], resting[(size_t)m]));
      std::vector<int> next((size_t)lc_max, 0);
      for (int m = 0; m < n_matched; ++m) next[(size_t)m] = lcmap_used_next(used_now[(size_t)m], frame, kept[(size_t)m], resting[(size_t)m]);
      for (int m = 0; m < n_matched; ++m) {               // as the kernel: the first position of an entry writes the OR of all of them
        int u = 0, first = 1;
        for (int j = 0; j < n_matched; ++j)
          if (list[(size_t)j] == list[(size_t)m]) { u |= next[(size_t)j]; first &= j >= m; }
        if (first) { last_seen[(size_t)list[(size_t)m]] = t; used[(size_t)list[(size_t)m]] = u; }
      }
      printf("\nv");
      for (int e = 0; e < count; ++e) printf(" %d %d", last_seen[(size_t)e], used[(size_t)e]);
      printf("\n");
    } else if (kind == 'C') {                             // (n is not used: one case a line)
      double c[6], a[3], b[3];
      for (double& v : c) if (scanf("%la", &v) != 1) return 2;
      for (double& v : a) if (scanf("%la", &v) != 1) return 2;
      for (double& v : b) if (scanf("%la", &v) != 1) return 2;
      const double C[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
      printf("q %a\n", lcmap_quad3(C, a, b));
    } else {
      return 2;
    }
  }
  // gap = 0: the visit rules are the rules without them, whatever the records say
  long bad = 0, tried = 0;
  for (int nm = 0; nm <= 7; ++nm)
    for (int nk = 0; nk <= nm; ++nk)
      for (int mm = 1; mm <= 8; ++mm)
        for (int ls = 0; ls <= 3; ++ls)
          for (int us = 0; us <= 1; ++us)
            for (int tt = 1; tt <= 4; ++tt) {
              const int un = lcmap_used_now(ls, us, tt, 0), rest = lcmap_resting(0, un);
              const int n_fresh = nk - (rest ? nk : 0);   // all of them resting or none: with gap = 0 none can
              const int f0 = lcmap_frame_decide(nm, nk, mm), f1 = lcmap_frame_decide_visit(nm, nk, n_fresh, mm);
              bad += rest != 0; bad += f0 != f1; tried += 2;
              for (int m = 0; m <= 7; ++m)
                for (int k = 0; k <= 1; ++k) {
                  bad += lcmap_pair_neutral(f0, m, nm, k) != lcmap_pair_neutral_visit(f1, m, nm, k, rest);
                  ++tried;
                }
            }
  printf("g %ld %ld\n", bad, tried);
  // a gamma that is not finite (on R_e as on Rlc I): never kept, so it neither counts as fresh nor uses its entry in a closing frame
  const double qnan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int kn = lcmap_kept(1, qnan, 0.0), ki = lcmap_kept(1, inf, 0.0);
  printf("n %d %d %d %d %d\n", kn, ki, lcmap_kept(1, qnan, 5.99), lcmap_used_next(0, LCMAP_FRAME_CLOSED, kn, 0),
         lcmap_pair_neutral_visit(LCMAP_FRAME_CLOSED, 0, 1, ki, 0));
  return 0;
}
