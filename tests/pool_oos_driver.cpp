// Stand-alone replay of the OOS rules of xivo_amd/csrc/pool_lifecycle_device.h (plife_hist_*, plife_obs_group, plife_valid_obs,
// plife_oos_dropped, plife_oos_decide, plife_oos_rows) under a host compiler: tests/test_pool_oos_cpu.py feeds it, frame by frame
// and filter by filter, the anchor tables at selection time, the entries whose track ended with what the device would know of
// them (READY, depth in range), and at the end of the frame the anchor created and the entries it observes. The driver keeps the
// observation rings itself and prints every decision and every append; the test holds that against
// SequenceRunner._frame_subfilter.
//
// stdin:  pool_max anchor_max n_groups max_obs min_obs oos_max B T
//         per frame and filter:
//           anc_used[anchor_max] / anc_born[anchor_max] / anc_link[anchor_max]      (three lines)
//           n_live   then n_live pairs   entry track(-1: none)                      every live entry, ascending
//           n_dropped then n_dropped triples  entry ready depth_ok                  what the device knows of the dropped ones
//           anchor frame                                                            created at the end of the frame, -1: none
//           n_taken  then the entries taken by new tracks this frame
//           n_seen   then the live entries with a track at the end of the frame
// stdout: D b e k decision g... s...   per dropped entry (valid observations: group slots, then ring slots, oldest first)
//         C b used short surplus       the filter's running counters
//         H b e cnt slot               per append
//         R rows                       once, first line
//         E                            end of frame
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pool_lifecycle_device.h"

using namespace xivo_hip;

static int rd() {
  int v;
  if (scanf("%d", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

int main() {
  const int pm = rd(), am = rd(), ng = rd(), max_obs = rd(), min_obs = rd(), oos_max = rd(), B = rd(), T = rd();
  printf("R %d\n", plife_oos_rows(oos_max, max_obs));
  std::vector<std::vector<int>> cnt(B, std::vector<int>(pm, 0)), ha(B, std::vector<int>((size_t)pm * max_obs, -1)),
      hb(B, std::vector<int>((size_t)pm * max_obs, -1));
  std::vector<long long> used(B, 0), n_short(B, 0), surplus(B, 0);
  std::vector<int> au(am), ab(am), al(am), slot(max_obs), grp(max_obs);
  for (int t = 0; t < T; ++t) {
    for (int b = 0; b < B; ++b) {
      for (int a = 0; a < am; ++a) au[a] = rd();
      for (int a = 0; a < am; ++a) ab[a] = rd();
      for (int a = 0; a < am; ++a) al[a] = rd();
      std::vector<long long> ent_id(pm, -1);
      std::vector<int> track(pm, -1);
      const int n_live = rd();
      for (int i = 0; i < n_live; ++i) { const int e = rd(); ent_id[e] = 1; track[e] = rd(); }
      const int n_drop = rd();
      std::vector<int> ready(pm, 0), depth(pm, 0), told(pm, 0);
      for (int i = 0; i < n_drop; ++i) { const int e = rd(); ready[e] = rd(); depth[e] = rd(); told[e] = 1; }
      int n_used = 0;
      for (int e = 0; e < pm; ++e) {
        if (!plife_oos_dropped(ent_id.data(), e, track[e])) continue;
        if (!told[e]) { fprintf(stderr, "frame %d filter %d: entry %d is dropped but the script does not say so\n", t, b, e); return 3; }
        const int k = plife_valid_obs(cnt[b].data(), ha[b].data(), hb[b].data(), e, max_obs, au.data(), ab.data(), al.data(), am, ng,
                                      slot.data(), grp.data());
        const int d = plife_oos_decide(ready[e] != 0, depth[e] != 0, k, min_obs, n_used, oos_max);
        if (d == PLIFE_OOS_USED) { ++n_used; ++used[b]; }
        else if (d == PLIFE_OOS_SHORT) ++n_short[b];
        else if (d == PLIFE_OOS_SURPLUS) ++surplus[b];
        printf("D %d %d %d %d", b, e, k, d);
        for (int q = 0; q < k; ++q) printf(" %d", grp[q]);
        for (int q = 0; q < k; ++q) printf(" %d", slot[q]);
        printf("\n");
      }
      printf("C %d %lld %lld %lld\n", b, used[b], n_short[b], surplus[b]);
      const int a = rd(), frame = rd();
      const int n_taken = rd();
      for (int i = 0; i < n_taken; ++i) plife_hist_reset(cnt[b].data(), rd());
      const int n_seen = rd();
      for (int i = 0; i < n_seen; ++i) {
        const int e = rd();
        if (a < 0) continue;   // a frame that creates no anchor records nothing
        const int s = plife_hist_append(cnt[b].data(), ha[b].data(), hb[b].data(), e, max_obs, a, frame);
        printf("H %d %d %d %d\n", b, e, cnt[b][e], s);
      }
    }
    printf("E\n");
  }
  return 0;
}
