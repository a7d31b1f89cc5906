// Driver of tests/test_frame_log_cpu.py: xivo_amd/csrc/frame_log.h alone, compiled with g++ -std=c++17 (no HIP). Each scenario
// prints "step key=value ..." lines that the test reads.
#include <climits>
#include <cstdio>
#include <cstring>

#include "frame_log.h"

using xivo_hip::capi::FrameLog;

static void state(const char* step, const FrameLog& l) {
  printf("%s configured=%d full=%d capacity=%d count=%d\n", step, (int)l.configured(), (int)l.full(), l.capacity(), l.count());
}

static int life() {
  FrameLog l;
  state("fresh", l);
  printf("fresh_commit index=%d count=%d\n", l.commit(5), l.count());   // not configured: nothing can be committed
  l.configure(1);
  state("one", l);
  const int first = l.commit(11);
  state("one_full", l);
  const int again = l.commit(12);
  long long ts = -1;
  l.stamps(0, 1, &ts);
  printf("one_refused first=%d again=%d count=%d stamp=%lld\n", first, again, l.count(), ts);
  l.configure(0);
  state("released", l);

  l.configure(5);
  int idx[4];
  for (int i = 0; i < 4; ++i) idx[i] = l.commit(100 + 10 * i);
  long long mid[2] = {-1, -1};
  l.stamps(1, 2, mid);
  l.stamps(0, 4, nullptr);   // (no destination: nothing to do)
  printf("order i0=%d i1=%d i2=%d i3=%d mid0=%lld mid1=%lld\n", idx[0], idx[1], idx[2], idx[3], mid[0], mid[1]);
  l.reset();
  state("reset", l);
  const int reused = l.commit(7);
  long long t0 = -1;
  l.stamps(0, 1, &t0);
  printf("reuse index=%d count=%d stamp=%lld\n", reused, l.count(), t0);
  l.configure(3);   // a new capacity empties the log
  state("reconfigured", l);
  return 0;
}

static int slices() {
  FrameLog l;
  l.configure(8);
  for (int i = 0; i < 3; ++i) l.commit(i);
  const int n = l.count();
  const int q[][2] = {{0, 0}, {n, 0}, {0, n}, {1, 2}, {0, 4}, {3, 1}, {-1, 1}, {0, -1}, {INT_MAX, INT_MAX}, {4, 0}, {INT_MAX, 0}};
  const char* name[] = {"empty_front", "empty_back", "all", "middle", "too_long", "past_end", "neg_t0", "neg_nt", "int_max", "empty_past", "empty_far"};
  for (size_t i = 0; i < sizeof(q) / sizeof(q[0]); ++i) printf("%s ok=%d\n", name[i], (int)l.slice_ok(q[i][0], q[i][1]));
  state("after", l);
  // frame-major offsets are taken in size_t: no wrap at the largest ints
  printf("at small=%zu big=%zu\n", FrameLog::at(2, 7, 3), FrameLog::at(INT_MAX, INT_MAX, INT_MAX));
  return 0;
}

static int sizing() {
  size_t n = 0;
  // T_max * Bmax = 2^40 entries: 2^23 bytes each is 2^63 (refused), one byte less per entry fits
  const int T = 1 << 20, B = 1 << 20;
  const bool below = FrameLog::fits(T, B, ((size_t)1 << 23) - 1, &n);
  printf("below ok=%d entries=%zu\n", (int)below, n);
  const bool exact = FrameLog::fits(T, B, (size_t)1 << 23, &n);
  printf("exact ok=%d entries=%zu\n", (int)exact, n);
  // the bound itself: 2^63 - 1 = 7^2 * 73 * 127 * 337 * 92737 * 649657, so (7 * 73 * 127 * 337) x (7 * 92737) entries of 649657 bytes
  const bool last = FrameLog::fits(7 * 73 * 127 * 337, 7 * 92737, 649657, &n);
  printf("last ok=%d entries=%zu\n", (int)last, n);
  const bool over = FrameLog::fits(7 * 73 * 127 * 337, 7 * 92737, 649658, &n);
  printf("over ok=%d entries=%zu\n", (int)over, n);
  const bool big1 = FrameLog::fits(INT_MAX, INT_MAX, 1, &n);
  printf("int_max_bytes ok=%d entries=%zu\n", (int)big1, n);
  const bool big = FrameLog::fits(INT_MAX, INT_MAX, 176, &n);
  printf("int_max ok=%d entries=%zu\n", (int)big, n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "life")) return life();
  if (!strcmp(argv[1], "slices")) return slices();
  if (!strcmp(argv[1], "sizing")) return sizing();
  return 2;
}
