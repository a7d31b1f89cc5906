// Drives DeviceBuffers (xivo_amd/csrc/device_buffers.h) against a counting allocator, the header alone under a host compiler:
// tests/test_device_buffers_cpu.py runs one scenario per call and asserts on the "key=value" lines printed here.
//
// The allocator hands out addresses that are never dereferenced and never reused (a serial number), so "this slot holds a
// freed pointer" is a set lookup. It counts live blocks, logs every free, and fails the k-th allocation on request.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "device_buffers.h"

using xivo_hip::capi::DeviceBuffers;

namespace {

struct Counting {
  std::map<void*, size_t> live;          // block -> bytes
  std::map<void*, int> freed;            // block -> times freed
  std::vector<int> zero_flags;           // the `zero` argument of every successful allocation, in order
  int allocs = 0, calls = 0, fail_at = 0, bad_frees = 0;
  size_t serial = 0;
} g;

int count_alloc(void** p, size_t bytes, int zero) {
  *p = nullptr;
  if (++g.calls == g.fail_at) return -4;   // (the status the caller sees: XIVO_HIP_ERR_NOMEM)
  *p = reinterpret_cast<void*>(0x1000 * ++g.serial);
  g.live[*p] = bytes; g.zero_flags.push_back(zero); ++g.allocs;
  return 0;
}
void count_free(void* p) {
  if (!g.live.erase(p)) ++g.bad_frees;
  ++g.freed[p];
}
void fail_next(int k) { g.calls = 0; g.fail_at = k; }
int max_freed() { int m = 0; for (auto& f : g.freed) m = f.second > m ? f.second : m; return m; }
size_t live_bytes() { size_t s = 0; for (auto& b : g.live) s += b.second; return s; }
bool dangling(void* p) { return p && !g.live.count(p); }

// the five slots of a "drop the group and re-allocate it" site, of different element types as in the context
struct Group { int* a = nullptr; double* b = nullptr; unsigned char* c = nullptr; double* d = nullptr; long* e = nullptr; };
int resize(DeviceBuffers& m, Group& s, size_t n) {
  m.release(&s.a, &s.b, &s.c, &s.d, &s.e);
  int rc = m.zeroed(&s.a, n);
  if (!rc) rc = m.zeroed(&s.b, n * 42);
  if (!rc) rc = m.raw(&s.c, n);
  if (!rc) rc = m.raw(&s.d, n * 2);
  if (!rc) rc = m.zeroed(&s.e, n);
  return rc;
}
int held(const Group& s) { return (s.a != nullptr) + (s.b != nullptr) + (s.c != nullptr) + (s.d != nullptr) + (s.e != nullptr); }
int dangling(const Group& s) { return dangling(s.a) + dangling(s.b) + dangling(s.c) + dangling(s.d) + dangling(s.e); }

void report(const char* step, const DeviceBuffers& m) {
  printf("%s owner_live=%d owner_bytes=%llu alloc_live=%zu alloc_bytes=%zu allocs=%d frees=%zu max_freed=%d bad_frees=%d\n", step,
         m.live(), m.bytes(), g.live.size(), live_bytes(), g.allocs, g.freed.size(), max_freed(), g.bad_frees);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  const int k = argc > 2 ? atoi(argv[2]) : 0;
  DeviceBuffers m(count_alloc, count_free);
  if (what == "mix") {   // fixed and grow-only allocations side by side, then free everything
    int* a = nullptr; double* b = nullptr; char* none = reinterpret_cast<char*>(8); double* g1 = nullptr; char* g2 = nullptr;
    size_t c1 = 0, c2 = 0;
    int rc = m.zeroed(&a, 10);
    rc |= m.raw(&b, 5); rc |= m.zeroed(&none, 0); rc |= m.grow(&g1, &c1, 100); rc |= m.grow(&g2, &c2, 7); rc |= m.grow(&g1, &c1, 300);
    printf("allocated rc=%d none_null=%d zero_flags=", rc, none == nullptr);
    for (int z : g.zero_flags) printf("%d", z);
    printf(" c1=%zu c2=%zu\n", c1, c2);
    report("before", m);
    m.free_all();
    report("after", m);
    m.free_all();   // (and the destructor after it: nothing is left to free twice)
    report("again", m);
  } else if (what == "grow") {
    double* p = nullptr; size_t cap = 0;
    int rc = m.grow(&p, &cap, 64);
    double* p1 = p; const int allocs1 = g.allocs;
    rc |= m.grow(&p, &cap, 32); rc |= m.grow(&p, &cap, 64);
    printf("within rc=%d same=%d new_allocs=%d cap=%zu frees=%zu\n", rc, p == p1, g.allocs - allocs1, cap, g.freed.size());
    rc = m.grow(&p, &cap, 65);
    printf("beyond rc=%d same=%d new_allocs=%d cap=%zu old_freed=%d bytes=%llu\n", rc, p == p1, g.allocs - allocs1, cap, g.freed[p1], m.bytes());
    report("end", m);
  } else if (what == "grow_fail") {
    double* p = nullptr; size_t cap = 0;
    int rc = m.grow(&p, &cap, 10);
    double* p1 = p;
    fail_next(1);
    rc = m.grow(&p, &cap, 20);
    printf("failed rc=%d null=%d cap=%zu old_freed=%d\n", rc, p == nullptr, cap, g.freed[p1]);
    report("failed_state", m);
    rc = m.grow(&p, &cap, 20);
    printf("retry rc=%d null=%d cap=%zu\n", rc, p == nullptr, cap);
    report("end", m);
  } else if (what == "group") {   // re-size a group of five with the k-th allocation failing
    for (int repeat = 0; repeat < 2; ++repeat) {   // 0: free everything right after the failure; 1: re-size again first
      DeviceBuffers o(count_alloc, count_free);
      Group s;
      int rc = resize(o, s, 16);
      fail_next(k);
      rc = resize(o, s, 40);
      printf("failed%d rc=%d held=%d dangling=%d\n", repeat, rc, held(s), dangling(s));
      report(repeat ? "failed_state1" : "failed_state0", o);
      if (repeat) {
        rc = resize(o, s, 40);
        printf("retry rc=%d held=%d dangling=%d\n", rc, held(s), dangling(s));
        report("retry_state", o);
      }
      o.free_all();
      report(repeat ? "freed1" : "freed0", o);
    }
  } else if (what == "release") {
    Group s; double* lone = nullptr;
    m.release(&lone, &s.a);
    report("null_release", m);
    int rc = resize(m, s, 16);
    report("once", m);
    rc |= resize(m, s, 16); rc |= resize(m, s, 16);
    printf("thrice rc=%d held=%d dangling=%d\n", rc, held(s), dangling(s));
    report("thrice_state", m);
    int* old = s.a;
    rc = m.zeroed(&s.a, 16);
    printf("refill rc=%d same=%d old_freed=%d\n", rc, s.a == old, g.freed[old]);
    report("refill_state", m);
  } else {
    fprintf(stderr, "usage: driver mix | grow | grow_fail | group K | release\n");
    return 2;
  }
  return 0;
}
