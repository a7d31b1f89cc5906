// The device memory of one context, under ONE owner: every block the host code of the C ABI allocates for a context is handed
// out here and recorded, so destroying the context frees what was allocated and not a hand-kept list of pointers (DESIGN.md,
// "Host files"). Host-only, plain C++17, no HIP: the allocate and free calls come in as two function pointers
// (capi.hip passes hipMalloc / hipFree), tests/device_buffers_driver.cpp passes a counting allocator.
//
// A slot is the pointer variable of the caller (a field of xivo_hip_ctx). What the owner keeps true for every slot it is given:
//   the slot is null, or it points to a block the owner holds - never to a freed block, whichever call failed.
// Three ways to fill a slot:
//   zeroed / raw   a block of fixed size, filled with zero bytes or left as the allocator returns it
//   grow           a buffer that only ever grows, with its capacity next to it; never filled (per-call staging)
//   release        give slots back; the "drop a group and re-allocate it" sites are a release followed by zeroed / raw
#pragma once
#include <cstddef>
#include <vector>

namespace xivo_hip::capi {

class DeviceBuffers {
 public:
  // *p = a block of `bytes` bytes, zero-filled when `zero`; returns 0, or the status to hand to the caller with *p = nullptr
  using AllocFn = int (*)(void** p, size_t bytes, int zero);
  using FreeFn = void (*)(void* p);

  DeviceBuffers(AllocFn alloc, FreeFn free) : alloc_(alloc), free_(free) {}
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  ~DeviceBuffers() { free_all(); }

  // n elements of T behind *slot; a block the slot still holds is released first (n = 0: the slot stays null, which is no error)
  template <class T> int zeroed(T** slot, size_t n) { return take(reinterpret_cast<void**>(slot), n * sizeof(T), 1); }
  template <class T> int raw(T** slot, size_t n) { return take(reinterpret_cast<void**>(slot), n * sizeof(T), 0); }

  // at least n elements behind *slot, *cap the elements it holds. Enough already: nothing happens, same pointer. Else the old
  // block is freed, the slot left null with capacity 0, and a block of exactly n elements allocated (its content is undefined);
  // if that fails the slot stays null with capacity 0 and the next call tries again.
  template <class T> int grow(T** slot, size_t* cap, size_t n) {
    if (n <= *cap) return 0;
    *cap = 0;   // (raw releases the old block and leaves the slot null if it fails)
    const int rc = raw(slot, n);
    if (rc == 0) *cap = n;
    return rc;
  }

  // free the blocks behind these slots and null them (a null slot: nothing to do)
  template <class... T> void release(T**... slot) { (drop(reinterpret_cast<void**>(slot)), ...); }

  // every block the owner holds, each exactly once; the slots of the caller are NOT visited (the context goes away with them)
  void free_all() {
    for (const Block& b : blocks_) free_(b.p);
    blocks_.clear();
  }

  int live() const { return (int)blocks_.size(); }
  unsigned long long bytes() const {
    unsigned long long s = 0;
    for (const Block& b : blocks_) s += b.bytes;
    return s;
  }

 private:
  struct Block { void* p; size_t bytes; };

  int take(void** slot, size_t bytes, int zero) {
    drop(slot);
    if (bytes == 0) return 0;
    void* p = nullptr;
    const int rc = alloc_(&p, bytes, zero);
    if (rc != 0 || !p) return rc != 0 ? rc : -1;
    blocks_.push_back(Block{p, bytes});
    *slot = p;
    return 0;
  }

  void drop(void** slot) {
    for (size_t i = 0; *slot && i < blocks_.size(); ++i) {
      if (blocks_[i].p != *slot) continue;
      free_(blocks_[i].p);
      blocks_[i] = blocks_.back();
      blocks_.pop_back();
      break;
    }
    *slot = nullptr;
  }

  AllocFn alloc_;
  FreeFn free_;
  std::vector<Block> blocks_;
};

}  // namespace xivo_hip::capi
