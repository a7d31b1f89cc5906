// The host bookkeeping of one per-frame device log (trajectory, landmark, innovation, the trajectory producer's ground truth):
// how many frames it holds, how many are written, their time stamps, and which slices of it may be read ("Host
// files"). Host-only, plain C++17, no HIP: the device blocks, the options and the kernels stay with each log,
// tests/frame_log_driver.cpp drives this header alone.
//
// A log is frame-major: frame t holds one entry per filter of the context, [capacity][Bmax] entries in all. What the type keeps
// true:
//   0 <= count <= capacity, and stamps.size() == count; capacity 0 means "not configured" (nothing can be committed).
//   A refused call (commit on a full log, a bad slice) changes nothing.
// The ground-truth log has no stamps: it commits a stamp nobody reads rather than making them an optional part of the type.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace xivo_hip::capi {

class FrameLog {
 public:
  // empty the log and give it room for T_max frames (0: not configured)
  void configure(int T_max) { T_ = T_max; reset(); }
  void reset() { n_ = 0; ts_.clear(); }   // (the capacity stays)

  bool configured() const { return T_ > 0; }
  bool full() const { return n_ >= T_; }
  int capacity() const { return T_; }
  int count() const { return n_; }

  // frame `count` is written: returns its index, or -1 from a full log
  int commit(long long ts_ns) { if (full()) return -1; ts_.push_back(ts_ns); return n_++; }

  // frames [t0, t0 + nt) are written ones (an empty slice is fine, at either end); no sum that could overflow
  bool slice_ok(int t0, int nt) const { return !(t0 < 0 || nt < 0 || t0 > n_ || nt > n_ - t0); }
  // the stamps of a slice that slice_ok accepts (ts null: nothing to do)
  void stamps(int t0, int nt, long long* ts) const { for (int t = 0; ts && t < nt; ++t) ts[t] = ts_[(size_t)t0 + t]; }

  // element offset of filter b0 of frame t
  static size_t at(int t, int Bmax, int b0) { return (size_t)t * (size_t)Bmax + (size_t)b0; }
  // sizing: *entries = T_max * Bmax (two ints: no overflow in 64 bits); false when that many entries of `per` bytes do not fit the
  // 63 bits an element offset is held in
  static bool fits(int T_max, int Bmax, size_t per, size_t* entries) {
    *entries = (size_t)T_max * (size_t)Bmax;
    return *entries <= (size_t)INT64_MAX / per;
  }

 private:
  int T_ = 0, n_ = 0;
  std::vector<long long> ts_;
};

}  // namespace xivo_hip::capi
