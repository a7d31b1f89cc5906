// The host mirrors of the out-of-state feature pool (xivo_hip_pool_*): who is live and who is linked, as the device has it, so
// that the entry points can refuse a bad record or edit before anything is launched ("Host files"). Host-only, plain
// C++17, no HIP: the device blocks and the kernels stay with the pool, tests/pool_mirror_driver.cpp drives this header alone.
//
// Two arrays per context:
//   entry  [Bmax][pool_max]    the anchor of a live entry, -1: the entry is free
//   link   [Bmax][anchor_max]  the group slot an anchor is linked to, -1: unlinked, -2: the anchor was never created
// What the type keeps true: every index is checked here (a query on an index out of range answers false / free), and the
// transitions of one Edit either all stay (commit) or the arrays are bit for bit what they were (its destructor).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace xivo_hip::capi {

class PoolMirror {
 public:
  // every entry free, no anchor created (Bmax = 0: no pool)
  void configure(int Bmax, int pool_max, int anchor_max) {
    B_ = Bmax; pm_ = pool_max; am_ = anchor_max;
    entry_.assign((size_t)Bmax * pool_max, -1);
    link_.assign((size_t)Bmax * anchor_max, -2);
  }
  int pool_max() const { return pm_; }
  int anchor_max() const { return am_; }
  // no live entry and no anchor created: what a device life cycle needs of the pool it takes over
  bool empty() const {
    for (int v : entry_) if (v != -1) return false;
    for (int v : link_) if (v != -2) return false;
    return true;
  }

  bool entry_in_range(int b, int e) const { return b >= 0 && b < B_ && e >= 0 && e < pm_; }
  bool anchor_in_range(int b, int a) const { return b >= 0 && b < B_ && a >= 0 && a < am_; }
  int entry_anchor(int b, int e) const { return entry_in_range(b, e) ? entry_[ie(b, e)] : -1; }        // -1: free
  int anchor_link(int b, int a) const { return anchor_in_range(b, a) ? link_[ia(b, a)] : -2; }
  bool anchor_exists(int b, int a) const { return anchor_link(b, a) != -2; }
  bool anchor_linked(int b, int a) const { return anchor_link(b, a) >= 0; }
  // some anchor of filter b is linked to group slot `slot`
  bool slot_linked(int b, int slot) const {
    for (int k = 0; b >= 0 && b < B_ && k < am_; ++k) if (link_[ia(b, k)] == slot) return true;
    return false;
  }
  // XIVO_EDIT_ADD_GROUP_ANCHOR: the anchor exists unlinked and no anchor of the filter holds the slot yet
  bool can_anchor_group(int b, int slot, int a) const { return anchor_link(b, a) == -1 && !slot_linked(b, slot); }
  // XIVO_EDIT_ADMIT_POOL: the entry is live and its anchor is linked to a group slot
  bool can_admit(int b, int e) const { const int a = entry_anchor(b, e); return a >= 0 && anchor_linked(b, a); }

  // xivo_hip_pool_anchor took the pose of anchor a (again): it exists, unlinked
  void anchor_created(int b, int a) { set(link_[ia(b, a)], -1); }
  // xivo_hip_pool_add wrote entry e on anchor a
  void entry_added(int b, int e, int a) { set(entry_[ie(b, e)], a); }
  // a step left live [B][pool_max]: the entries of filters [0, B) it found dead are free
  void entries_dead(const unsigned char* live, int B) {
    for (size_t i = 0; i < (size_t)B * pm_; ++i) if (!live[i]) set(entry_[i], -1);
  }
  // the mirrors as the device has them: the pool [Bmax][pool_max] (ref_sind: the anchor), the anchors [Bmax][anchor_max] (slot)
  // and the device life cycle's anc_used [Bmax][anchor_max]
  template <class Entry, class Anchor> void reread(const Entry* ent, const Anchor* anc, const int* used) {
    for (size_t i = 0; i < entry_.size(); ++i) entry_[i] = ent[i].ref_sind >= 0 && ent[i].ref_sind < am_ ? ent[i].ref_sind : -1;
    for (size_t i = 0; i < link_.size(); ++i) link_[i] = !used[i] ? -2 : (anc[i].slot >= 0 ? anc[i].slot : -1);
  }

  // The transitions of one xivo_hip_edit_batch call, in the order of its ops (an op may rely on a link an earlier op of the call
  // made). Unless commit() is reached the mirrors are put back exactly.
  class Edit {
   public:
    explicit Edit(PoolMirror& m) : m_(m) { m_.journal_.clear(); m_.journal_on_ = true; }
    ~Edit() {
      for (size_t k = m_.journal_.size(); k-- > 0;) *m_.journal_[k].first = m_.journal_[k].second;
      close();
    }
    Edit(const Edit&) = delete;
    Edit& operator=(const Edit&) = delete;
    void commit() { close(); }
    void group_anchored(int b, int slot, int a) { m_.set(m_.link_[m_.ia(b, a)], slot); }   // (after can_anchor_group)
    void group_removed(int b, int slot) {                                                  // every link to that slot
      for (int k = 0; b >= 0 && b < m_.B_ && k < m_.am_; ++k) if (m_.link_[m_.ia(b, k)] == slot) m_.set(m_.link_[m_.ia(b, k)], -1);
    }
    void entry_admitted(int b, int e) { m_.set(m_.entry_[m_.ie(b, e)], -1); }              // (after can_admit)
   private:
    void close() { m_.journal_.clear(); m_.journal_on_ = false; }
    PoolMirror& m_;
  };

 private:
  size_t ie(int b, int e) const { return (size_t)b * pm_ + e; }
  size_t ia(int b, int a) const { return (size_t)b * am_ + a; }
  void set(int& cell, int v) { if (journal_on_) journal_.emplace_back(&cell, cell); cell = v; }

  int B_ = 0, pm_ = 0, am_ = 0;
  std::vector<int> entry_, link_;
  std::vector<std::pair<int*, int>> journal_;   // of the open Edit: cell, value before
  bool journal_on_ = false;
};

}  // namespace xivo_hip::capi
