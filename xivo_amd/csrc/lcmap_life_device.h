// The rules of loop closure inside the device life cycle (xivo_hip_lcmap_life_config, include/xivo_hip.h): which slot of the
// in-state book yields an add record, which was tracked, which yields a query, and where a record or a query lies in its
// filter's list - what SequenceRunner._lc_add / _lc_close (xivo_amd/sequence.py) decide on the host. What becomes of a record
// or a query stays with lcmap_device.h. Plain functions of integers, shared by the kernels (lifecycle_kernels.hip,
// lcmap_kernels.hip) and by a host program that holds them against a restatement (tests/lcmap_life_driver.cpp): this file
// includes no project header and takes HIP's only under __HIPCC__.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LCLIFE_HD __host__ __device__ __forceinline__
#else
#define LCLIFE_HD inline
#endif

namespace xivo_hip {

// the key of a free slot, and of every track of a begin call that brings no keys: it matches nothing and adds nothing
LCLIFE_HD long long lclife_no_key() { return -1; }

// begin: a slot that holds a feature and was associated with no track of the frame (slot_track < 0) leaves - one add record
// {b, slot, feat_key[slot]}, whatever the key (a negative one is the add kernel's to skip and count)
LCLIFE_HD int lclife_leaves(long long feat_id, int slot_track) { return feat_id >= 0 && slot_track < 0; }
// begin: a slot that holds a feature and was associated with a track whose pixel is a number was tracked this frame
// (u_is_nan: the track's u; the host life cycle looks at u alone)
LCLIFE_HD int lclife_tracked(long long feat_id, int slot_track, int u_is_nan) { return feat_id >= 0 && slot_track >= 0 && !u_is_nan; }
// close: a slot that holds a feature, was tracked and is in the update's inlier mask yields one query {b, -1, feat_key[slot], xp}
LCLIFE_HD int lclife_queries(long long feat_id, int mask, int tracked) { return feat_id >= 0 && mask != 0 && tracked != 0; }
// Records and queries go in ascending slot order: the one with `rank` yielding slots before it takes position rank of its
// filter's row; the rows are `row` long (one position per feature slot: the worst case) and lie one behind the other, so no
// position depends on another filter's count
LCLIFE_HD long lclife_list_pos(int b, int row, int rank) { return (long)b * row + rank; }
// the part of a filter's row the consumers walk: its count, which is an address and not trusted beyond the row
LCLIFE_HD int lclife_list_count(int count, int row) { return count < 0 ? 0 : (count > row ? row : count); }

}  // namespace xivo_hip
