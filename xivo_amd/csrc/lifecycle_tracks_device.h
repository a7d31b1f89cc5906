// Where the frame's tracks of one filter lie in the track block of the device life cycles (LifeArgs, ekf_kernels.h): the only
// place that tells the packed form (behind offsets, as the host uploads them) from the strided one (one row per filter with a
// count, as pcw_tracks_kernel leaves them). lifecycle_kernels.hip and pool_lifecycle_kernels.hip read the tracks through
// these two accessors alone.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"

namespace xivo_hip {

// where filter b's tracks start and how many there are, in either form of the track block (ekf_kernels.h)
__device__ __forceinline__ int life_track_begin(const LifeArgs& a, int b) { return a.cnt ? b * a.track_ld : a.off[b]; }
__device__ __forceinline__ int life_track_count(const LifeArgs& a, int b) {
  return min(a.cnt ? a.cnt[b] : a.off[b + 1] - a.off[b], XIVO_LIFE_MAX_TRACKS);
}

}  // namespace xivo_hip
