// The trajectory producer on the device (gfx950): what BatchTrajectorySim.meas / .gsb (xivo_amd/pcw.py) and ImuFeeder.imu
// (xivo_amd/sequence.py) compute on the host between two camera frames - the feeder's records of samples k0 + 1 .. k0 + n of
// every filter, in the layout xivo_hip_propagate takes, and the ground truth at t_{k0 + n}: the camera pose the track producer
// reads and the body pose of the ground-truth log. The rules and the arithmetic are the functions of trajsim_device.h.
//
// One thread per item, items = B x (n + 1): item j < n of a filter is record k0 + 1 + j, item n its two poses. A record needs
// the measurements at k - 1 and at k; each thread evaluates BOTH itself (a few dozen transcendentals each) instead of sharing one
// evaluation with its neighbour through LDS: the kernel is launch bound at every size it is used at, a filter's items may
// straddle workgroups, and this way a value's bits do not depend on the launch shape. Nothing crosses threads, let alone
// workgroups; no LDS, no atomics, plain vector stores only.
#include "ekf_kernels.h"
#include "trajsim_device.h"

namespace xivo_hip {

static_assert(sizeof(TrajsimRecord) == sizeof(xivo_imu_in), "TrajsimRecord restates xivo_imu_in");

namespace {

constexpr int kTrajsimThreads = 256;

__global__ __launch_bounds__(kTrajsimThreads) void trajsim_frame_kernel(TrajsimArgs a) {
  const long per = (long)a.n + 1;
  const long item = (long)blockIdx.x * kTrajsimThreads + threadIdx.x;
  if (item >= (long)a.batch * per) return;
  const int b = (int)(item / per), j = (int)(item % per);
  const int motion = a.motion[b];
  const double rate = a.rate[b];
  if (j < a.n) {
    TrajsimRecord r;
    trajsim_record(a.m, motion, rate, b, a.k0 + 1ull + (unsigned long long)j, &r);
    TrajsimRecord* out = reinterpret_cast<TrajsimRecord*>(a.recs) + (long)b * a.n + j;   // < batch * n <= Bmax * n_max records
    *out = r;
  } else {
    double gt[12], gsc[12];
    trajsim_truth(a.m, motion, rate, a.k0 + (unsigned long long)a.n, gt, gsc);
    for (int i = 0; i < 12; ++i) { a.gsc[(long)b * 12 + i] = gsc[i]; a.gt[(long)b * 12 + i] = gt[i]; }
  }
}

}  // namespace

int launch_trajsim_frame(const TrajsimArgs& a, hipStream_t s) {
  const long items = (long)a.batch * ((long)a.n + 1);
  const long blocks = (items + kTrajsimThreads - 1) / kTrajsimThreads;
  if (items <= 0 || blocks > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(trajsim_frame_kernel, dim3((unsigned)blocks), dim3(kTrajsimThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace xivo_hip
