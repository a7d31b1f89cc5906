// C ABI, trajectory score (include/xivo_hip.h, "trajectory score"): aligned / unaligned ATE and RPE of a slice of the trajectory
// log against ground truth, one record per filter. Host orchestration only - the kernel is in score_kernels.hip. The arguments
// are checked before the device is touched.
#include <stdint.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// what a filter without a used frame gets (the kernel writes the same for n_used = 0)
xivo_traj_score empty_score() {
  xivo_traj_score o{};
  o.ate = o.ate_raw = o.rpe_pos = o.rpe_rot = -1.0;
  o.R[0] = o.R[4] = o.R[8] = 1.0;
  o.flags = XIVO_TRAJ_SCORE_UNDETERMINED;
  return o;
}

}  // namespace

extern "C" {

int xivo_hip_traj_score(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, const double* gt, const xivo_traj_score_opts* o,
                        xivo_traj_score* out) {
  if (!c || !gt || !o || !out || o->rpe_lag < 0) return XIVO_HIP_ERR_INVALID;
  if (bad_slice(c, c->traj.log, b0, nb, t0, nt)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (nt == 0) {
    for (int b = 0; b < nb; ++b) out[b] = empty_score();
    return XIVO_HIP_OK;
  }
  // one wave of 64 lanes per filter, and a launch holds fewer than 2^32 threads. A guard on the launch shape, stated where the
  // other refusals are: bad_range has bounded nb by batch_max, so only a context of 2^26 filters could get here.
  // launch_traj_score checks its own arguments again, as every launch helper does - it does not know who calls it.
  if ((long long)nb * 64 > 0xffffffffLL) return XIVO_HIP_ERR_UNSUPPORTED;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // per-call staging (the trajectory log's, shared with xivo_hip_traj_nees): gt in | nb records out
  const size_t n_gt = (size_t)nt * nb * 12 * sizeof(double), bytes = n_gt + (size_t)nb * sizeof(xivo_traj_score);
  int rc = c->mem.grow(&c->traj.io, &c->traj.io_cap, bytes);
  if (rc) return rc;
  TrajScoreArgs a{};
  a.rec = c->traj.rec; a.Bmax = c->Bmax; a.b0 = b0; a.nb = nb; a.t0 = t0; a.nt = nt;
  a.align = o->align != 0; a.rpe_lag = o->rpe_lag;
  a.gt = reinterpret_cast<const double*>(c->traj.io);
  a.out = reinterpret_cast<xivo_traj_score*>(c->traj.io + n_gt);
  HIP_TRY(hipMemcpyAsync(c->traj.io, gt, n_gt, hipMemcpyHostToDevice, c->stream));
  {
    StageTimer st(c, ST_OTHER, 0.0, "traj_score_kernel", 4.0 * nt * (double)nb * 2.0 * 96.0);
    if (launch_traj_score(a, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  HIP_TRY(hipMemcpyAsync(out, a.out, (size_t)nb * sizeof(xivo_traj_score), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

}  // extern "C"
