// C ABI, trajectory producer (include/xivo_hip.h, "trajectory producer"): the simulated IMU records and ground-truth poses of a
// camera frame produced on the device, the ground-truth log, and the propagation over the resident records. Host
// orchestration only - the kernel is in trajsim_kernels.hip, its rules in trajsim_device.h. The frame calls check their
// arguments before they touch the device, allocate nothing and do not synchronise the stream.
//
// The camera poses stay in the module's own block whether or not worlds are configured: xivo_hip_pcw_tracks_resident
// (capi_pcw.hip) hands that block to the track kernel, so the two modules share no buffer and neither has to know when the other
// is re-configured.
#include <math.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

void trajsim_release(xivo_hip_ctx* c) {
  c->mem.release(&c->trajsim.motion, &c->trajsim.rate, &c->trajsim.recs, &c->trajsim.gsc, &c->trajsim.gt, &c->trajsim.Q);
  c->trajsim = TrajSim{};
}

bool trajsim_ready(const xivo_hip_ctx* c) { return c && c->trajsim.configured() && c->trajsim.opts.n_max > 0; }

bool opts_ok(const xivo_trajsim_opts* o) {
  if (o->T_max <= 0 || !(o->imu_dt > 0.0) || !(o->noise_accel >= 0.0) || !(o->noise_gyro >= 0.0)) return false;
  const double* blocks[] = {&o->imu_dt, &o->rot_amp, o->rot_w, &o->noise_accel, &o->noise_gyro, o->grav_s, o->Rbc, o->Tbc};
  const int len[] = {1, 1, 3, 1, 1, 3, 9, 3};
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < len[i]; ++j) if (!isfinite(blocks[i][j])) return false;
  return true;
}

TrajsimModel model_of(const xivo_trajsim_opts& o) {
  TrajsimModel m{};
  m.imu_dt = o.imu_dt; m.rot_amp = o.rot_amp; m.noise_accel = o.noise_accel; m.noise_gyro = o.noise_gyro; m.seed = o.seed;
  for (int i = 0; i < 3; ++i) { m.rot_w[i] = o.rot_w[i]; m.grav_s[i] = o.grav_s[i]; m.Tbc[i] = o.Tbc[i]; }
  for (int i = 0; i < 9; ++i) m.Rbc[i] = o.Rbc[i];
  return m;
}

}  // namespace

extern "C" {

int xivo_hip_trajsim_config(xivo_hip_ctx* c, const xivo_trajsim_opts* o) {
  if (!c || !o || o->struct_size != (int)sizeof(xivo_trajsim_opts) || o->n_max < 0) return XIVO_HIP_ERR_INVALID;
  if (o->n_max > 0 && !opts_ok(o)) return XIVO_HIP_ERR_INVALID;
  if (track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;   // an open frame's tracks came from the poses given back here
  const size_t B = (size_t)c->Bmax;
  // (sizes in bytes stay far below 2^63: Bmax, n_max, T_max are ints; the products below are taken in size_t)
  if (o->n_max > 0 && (B * (size_t)o->n_max > ((size_t)1 << 40) / sizeof(xivo_imu_in) || B * (size_t)o->T_max > ((size_t)1 << 40) / 96))
    return XIVO_HIP_ERR_INVALID;
  if (o->n_max > 0 && c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipStreamSynchronize(c->stream));   // a frame call may still be using the blocks given back here
  trajsim_release(c);
  if (o->n_max == 0) return XIVO_HIP_OK;
  int rc = c->mem.zeroed(&c->trajsim.motion, B);              // Lissajous
  if (!rc) rc = c->mem.zeroed(&c->trajsim.rate, B);            // rate 0: stationary
  if (!rc) rc = c->mem.zeroed(&c->trajsim.recs, B * (size_t)o->n_max);
  if (!rc) rc = c->mem.zeroed(&c->trajsim.gsc, B * 12);
  if (!rc) rc = c->mem.zeroed(&c->trajsim.gt, B * 12 * (size_t)o->T_max);
  if (!rc) rc = c->mem.zeroed(&c->trajsim.Q, (size_t)144 + 529);
  if (!rc) rc = ensure_staging(c, 2 * (size_t)529 * B);   // Phi | P_mm of xivo_hip_propagate_resident, at their final size
  if (rc) { trajsim_release(c); return rc; }
  c->trajsim.opts = *o; c->trajsim.log.configure(o->T_max);
  return XIVO_HIP_OK;
}

int xivo_hip_trajsim_set(xivo_hip_ctx* c, int b0, int nb, const int* motion, const double* rate) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !trajsim_ready(c) || track_block_frame_open(c) || (nb > 0 && (!motion || !rate))) return XIVO_HIP_ERR_INVALID;
  for (int b = 0; b < nb; ++b)
    if ((motion[b] != 0 && motion[b] != 1) || !isfinite(rate[b])) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(c->trajsim.motion + b0, motion, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->trajsim.rate + b0, rate, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // pageable sources
  return XIVO_HIP_OK;
}

int xivo_hip_trajsim_frame(xivo_hip_ctx* c, int B, unsigned long long k0, int n) {
  if (!trajsim_ready(c) || B <= 0 || B > c->Bmax || n < 0 || n > c->trajsim.opts.n_max || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  if (c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
  // every record's dt must be positive and finite (xivo_hip_propagate's rule; xivo_hip_propagate_resident cannot read the
  // records): t_k stops resolving imu_dt far beyond any run's length, and a finite imu_dt times a large k can still leave the
  // finite range - the last time finite makes every t_k, so every dt_k, of the frame finite
  if (n > 0 && (k0 + (unsigned long long)n < k0 || !(trajsim_dt(k0 + 1, c->trajsim.opts.imu_dt) > 0.0) ||
                !(trajsim_dt(k0 + (unsigned long long)n, c->trajsim.opts.imu_dt) > 0.0) ||
                !std::isfinite(trajsim_time(k0 + (unsigned long long)n, c->trajsim.opts.imu_dt))))
    return XIVO_HIP_ERR_INVALID;
  if (c->trajsim.log.full()) return XIVO_HIP_ERR_FULL;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  TrajsimArgs a{};
  a.m = model_of(c->trajsim.opts); a.motion = c->trajsim.motion; a.rate = c->trajsim.rate; a.k0 = k0; a.n = n; a.batch = B;
  a.recs = c->trajsim.recs; a.gsc = c->trajsim.gsc; a.gt = c->trajsim.gt + FrameLog::at(c->trajsim.log.count(), c->Bmax, 0) * 12;
  c->trajsim.B = 0; c->trajsim.fresh = false;   // (whatever the blocks held is being overwritten)
  {
    // per filter: n records of 104 bytes and two poses of 96 bytes out, curve and rate in
    StageTimer st(c, ST_OTHER, 0.0, "trajsim_frame_kernel", (double)B * (n * sizeof(xivo_imu_in) + 2.0 * 96.0 + 12.0));
    if (launch_trajsim_frame(a, c->stream)) return XIVO_HIP_ERR_HIP;
  }
  c->trajsim.B = B; c->trajsim.n = n; c->trajsim.fresh = n > 0; c->trajsim.log.commit(0);
  return XIVO_HIP_OK;
}

int xivo_hip_propagate_resident(xivo_hip_ctx* c, int B, const xivo_prop_opts* o) {
  if (!trajsim_ready(c) || !o || B <= 0 || B != c->trajsim.B || !c->trajsim.fresh) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c->trajsim.prop_valid || memcmp(c->trajsim.prop.Qimu, o->Qimu, sizeof(o->Qimu)) != 0 ||
      memcmp(c->trajsim.prop.Qmodel, o->Qmodel, sizeof(o->Qmodel)) != 0) {
    // the noise changed (or this is the first call): one synchronous upload - opts is borrowed, and propagations already
    // enqueued read the old values
    c->trajsim.prop_valid = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->trajsim.Q, o->Qimu, 144 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->trajsim.Q + 144, o->Qmodel, 529 * sizeof(double), hipMemcpyHostToDevice));
    c->trajsim.prop = *o; c->trajsim.prop_valid = true;
  }
  const int rc = propagate_device(c, B, c->trajsim.n, c->trajsim.recs, c->trajsim.Q, c->trajsim.Q + 144, o, c->trajsim.opts.imu_dt);
  if (rc) return rc;
  c->trajsim.fresh = false;
  return XIVO_HIP_OK;
}

int xivo_hip_trajsim_get(xivo_hip_ctx* c, int b0, int nb, xivo_imu_in* recs, double* gsc, int* n_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !trajsim_ready(c) || b0 + nb > c->trajsim.B) return XIVO_HIP_ERR_INVALID;
  if (n_out) *n_out = c->trajsim.n;
  if (nb == 0) return XIVO_HIP_OK;
  const size_t row = (size_t)c->trajsim.n * sizeof(xivo_imu_in);
  if (recs && row) {
    int rc = d2h_rows(c, recs, row, c->trajsim.recs + (size_t)b0 * c->trajsim.n, row, row, nb);
    if (rc) return rc;
  }
  if (gsc) {
    int rc = d2h_rows(c, gsc, 96, c->trajsim.gsc + (size_t)b0 * 12, 96, 96, nb);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_trajsim_get_gt(xivo_hip_ctx* c, int b0, int nb, int t0, int nt, double* gt) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || bad_slice(c, c->trajsim.log, b0, nb, t0, nt) || (nb > 0 && nt > 0 && !gt))
    return XIVO_HIP_ERR_INVALID;
  if (nb == 0 || nt == 0) return XIVO_HIP_OK;
  // frame t of the log is [Bmax][12]: nt rows of nb * 96 bytes, Bmax * 96 apart
  return d2h_rows(c, gt, (size_t)nb * 96, c->trajsim.gt + FrameLog::at(t0, c->Bmax, b0) * 12, (size_t)c->Bmax * 96, (size_t)nb * 96, nt);
}

int xivo_hip_trajsim_count(xivo_hip_ctx* c) { return trajsim_ready(c) ? c->trajsim.log.count() : 0; }

int xivo_hip_trajsim_reset(xivo_hip_ctx* c) {
  if (!trajsim_ready(c) || track_block_frame_open(c)) return XIVO_HIP_ERR_INVALID;
  c->trajsim.log.reset(); c->trajsim.B = 0; c->trajsim.n = 0; c->trajsim.fresh = false;
  return XIVO_HIP_OK;
}

}  // extern "C"
