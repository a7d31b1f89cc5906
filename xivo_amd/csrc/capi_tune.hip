// C ABI, tuning table (include/xivo_hip.h, "tuning table"): per-filter R, MH_thresh, var_xyz, Qimu and Qmodel as five resident
// arrays, their configuration, the staged set call and the read-back. Host orchestration only (capi_internal.h) - and no kernel
// of its own: the readers are the in-state gate (capi_glevel.hip: gate_impl), the stacking (stack_impl), propagation
// (capi_propagate.hip: prop_args) and xivo_hip_life_end, each of which hands its kernel the arrays while c->tune.configured().
#include <math.h>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// doubles per filter of the five arrays, in the order a staged block holds them: the largest leads, because
// PinnedUpload::enqueue uploads the block's leading bytes and records the block's event behind everything enqueued before it
constexpr size_t kQm = 529, kQi = 144, kVar = 3;
constexpr size_t kPer = kQm + kQi + kVar + 2;
static_assert(sizeof(xivo_tune_in) == kPer * sizeof(double), "xivo_tune_in is 678 doubles");

// what the scalar arguments would be refused for (bad_gate_params, xivo_hip_life_config), and a non-finite noise entry
bool tune_entry_bad(const xivo_tune_in& t) {
  if (!(t.R > 0.0) || !isfinite(t.R) || !(t.mh_thresh > 0.0) || !isfinite(t.mh_thresh)) return true;
  for (int i = 0; i < 3; ++i) if (!(t.var_xyz[i] >= 0.0) || !isfinite(t.var_xyz[i])) return true;
  for (size_t i = 0; i < kQi; ++i) if (!isfinite(t.Qimu[i])) return true;
  for (size_t i = 0; i < kQm; ++i) if (!isfinite(t.Qmodel[i])) return true;
  return false;
}

void tune_release(xivo_hip_ctx* c) {
  TuneTable& t = c->tune;
  c->mem.release(&t.R, &t.thresh, &t.var, &t.Qimu, &t.Qmodel);
  t.up.release();
}

// rows [b0, b0 + nb) <- entry(i), i < nb: field by field into the staging block the last call did not use, five uploads
template <class Entry> int tune_upload(xivo_hip_ctx* c, int b0, int nb, Entry entry) {
  TuneTable& t = c->tune;
  char* hb = nullptr;
  if (int rc = t.up.stage(&hb)) return rc;
  const size_t n = (size_t)nb;
  double* hQm = reinterpret_cast<double*>(hb); double* hQi = hQm + kQm * n; double* hVar = hQi + kQi * n;
  double* hR = hVar + kVar * n; double* hTh = hR + n;
  for (size_t i = 0; i < n; ++i) {
    const xivo_tune_in& e = entry(i);
    memcpy(hQm + kQm * i, e.Qmodel, kQm * sizeof(double));
    memcpy(hQi + kQi * i, e.Qimu, kQi * sizeof(double));
    memcpy(hVar + kVar * i, e.var_xyz, kVar * sizeof(double));
    hR[i] = e.R; hTh[i] = e.mh_thresh;
  }
  HIP_TRY(hipMemcpyAsync(t.Qimu + kQi * b0, hQi, kQi * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t.var + kVar * b0, hVar, kVar * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t.R + b0, hR, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t.thresh + b0, hTh, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return t.up.enqueue(t.Qmodel + kQm * b0, kQm * n * sizeof(double), c->stream);
}

}  // namespace

extern "C" {

int xivo_hip_tune_config(xivo_hip_ctx* c, const xivo_tune_in* all) {
  if (!c) return XIVO_HIP_ERR_INVALID;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!all) {
    if (!c->tune.configured()) return XIVO_HIP_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));   // a call enqueued earlier may still be reading the table
    tune_release(c);
    return XIVO_HIP_OK;
  }
  if (tune_entry_bad(*all)) return XIVO_HIP_ERR_INVALID;
  if (c->calib_on || c->calib_motion) return XIVO_HIP_ERR_UNSUPPORTED;
  TuneTable& t = c->tune;
  if (!t.configured()) {
    const size_t B = (size_t)c->Bmax;
    int rc = t.up.alloc(kPer * B * sizeof(double));
    if (!rc) rc = c->mem.raw(&t.thresh, B);
    if (!rc) rc = c->mem.raw(&t.var, kVar * B);
    if (!rc) rc = c->mem.raw(&t.Qimu, kQi * B);
    if (!rc) rc = c->mem.raw(&t.Qmodel, kQm * B);
    if (!rc) rc = c->mem.raw(&t.R, B);   // (last: configured() reads it)
    if (rc) { tune_release(c); return rc; }
  }
  const int rc = tune_upload(c, 0, c->Bmax, [&](size_t) -> const xivo_tune_in& { return *all; });
  if (rc) { (void)hipStreamSynchronize(c->stream); tune_release(c); }
  return rc;
}

int xivo_hip_tune_set(xivo_hip_ctx* c, int b0, int nb, const xivo_tune_in* t) {
  if (bad_range(c, b0, nb) || !c->tune.configured() || (nb > 0 && !t)) return XIVO_HIP_ERR_INVALID;
  for (int i = 0; i < nb; ++i) if (tune_entry_bad(t[i])) return XIVO_HIP_ERR_INVALID;   // every row before any is staged
  if (nb == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  return tune_upload(c, b0, nb, [&](size_t i) -> const xivo_tune_in& { return t[i]; });
}

int xivo_hip_tune_get(xivo_hip_ctx* c, int b0, int nb, xivo_tune_in* out) {
  if (bad_range(c, b0, nb) || !c->tune.configured() || (nb > 0 && !out)) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const TuneTable& t = c->tune;
  const size_t n = (size_t)nb;
  std::vector<double> h(kPer * n);
  double* hQm = h.data(); double* hQi = hQm + kQm * n; double* hVar = hQi + kQi * n; double* hR = hVar + kVar * n; double* hTh = hR + n;
  HIP_TRY(hipMemcpyAsync(hQm, t.Qmodel + kQm * b0, kQm * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hQi, t.Qimu + kQi * b0, kQi * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hVar, t.var + kVar * b0, kVar * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hR, t.R + b0, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hTh, t.thresh + b0, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i) {
    xivo_tune_in& e = out[i];
    e.R = hR[i]; e.mh_thresh = hTh[i];
    memcpy(e.var_xyz, hVar + kVar * i, kVar * sizeof(double));
    memcpy(e.Qimu, hQi + kQi * i, kQi * sizeof(double));
    memcpy(e.Qmodel, hQm + kQm * i, kQm * sizeof(double));
  }
  return XIVO_HIP_OK;
}

}  // extern "C"
