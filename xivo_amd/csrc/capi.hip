// C ABI of the MI355X EKF measurement-update path (include/xivo_hip.h): the context, P residency, resident device buffers,
// timing / profile, and the host helpers every part of the ABI shares (capi_internal.h). The update pipelines are in
// capi_update.hip, the feature level in capi_glevel.hip, the other areas in the files capi_internal.h lists. Host-side orchestration only:
// owns the device buffers of a batch of filters, sequences the kernels on one HIP stream, never throws and never aborts.
#include <new>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace xivo_hip::capi {

static int collect_profile(xivo_hip_ctx* c) {
  Profiler& p = c->prof;
  if (p.used == 0) return XIVO_HIP_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < p.used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.events[i].a, p.events[i].b) == hipSuccess) p.ms[p.events[i].stage] += ms;
  }
  p.used = 0;
  return XIVO_HIP_OK;
}

// the owner's allocator: the only hipMalloc / hipFree of a context's own memory
int device_alloc(void** p, size_t bytes, int zero) {
  *p = nullptr;
  if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return XIVO_HIP_ERR_NOMEM; }
  if (zero && hipMemset(*p, 0, bytes) != hipSuccess) { hipFree(*p); *p = nullptr; return XIVO_HIP_ERR_HIP; }
  return XIVO_HIP_OK;
}
void device_free(void* p) { hipFree(p); }

// ---- the double-buffered page-locked upload (the only page-locked blocks with an event each of the C ABI)
int PinnedUpload::alloc(size_t bytes) {
  int rc = XIVO_HIP_OK;
  for (int i = 0; i < 2 && !rc; ++i) {
    if (hipHostMalloc(reinterpret_cast<void**>(&pin[i]), bytes, hipHostMallocDefault) != hipSuccess) {
      pin[i] = nullptr; (void)hipGetLastError(); rc = XIVO_HIP_ERR_NOMEM;
    }
    if (!rc && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { ev[i] = nullptr; rc = XIVO_HIP_ERR_HIP; }
  }
  if (rc) release();
  return rc;
}
void PinnedUpload::release() {
  for (int i = 0; i < 2; ++i) {
    if (pin[i]) { hipHostFree(pin[i]); pin[i] = nullptr; }
    if (ev[i]) { hipEventDestroy(ev[i]); ev[i] = nullptr; }
  }
  cur = 0;
}
PinnedUpload& PinnedUpload::operator=(PinnedUpload&& o) noexcept {
  if (this != &o) {
    release();
    for (int i = 0; i < 2; ++i) { pin[i] = o.pin[i]; ev[i] = o.ev[i]; o.pin[i] = nullptr; o.ev[i] = nullptr; }
    cur = o.cur; o.cur = 0;
  }
  return *this;
}
int PinnedUpload::stage(char** h) {
  HIP_TRY(hipEventSynchronize(ev[cur ^ 1]));
  *h = pin[cur ^ 1];
  return XIVO_HIP_OK;
}
int PinnedUpload::enqueue(void* dev, size_t bytes, hipStream_t stream) {
  const int set = cur ^ 1;
  HIP_TRY(hipMemcpyAsync(dev, pin[set], bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(ev[set], stream));
  cur = set;
  return XIVO_HIP_OK;
}

MeasBuffers meas_buffers(xivo_hip_ctx* c, int b0) {
  MeasBuffers mb;
  c->H.from(b0).to(mb.H, mb.strideH, mb.ldh);
  c->HT.from(b0).to(mb.HT, mb.strideHT, mb.ldht);
  c->inn.from(b0).to(mb.inn, mb.strideInn);
  c->diagR.from(b0).to(mb.diagR, mb.strideR);
  return mb;
}

bool calib_sparse(const xivo_hip_ctx* c) {   // (XIVO_HIP_FLAG_DENSE_H keeps the round-4 dense stacking of these builds)
  return c->calib_on && c->Hlead.p && c->cl.cam_begin + 9 <= LEAD_K && c->Np >= LEAD_K &&
         !(c->flags & (XIVO_HIP_FLAG_DENSE_H | XIVO_HIP_FLAG_SYMMETRIC_FORM | XIVO_HIP_FLAG_STANDALONE_TAIL));
}

SceneBuffers scene_buffers(xivo_hip_ctx* c) {
  SceneBuffers sb;
  sb.poses = c->poses; sb.groups = c->groups; sb.feats = c->feats;
  sb.J = c->J; sb.finn = c->finn; sb.mask = c->mask; sb.dist = c->dist;
  sb.Fmax = c->Fmax; sb.F = c->F;
  sb.calib = c->calib_on ? c->calib : nullptr; sb.Jc = c->calib_on ? c->Jc : nullptr; sb.cl = c->cl;
  if (!c->calib_on) sb.cl = xivo_calib_layout{-1, -1, 0, 0};
  sb.invdepth = (c->flags & XIVO_HIP_FLAG_INVDEPTH) ? 1 : 0;
  return sb;
}

// Device -> host copy of `rows` rows of `width` bytes (device pitch dpitch, host pitch hpitch). hipMemcpy2D issues one
// small DMA per row - 13 ms for 2048 rows of 30 bytes - so short rows come over as one contiguous block and are
// repacked on the host. The block includes the gaps between the rows: right for the ground-truth log's 96-byte entries
// (capi_trajsim.hip), wrong for a few filters of the trajectory / landmark / innovation logs, whose frames are Bmax entries of up
// to kilobytes apart - those keep the strided copy (d2h_frames).
int d2h_rows(xivo_hip_ctx* c, void* dst, size_t hpitch, const void* src, size_t dpitch, size_t width, size_t rows) {
  if (rows == 0 || width == 0) return XIVO_HIP_OK;
  if (width == dpitch && width == hpitch) {
    HIP_TRY(hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return XIVO_HIP_OK;
  }
  const size_t span = dpitch * (rows - 1) + width;
  if (c->hstage.size() < span) c->hstage.resize(span);
  HIP_TRY(hipMemcpyAsync(c->hstage.data(), src, span, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t r = 0; r < rows; ++r) memcpy((char*)dst + r * hpitch, c->hstage.data() + r * dpitch, width);
  return XIVO_HIP_OK;
}

// Frame-major storage: the filters [b0, b0 + nb) of one frame are contiguous, frames are Bmax entries apart - one row per frame,
// as a strided copy (see d2h_rows for why not through it).
int d2h_frames(xivo_hip_ctx* c, void* dst, const void* src, size_t per, int b0, int nb, int t0, int nt) {
  if (!dst) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)nb * per, (const char*)src + FrameLog::at(t0, c->Bmax, b0) * per, (size_t)c->Bmax * per,
                           (size_t)nb * per, nt, hipMemcpyDeviceToHost, c->stream));
  return XIVO_HIP_OK;
}

int NeesStaging::up(xivo_hip_ctx* c, char** io, size_t* io_cap, size_t per, int nt_, int gt_w, int err_w_, const double* gt_h) {
  n = (size_t)nt_ * per; nt = (size_t)nt_; err_w = (size_t)err_w_;
  const size_t o_err = n * gt_w, o_nees = o_err + n * err_w, o_an = o_nees + n, dbl = o_an + nt;
  const int rc = c->mem.grow(io, io_cap, dbl * sizeof(double) + nt * sizeof(int));
  if (rc) return rc;
  gt = reinterpret_cast<double*>(*io);
  err = gt + o_err; nees = gt + o_nees; anees = gt + o_an; n_used = reinterpret_cast<int*>(gt + dbl);
  HIP_TRY(hipMemcpyAsync(gt, gt_h, n * gt_w * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return XIVO_HIP_OK;
}

int NeesStaging::down(xivo_hip_ctx* c, double* err_h, double* nees_h, double* anees_h, int* n_used_h) const {
  if (err_h) HIP_TRY(hipMemcpyAsync(err_h, err, n * err_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (nees_h) HIP_TRY(hipMemcpyAsync(nees_h, nees, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (anees_h) HIP_TRY(hipMemcpyAsync(anees_h, anees, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (n_used_h) HIP_TRY(hipMemcpyAsync(n_used_h, n_used, nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int ensure_staging(xivo_hip_ctx* c, size_t elems) {
  return c->mem.grow(&c->staging, &c->staging_elems, elems);
}

// copy nb host matrices (rows x cols, leading dim ld, `stride` elements apart)
// into a packed device staging area (ld = rows)
int h2d_packed(xivo_hip_ctx* c, double* dst, const double* src, int nb, int rows, int cols, long stride, int ld) {
  if (ld == rows) {
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)rows * cols * sizeof(double), src, (size_t)stride * sizeof(double),
                             (size_t)rows * cols * sizeof(double), nb, hipMemcpyHostToDevice, c->stream));
  } else {
    for (int b = 0; b < nb; ++b)
      HIP_TRY(hipMemcpy2DAsync(dst + (size_t)b * rows * cols, (size_t)rows * sizeof(double), src + (size_t)b * stride,
                               (size_t)ld * sizeof(double), (size_t)rows * sizeof(double), cols,
                               hipMemcpyHostToDevice, c->stream));
  }
  return XIVO_HIP_OK;
}

int d2h_packed(xivo_hip_ctx* c, double* dst, const double* src, int nb, int rows, int cols, long stride, int ld) {
  if (ld == rows) {
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)stride * sizeof(double), src, (size_t)rows * cols * sizeof(double),
                             (size_t)rows * cols * sizeof(double), nb, hipMemcpyDeviceToHost, c->stream));
  } else {
    for (int b = 0; b < nb; ++b)
      HIP_TRY(hipMemcpy2DAsync(dst + (size_t)b * stride, (size_t)ld * sizeof(double), src + (size_t)b * rows * cols,
                               (size_t)rows * sizeof(double), (size_t)rows * sizeof(double), cols,
                               hipMemcpyDeviceToHost, c->stream));
  }
  return XIVO_HIP_OK;
}

bool bad_range(xivo_hip_ctx* c, int b0, int nb) { return !c || b0 < 0 || nb < 0 || b0 + nb > c->Bmax; }

int gemm(xivo_hip_ctx* c, int stage, int B, int rows, int cols, const GemmProduct& seg, const BatchMat& C, const GemmExtra& x) {
  const double *A0 = seg.A.p, *B0 = seg.B.p, *A1 = x.seg1.A.p;
  const int K0 = seg.K, K1 = x.seg1.K;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.seg[0] = GemmSeg{A0, B0, x.scale0, seg.A.stride, seg.B.stride, 0, seg.A.ld, seg.B.ld, K0, x.a_f32, x.b_f32};
  g.nseg = 1;
  if (A1) {
    g.seg[1] = GemmSeg{A1, x.seg1.B.p, x.scale1.p, x.seg1.A.stride, x.seg1.B.stride, x.scale1.stride, x.seg1.A.ld, x.seg1.B.ld, K1, 0, 0};
    g.nseg = 2;
  }
  C.to(g.C, g.strideC, g.ldc); g.Mp = rows; g.Np = cols;
  x.C2.to(g.C2, g.strideC2, g.ldc2); g.c2_rows = x.c2_rows;
  x.diag.to(g.diag, g.strideDiag); x.msub.to(g.Msub, g.strideMsub, g.ldmsub);
  x.mcol.to(g.McolScale, g.strideMcol);
  g.epilogue = x.epi; g.lower_only = x.lower_only; g.no_mirror = x.no_mirror; g.batch = B; g.fp32 = x.fp32;
  g.skip_status = x.skip; g.small_tiles = x.small_tiles;
  // algorithmic flops of the product: a symmetric output needs its lower triangle only
  const double outs = x.lower_only ? 0.5 * rows * (cols + 1.0) : (double)rows * cols;
  const double flops = 2.0 * outs * (double)(K0 + (A1 ? K1 : 0)) * B;
  const bool sym = g.lower_only && rows == cols && gemm_sym_supported(rows) && !g.C2 && !g.fp32 &&
                   (g.epilogue == EPI_NONE || g.epilogue == EPI_ADD_DIAG);
  char label[64] = "gemm_sym_f64_kernel";
  if (!sym) gemm_kernel_label(g, label, sizeof(label));
  const double bytes = 8.0 * B * ((double)rows * K0 * (x.a_f32 ? 0.5 : 1.0) + (double)cols * K0 * (x.b_f32 ? 0.5 : 1.0) + (A1 ? ((double)rows + cols) * K1 : 0.0) +
                                  (x.msub.p ? outs : 0.0) + (double)rows * cols + (x.C2.p ? (double)rows * cols : 0.0))
                       - (A0 == B0 ? 8.0 * B * (double)cols * K0 : 0.0);   // a symmetric product reads its one operand once
  StageTimer st(c, stage, flops, label, bytes);
  const int rc = sym ? launch_gemm_sym_f64(g, c->stream) : launch_gemm_nt_f64(g, c->stream);
  if (rc != 0 && debug_on()) fprintf(stderr, "xivo_hip: gemm launch (%s) -> %s\n", label, hipGetErrorString((hipError_t)rc));
  return rc == 0 ? XIVO_HIP_OK : XIVO_HIP_ERR_HIP;
}

}  // namespace xivo_hip::capi

extern "C" {

const char* xivo_hip_strerror(int s) {
  switch (s) {
    case XIVO_HIP_OK: return "ok";
    case XIVO_HIP_ERR_INVALID: return "invalid argument";
    case XIVO_HIP_ERR_HIP: return "HIP runtime error";
    case XIVO_HIP_ERR_NOT_SPD: return "innovation covariance S is not positive definite";
    case XIVO_HIP_ERR_NOMEM: return "out of device memory";
    case XIVO_HIP_ERR_UNSUPPORTED: return "size not supported by the compiled kernels";
    case XIVO_HIP_ERR_FULL: return "the log is full (trajectory / landmark log)";
    default: return "unknown status";
  }
}

void xivo_hip_destroy(xivo_hip_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  c->mem.free_all();         // (the page-locked staging of the tracks and of the world's poses goes with its record: delete below)
  if (c->ell_flags_h) hipHostFree(c->ell_flags_h);
  if (c->pin_h) hipHostFree(c->pin_h);
  for (auto& ep : c->prof.events) { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
  if (c->prof.t0) hipEventDestroy(c->prof.t0);
  if (c->prof.t1) hipEventDestroy(c->prof.t1);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

int xivo_hip_create(xivo_hip_ctx** out, int device, int N, int M_max, int batch_max, unsigned flags) {
  if (!out || N <= 0 || M_max <= 0 || batch_max <= 0) return XIVO_HIP_ERR_INVALID;
  *out = nullptr;
  if (round_up16(M_max) / 16 > 24) return XIVO_HIP_ERR_UNSUPPORTED;  // trsm register budget
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return XIVO_HIP_ERR_HIP;
  HIP_TRY(hipSetDevice(device));
  xivo_hip_ctx* c = new (std::nothrow) xivo_hip_ctx();
  if (!c) return XIVO_HIP_ERR_NOMEM;
  c->device = device; c->N = N; c->Np = round_up16(N); c->Mmax = M_max; c->Mpmax = round_up16(M_max);
  c->Bmax = batch_max; c->flags = flags;
  if (const char* e = getenv("XIVO_HIP_CHUNK")) c->chunk = atoi(e);
  const size_t B = batch_max;
  const size_t Np = c->Np, Mp = c->Mpmax;
  int rc = XIVO_HIP_OK;
  auto A = [&](auto** p, size_t n) { if (rc == XIVO_HIP_OK) rc = c->mem.zeroed(p, n); };
  // a view gets its stride and leading dimension here, once, and B * stride elements behind it
  auto mat = [&](BatchMat& m, size_t rows, size_t cols, size_t stride = 0) {
    m.stride = (long)(stride ? stride : rows * cols); m.ld = (int)rows; A(&m.p, B * m.stride);
  };
  auto vec = [&](BatchVec& v, size_t n) { v.stride = (long)n; A(&v.p, B * n); };
  if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return XIVO_HIP_ERR_HIP; }
  mat(c->P, Np, Np); mat(c->H, Mp, Np); mat(c->HT, Np, Mp); mat(c->HP, Mp, Np); mat(c->PHT, Np, Mp);
  mat(c->S, Mp, Mp); mat(c->K, Np, Mp); mat(c->G, Np, Mp, Np > Mp ? Np * Np : Np * Mp); mat(c->T, Np, Np);
  c->KHI = BatchMat{c->G.p, c->P.stride, c->P.ld};
  vec(c->invD, Mp / 16 * 512); vec(c->inn, Mp); vec(c->diagR, Mp); vec(c->err, Np);
  A(&c->status, B); A(&c->ldlt_used, B); A(&c->scratch, B * Np);
  vec(c->yvec, Mp);
  c->Hlead.stride = (long)(Mp * LEAD_K); c->Hlead.ld = (int)Mp;   // (allocated by xivo_hip_set_calib)
  c->ell.pairs_max = (int)(Mp / 2);
  A(&c->ell.idx, B * c->ell.stride_idx()); A(&c->ell.val, B * c->ell.stride_val()); A(&c->ell.nc, B); A(&c->ell.pw, B); A(&c->ell.over, B);
  c->rows.sized(batch_max, ELL_CW, ELL_PW);
  // the hand-over kernel mirrors its three per-filter flags into host-mapped pinned memory: the host picks the kernel
  // instantiations from them after one stream synchronisation. (Three device-to-host copies into pageable vectors cost
  // 85 us of idle GPU per call - a third of a B = 1 step.) If the mapping is refused the copies are used.
  if (rc == XIVO_HIP_OK && hipHostMalloc(reinterpret_cast<void**>(&c->ell_flags_h), (size_t)B * 3 * sizeof(int), hipHostMallocMapped) == hipSuccess) {
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->ell_flags_d), c->ell_flags_h, 0) != hipSuccess) {
      hipHostFree(c->ell_flags_h); c->ell_flags_h = nullptr; c->ell_flags_d = nullptr;
    }
  } else c->ell_flags_h = nullptr;
  if (rc == XIVO_HIP_OK && hipEventCreate(&c->prof.t0) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc == XIVO_HIP_OK && hipEventCreate(&c->prof.t1) != hipSuccess) rc = XIVO_HIP_ERR_HIP;
  if (rc != XIVO_HIP_OK) { xivo_hip_destroy(c); return rc; }
  *out = c;
  return XIVO_HIP_OK;
}

int xivo_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// NUMA node of the host memory / cores next to `device` (sysfs of its PCI function), -1 when unknown: the launcher binds
// one rank per GPU to that node's cores (xivo_amd/shard.py) - eight ranks of an 8-GPU node must not pile up on socket 0
int xivo_hip_device_numa_node(int device) {
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) return -1;
  for (char* q = bdf; *q; ++q) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}

int xivo_hip_sync(xivo_hip_ctx* c) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_set_flags(xivo_hip_ctx* c, unsigned flags) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  c->flags = flags;
  return XIVO_HIP_OK;
}

// ------------------------------------------------------------------ P residency
int xivo_hip_upload_P(xivo_hip_ctx* c, int b0, int nb, const double* P, long stride, int ld) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !P || ld < c->N) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const int N = c->N;
  int rc = ensure_staging(c, (size_t)nb * N * N);
  if (rc) return rc;
  rc = h2d_packed(c, c->staging, P, nb, N, N, stride, ld);
  if (rc) return rc;
  HIP_TRY((hipError_t)launch_unpack_P(c->staging, c->P.from(b0).p, N, c->Np, c->P.ld, c->P.stride, nb, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // host buffer is only borrowed for the call
  return XIVO_HIP_OK;
}

int xivo_hip_download_P(xivo_hip_ctx* c, int b0, int nb, double* P, long stride, int ld) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !P || ld < c->N) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const int N = c->N;
  int rc = ensure_staging(c, (size_t)nb * N * N);
  if (rc) return rc;
  HIP_TRY((hipError_t)launch_pack_P(c->P.from(b0).p, c->staging, N, c->P.ld, c->P.stride, nb, c->stream));
  rc = d2h_packed(c, P, c->staging, nb, N, N, stride, ld);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_snapshot_P(xivo_hip_ctx* c) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  const size_t elems = (size_t)c->Bmax * c->P.stride;
  if (!c->Psnap) { int rc = c->mem.raw(&c->Psnap, elems); if (rc) return rc; }
  HIP_TRY(hipMemcpyAsync(c->Psnap, c->P.p, elems * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_restore_P(xivo_hip_ctx* c) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !c->Psnap) return XIVO_HIP_ERR_INVALID;
  c->dx_clear();   // (innovation log: the restored covariance is not the one dx was computed against)
  HIP_TRY(hipMemcpyAsync(c->P.p, c->Psnap, (size_t)c->Bmax * c->P.stride * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_p_zero_rc(xivo_hip_ctx* c, int b, int off, int len) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b, 1) || off < 0 || len < 0 || off + len > c->N) return XIVO_HIP_ERR_INVALID;
  return launch_p_zero_rc(c->P.from(b).p, c->P.ld, c->Np, off, len, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_p_copy_rc(xivo_hip_ctx* c, int b, int dst, int src, int len) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b, 1) || dst < 0 || src < 0 || len < 0 || dst + len > c->N || src + len > c->N) return XIVO_HIP_ERR_INVALID;
  return launch_p_copy_rc(c->P.from(b).p, c->P.ld, c->Np, dst, src, len, c->stream) ? XIVO_HIP_ERR_HIP : XIVO_HIP_OK;
}

int xivo_hip_p_set_block3(xivo_hip_ctx* c, int b, int off, const double* P3) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b, 1) || !P3 || off < 0 || off + 3 > c->N) return XIVO_HIP_ERR_INVALID;
  const BatchMat dst = c->P.from(b).at(off, off);
  HIP_TRY(hipMemcpy2DAsync(dst.p, (size_t)dst.ld * sizeof(double), P3, 3 * sizeof(double), 3 * sizeof(double), 3,
                           hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_p_diag(xivo_hip_ctx* c, int b, double* out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b, 1) || !out) return XIVO_HIP_ERR_INVALID;
  HIP_TRY((hipError_t)launch_p_diag(c->P.from(b).p, c->P.ld, c->N, c->scratch, c->stream));
  HIP_TRY(hipMemcpyAsync(out, c->scratch, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

// ------------------------------------------------------------------ device buffers for resident inputs (bench / tests)
int xivo_hip_dev_alloc(xivo_hip_ctx* c, size_t bytes, void** out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !out || bytes == 0) return XIVO_HIP_ERR_INVALID;
  *out = nullptr;
  return hipMalloc(out, bytes) == hipSuccess ? XIVO_HIP_OK : XIVO_HIP_ERR_NOMEM;
}

int xivo_hip_dev_free(xivo_hip_ctx* c, void* p) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (p) HIP_TRY(hipFree(p));
  return XIVO_HIP_OK;
}

int xivo_hip_dev_upload(xivo_hip_ctx* c, void* dst, const void* src, size_t bytes, size_t total_bytes) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !dst || !src || bytes == 0 || total_bytes < bytes) return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  // replicate the uploaded block over the rest of the buffer (doubling device-to-device copies)
  for (size_t have = bytes; have < total_bytes;) {
    const size_t n = have < total_bytes - have ? have : total_bytes - have;
    HIP_TRY(hipMemcpyAsync((char*)dst + have, dst, n, hipMemcpyDeviceToDevice, c->stream));
    have += n;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

// test hook: what the context's owner holds right now (device_buffers.h)
int xivo_hip_selftest_ctx_allocs(xivo_hip_ctx* c, int* live, unsigned long long* bytes) {
  if (!c) return XIVO_HIP_ERR_INVALID;
  if (live) *live = c->mem.live();
  if (bytes) *bytes = c->mem.bytes();
  return XIVO_HIP_OK;
}

// ------------------------------------------------------------------ timing
int xivo_hip_timer_begin(xivo_hip_ctx* c) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipEventRecord(c->prof.t0, c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_timer_end(xivo_hip_ctx* c, float* ms) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !ms) return XIVO_HIP_ERR_INVALID;
  HIP_TRY(hipEventRecord(c->prof.t1, c->stream));
  HIP_TRY(hipEventSynchronize(c->prof.t1));
  HIP_TRY(hipEventElapsedTime(ms, c->prof.t0, c->prof.t1));
  return XIVO_HIP_OK;
}

int xivo_hip_profile_reset(xivo_hip_ctx* c) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c) return XIVO_HIP_ERR_INVALID;
  int rc = collect_profile(c);
  for (int i = 0; i < ST_COUNT; ++i) { c->prof.ms[i] = 0.f; c->prof.launches[i] = 0; c->prof.flops[i] = 0.0; }
  return rc;
}

int xivo_hip_profile_get(xivo_hip_ctx* c, int* n, const char** names, float* ms, int* launches, double* flops) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || !n) return XIVO_HIP_ERR_INVALID;
  int rc = collect_profile(c);
  if (rc) return rc;
  *n = ST_COUNT;
  for (int i = 0; i < ST_COUNT; ++i) {
    if (names) names[i] = kStageNames[i];
    if (ms) ms[i] = c->prof.ms[i];
    if (launches) launches[i] = c->prof.launches[i];
    if (flops) flops[i] = c->prof.flops[i];
  }
  return XIVO_HIP_OK;
}

int xivo_hip_bench_mfma_peak(xivo_hip_ctx* c, double* out4) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  // out4[0] = TFLOP/s with the chip full (8 workgroups / CU)
  // out4[1] = shader cycles per MFMA per SIMD, one wave per SIMD (256 workgroups)
  // out4[2] = sustained shader clock (GHz) during the full-chip run
  // out4[3] = TFLOP/s with one wave per SIMD
  if (!c || !out4) return XIVO_HIP_ERR_INVALID;
  const int iters = 2000;
  double res[2][2];
  for (int mode = 0; mode < 2; ++mode) {
    const int blocks = mode == 0 ? 256 * 8 : 256;
    HIP_TRY((hipError_t)launch_mfma_peak(c->scratch, 10, blocks, c->stream));
    HIP_TRY(hipEventRecord(c->prof.t0, c->stream));
    HIP_TRY((hipError_t)launch_mfma_peak(c->scratch, iters, blocks, c->stream));
    HIP_TRY(hipEventRecord(c->prof.t1, c->stream));
    HIP_TRY(hipEventSynchronize(c->prof.t1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->prof.t0, c->prof.t1));
    double cyc = 0.0;
    HIP_TRY(hipMemcpy(&cyc, c->scratch + 1, sizeof(double), hipMemcpyDeviceToHost));
    const double flops = 2.0 * 16 * 16 * 4 * 8.0 * iters * 4.0 /*waves*/ * blocks;
    res[mode][0] = flops / (ms * 1e-3) / 1e12;
    res[mode][1] = cyc;
    if (mode == 0) out4[2] = cyc / (ms * 1e-3) / 1e9;  // cycles of one resident wave / wall time (lower bound)
  }
  out4[0] = res[0][0];
  out4[3] = res[1][0];
  out4[1] = res[1][1] / (8.0 * iters);
  return XIVO_HIP_OK;
}

void xivo_hip_gemm_tile(int rows, int cols, int symmetric, int* bm, int* bn) {
  int wm, wn;
  gemm_pick_tile(round_up16(rows), round_up16(cols), symmetric, &wm, &wn);
  if (bm) *bm = 32 * wm;
  if (bn) *bn = 32 * wn;
}

}  // extern "C"
