// Host-side internals shared by the translation units of the C ABI (include/xivo_hip.h):
//   capi.hip            context, P residency, resident device buffers, timing / profile, the helpers declared below (among
//                       them what the per-frame logs share: the slice check, the frame-major read, the NEES staging)
//   capi_update.hip     route table, measurement hand-over, the update pipelines, the L D L^T fallback, the one-filter call
//   capi_glevel.hip     feature level: scene, Jacobians, gate, stacking, OOS rows, RANSAC, loop closure, Givens / QR, edits
//   capi_propagate.hip  propagation
//   capi_traj.hip       trajectory log: per-frame records, read-out, NEES against ground truth
//   capi_score.hip      trajectory score: aligned / unaligned ATE and RPE of the logged poses against ground truth
//   capi_map.hip        landmark log: per-frame in-state features, world positions and covariances, read-out, landmark NEES
//   capi_innov.hip      innovation log: per-frame NIS / pre- and post-fit sums of every filter's update, read-out, ensemble sums
//   capi_lifecycle.hip  device life cycle: the frame calls around the update, counters; the in-state slot book and the track
//                       block that both device life cycles use
//   capi_pool_lifecycle.hip  device pool life cycle ("subfilter" mode): the pool book, the two frame calls, counters
//   capi_pcw.hip        point-cloud world: the resident worlds, the per-frame track producer, read-back
//   capi_trajsim.hip    trajectory producer: the simulated IMU records and ground-truth poses of a frame, the ground-truth log
// Host code only (no kernels). Nothing here is exported from the library: the shared functions live in xivo_hip::capi, each
// defined once, in the file named next to its declaration, and are hidden (the declarations below carry the visibility).
//
// Three things those files go through:
//   c->mem (device_buffers.h)  owns every device block of the context. Allocation is c->mem.zeroed / raw / grow, re-sizing a
//                              group of buffers is c->mem.release + allocation, xivo_hip_destroy is c->mem.free_all(). The only
//                              hipMalloc / hipFree of the C ABI are the owner's two function pointers (capi.hip) and the
//                              caller-owned blocks of xivo_hip_dev_alloc / xivo_hip_dev_free.
//   BatchMat / BatchVec        a per-filter matrix (vector) of the context: pointer, per-filter stride and leading dimension as
//                              ONE value. The context holds its buffers as such views, from(b0) is the view of the filters from
//                              b0 on, to(...) writes the three into a kernel argument struct - a pointer cannot be passed with
//                              another buffer's stride. A descriptor only: owns nothing, allocates nothing.
//   FrameLog (frame_log.h)     the host bookkeeping of a per-frame log: capacity, frames written, stamps, the slice check. The
//                              four logs (capi_traj / _map / _innov / _trajsim.hip) hold one each next to their device blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/xivo_hip.h"
#include "common.h"
#include "ekf_kernels.h"
#include "ell.h"
#include "fused_update.h"
#include "staged_rows.h"
#include "device_buffers.h"
#include "frame_log.h"

namespace xivo_hip::capi {

enum Stage : int {
  ST_JAC = 0, ST_GATE, ST_STACK, ST_HP, ST_S, ST_CHOL, ST_TRSM, ST_KH, ST_AP, ST_PNEW, ST_OTHER, ST_PROP_STATE, ST_PROP_TAIL, ST_COUNT
};
inline const char* const kStageNames[ST_COUNT] = {"jac_instate", "mh_gate", "stack_H", "gemm_HP", "gemm_S", "chol_S",
                                                  "trsm_gain", "gemm_KH_I", "gemm_AP", "gemm_Pnew", "other", "propagate_state",
                                                  "propagate_tail"};

struct EventPair { hipEvent_t a, b; int stage; };

// the owner's allocator (capi.hip): hipMalloc (+ hipMemset), hipFree
__attribute__((visibility("hidden"))) int device_alloc(void** p, size_t bytes, int zero);
__attribute__((visibility("hidden"))) void device_free(void* p);

// leading state columns the calibration blocks live in: td 23, Cg 24..32, (Ca 33..38,) bg 9..11, intrinsics up to 39..47
constexpr int LEAD_K = 48;

// A per-filter vector: filter b starts at p + b * stride.
struct BatchVec {
  double* p = nullptr; long stride = 0;
  BatchVec from(int b0) const { return {p ? p + (long)b0 * stride : nullptr, stride}; }
  template <class P, class S> void to(P& ptr, S& str) const { ptr = p; str = stride; }
};
// A per-filter column-major matrix: element (i, j) of filter b at p[b * stride + i + j * ld].
struct BatchMat {
  double* p = nullptr; long stride = 0; int ld = 0;
  BatchMat from(int b0) const { return {p ? p + (long)b0 * stride : nullptr, stride, ld}; }
  BatchMat at(int i, int j) const { return {p + i + (long)j * ld, stride, ld}; }   // the block that starts at (i, j)
  template <class P, class S, class L> void to(P& ptr, S& str, L& l) const { ptr = p; str = stride; l = ld; }
};

// The in-state slot book of the device life cycle that is configured (capi_lifecycle.hip or capi_pool_lifecycle.hip: the two
// exclude each other): feat_id [Bmax][ld] (-1: free slot), group_refs [Bmax][n_groups] (-1: free); null until book_alloc
struct InstateBookBuffers {
  long long* feat_id = nullptr; int* group_refs = nullptr; int ld = 0;
};

// The track block of the device life cycle that is configured: one device block that holds a frame's tracks and two page-locked
// staging blocks of that size, each with the event of its last upload (cur: the one the last upload filled). Two forms share the
// device block: packed, off [B + 1] | ids [n] | meas [n][3] as track_block_upload leaves them, and strided behind the offsets'
// space, ids [Bmax][tracks_max] | meas [Bmax][tracks_max][3] with the counts in pcw_cnt, as the track producer (capi_pcw.hip)
// leaves them. B > 0: a frame is open between a begin and an end call, on n packed tracks or (strided) on the producer's.
// The track_block_* functions (capi_lifecycle.hip) are its interface; nothing else touches the fields.
struct TrackBlock {
  char* dev = nullptr; char* pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
  size_t set_bytes = 0;
  int tracks_max = 0, cur = 0, B = 0, n = 0;
  bool strided = false;
};


}  // namespace xivo_hip::capi

struct xivo_hip_ctx {
  int device = 0;
  int N = 0, Np = 0, Mmax = 0, Mpmax = 0, Bmax = 0;
  unsigned flags = 0;
  hipStream_t stream = nullptr;
  xivo_hip::capi::DeviceBuffers mem{xivo_hip::capi::device_alloc, xivo_hip::capi::device_free};   // every device block below
  // per-filter device buffers, each with the stride and leading dimension it is allocated with (xivo_hip_create). The A buffer
  // [max(N x N, N x M)] is read with two strides: G (G of the whitened / tail forms, the fallback's A) and KHI (A = K H - I of
  // the as-coded dense pipeline, laid out like P)
  xivo_hip::capi::BatchMat P, H, HT, HP, PHT, S, K, G, KHI, T;
  xivo_hip::capi::BatchVec invD, inn, diagR, err;
  xivo_hip::capi::BatchVec yvec;   // symmetric form: y = L^-1 inn per filter
  double *Psnap = nullptr, *staging = nullptr, *scratch = nullptr;
  int* status = nullptr;
  // row-pair compressed H (ell.h); which representations of the staged rows are valid right now: staged_rows.h
  xivo_hip::EllBuffers ell{};
  xivo_hip::capi::StagedRows rows;
  int* ell_flags_h = nullptr;   // pinned, device-mapped [Bmax][3]: over / nc / pw as the hand-over kernel leaves them
  int* ell_flags_d = nullptr;   // its device alias
  int last_path = 0;
  int last_route = 0;   // UpdateRoute of the last pass (xivo_hip_last_route)
  size_t staging_elems = 0;
  int chunk = 0;      // filters per pipeline pass (0 = whole batch)
  int call_batch = 0; // filters of the whole update call being walked in chunks (0: not chunked)
  int* ldlt_used = nullptr;     // per filter: 1 = the last update went through the pivoted L D L^T fallback
  // G-level
  xivo_layout lay{};
  xivo_cam cam{};
  bool have_layout = false;
  // online-calibration builds, measurement side (xivo_hip_set_calib): extra Jacobian blocks, dense stacking
  bool calib_on = false;       // measurement side of an online-calibration build (td / Cg / bg / intrinsics blocks)
  bool calib_motion = false;   // motion side: kMotionSize > 23 (xivo_hip_propagate_calib)
  xivo_calib_layout cl{-1, -1, 0, 0};
  xivo_calib_in* calib = nullptr;   // [Bmax]
  double* Jc = nullptr;             // [Bmax x Fmax x 44]
  int Fmax = 0, F = 0;
  xivo_pose_in* poses = nullptr;
  int* absorb_count = nullptr;   // State::counter of every filter (src/core.h:120-122)
  // OnePointRANSAC scratch (allocated on first use): BackupState copies, selection results
  double* Prs = nullptr; xivo_pose_in* poses_rs = nullptr; xivo_group_in* groups_rs = nullptr;
  unsigned char *rs_low = nullptr, *rs_lowkeep = nullptr, *rs_keep = nullptr;
  unsigned long long *rs_zg = nullptr, *rs_gmask = nullptr;
  int *rs_state = nullptr, *rs_gauge = nullptr, *rs_nrej = nullptr;
  double* rs_chi = nullptr;
  int rs_Fmax = 0;
  xivo_group_in* groups = nullptr;
  xivo_feat_in* feats = nullptr;
  double *J = nullptr, *finn = nullptr, *dist = nullptr;
  unsigned char* mask = nullptr;
  int* rows_instate = nullptr;
  xivo_oos_in* oos = nullptr;
  size_t oos_cap = 0;
  double* pd_h = nullptr; double pd_h0 = 0.0;   // step-size-controlled Dormand-Prince: the step each filter carries (xivo_hip_propagate)
  int oos_nb = 0, oos_n = 0, oos_whole = 0;   // shape of the resident OOS list (xivo_hip_oos_project with feats == NULL; its row bound: rows)
  int* oos_rows = nullptr;
  xivo_calib_in* calib_rs = nullptr;            // BackupState of the calibration state (OnePointRANSAC, online-calibration builds)
  // online-calibration builds on the sparse pipeline (round 5): the calibration columns of the stacked rows as a dense
  // [Mpmax x LEAD_K] block per filter next to the row-pair compressed rows (rows.has_lead(): the current stacking has one)
  xivo_hip::capi::BatchMat Hlead;
  char* lc_buf = nullptr; size_t lc_cap = 0;   // xivo_hip_close_loop_stack: matches | dense rows | inn | diagR
  xivo_subfilter_feat* sub = nullptr;   // staging of xivo_hip_subfilter_update
  // out-of-state feature pool (xivo_hip_pool_*): entries [Bmax][pool_max] (ref_sind = the entry's anchor, -1: free), anchors
  // [Bmax][anchor_max]; host mirrors of who is live / linked, which validate pool_add and the pool's edit kinds
  int pool_max = 0, anchor_max = 0;
  xivo_subfilter_opts pool_opts{};
  double pool_remove_outlier = 0.0;
  xivo_subfilter_feat* fpool = nullptr;
  xivo_hip::PoolAnchor* anchors = nullptr;
  char* pool_io = nullptr; size_t pool_io_cap = 0;   // per-call device staging: records / pixels in, order / counts / live out
  std::vector<int> pool_anchor_h;   // [Bmax][pool_max]: anchor of a live entry, -1 = free
  std::vector<int> anchor_link_h;   // [Bmax][anchor_max]: linked group slot, -1 = unlinked
  // depth initialisation of new tracks (xivo_hip_pool_triangulation / xivo_hip_pool_adapt_depth*): triangulation options
  // (method XIVO_TRI_OFF: off), per-filter good / bad counters and the resident init_z [Bmax] (allocated by pool_config)
  xivo_triangulate_opts pool_tri{};
  int* tri_counts = nullptr;        // [2][Bmax]: good, bad
  double* init_z = nullptr;         // [Bmax]
  xivo_adapt_depth_opts adapt{};
  bool adapt_on = false;
  // The three per-frame logs below and the trajectory producer's ground truth: device pointers, options, the FrameLog (frame_log.h:
  // capacity in frames, frames written, stamps), staging. A log's blocks are allocated exactly while its FrameLog is configured.
  // trajectory log (xivo_hip_traj_*, capi_traj.hip): [capacity][Bmax] records and packed covariance blocks of traj_cols.
  // traj_io: per-call staging of xivo_hip_traj_nees / xivo_hip_traj_score
  xivo_traj_rec* traj_rec = nullptr; double* traj_cov = nullptr;
  int traj_ncols = 0, traj_cols[XIVO_TRAJ_MAX_COLS] = {0};
  xivo_hip::capi::FrameLog traj_log;
  char* traj_io = nullptr; size_t traj_io_cap = 0;
  // landmark log (xivo_hip_map_*, capi_map.hip): [capacity][Bmax][map_nout] entries and [capacity][Bmax] counts. map_io: per-call
  // staging of xivo_hip_map_nees
  xivo_map_pt* map_pts = nullptr; int* map_npts = nullptr;
  int map_nout = 0; unsigned map_flags = 0;
  xivo_hip::capi::FrameLog map_log;
  char* map_io = nullptr; size_t map_io_cap = 0;
  // innovation log (xivo_hip_innov_*, capi_innov.hip): [capacity][Bmax] records. innov_io: the output staging of
  // xivo_hip_innov_stats, allocated by xivo_hip_innov_config for the largest slice. dx_ok[b]: the err buffer of filter b holds the
  // dx of the rows staged for it right now (set by the update calls for the filters they update; cleared by absorb, new rows,
  // restore_P) - a record of filters [0, B) needs it of every one of them
  xivo_innov_rec* innov_rec = nullptr;
  xivo_hip::capi::FrameLog innov_log;
  char* innov_io = nullptr;
  std::vector<char> dx_ok;
  void dx_set(int b0, int nb, bool v) { if (dx_ok.size() != (size_t)Bmax) dx_ok.assign((size_t)Bmax, 0); std::fill_n(dx_ok.begin() + b0, nb, (char)v); }
  void dx_clear() { std::fill(dx_ok.begin(), dx_ok.end(), (char)0); }
  bool dx_current(int B) const { return dx_ok.size() >= (size_t)B && std::all_of(dx_ok.begin(), dx_ok.begin() + B, [](char v) { return v != 0; }); }
  // the device life cycles (capi_lifecycle.hip, capi_pool_lifecycle.hip; at most one of the two is configured): the in-state book
  // and the track block of whichever is, both null when neither
  xivo_hip::capi::InstateBookBuffers book;
  xivo_hip::capi::TrackBlock tracks;
  // device life cycle (xivo_hip_life_*): its options and counters [Bmax]; life_stats is null until xivo_hip_life_config - "the
  // immediate life cycle is configured"
  xivo_life_opts life_opts{};
  xivo_life_stats* life_stats = nullptr;
  // device pool life cycle (xivo_hip_pool_life_*): the pool book [Bmax][pool_max] / [Bmax][anchor_max], the counters [Bmax], what
  // a frame's kernels hand each other (slot_track, ent_track, the step's xp / order / n / live); null until
  // xivo_hip_pool_life_config. plife_frame: the frame counter
  bool plife_on = false;
  xivo_pool_life_opts plife_opts{};
  long long* plife_ent_id = nullptr; int* plife_ent_born = nullptr; int* plife_anc_used = nullptr; int* plife_anc_life = nullptr;
  xivo_pool_life_stats* plife_stats = nullptr;
  int* plife_slot_track = nullptr; int* plife_ent_track = nullptr;
  double* plife_xp = nullptr; int* plife_order = nullptr; int* plife_n = nullptr; unsigned char* plife_live = nullptr;
  int plife_frame = 0;
  // point-cloud world (xivo_hip_pcw_*, capi_pcw.hip): the resident worlds Xs [Bmax][npts][3] / ids [Bmax][npts] / next_id [Bmax],
  // the frame's camera poses [Bmax][12] with two page-locked staging blocks (the scheme of the track block) and cnt [Bmax]; null until
  // xivo_hip_pcw_config. The producer writes the strided form of the track block: pcw_tracks_B is the B whose tracks the block
  // holds (0: none - a host-track life_begin overwrote them), pcw_fresh whether a life_begin_tracks may still consume them
  xivo_pcw_opts pcw_opts{};
  double* pcw_Xs = nullptr; long long* pcw_ids = nullptr; long long* pcw_next_id = nullptr; int* pcw_cnt = nullptr;
  double* pcw_gsc = nullptr; double* pcw_pin[2] = {nullptr, nullptr}; hipEvent_t pcw_ev[2] = {nullptr, nullptr};
  int pcw_cur = 0, pcw_tracks_B = 0; bool pcw_fresh = false;
  // the camera of xivo_hip_pcw_camera in place of the pinhole of pcw_opts (pcw_use_cam), and its radius guard
  bool pcw_use_cam = false; xivo_cam pcw_cam{}; double pcw_max_radius = 0.0;
  // trajectory producer (xivo_hip_trajsim_*, capi_trajsim.hip): curve / rate per filter [Bmax], the last frame's records
  // [Bmax][n_max] (read as [B][n]) and camera poses [Bmax][12], the ground-truth log ts_gt [T_max][Bmax][12] with its FrameLog
  // ts_log (no stamps: it commits 0), the device copy of the propagation noise (Qimu 144 | Qmodel 529) with the host copy it was
  // uploaded from; null until xivo_hip_trajsim_config. ts_B / ts_n: the shape of the last frame (ts_B = 0: none), ts_fresh: its
  // records may still be consumed by xivo_hip_propagate_resident
  xivo_trajsim_opts ts_opts{};
  int* ts_motion = nullptr; double* ts_rate = nullptr; xivo_imu_in* ts_recs = nullptr; double* ts_gsc = nullptr;
  double* ts_Q = nullptr;
  double* ts_gt = nullptr; xivo_hip::capi::FrameLog ts_log;
  xivo_prop_opts ts_prop{}; bool ts_prop_valid = false;
  int ts_B = 0, ts_n = 0; bool ts_fresh = false;
  std::vector<char> hstage;                        // host staging of d2h_rows
  char* edit_buf = nullptr; size_t edit_cap = 0;   // device copy of the ops of xivo_hip_edit_batch
  // one-filter plumbing call (xivo_hip_update_joseph_host): page-locked, device-mapped staging block owned by the context,
  // scratch of the host-side row compression
  char* pin_h = nullptr; char* pin_d = nullptr;
  struct HostCompressScratch { std::vector<int> cnt, occ, cslot, n; std::vector<double> v; } hc;
  size_t sub_cap = 0;   // entries
  // timing
  hipEvent_t t0 = nullptr, t1 = nullptr;
  std::vector<xivo_hip::capi::EventPair> pool;
  size_t pool_used = 0;
  float stage_ms[xivo_hip::capi::ST_COUNT] = {0};
  int stage_launches[xivo_hip::capi::ST_COUNT] = {0};
  double stage_flops[xivo_hip::capi::ST_COUNT] = {0};
  double stage_bytes[xivo_hip::capi::ST_COUNT] = {0};         // algorithmic HBM bytes of the stage's last launch (inputs once + outputs once)
  char stage_kernel[xivo_hip::capi::ST_COUNT][64] = {{0}};   // kernel instantiation of the stage's last launch (as rocprofv3 names it)
};

#pragma GCC visibility push(hidden)
namespace xivo_hip::capi {

// XIVO_HIP_DEBUG=1: name the failing runtime call on stderr (the C ABI itself only returns a status)
inline bool debug_on() { static const bool on = getenv("XIVO_HIP_DEBUG") != nullptr; return on; }
#define HIP_TRY(expr)                              \
  do {                                             \
    hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) {                        \
      if (xivo_hip::capi::debug_on()) fprintf(stderr, "xivo_hip: %s -> %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return XIVO_HIP_ERR_HIP;                     \
    }                                              \
  } while (0)

struct StageTimer {
  xivo_hip_ctx* c; EventPair* ep = nullptr;
  StageTimer(xivo_hip_ctx* ctx, int stage, double flops, const char* kernel = nullptr, double bytes = 0.0) : c(ctx) {
    if (!(c->flags & XIVO_HIP_FLAG_PROFILE)) return;
    c->stage_bytes[stage] = bytes;
    if (kernel) { strncpy(c->stage_kernel[stage], kernel, 63); c->stage_kernel[stage][63] = 0; }
    if (c->pool_used >= c->pool.size()) {
      EventPair np; np.stage = stage;
      if (hipEventCreate(&np.a) != hipSuccess || hipEventCreate(&np.b) != hipSuccess) return;
      c->pool.push_back(np);
    }
    ep = &c->pool[c->pool_used++];
    ep->stage = stage;
    c->stage_launches[stage]++;
    c->stage_flops[stage] = flops;
    hipEventRecord(ep->a, c->stream);
  }
  ~StageTimer() { if (ep) hipEventRecord(ep->b, c->stream); }
};

// One K-segment of a batched product: A [rows x K] times B^T, B [cols x K]
struct GemmProduct { BatchMat A, B; int K = 0; };

struct GemmExtra {
  int epi = EPI_NONE;
  BatchVec diag;   // EPI_ADD_DIAG
  BatchMat msub;   // EPI_SUB_MAT / EPI_ADD_MAT / EPI_RSUB_MAT operand, same shape as C
  BatchVec mcol;   // optional per-column scale of msub
  BatchMat C2;     // optional second output = C^T
  int c2_rows = 0;   // > 0: the transposed copy only of the leading c2_rows rows of C (the columns of C2 a consumer reads)
  int lower_only = 0;
  int fp32 = 0;
  int a_f32 = 0;   // first operand stored as float
  int b_f32 = 0;   // second operand stored as float
  int no_mirror = 0;
  const int* skip = nullptr;   // per-filter status: non-zero = leave the output of that filter untouched
  const double* scale0 = nullptr;   // per-k scale of the first segment's B operand (same vector for every filter)
  int small_tiles = 0;   // symmetric output on 64 x 64 tiles (latency route)
  GemmProduct seg1;      // optional second segment (seg1.A.p set): + A1 diag(scale1) B1^T
  BatchVec scale1;       // per-k scale of the second segment's B operand, per filter
};

// ---- capi.hip
bool bad_range(xivo_hip_ctx* c, int b0, int nb);
MeasBuffers meas_buffers(xivo_hip_ctx* c, int b0 = 0);   // the dense rows, inn and diagR of the filters from b0 on
SceneBuffers scene_buffers(xivo_hip_ctx* c);
bool calib_sparse(const xivo_hip_ctx* c);
// C [rows x cols] = seg.A seg.B^T (+ x.seg1.A diag(x.scale1) x.seg1.B^T) over B filters, on the MFMA product kernels, timed as
// `stage`
int gemm(xivo_hip_ctx* c, int stage, int B, int rows, int cols, const GemmProduct& seg, const BatchMat& C, const GemmExtra& x);
int ensure_staging(xivo_hip_ctx* c, size_t elems);
int d2h_rows(xivo_hip_ctx* c, void* dst, size_t hpitch, const void* src, size_t dpitch, size_t width, size_t rows);
int h2d_packed(xivo_hip_ctx* c, double* dst, const double* src, int nb, int rows, int cols, long stride, int ld);
int d2h_packed(xivo_hip_ctx* c, double* dst, const double* src, int nb, int rows, int cols, long stride, int ld);
// what the per-frame logs share (FrameLog, frame_log.h; c is not null).
// the one slice check: filters [b0, b0 + nb) of the context, a configured log, frames [t0, t0 + nt) of its written ones
inline bool bad_slice(xivo_hip_ctx* c, const FrameLog& log, int b0, int nb, int t0, int nt) {
  return bad_range(c, b0, nb) || !log.configured() || !log.slice_ok(t0, nt);
}
// that slice of a frame-major block src of `per` bytes per filter entry to dst [nt][nb], enqueued (dst null: nothing)
int d2h_frames(xivo_hip_ctx* c, void* dst, const void* src, size_t per, int b0, int nb, int t0, int nt);
// the two blocks of a log for T_max frames (the stream must be idle): the old ones given back and the log emptied, then for
// T_max > 0 na / nb elements behind *a / *b - both or neither - and the log configured
template <class A, class B> int log_realloc(xivo_hip_ctx* c, FrameLog& log, int T_max, A** a, size_t na, B** b, size_t nb) {
  c->mem.release(a, b);
  log.configure(0);
  if (T_max == 0) return XIVO_HIP_OK;
  int rc = c->mem.raw(a, na);
  if (!rc) rc = c->mem.raw(b, nb);
  if (rc) c->mem.release(a, b); else log.configure(T_max);
  return rc;
}
// the tail of a record call whose launch went out: the frame counts, with its stamp
inline void log_commit(FrameLog& log, long long ts_ns, int* frame_out) { const int t = log.commit(ts_ns); if (frame_out) *frame_out = t; }
// The per-call staging of a NEES entry point (xivo_hip_traj_nees, xivo_hip_map_nees) in the log's growing block io: gt in | err,
// nees, anees out (doubles), then n_used (ints), for nt frames of `per` entries with gt_w / err_w doubles an entry.
struct NeesStaging {
  double *gt, *err, *nees, *anees; int* n_used;
  size_t n, nt, err_w;
  // lay the block out, grow it and enqueue the upload of gt
  int up(xivo_hip_ctx* c, char** io, size_t* io_cap, size_t per, int nt_, int gt_w, int err_w_, const double* gt_h);
  // behind the kernels: the downloads the caller asked for (null: not that one), then the synchronise
  int down(xivo_hip_ctx* c, double* err_h, double* nees_h, double* anees_h, int* n_used_h) const;
};

// ---- capi_update.hip
int stage_measurements(xivo_hip_ctx* c, int b0, int nb, int M, const double* dH, long strideH, int ldh,
                       const double* dInn, long strideInn, const double* dR, long strideR);

// ---- capi_lifecycle.hip
// the track block (TrackBlock above)
int track_block_alloc(xivo_hip_ctx* c, int tracks_max);
void track_block_release(xivo_hip_ctx* c);   // (the stream must be idle)
inline int track_block_frame(const xivo_hip_ctx* c) { return c->tracks.B; }   // the B of the open frame, 0: none
inline bool track_block_frame_open(const xivo_hip_ctx* c) { return c->tracks.B != 0; }
// a frame's packed tracks as the caller hands them: off [B + 1] with off[0] = 0, non-decreasing, no filter above tracks_max; ids /
// meas present when there is a track
bool track_block_frame_ok(const xivo_hip_ctx* c, int B, const int* off, const long long* ids, const double* meas);
int track_block_upload(xivo_hip_ctx* c, int B, const int* off, const long long* ids, const double* meas);
// the strided form: row length, ids [Bmax][row], meas [Bmax][row][3]
inline int track_block_row(const xivo_hip_ctx* c) { return c->tracks.tracks_max; }
long long* track_block_strided_ids(xivo_hip_ctx* c);
double* track_block_strided_meas(xivo_hip_ctx* c);
inline void track_block_use_strided(xivo_hip_ctx* c) { c->tracks.strided = true; c->tracks.n = 0; }   // (an upload: packed again)
// a frame of B filters opens on the tracks the block holds in the form it is in / closes
inline void track_block_open_frame(xivo_hip_ctx* c, int B) { c->tracks.B = B; }
inline void track_block_close_frame(xivo_hip_ctx* c) { c->tracks.B = 0; }
// the in-state book (InstateBookBuffers above): every slot free / released; xivo_hip_life_set_book / _get_book
int book_alloc(xivo_hip_ctx* c);   // (enqueues the fill: the caller synchronises)
void book_release(xivo_hip_ctx* c);
int book_set(xivo_hip_ctx* c, int b0, int nb, const long long* feat_id);
int book_get(xivo_hip_ctx* c, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs);
// what every frame call of either life cycle checks first: context, layout and poses present, B and F (against the book) in
// range, the rows of F features fit, no frame open
bool frame_can_begin(const xivo_hip_ctx* c, int B, int F);
// what the kernels of either life cycle take of a frame of B filters: P, the scene, the book and the tracks of the open frame in
// the form they are in; and what their end kernels take of the update
LifeArgs life_args_common(xivo_hip_ctx* c, int B);
void life_args_update(xivo_hip_ctx* c, LifeArgs& a);

// ---- capi_pool_lifecycle.hip
void pool_life_release(xivo_hip_ctx* c);   // everything xivo_hip_pool_life_config allocated (the stream must be idle)

// ---- capi_pcw.hip
void pcw_release(xivo_hip_ctx* c);   // the worlds and the pose staging (the stream must be idle)
// the track producer over device-resident camera poses gsc [B][12] (what xivo_hip_pcw_tracks enqueues behind its upload)
int pcw_produce(xivo_hip_ctx* c, int B, const double* gsc, double noise_px_std, unsigned long long seed, unsigned long long frame);

// ---- capi_propagate.hip
// Estimator::Propagate of filters [0, B) of a default-build context over device-resident records [B][n_imu] and noise blocks;
// mean_dt: the samples' length for the profile's flop count. Enqueues only
int propagate_device(xivo_hip_ctx* c, int B, int n_imu, const xivo_imu_in* recs, const double* dQimu, const double* dQmodel,
                     const xivo_prop_opts* o, double mean_dt);

// ---- capi_glevel.hip
int ensure_gate_buffers(xivo_hip_ctx* c, int F);
// the arguments of one pool step but xp / order / n / live (xivo_hip_pool_step and the device pool life cycle share them)
PoolStepArgs pool_step_args(xivo_hip_ctx* c, int B, int strict);
int ensure_dense(xivo_hip_ctx* c);
int ensure_HT(xivo_hip_ctx* c);
// H P (+ P H^T) of the stacked dense rows of filters [0, B) and the dense-row gate on them (gate_dense_kernel); `a` brings the
// gate's own parameters and outputs, the row buffers are filled in here
int gate_dense_rows(xivo_hip_ctx* c, int B, GateDenseArgs a);

}  // namespace xivo_hip::capi
#pragma GCC visibility pop
