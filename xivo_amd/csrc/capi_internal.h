// Host-side internals shared by the translation units of the C ABI (include/xivo_hip.h):
//   capi.hip            context, P residency, resident device buffers, timing / profile, the helpers declared below (among
//                       them what the per-frame logs share: the slice check, the frame-major read, the NEES staging)
//   capi_update.hip     route table, measurement hand-over, the update pipelines, the L D L^T fallback, the one-filter call
//   capi_glevel.hip     feature level: layout, scene, calibration, Jacobians, gate, stacking, filter_update, absorb, edits, pixels
//   capi_oos.hip        OOS rows, loop-closure stacking, OOS compression, Givens / QR
//   capi_ransac.hip     OnePointRANSAC on the resident state
//   capi_pool.hip       sub-filter, candidate order, the feature pool, triangulation, AdaptInitialDepth
//   capi_pool_oos.hip   MSCKF update from dropped pool entries: the frame's list, its fixed row block, the chi-square gate
//   capi_propagate.hip  propagation
//   capi_traj.hip       trajectory log: per-frame records, read-out, NEES against ground truth
//   capi_score.hip      trajectory score: aligned / unaligned ATE and RPE of the logged poses against ground truth
//   capi_map.hip        landmark log: per-frame in-state features, world positions and covariances, read-out, landmark NEES
//   capi_innov.hip      innovation log: per-frame NIS / pre- and post-fit sums of every filter's update, read-out, ensemble sums
//   capi_lifecycle.hip  device life cycle: the frame calls around the update, counters; the in-state slot book and the track
//                       block that both device life cycles use
//   capi_pool_lifecycle.hip  device pool life cycle ("subfilter" mode): the pool book, the two frame calls, counters
//   capi_pcw.hip        point-cloud world: the resident worlds, the per-frame track producer, read-back
//   capi_lcmap.hip      loop closure: the resident landmark map, its add / close calls, load / read-out, counters; inside the
//                       device life cycle: the keys beside the track block and the book, the resident add / close calls
//   capi_trajsim.hip    trajectory producer: the simulated IMU records and ground-truth poses of a frame, the ground-truth log
//   capi_tune.hip       tuning table: per-filter R, MH_thresh, var_xyz, Qimu, Qmodel and who reads them
// Host code only (no kernels). Nothing here is exported from the library: the shared functions live in xivo_hip::capi, each
// defined once, in the file named next to its declaration, and are hidden (the declarations below carry the visibility).
//
// Four things those files go through:
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
//   the records below          the state of one area each (profiler, RANSAC scratch, resident OOS list, feature pool, the two device
//                              life cycles, world, trajectory producer, the three logs), held by the context by value. A record
//                              says itself whether its area is configured(), is reset by assigning a default-constructed one once
//                              its device blocks went back to c->mem, and is changed from outside only through its named functions.
//                              Records own no device memory. PoolMirror (pool_mirror.h) is the pool's host mirrors;
//                              PinnedUpload the one double-buffered page-locked upload (the track block's, the world's poses).
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
#include "pool_mirror.h"

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

// A double-buffered page-locked upload (capi.hip): two page-locked blocks of one size, each with the event of its last upload
// (cur: the one the last upload filled), so that the host writes the next frame's bytes while the previous upload may still be
// reading. A frame is stage() - the block the previous frame did not use, once its last upload has finished -, the host copy,
// enqueue(). It gives its blocks back when it is released, assigned over or destroyed with the context.
struct __attribute__((visibility("hidden"))) PinnedUpload {
  PinnedUpload() = default;
  PinnedUpload(const PinnedUpload&) = delete;
  PinnedUpload& operator=(PinnedUpload&& o) noexcept;
  ~PinnedUpload() { release(); }
  int alloc(size_t bytes);   // all or nothing: XIVO_HIP_ERR_NOMEM (sticky error cleared) / XIVO_HIP_ERR_HIP
  void release();            // (nothing of it may still be in flight)
  int stage(char** h);
  int enqueue(void* dev, size_t bytes, hipStream_t stream);   // the staged block's leading bytes to dev, record, flip
 private:
  char* pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
  int cur = 0;
};

// The track block of the device life cycle that is configured: one device block that holds a frame's tracks and the page-locked
// staging of that size. Two forms share the
// device block: packed, off [B + 1] | ids [n] | meas [n][3] as track_block_upload leaves them, and strided behind the offsets'
// space, ids [Bmax][tracks_max] | meas [Bmax][tracks_max][3] with the counts in the world's cnt, as the track producer (capi_pcw.hip)
// leaves them. B > 0: a frame is open between a begin and an end call, on n packed tracks or (strided) on the producer's.
// The track_block_* functions (capi_lifecycle.hip) are its interface; nothing else touches the fields.
struct TrackBlock {
  char* dev = nullptr; PinnedUpload up;
  size_t set_bytes = 0;
  int tracks_max = 0, B = 0, n = 0;
  bool strided = false;
};

// ---- one record per area

// timing / profile (StageTimer, xivo_hip_timer_*, xivo_hip_profile_*): the timer's two events, the stage event pairs of the
// launches since the last collection (used of them taken), the sums per stage
struct Profiler {
  hipEvent_t t0 = nullptr, t1 = nullptr;
  std::vector<EventPair> events;
  size_t used = 0;
  float ms[ST_COUNT] = {0};
  int launches[ST_COUNT] = {0};
  double flops[ST_COUNT] = {0};
  double bytes[ST_COUNT] = {0};         // algorithmic HBM bytes of the stage's last launch (inputs once + outputs once)
  char kernel[ST_COUNT][64] = {{0}};   // kernel instantiation of the stage's last launch (as rocprofv3 names it)
};

// OnePointRANSAC scratch (capi_ransac.hip, allocated on first use for Fmax features): BackupState copies of P, the nominal state,
// the groups and (online-calibration builds) the calibration state; selection results
struct RansacScratch {
  double* P = nullptr; xivo_pose_in* poses = nullptr; xivo_group_in* groups = nullptr; xivo_calib_in* calib = nullptr;
  unsigned char *low = nullptr, *lowkeep = nullptr, *keep = nullptr;
  unsigned long long *zg = nullptr, *gmask = nullptr;
  int *state = nullptr, *gauge = nullptr, *nrej = nullptr;
  double* chi = nullptr;
  int Fmax = 0;
  bool sized_for(int F) const { return Fmax == F; }
};

// the resident OOS list (capi_oos.hip): what the last xivo_hip_oos_project with a list uploaded - nb filters of n features,
// `whole` as its option set it - and the rows every filter got of it
struct OosList {
  xivo_oos_in* feats = nullptr; size_t cap = 0;
  int nb = 0, n = 0, whole = 0;
  int* rows = nullptr;   // [Bmax]
  // xivo_hip_oos_project with feats == NULL: that very list is resident
  bool holds(int nb_, int n_, int whole_) const { return feats && nb == nb_ && n == n_ && whole == whole_; }
};

// out-of-state feature pool (capi_pool.hip): entries [Bmax][pool_max] (ref_sind = the entry's anchor, -1: free), anchors
// [Bmax][anchor_max] (their shapes: the mirror's); the host mirrors of who is live / linked, which validate pool_add and the pool's
// edit kinds. Depth initialisation of new tracks (xivo_hip_pool_triangulation / xivo_hip_pool_adapt_depth*): triangulation
// options (method XIVO_TRI_OFF: off), per-filter good / bad counters and the resident init_z (allocated by pool_config)
struct FeaturePool {
  xivo_subfilter_feat* entries = nullptr;
  xivo_hip::PoolAnchor* anchors = nullptr;
  PoolMirror mirror;
  xivo_subfilter_opts opts{};
  double remove_outlier = 0.0;
  xivo_triangulate_opts tri{};
  int* tri_counts = nullptr;        // [2][Bmax]: good, bad
  double* init_z = nullptr;         // [Bmax]
  xivo_adapt_depth_opts adapt{};
  bool adapt_on = false;
  // per-call device staging: records / pixels in, order / counts / live out. Not part of a pool's configuration -
  // xivo_hip_triangulate stages through it without a pool -, so reset() keeps it
  char* io = nullptr; size_t io_cap = 0;
  bool configured() const { return entries != nullptr; }
  int pool_max() const { return mirror.pool_max(); }
  int anchor_max() const { return mirror.anchor_max(); }
  void reset() { char* p = io; const size_t n = io_cap; *this = FeaturePool{}; io = p; io_cap = n; }
};

// MSCKF update from dropped pool entries (xivo_hip_pool_oos_*, capi_pool_oos.hip): options, the per-feature gate distances
// gamma [Bmax][oos_max], the counters [Bmax]; the list itself is the resident OOS list (OosList). B: the filters whose list the last
// collect call (host life cycle) or begin call (device life cycle) filled, 0: none; projected: its rows are in the block and not
// gated yet. The device life cycle's part, next to the pool: the anchors' creation frames anc_born [Bmax][anchor_max] and the
// observation rings hist_cnt [Bmax][pool_max], hist_anchor / hist_born [Bmax][pool_max][max_obs], hist_xp [..][max_obs][2]
struct PoolOos {
  xivo_pool_oos_opts opts{};
  double* gamma = nullptr;
  xivo_pool_oos_stats* stats = nullptr;
  int *anc_born = nullptr, *hist_cnt = nullptr, *hist_anchor = nullptr, *hist_born = nullptr;
  double* hist_xp = nullptr;
  int B = 0; bool projected = false;
  bool configured() const { return stats != nullptr; }
  int rows() const { return opts.oos_max * (2 * opts.max_obs - 3); }
};

// device life cycle (xivo_hip_life_*, "the immediate life cycle"): its options and counters [Bmax]
struct ImmediateLife {
  xivo_life_opts opts{};
  xivo_life_stats* stats = nullptr;
  bool configured() const { return stats != nullptr; }
};

// device pool life cycle (xivo_hip_pool_life_*): the pool book [Bmax][pool_max] / [Bmax][anchor_max], the counters [Bmax], what
// a frame's kernels hand each other (slot_track, ent_track, the step's xp / order / n / live); frame: the frame counter
struct PoolLife {
  bool on = false;
  xivo_pool_life_opts opts{};
  long long* ent_id = nullptr; int* ent_born = nullptr; int* anc_used = nullptr; int* anc_life = nullptr;
  xivo_pool_life_stats* stats = nullptr;
  int* slot_track = nullptr; int* ent_track = nullptr;
  double* xp = nullptr; int* order = nullptr; int* n = nullptr; unsigned char* live = nullptr;
  int frame = 0;
  bool configured() const { return on; }
};

// point-cloud world (xivo_hip_pcw_*, capi_pcw.hip): the resident worlds Xs [Bmax][npts][3] / ids [Bmax][npts] / next_id [Bmax],
// the frame's camera poses gsc [Bmax][12] with their page-locked staging and cnt [Bmax]. The producer writes the strided form of
// the track block: tracks_B is the B whose tracks the block holds (0: none), fresh whether a begin_tracks call may still
// consume them. cam: the camera of xivo_hip_pcw_camera in place of the pinhole of opts (use_cam), with its radius guard
struct World {
  xivo_pcw_opts opts{};
  double* Xs = nullptr; long long* ids = nullptr; long long* next_id = nullptr; int* cnt = nullptr;
  double* gsc = nullptr; PinnedUpload up;
  int tracks_B = 0; bool fresh = false;
  bool use_cam = false; xivo_cam cam{}; double max_radius = 0.0;
  // track faults (xivo_hip_pcw_fault_*): the options, the resident bias [Bmax][npts][2], the flag row [Bmax][tracks_max] and the
  // counters [Bmax], allocated exactly while faults are on; scored: the score ran on the tracks the block holds. stream_mod:
  // xivo_hip_pcw_stream_share
  xivo_pcw_fault_opts fault{};
  double* bias = nullptr; unsigned char* flags = nullptr; xivo_pcw_fault_stats* fstats = nullptr;
  bool scored = false; int stream_mod = 0;
  bool faults_on() const { return fstats != nullptr; }
  bool configured() const { return Xs != nullptr; }
  // what the life cycles ask and tell (capi_lifecycle.hip, capi_pool_lifecycle.hip)
  const int* track_counts() const { return cnt; }
  bool tracks_fresh_for(int B) const { return cnt && fresh && tracks_B == B; }
  void tracks_consumed() { fresh = false; }
  void tracks_overwritten() { tracks_B = 0; fresh = false; }   // (a host-track upload, or the producer about to write)
};

// trajectory producer (xivo_hip_trajsim_*, capi_trajsim.hip): curve / rate per filter [Bmax], the last frame's records
// [Bmax][n_max] (read as [B][n]) and camera poses [Bmax][12], the ground-truth log gt [T_max][Bmax][12] with its FrameLog
// (no stamps: it commits 0), the device copy of the propagation noise (Qimu 144 | Qmodel 529) with the host copy it was
// uploaded from. B / n: the shape of the last frame (B = 0: none), fresh: its records may still be consumed by
// xivo_hip_propagate_resident
struct TrajSim {
  xivo_trajsim_opts opts{};
  int* motion = nullptr; double* rate = nullptr; xivo_imu_in* recs = nullptr; double* gsc = nullptr;
  double* Q = nullptr;
  double* gt = nullptr; FrameLog log;
  xivo_prop_opts prop{}; bool prop_valid = false;
  int B = 0, n = 0; bool fresh = false;
  bool configured() const { return recs != nullptr; }
  // the camera poses of the last frame if it was one of B_ filters, else null (capi_pcw.hip)
  const double* frame_poses(int B_) const { return B == B_ ? gsc : nullptr; }
};

// The three per-frame logs: device pointers, options, the FrameLog (frame_log.h: capacity in frames, frames written, stamps),
// staging. A log's blocks are allocated exactly while its FrameLog is configured.
// trajectory log (xivo_hip_traj_*, capi_traj.hip): [capacity][Bmax] records and packed covariance blocks of cols. io: per-call
// staging of xivo_hip_traj_nees / xivo_hip_traj_score
struct TrajLog {
  xivo_traj_rec* rec = nullptr; double* cov = nullptr;
  int ncols = 0, cols[XIVO_TRAJ_MAX_COLS] = {0};
  FrameLog log;
  char* io = nullptr; size_t io_cap = 0;
  bool configured() const { return log.configured(); }
};
// landmark log (xivo_hip_map_*, capi_map.hip): [capacity][Bmax][nout] entries and [capacity][Bmax] counts. io: per-call staging of
// xivo_hip_map_nees
struct MapLog {
  xivo_map_pt* pts = nullptr; int* npts = nullptr;
  int nout = 0; unsigned flags = 0;
  FrameLog log;
  char* io = nullptr; size_t io_cap = 0;
  bool configured() const { return log.configured(); }
};
// innovation log (xivo_hip_innov_*, capi_innov.hip): [capacity][Bmax] records. io: the output staging of xivo_hip_innov_stats,
// allocated by xivo_hip_innov_config for the largest slice
struct InnovLog {
  xivo_innov_rec* rec = nullptr;
  FrameLog log;
  char* io = nullptr;
  bool configured() const { return log.configured(); }
};

// resident landmark map (xivo_hip_lcmap_*, capi_lcmap.hip): entries [Bmax][map_max], count [Bmax], the counters [Bmax], the
// last close call's match lists [Bmax][lc_max] and closing flags [Bmax]; io: the device block a call's records / queries and
// offsets are uploaded to, up: its page-locked staging (both only ever grow, up_cap bytes each). xivo_hip_lcmap_cov_config's
// options: cov [Bmax][map_max][6] while point_cov is on, visit [Bmax][map_max][2] = {last_seen, used} while revisit_gap > 0,
// their counters [Bmax] while either is; t: close calls since that configuration
struct LcMap {
  xivo_lcmap_opts opts{};
  xivo_lcmap_entry* entries = nullptr; int* count = nullptr; xivo_lcmap_stats* stats = nullptr;
  xivo_lcmap_match* matches = nullptr; int* closing = nullptr;
  xivo_lcmap_cov_opts cov_opts{};
  double* cov = nullptr; int* visit = nullptr; xivo_lcmap_cov_stats* cov_stats = nullptr;
  int t = 0;
  char* io = nullptr; size_t io_cap = 0;
  PinnedUpload up; size_t up_cap = 0;
  bool configured() const { return entries != nullptr; }
};

// loop closure inside the device life cycle (xivo_hip_lcmap_life_config, capi_lcmap.hip): keys [Bmax][tracks_max] beside the
// track block (in the form the tracks are in) with their page-locked staging; feat_key [Bmax][book.ld] beside the book's
// feat_id; the frame's add records recs [Bmax][book.ld] / n_recs [Bmax] and queries / n_queries of the same shape; tracked
// [Bmax][book.ld] and rm [Bmax][2 + book.ld + n_groups], which the begin kernel leaves for the close and the add call; status
// [Bmax], the first update's. stage: where the open frame stands
struct LcLife {
  enum Stage { kNone = 0, kBegun, kAdded, kClosed };
  long long* keys = nullptr; PinnedUpload up;
  long long* feat_key = nullptr;
  xivo_lcmap_add_rec* recs = nullptr; int* n_recs = nullptr;
  xivo_lcmap_query* queries = nullptr; int* n_queries = nullptr;
  unsigned char* tracked = nullptr; int* rm = nullptr; int* status = nullptr;
  Stage stage = kNone;
  bool configured() const { return feat_key != nullptr; }
};

// tuning table (xivo_hip_tune_*, capi_tune.hip): one array [Bmax] per field, all five or none; up: the page-locked staging of
// a set call. While configured() the in-state gate, the stacking, propagation and life_end are handed the arrays and read
// filter b's entry in place of their scalar arguments
struct TuneTable {
  double *R = nullptr, *thresh = nullptr, *var = nullptr, *Qimu = nullptr, *Qmodel = nullptr;
  PinnedUpload up;
  bool configured() const { return R != nullptr; }
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
  // G-level: layout, camera, the scene (poses, groups, feats, J, finn, dist, mask of F of Fmax features)
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
  xivo_group_in* groups = nullptr;
  xivo_feat_in* feats = nullptr;
  double *J = nullptr, *finn = nullptr, *dist = nullptr;
  unsigned char* mask = nullptr;
  int* rows_instate = nullptr;
  double* pd_h = nullptr; double pd_h0 = 0.0;   // step-size-controlled Dormand-Prince: the step each filter carries (xivo_hip_propagate)
  // online-calibration builds on the sparse pipeline (round 5): the calibration columns of the stacked rows as a dense
  // [Mpmax x LEAD_K] block per filter next to the row-pair compressed rows (rows.has_lead(): the current stacking has one)
  xivo_hip::capi::BatchMat Hlead;
  char* lc_buf = nullptr; size_t lc_cap = 0;   // xivo_hip_close_loop_stack: matches | dense rows | inn | diagR
  xivo_subfilter_feat* sub = nullptr; size_t sub_cap = 0;   // staging of xivo_hip_subfilter_update (entries)
  // dx_ok[b]: the err buffer of filter b holds the dx of the rows staged for it right now (set by the update calls for the filters
  // they update; cleared by absorb, new rows, restore_P) - an innovation record of filters [0, B) needs it of every one of them
  std::vector<char> dx_ok;
  void dx_set(int b0, int nb, bool v) { if (dx_ok.size() != (size_t)Bmax) dx_ok.assign((size_t)Bmax, 0); std::fill_n(dx_ok.begin() + b0, nb, (char)v); }
  void dx_clear() { std::fill(dx_ok.begin(), dx_ok.end(), (char)0); }
  bool dx_current(int B) const { return dx_ok.size() >= (size_t)B && std::all_of(dx_ok.begin(), dx_ok.begin() + B, [](char v) { return v != 0; }); }
  // the device life cycles (capi_lifecycle.hip, capi_pool_lifecycle.hip; at most one of the two is configured): the in-state book
  // and the track block of whichever is, both null when neither
  xivo_hip::capi::InstateBookBuffers book;
  xivo_hip::capi::TrackBlock tracks;
  std::vector<char> hstage;                        // host staging of d2h_rows
  char* edit_buf = nullptr; size_t edit_cap = 0;   // device copy of the ops of xivo_hip_edit_batch
  // one-filter plumbing call (xivo_hip_update_joseph_host): page-locked, device-mapped staging block owned by the context,
  // scratch of the host-side row compression
  char* pin_h = nullptr; char* pin_d = nullptr;
  struct HostCompressScratch { std::vector<int> cnt, occ, cslot, n; std::vector<double> v; } hc;
  // one record per area (above)
  xivo_hip::capi::Profiler prof;
  xivo_hip::capi::RansacScratch rs;
  xivo_hip::capi::OosList resident_oos;
  xivo_hip::capi::FeaturePool pool;
  xivo_hip::capi::PoolOos pool_oos;
  xivo_hip::capi::ImmediateLife life;
  xivo_hip::capi::PoolLife plife;
  xivo_hip::capi::World world;
  xivo_hip::capi::TrajSim trajsim;
  xivo_hip::capi::TrajLog traj;
  xivo_hip::capi::MapLog map;
  xivo_hip::capi::InnovLog innov;
  xivo_hip::capi::LcMap lcmap;
  xivo_hip::capi::LcLife lclife;
  xivo_hip::capi::TuneTable tune;
  // "a device life cycle exists" (whichever: the book and the track block are its)
  bool life_cycle_configured() const { return life.configured() || plife.configured(); }
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
    Profiler& p = c->prof;
    p.bytes[stage] = bytes;
    if (kernel) { strncpy(p.kernel[stage], kernel, 63); p.kernel[stage][63] = 0; }
    if (p.used >= p.events.size()) {
      EventPair np; np.stage = stage;
      if (hipEventCreate(&np.a) != hipSuccess || hipEventCreate(&np.b) != hipSuccess) return;
      p.events.push_back(np);
    }
    ep = &p.events[p.used++];
    ep->stage = stage;
    p.launches[stage]++;
    p.flops[stage] = flops;
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

// Gate parameters that cannot mean anything, refused before anything is uploaded or launched (every gating entry point and
// OnePointRANSAC): a measurement variance R that is not a positive finite number (S = J P J^T + R I2 is then no covariance), a
// NaN threshold (every comparison false), and a relaxation factor that is NaN or below 1 - the reference's loop
// (src/update.cpp:73-96) then shrinks its threshold and never ends; the device's 4096-pass guard would return an empty
// mask that no run of the reference produces. mult = 1 is accepted and pinned as coded (the guard ends it).
// (OnePointRANSAC has no relaxation: it hands its R and threshold over with mult = 1)
inline bool bad_gate_params(const GateParams& gp) {
  return !(gp.R > 0.0) || gp.R > 1.7976931348623157e308 || gp.thresh != gp.thresh || !(gp.mult >= 1.0);
}

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
// the two blocks of a log whose record was just reset (its old blocks given back, the stream idle), for T_max frames: for
// T_max > 0 na / nb elements behind *a / *b - both or neither - and the log configured
template <class A, class B> int log_alloc(xivo_hip_ctx* c, FrameLog& log, int T_max, A** a, size_t na, B** b, size_t nb) {
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

// ---- capi_lcmap.hip
// loop closure inside the device life cycle (LcLife above). Everything xivo_hip_lcmap_life_config allocated goes back (the
// stream must be idle): called by whoever releases the track block or the map
void lclife_release(xivo_hip_ctx* c);
// the begin calls' part: the frame's keys to the key block (keys null: every track gets lclife_no_key()), in the packed form
// of n tracks - behind track_block_upload; and what the life cycle's kernels take of the option (nothing while it is off)
int lclife_upload_keys(xivo_hip_ctx* c, int n, const long long* keys);
void lclife_args(xivo_hip_ctx* c, LifeArgs& a);

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

// ---- capi_pool.hip
// the arguments of one pool step but xp / order / n / live (xivo_hip_pool_step and the device pool life cycle share them)
PoolStepArgs pool_step_args(xivo_hip_ctx* c, int B, int strict);

// ---- capi_oos.hip
// the two halves of an OOS append that xivo_hip_oos_project_ex and xivo_hip_pool_oos_project share. oos_rows_begin: max_rows more
// rows fit behind the staged ones (else XIVO_HIP_ERR_INVALID); *mixed: the mixed stacking applies (the block's columns are
// cleared), else every row is made dense. oos_rows_launch: oos_kernel over the resident list of n_oos features per filter into
// rows from M on; enqueues only
int oos_rows_begin(xivo_hip_ctx* c, int b0, int nb, int max_rows, bool* mixed);
int oos_rows_launch(xivo_hip_ctx* c, int nb, int n_oos, int M, double Roos, int whole, bool mixed);

// ---- capi_pool_oos.hip
void pool_oos_release(xivo_hip_ctx* c);   // everything xivo_hip_pool_oos_config allocated (the stream must be idle)
// the device pool life cycle's two hooks (no-ops unless xivo_hip_pool_oos_config is on; enqueue only): the frame's list between
// the begin kernel and the pool step of a frame of B filters, and the frame's observations behind the end kernel of frame `frame`
int pool_oos_life_select(xivo_hip_ctx* c, int B);
int pool_oos_life_record(xivo_hip_ctx* c, int B, int frame);

// ---- capi_glevel.hip
int ensure_gate_buffers(xivo_hip_ctx* c, int F);
// the stacking of the gated scene of filters [0, B) (mask_override: another mask than the scene's, full_rows: the whole rows J()
// of the dense-row gate / RANSAC). The gate helpers next to it (gate_impl, calib_gate) have no caller outside capi_glevel.hip
int stack_impl(xivo_hip_ctx* c, int B, double R, int write_dense, unsigned char* mask_override = nullptr, int full_rows = 0);
int ensure_dense(xivo_hip_ctx* c);
int ensure_HT(xivo_hip_ctx* c);
// H P (+ P H^T) of the stacked dense rows of filters [0, B) and the dense-row gate on them (gate_dense_kernel); `a` brings the
// gate's own parameters and outputs, the row buffers are filled in here
int gate_dense_rows(xivo_hip_ctx* c, int B, GateDenseArgs a);

}  // namespace xivo_hip::capi
#pragma GCC visibility pop
