// Launchers of the EKF-specific (non-GEMM) kernels, one section per translation unit: state_kernels.hip,
// traj_kernels.hip, score_kernels.hip, map_kernels.hip, glevel_kernels.hip, gate_kernels.hip, pool_kernels.hip, propagate_kernels.hip, then ldlt_fallback.hip and dropin.hip.
#pragma once
#include "common.h"
#include "ell.h"
#include "../../include/xivo_hip.h"
#include "trajsim_device.h"

namespace xivo_hip {

struct PoolAnchor;   // pool_kernels.hip section

// ================================================================ state_kernels.hip: resident-state plumbing

// raw (n x n, ld = n, contiguous per filter) <-> padded (ld = ldp) covariance
int launch_unpack_P(const double* raw, double* P, int N, int Np, int ldp, long strideP, int batch,
                    hipStream_t s);
int launch_pack_P(const double* P, double* raw, int N, int ldp, long strideP, int batch, hipStream_t s);

// raw H (M x N, ld = M), inn (M), diagR (M)  ->  padded H (Mp x Np, ld ldh),
// H^T (Np x Mp, ld ldht), inn (Mp, zero pad), diagR (Mp, pad = 1)
struct MeasBuffers {
  double* H; long strideH; int ldh;
  double* HT; long strideHT; int ldht;
  double* inn; long strideInn;
  double* diagR; long strideR;
};
int launch_unpack_meas(const double* rawH, long strideRaw, int ldraw, const int* only_if, MeasBuffers mb,
                       int M, int Mp, int N, int Np, int batch, hipStream_t s);
// H^T rebuilt from the dense H of every filter (the G-level producers may skip writing it: staged_rows.h, ht_alive)
int launch_transpose_H(const double* H, long strideH, int ldh, double* HT, long strideHT, int ldht, int Mp, int Np, int batch,
                       hipStream_t s);

// P edits
int launch_p_zero_rc(double* P, int ldp, int Np, int off, int len, hipStream_t s);
int launch_p_copy_rc(double* P, int ldp, int Np, int dst, int src, int len, hipStream_t s);
int launch_p_diag(const double* P, int ldp, int N, double* out, hipStream_t s);

// batched resident edits (xivo_hip_edit_batch): wg_filter[w] = filter of workgroup w, its ops are
// ops[wg_begin[w] .. wg_begin[w + 1])
struct EditArgs {
  const xivo_edit_op* ops; const int* wg_filter; const int* wg_begin;
  double* P; long strideP; int ldp, Np; xivo_layout lay;
  xivo_pose_in* poses; xivo_group_in* groups; xivo_feat_in* feats; int Fmax;
  xivo_subfilter_feat* pool; PoolAnchor* anchors; int pool_max, anchor_max;   // null / 0: no pool configured
};
int launch_edit_batch(const EditArgs& a, int n_wg, hipStream_t s);
int launch_set_pixels(xivo_feat_in* feats /* already offset to b0 */, int Fmax, int F, const double* xp, int nb, hipStream_t s);

// AbsorbError on the resident scene (estimator.cpp:875-921)
struct AbsorbArgs {
  xivo_pose_in* poses; xivo_group_in* groups; xivo_feat_in* feats; const unsigned char* mask;
  double* err; long strideErr; xivo_layout lay; int F, Fmax, batch;
  const int* status;   // [batch] factorisation status of the update that produced err: non-zero -> nothing is absorbed, err <- 0
  const unsigned long long* group_mask;   // optional [batch]: bit g = group slot g is in instate_groups_ (null: every slot)
  int* counter;   // [batch] State::counter (core.h:120-122): absorbs so far, drives the periodic SO3 re-normalisation
  xivo_calib_in* calib; xivo_calib_layout cl;   // online-calibration builds: td / Cg / Ca / intrinsics retracted too (null: default build)
};
int launch_absorb_error(const AbsorbArgs& a, hipStream_t s);

int launch_mfma_peak(double* sink, int iters, int blocks, hipStream_t s);

// ================================================================ traj_kernels.hip: trajectory log (capi_traj.hip)

// one frame of the log: rec / cov already point at the frame; pack = n_cols (n_cols + 1) / 2 doubles per filter
struct TrajRecordArgs {
  const xivo_pose_in* poses; const int* status; const double* P; long strideP; int ldp;
  xivo_traj_rec* rec; double* cov; int n_cols, pack; int cols[XIVO_TRAJ_MAX_COLS];
};
int launch_traj_record(const TrajRecordArgs& a, int batch, hipStream_t s);
// NEES of the slice frames [t0, t0 + nt) x filters [b0, b0 + nb) against gt [nt][nb][12]; pos6[k] = list position of
// error-state column k; outputs err6 [nt][nb][6], nees [nt][nb], anees [nt], n_used [nt] (device)
struct TrajNeesArgs {
  const xivo_traj_rec* rec; const double* cov; int Bmax, pack, b0, nb, t0, nt; int pos6[6];
  const double* gt; double* err6; double* nees; double* anees; int* n_used;
};
int launch_traj_nees(const TrajNeesArgs& a, hipStream_t s);
// anees [nt], n_used [nt] = mean and number of the finite values of every frame of nees [nt][per], in one fixed summation order
// (what launch_traj_nees and launch_map_nees both end with)
int launch_frame_anees(const double* nees, long per, int nt, double* anees, int* n_used, hipStream_t s);

// ================================================================ score_kernels.hip: trajectory score (capi_score.hip)

// aligned / unaligned ATE and RPE of the slice frames [t0, t0 + nt) x filters [b0, b0 + nb) against gt [nt][nb][12];
// out [nb] (device). One wave per filter: returns non-zero without launching when nb does not fit a grid dimension
struct TrajScoreArgs {
  const xivo_traj_rec* rec; int Bmax, b0, nb, t0, nt, align, rpe_lag;
  const double* gt; xivo_traj_score* out;
};
int launch_traj_score(const TrajScoreArgs& a, hipStream_t s);

// ================================================================ map_kernels.hip: landmark log (capi_map.hip)

// one frame of the log: pts / n_pts already point at the frame ([batch][n_out] entries, [batch] counts). F = length of the
// resident feature list (<= XIVO_MAP_MAX_OUT), world = XIVO_MAP_WORLD_COV
struct MapRecordArgs {
  const xivo_pose_in* poses; const xivo_group_in* groups; const xivo_feat_in* feats; int F, Fmax;
  const double* P; long strideP; int ldp; xivo_layout lay; int invdepth, world;
  xivo_map_pt* pts; int* n_pts; int n_out;
};
int launch_map_record(const MapRecordArgs& a, int batch, hipStream_t s);
// NEES of the slice frames [t0, t0 + nt) x filters [b0, b0 + nb) x n_out slots against gt [nt][nb][n_out][3]; outputs
// err3 [nt][nb][n_out][3] (may be null), nees [nt][nb][n_out], anees [nt], n_used [nt] (device)
struct MapNeesArgs {
  const xivo_map_pt* pts; const int* n_pts; int Bmax, n_out, b0, nb, t0, nt;
  const double* gt; double* err3; double* nees; double* anees; int* n_used;
};
int launch_map_nees(const MapNeesArgs& a, hipStream_t s);

// ================================================================ innov_kernels.hip: innovation log (capi_innov.hip)

// one frame of the log: rec already points at the frame. Rows of filter b: dense (dense_all, or over[b] != 0) - all M rows from
// H; else rows [0, ell_rows) row-pair compressed (+ the lead block's lead_k leading columns when lead != null) and rows
// [ell_rows, M) dense from H (the mixed stacking's OOS rows)
struct InnovRecordArgs {
  const int* ell_idx; const double* ell_val; const int* over; long stride_idx, stride_val;
  const double* H; long strideH; int ldh;
  const double* lead; long strideLead; int ldlead, lead_k;
  const double* inn; long strideInn; const double* diagR; long strideR; const double* err; long strideErr;
  const int* status; const int* ldlt_used;
  int M, N, ell_rows, dense_all;
  xivo_innov_rec* rec;
};
int launch_innov_record(const InnovRecordArgs& a, int batch, hipStream_t s);
size_t innov_record_lds(int M, int N);   // dynamic LDS of that launch; over 48 KiB (N + M beyond ~6000) it is refused
// sums of nis / dof over the records that enter the statistic (innov_in_stats): group g of n_groups adds its n_elems records
// rec[base + g * g_stride + e * e_stride], e ascending per thread of 256 (e = t, t + 256, ...), then a fixed tree
struct InnovStatsArgs {
  const xivo_innov_rec* rec; long base, g_stride, e_stride; int n_groups, n_elems;
  double* nis; long long* dof; int* used;
};
int launch_innov_stats(const InnovStatsArgs& a, hipStream_t s);

// ================================================================ lifecycle_kernels.hip: device life cycle (capi_lifecycle.hip)

// one frame of every filter [0, batch): the resident scene and P, the filter's book (feat_id [batch][slot_ld], group_refs
// [batch][n_groups], counters [batch]) and the frame's tracks (off [batch + 1]; ids, meas [off[batch]][3]). F <= slot_ld,
// F <= XIVO_LIFE_MAX_SLOTS, n_groups <= XIVO_LIFE_MAX_SLOTS, every filter's track count <= XIVO_LIFE_MAX_TRACKS (the host
// checks all four before a launch).
// The tracks come in one of two forms. Packed (cnt == nullptr): filter b's are ids[off[b] + k], meas[3 (off[b] + k)], k <
// off[b + 1] - off[b] - what the host uploads. Strided (cnt != nullptr; off is not read): ids[b track_ld + k],
// meas[3 (b track_ld + k)], k < cnt[b] - what pcw_tracks_kernel leaves, which cannot know the other filters' counts.
struct LifeArgs {
  double* P; long strideP; int ldp, Np; xivo_layout lay;
  const xivo_pose_in* poses; xivo_group_in* groups; xivo_feat_in* feats; int Fmax, F;
  long long* feat_id; int slot_ld; int* group_refs; xivo_life_stats* stats;
  const int* off; const long long* ids; const double* meas;
  const int* cnt; int track_ld;
  // life_end only: the update's inlier mask (row stride mask_ld) and status, the admission options, the camera
  const unsigned char* mask; int mask_ld; const int* status;
  int min_new_features, invdepth; double min_depth, max_depth, var_xyz[3], fx, fy, cx, cy;
  const double* tune_var;   // tuning table: [batch][3], filter b's variances in place of var_xyz (null: var_xyz)
  // loop closure inside the life cycle (xivo_hip_lcmap_life_config; all null while it is off, and always in the pool life cycle):
  // keys - one per track, indexed as ids; feat_key [batch][slot_ld]; what the begin kernel leaves for the add and the close call:
  // lc_recs [batch][slot_ld] / lc_n_recs [batch] the add records, lc_tracked [batch][slot_ld], lc_rm [batch][2 + slot_ld +
  // n_groups] = n_rm_feat, n_rm_group, rm_feat, rm_group - the removals it decided and life_lc_apply_kernel makes
  const long long* keys; long long* feat_key;
  xivo_lcmap_add_rec* lc_recs; int* lc_n_recs; unsigned char* lc_tracked; int* lc_rm;
};
int launch_life_begin(const LifeArgs& a, int batch, hipStream_t s);
int launch_life_end(const LifeArgs& a, int batch, hipStream_t s);
int launch_life_lc_apply(const LifeArgs& a, int batch, hipStream_t s);

// ================================================================ pool_lifecycle_kernels.hip: device pool life cycle (capi_pool_lifecycle.hip)

// one frame of every filter [0, batch) in the "subfilter" mode. life: P, the scene, the in-state book, the tracks, the mask and
// the status as the immediate life cycle's kernels take them (life.stats and its admission options are not read). The pool
// book: ent_id / ent_born [batch][pool_max], anc_used / anc_life [batch][anchor_max]. Between the kernels of a frame:
// slot_track [batch][slot_ld] and ent_track [batch][pool_max] (the track that feeds a slot / an entry, -1: none), the step's
// xp in, order / n / live out. pool_max <= XIVO_POOL_MAX_ENTRIES, anchor_max <= XIVO_POOL_LIFE_MAX_ANCHORS and LifeArgs' limits
// (the host checks all before a launch).
struct PoolLifeArgs {
  LifeArgs life;
  xivo_subfilter_feat* pool; PoolAnchor* anchors; int pool_max, anchor_max;
  long long* ent_id; int* ent_born; int* anc_used; int* anc_life; xivo_pool_life_stats* stats;
  int* slot_track; int* ent_track;
  double* xp; const int* order; const int* n; const unsigned char* live;
  int frame;   // the frame counter (vision_counter)
  // pool_life_end only: EnforceMaxGroupLifetime's bound, Feature::Initialize of a new entry
  int max_group_lifetime; double initial_z, std_xyz[3]; const double* init_z;   // init_z non-null: z0 is the resident init_z
  xivo_cam cam; const xivo_calib_in* calib; int cam_dim;
};
int launch_pool_life_begin(const PoolLifeArgs& a, int batch, hipStream_t s);
int launch_pool_life_admit(const PoolLifeArgs& a, int batch, hipStream_t s);
int launch_pool_life_end(const PoolLifeArgs& a, int batch, hipStream_t s);

// ================================================================ pcw_kernels.hip: the point-cloud world's track producer (capi_pcw.hip)

// one frame of the worlds of filters [0, batch): Xs [batch][npts][3], ids [batch][npts] (-1: no track), next_id [batch] and the
// frame's camera poses gsc [batch][12] (Rsc row-major, Tsc) -> the strided track block (track_ids / track_meas, row length
// track_ld >= npts) and cnt [batch]; the rules are pcw_device.h
struct PcwArgs {
  const double* Xs; long long* ids; long long* next_id; const double* gsc; int npts;
  double fx, fy, cx, cy, imw, imh, noise_px_std; unsigned long long seed, frame;
  long long* track_ids; double* track_meas; int* cnt; int track_ld;
  long long* track_keys;   // null, or [batch][track_ld]: the world-point index of every track (xivo_hip_lcmap_life_config)
  int use_cam; xivo_cam cam; double max_radius;   // use_cam != 0 (xivo_hip_pcw_camera): project through cam instead of fx .. imh
  // The fault path (pcw_device.h "Track faults"), its own instances of the kernel: launched when fault_path != 0, which the host
  // sets when faults are configured or a stream is shared; the instances without it read none of these fields. t1 .. sticky: PcwFault
  // (all 0: no event ever); stream_mod: pcw_stream_filter; bias [batch][npts][2] (sticky only), flags [batch][track_ld] and
  // fstats [batch] may be null (faults off, a shared stream alone)
  int fault_path, sticky, stream_mod;
  double t1, t2, t3, outlier_min_px, outlier_max_px, tail_scale;
  double* bias; unsigned char* flags; xivo_pcw_fault_stats* fstats;
};
int launch_pcw_tracks(const PcwArgs& a, int batch, hipStream_t s);

// the score of one frame of filters [0, batch) (xivo_hip_pcw_fault_score): life - the book (feat_id, slot_ld, F), the strided
// tracks of the open frame and the update's mask as the life cycles' end kernels take them; flags [batch][life.track_ld] as the
// producer left them; the four cells are added to stats [batch]
struct PcwScoreArgs { LifeArgs life; const unsigned char* flags; xivo_pcw_fault_stats* stats; };
int launch_pcw_fault_score(const PcwScoreArgs& a, int batch, hipStream_t s);

// ================================================================ trajsim_kernels.hip: the trajectory producer (capi_trajsim.hip)

// One frame of filters [0, batch): records k0 + 1 .. k0 + n as recs [batch][n], and at t_{k0 + n} the camera poses gsc [batch][12]
// and the body poses gt [batch][12] (the frame's row of the ground-truth log). The rules: trajsim_device.h
struct TrajsimArgs {
  TrajsimModel m; const int* motion; const double* rate;   // [batch]
  unsigned long long k0; int n, batch;
  xivo_imu_in* recs; double* gsc; double* gt;
};
int launch_trajsim_frame(const TrajsimArgs& a, hipStream_t s);

// ================================================================ glevel_kernels.hip: feature-level kernels (capi_glevel.hip)

struct SceneBuffers {
  const xivo_pose_in* poses;     // [batch]
  const xivo_group_in* groups;   // [batch x n_groups]
  const xivo_feat_in* feats;     // [batch x Fmax]
  double* J;                     // [batch x Fmax x 42]  (2 x 21 row-major)
  double* finn;                  // [batch x Fmax x 2]
  unsigned char* mask;           // [batch x Fmax]
  double* dist;                  // [batch x Fmax]
  int Fmax, F;
  // online-calibration builds (include/xivo_hip.h, xivo_hip_set_calib): null / td = -1, cam_dim = 0 when switched off
  const xivo_calib_in* calib;    // [batch]
  double* Jc;                    // [batch x Fmax x 44]  (2 x 22 row-major: td | Cg 9 | bg 3 | intrinsics 9)
  xivo_calib_layout cl;
  int invdepth;                  // XIVO_HIP_FLAG_INVDEPTH: features are (X/Z, Y/Z, 1/Z) (USE_INVDEPTH build, feature.cpp:98-105)
};
int launch_jac_instate(const SceneBuffers& sb, const xivo_layout& lay, const xivo_cam& cam, int batch,
                       hipStream_t s);
struct StackArgs {
  SceneBuffers sb; xivo_layout lay; MeasBuffers mb;
  int Mp, Np, batch; double R; int fix_group_block;
  int* rows_instate;   // [batch] out: 2 * F (rows reserved for in-state features)
  EllBuffers ell; int emit_ell;   // also emit the row-pair compressed form (ell.h)
  int write_dense;                // 0: only inn / diagR / ELL (the dense H, H^T are materialised on demand)
  // online-calibration builds on the sparse pipeline: [batch] dense blocks [Mp x lead_k] (leading dimension Mp) that take the
  // calibration columns of every row pair; null: those builds stack dense rows
  double* lead; long strideLead; int lead_k;
  const double* tune_R;   // tuning table: [batch], filter b's R in place of R (null: R)
};
int launch_stack(const StackArgs& a, hipStream_t s);

// OOS (MSCKF) rows: oos.cpp:39-89 + helpers.cpp:13-23
struct OosArgs {
  const xivo_oos_in* feats; int n_oos;          // [batch x n_oos]
  const xivo_pose_in* poses; const xivo_group_in* groups;
  xivo_layout lay; xivo_cam cam; MeasBuffers mb;
  const xivo_calib_in* calib; int cam_dim;   // online camera calibration: per-filter intrinsics (null / 0: the context's camera)
  int row0;            // first free row (after the in-state rows)
  int Mp, Np, batch; double Roos;
  int* rows_out;       // [batch]
  int whole;           // 0, or the 2 kMaxGroup rows of the reference's per-feature buffers (XIVO_HIP_OOS_WHOLE_BUFFER)
};
int launch_oos(const OosArgs& a, hipStream_t s);

// the fixed OOS block of the pool's MSCKF update (xivo_hip_pool_oos_project / _gate): the rows [row0, row0 + rows) of every filter
// start as inn = 0, diagR = Roos (oos_kernel then overwrites the rows a feature fills)
int launch_oos_block_init(const MeasBuffers& mb, int row0, int rows, double Roos, int batch, hipStream_t s);
// chi-square gate of the projected rows, one workgroup per (filter, list position)
struct OosGateArgs {
  const xivo_oos_in* feats; int n_oos;          // [batch x n_oos], the list oos_kernel projected
  xivo_layout lay;
  double* H; long strideH; int ldh;             // dense rows (no H^T: the mixed stacking keeps none)
  double* inn; long strideInn;
  const double* P; long strideP; int ldp;
  int row0, Mp; double Roos;
  double chi2[32];
  double* gamma;                                // [batch x n_oos]
  long long* gated;                             // per filter counter, stride gated_stride (in long long)
  int gated_stride, batch;
};
int launch_oos_gate(const OosGateArgs& a, hipStream_t s);

// loop-closure rows: oos.cpp:92-145 + the stacking of update.cpp:183-196
struct LcArgs {
  const xivo_lc_match* matches; int n;          // [batch x n]
  const xivo_pose_in* poses; const xivo_group_in* groups; const xivo_feat_in* feats; int Fmax;
  xivo_layout lay; xivo_cam cam; const xivo_calib_in* calib; xivo_calib_layout cl; int invdepth;
  double* H; long strideH; int ldh;             // [batch] 2n x N column-major, zero-filled
  double* inn; double* diagR; long strideV;     // [batch] 2n each
  double Rlc; int batch;
};
int launch_lc_rows(const LcArgs& a, hipStream_t s);

// the resident landmark map (xivo_hip_lcmap_*, lcmap_kernels.hip). What both kernels take of it: entries [batch][map_max],
// count [batch], the counters [batch]
struct LcMapBuffers {
  xivo_lcmap_entry* entries; int* count; xivo_lcmap_stats* stats; int map_max;
};
// what xivo_hip_lcmap_cov_config adds, parallel to the entries: cov [batch][map_max][6] (null: the points are exact), visit
// [batch][map_max] {last_seen, used} (null: gap = 0), the counters [batch]; t: the number of this close call. on(): either
// option is set - the launchers then take the kernels' second instantiation, else the first, which never reads this
struct LcMapCovBuffers {
  double* cov; int* visit; xivo_lcmap_cov_stats* stats; int gap, t;
  bool on() const { return cov != nullptr || visit != nullptr; }
};
// add: the records of filter b are recs[off[b], off[b + 1])
struct LcMapAddArgs {
  LcMapBuffers map;
  const xivo_lcmap_add_rec* recs; const int* off;
  const xivo_pose_in* poses; const xivo_group_in* groups; const xivo_feat_in* feats; int Fmax, F;
  xivo_layout lay; int invdepth;
  const double* P; long strideP; int ldp;
  double max_depth_var; int batch;
  LcMapCovBuffers ext;   // (the arguments before it keep their places)
  // the resident form (xivo_hip_lcmap_add_resident): cnt non-null - off is not read, the records of filter b are
  // recs[b row, b row + cnt[b]) (lclife_list_pos, lcmap_life_device.h)
  const int* cnt; int row;
};
int launch_lcmap_add(const LcMapAddArgs& a, hipStream_t s);
// close: match, rows, verify. The queries of filter b are queries[off[b], off[b + 1]); H [batch] 2 lc_max x N zero-filled
struct LcMapCloseArgs {
  LcMapBuffers map;
  const xivo_lcmap_query* queries; const int* off;
  const xivo_pose_in* poses; const xivo_group_in* groups;
  xivo_layout lay; xivo_cam cam;
  // always {-1, -1, 0, 0} (no online calibration here), but a run-time value: lc_row_pair is then compiled as in lc_rows_kernel,
  // intrinsics branch included, and rounds as it does there (a product shared with that branch is not fused into an fma)
  xivo_calib_layout cl;
  const double* P; long strideP; int ldp;
  double* H; long strideH; int ldh;
  double* inn; double* diagR; long strideV;
  xivo_lcmap_match* matches;   // [batch][lc_max]
  int* closing;                // [batch] 1: the filter closes
  int lc_max, min_matches; double Rlc, chi2; int batch;
  LcMapCovBuffers ext;         // (the arguments before it keep their places)
  const int* cnt; int row;     // the resident form (xivo_hip_lcmap_close_resident), as LcMapAddArgs'
};
int launch_lcmap_close(const LcMapCloseArgs& a, hipStream_t s);
// the queries of a frame of the device life cycle, made where the book is (xivo_hip_lcmap_close_resident): per filter one query
// per slot lclife_queries names, in slot order, into queries [batch][slot_ld] / n_queries [batch]; the update's status of every
// filter is copied to status_out, where the second update does not reach it
struct LcLifeQueryArgs {
  const long long* feat_id; const long long* feat_key; int slot_ld;
  const unsigned char* tracked; const unsigned char* mask; int mask_ld;
  const xivo_feat_in* feats; int Fmax, F;
  const int* status; int* status_out;
  xivo_lcmap_query* queries; int* n_queries; int batch;
};
int launch_lclife_queries(const LcLifeQueryArgs& a, hipStream_t s);

// measurement compression of the appended OOS rows (estimator.h:399-402, helpers.cpp:77-101)
struct OosCompressArgs {
  xivo_layout lay; MeasBuffers mb;
  int row0;              // first OOS row
  const int* rows;       // [batch] OOS rows of each filter (as written by launch_oos)
  int* rows_out;         // [batch] rows after compression (may alias rows)
  double ratio, Roos;
  int batch;
};
// the instantiation for n_groups group slots (6 + 6 n_groups candidate columns + the residual) and rows_max rows:
// 0 <36,1> (<= 64 columns, <= 144 rows), 1 <64,1> (<= 64, <= 256), 2 <36,2> (<= 128, <= 144), -1 none is built
int oos_compress_pick(int n_groups, int rows_max, char* label, size_t n);
// returns -1 (nothing launched) when the block is larger than the built instantiations
int launch_oos_compress(const OosCompressArgs& a, int rows_max, hipStream_t s);

// xivo::Givens / xivo::QR (helpers.cpp:27-101), one wave per problem, in place
struct GivensArgs {
  double* x; double* Hx; double* Hf;   // per problem: x [rows], Hx [rows x nx], Hf [rows x nf] (null for QR)
  int rows, nx, nf, eff, batch, qr;
};
int launch_givens(const GivensArgs& a, hipStream_t s);

// Estimator::OnePointRANSAC on the resident state (update.cpp:213-393): selection, P zeroing, rescue test
struct RansacArgs {
  SceneBuffers sb; xivo_layout lay;
  const double* P; long strideP; int ldp; int Np;
  double R, thresh, chi2;
  const int* gauge;                 // [batch] slot of gauge_group_ptr_ (-1: none), may be null
  unsigned char* low;               // [batch x Fmax] out: low-innovation set (all 0 for filters in state 0 / 2)
  const unsigned char* low_keep;    // rescue: the set select found (a copy - `low` doubles as the stacking mask)
  unsigned long long* zero_groups;  // [batch] out
  int* state;                       // [batch] out: 0 nothing to do, 1 partial update + rescue, 2 rescue against the prior
  unsigned char* keep; double* chi; int* n_rejected;   // rescue outputs
  int batch;
};
int launch_ransac_select(const RansacArgs& a, hipStream_t s);
int launch_ransac_zero(const RansacArgs& a, double* P, hipStream_t s);
int launch_ransac_rescue(const RansacArgs& a, hipStream_t s);
int launch_ransac_rescue_dist(const RansacArgs& a, const double* dist /* [batch x ld] */, int ld, hipStream_t s);

// ================================================================ gate_kernels.hip: the stand-alone MH gates (capi_glevel.hip, capi_update.hip, capi_ransac.hip)
// (gate_ell_kernel, the third of them, takes the compressed rows: its arguments and launcher are in ell.h)

struct GateArgs {
  SceneBuffers sb; xivo_layout lay;
  const double* P; long strideP; int ldp;
  GateParams gp; int batch; int use_gating;
  const double* tune_R; const double* tune_thresh;   // tuning table: [batch] each, filter b's R / thresh in place of gp's (both null: gp's)
};
int launch_gate_sparse(const GateArgs& a, hipStream_t s);
// the launch choices below are made here only: the launch and xivo_hip_selftest_glevel_launch (capi_glevel.hip) call the same
// functions. Each writes the stage label (the kernel as rocprofv3 names it; the gate's block size after an '@') to label[n].
// gate_sparse_kernel: threads per filter - 1024 below 256 filters, 256 from there, halved while the LDS passes 64 KB
// (online-calibration builds, wide != 0, carry more scratch per wave)
int gate_sparse_threads(int batch, int F, int wide, char* label, size_t n);

// dense-row Mahalanobis gating (update.cpp:60-96) + neutralising rejected rows
struct GateDenseArgs {
  // candidate rows (J of feature f = rows 2f, 2f+1): H [Mp x Np] and H^T [Np x Mp], read through H^T and neutralised in both
  double* Hw; long strideH; int ldh;
  double* HTw; long strideHT; int ldht;
  double* HPw; long strideHP; int ldhp;              // optional: H P / (HP)^T rows to neutralise too (PHTw: strides of H^T)
  double* PHTw;
  const double* PHTr;                                // (HP)^T = P H^T of the candidate rows [Np x Mp]
  double* inn; long strideInn;
  double* diagR; long strideR;
  unsigned char* mask; double* dist;            // [batch x F]  (row stride mask_ld when it is set)
  int F, Np, batch;
  GateParams gp;
  EllBuffers ell; int have_ell;                 // also zero the rejected pairs of the compressed form (ell.h)
  int mask_ld;                                  // 0: rows of mask / dist are F entries apart
  const xivo_feat_in* feats; int Fmax;          // optional [batch x Fmax]: entries with sind < 0 are absent (ragged batches)
  int no_relax;                                 // 1: inlier <=> distance < thresh, no relaxation loop (min_inliers = -1: every filter tested)
};
int launch_gate_dense(const GateDenseArgs& a, hipStream_t s);

// ================================================================ pool_kernels.hip: depth sub-filter and feature pool

// Feature::SubfilterUpdate + candidate tests (feature.cpp:246-297, options.cpp:10-33)
int launch_subfilter(xivo_subfilter_feat* feats, int n, const xivo_pose_in* poses, const xivo_group_in* groups,
                     int n_groups, xivo_cam cam, xivo_subfilter_opts o, int batch, hipStream_t s,
                     const xivo_calib_in* calib = nullptr, int cam_dim = 0, int invdepth = 0);

// One anchor of the out-of-state feature pool (xivo_hip_pool_config): the frozen pose of its group and the in-state group slot
// it is linked to (-1: unlinked, the frozen pose is the anchor's pose)
struct PoolAnchor {
  xivo_group_in g;
  int slot, reserved;
};
// Out-of-state feature pool (xivo_hip_pool_*): entries are xivo_subfilter_feat with ref_sind = the entry's anchor (-1: free)
int launch_pool_anchor(PoolAnchor* anchors, int anchor_max, const xivo_pose_in* poses, const int* slot, int nb, hipStream_t s);
int launch_pool_add(xivo_subfilter_feat* pool, int pool_max, const xivo_pool_new* recs, int n, xivo_cam cam,
                    const xivo_calib_in* calib, int cam_dim, int invdepth, hipStream_t s, const double* init_z = nullptr);
struct PoolStepArgs {
  xivo_subfilter_feat* pool; const PoolAnchor* anchors; int pool_max, anchor_max;   // [batch][pool_max] / [batch][anchor_max]
  const xivo_pose_in* poses; const xivo_group_in* groups; int n_groups;
  xivo_cam cam; const xivo_calib_in* calib; int cam_dim, invdepth;
  xivo_subfilter_opts o; double remove_outlier; int strict, batch;
  const double* xp;                                  // [batch][pool_max][2]
  int* order; int* n; unsigned char* live;           // out: [batch][pool_max], [batch], [batch][pool_max]
  xivo_triangulate_opts tri;                         // method XIVO_TRI_OFF: no triangulation
  int* tri_good; int* tri_bad;                       // [batch]: accumulated while tri is on
};
int launch_pool_step(const PoolStepArgs& a, hipStream_t s);
// The frame's OOS list from the dropped entries the host life cycle hands over (pool_oos_kernels.hip): one wave per filter
struct PoolOosCollectArgs {
  const xivo_subfilter_feat* pool; const PoolAnchor* anchors; int pool_max, anchor_max;
  const xivo_pose_in* poses; const xivo_group_in* groups; int n_groups;
  int invdepth; double min_depth, max_depth;
  const xivo_pool_oos_cand* cands; const int* off;   // records of filter b: [off[b], off[b + 1])
  int oos_max, max_obs, min_obs;
  xivo_oos_in* list;                                 // [batch][oos_max]
  xivo_pool_oos_stats* stats;                        // [batch]
  int batch;
};
int launch_pool_oos_collect(const PoolOosCollectArgs& a, hipStream_t s);
// The same list made in the device pool life cycle (select: between its begin kernel and the step) and the observation rings it
// reads (record: behind its end kernel). Rings per filter: hist_cnt [pool_max], hist_anchor / hist_born [pool_max][max_obs],
// hist_xp [pool_max][max_obs][2]; anc_born [anchor_max]
struct PoolOosLifeArgs {
  const xivo_subfilter_feat* pool; const PoolAnchor* anchors; int pool_max, anchor_max;
  const xivo_pose_in* poses; const xivo_group_in* groups; int n_groups;
  int invdepth; double min_depth, max_depth;
  const long long* ent_id; const int* ent_born; const int* anc_used; const int* anc_life;   // the device life cycle's pool book
  const double* xp;                                  // [batch][pool_max][2] the step's pixels (NaN: dropped)
  int* anc_born; int* hist_cnt; int* hist_anchor; int* hist_born; double* hist_xp;
  int oos_max, max_obs, min_obs, frame;
  xivo_oos_in* list; xivo_pool_oos_stats* stats;
  int batch;
};
int launch_pool_oos_select(const PoolOosLifeArgs& a, hipStream_t s);
int launch_pool_oos_record(const PoolOosLifeArgs& a, hipStream_t s);
// Feature::Triangulate's triangulators on host-array problems (xivo_hip_triangulate)
int launch_triangulate(const xivo_tri_in* in, xivo_tri_out* out, int n, const xivo_triangulate_opts& o, hipStream_t s);
// AdaptInitialDepth (xivo_hip_pool_adapt_depth): one workgroup per filter
struct AdaptDepthArgs {
  const xivo_feat_in* feats; int F, Fmax;            // resident feature list [batch][Fmax], first F entries read
  const xivo_subfilter_feat* pool; int pool_max;     // [batch][pool_max]
  double* init_z; double* init_z_out;                // [batch] resident / copy out (may be null)
  double beta, min_z, max_z; int min_lifetime, invdepth, batch;
};
size_t adapt_depth_lds(int F, int pool_max);
int launch_adapt_depth(const AdaptDepthArgs& a, hipStream_t s);

// ================================================================ propagate_kernels.hip: propagation (capi_propagate.hip)

// Estimator::Propagate state + covariance stages (rk4.cpp, princedormand.cpp, estimator.cpp:598-704): one wave per
// filter; writes the accumulated transition Phi and the new P_mm (23 x 23 each, column-major) for the tail kernel
struct PropStateArgs {
  xivo_pose_in* poses; const xivo_imu_in* imu;      // [nb] / [nb][n_imu] (poses already offset to b0)
  int n_imu;
  const double* Qimu; const double* Qmodel;         // device copies
  double g[3]; int method; double stepsize;
  const double* P; long strideP; int ldp;           // resident covariance (offset to b0)
  double* Phi_out; double* Pmm_out;                 // [nb][529] ([nb][nm * nm] for the calibration kernel)
  int batch;
  // online-calibration builds (launch_propagate_state_calib): motion size, slot of Cg (-1: none; Ca follows at + 9), the
  // resident calibration state (offset to b0); Qmodel is nm x nm
  int nm, iCg; const xivo_calib_in* calib;
  // step-size-controlled Dormand-Prince (princedormand.cpp:26-60; default-build kernel only): the per-filter step carried between
  // samples and calls (the reference's function-local static h), null = fixed steps
  double* pd_h; double pd_tol, pd_min_scale, pd_max_scale;
  // tuning table: Qimu / Qmodel of filter b start b * strideQimu / b * strideQmodel doubles in (144 / 529); 0: one pair for all
  long strideQimu, strideQmodel;
};
int launch_propagate_state(const PropStateArgs& a, hipStream_t s);
int launch_propagate_state_calib(const PropStateArgs& a, hipStream_t s);

// propagation tail (rk4.cpp:92-102): the kernel for motion size nm (propagate_cov_fixed_kernel<23> for 23, else
// propagate_cov_kernel) and the passes of 256 tail columns it makes over N - nm; -1 for nm outside 1..40 (MAXM)
int propagate_cov_pick(int nm, int N, char* label, size_t n);
int launch_propagate_cov(double* P, long strideP, int ldp, int N, int Np, int nm, const double* Phi,
                         const double* Pmm, int b0, int nb, hipStream_t s);

// ================================================================ ldlt_fallback.hip

// Diagonally pivoted L D L^T fallback (Eigen's S.ldlt().solve of src/estimator.cpp:1266) + the as-coded Joseph update for
// the filters whose status is non-zero (ldlt_fallback.hip); clears their status and sets used[filt]
struct LdltFallbackArgs {
  int* status; int* used;
  EllBuffers ell; const double* H; long strideH; int ldh; int use_dense;
  int mixed_row0;   // >= 0: rows below it are row-pair compressed, rows from it on are dense (OOS rows behind in-state rows)
  const double* lead; long strideLead; int ldlead, lead_k;   // leading dense block next to the compressed rows (online-calibration stacking), or null
  const double* PHT; long stridePHT; int ldpht;
  double* S; long strideS; int lds;
  double* K; long strideK; int ldk;
  double* A; long strideA; int lda;     // scratch: I - K H
  double* T; long strideT; int ldt;     // scratch: (I - K H) P
  double* P; long strideP; int ldp;
  const double* inn; long strideInn;
  const double* diagR; long strideR;
  double* err; long strideErr;
  int N, M, batch;
};
int launch_ldlt_fallback(const LdltFallbackArgs& a, hipStream_t s);

// ================================================================ dropin.hip

// One-filter plumbing call (dropin.hip, capi_update.hip: xivo_hip_update_joseph_host): the boundary kernels address page-locked
// host memory directly. `block` = the staged compressed rows of the filter: ints idx[pairs_clear][ELL_W] at off_idx,
// doubles val[pairs_clear][ELL_W][2] at off_val, inn[Mpmax] at off_inn, diagR[Mpmax] at off_R, ints {nc, pw, over} at off_flags.
struct DropinInArgs {
  const double* Psrc; int ldps;          // host-mapped N x N covariance (null: the device copy is current)
  double* P; int N, Np, ldp;             // the filter's padded device covariance
  const void* block; int off_idx, off_val, off_inn, off_R, off_flags;
  int pairs_clear, Mpmax;
  int* idx; double* val; double* inn; double* diagR; int* nc; int* pw; int* over;   // the filter's device buffers
};
struct DropinOutArgs {
  const double* P; int N, ldp;           // the filter's padded device covariance
  double* Pdst; int ldpd;                // host-mapped destination (null: P stays on the device)
  const double* err; double* err_dst;    // dx [N]
  const int* status; const int* ldlt_used; int* flags_dst;   // -> {status, ldlt_used}
};
int launch_dropin_in(const DropinInArgs& a, hipStream_t s);
int launch_dropin_out(const DropinOutArgs& a, hipStream_t s);

}  // namespace xivo_hip
