/* xivo_hip.h - C ABI of the MI355X-native EKF measurement-update path for XIVO.
 *
 * Drop-in boundary for the reference's private hot path (the reference has no
 * FFI of its own - SURVEY.md section 8b): each entry point below names the
 * reference member function / lines it replaces, relative to /root/reference.
 *
 * Conventions
 *  - plain C, no exceptions, no aborts: every call returns XIVO_HIP_OK (0) or a
 *    negative status (the reference LOG(FATAL)s / throws instead,
 *    src/estimator.cpp:121,587,821,844 - the C++ adapter in
 *    xivo_amd/host/estimator_hip.h converts a non-zero status back to that).
 *  - all matrices are column-major double (common/alias.h:11, Eigen default),
 *    with an explicit leading dimension where the caller owns the buffer.
 *  - batch-first: a context holds `batch_max` independent filters (the
 *    reference is one singleton filter per process, src/estimator.cpp:26);
 *    "b0, nb" = first filter and number of filters a call touches.
 *  - the covariance P of every filter is device resident; host edits of P go
 *    through the xivo_hip_p_* calls (mirrors of the host edits listed in
 *    SURVEY.md a17) or through upload/download.
 *  - a context is single threaded (like the reference's estimator); different
 *    contexts may be driven from different host threads / processes (one per GPU).
 *  - host pointers are borrowed for the duration of the call only.
 */
#ifndef XIVO_HIP_H_
#define XIVO_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xivo_hip_ctx xivo_hip_ctx;

enum {
  XIVO_HIP_OK = 0,
  XIVO_HIP_ERR_INVALID = -1,     /* bad argument / size                         */
  XIVO_HIP_ERR_HIP = -2,         /* a HIP runtime call failed                   */
  XIVO_HIP_ERR_NOT_SPD = -3,     /* S = HPH^T + R not positive definite         */
  XIVO_HIP_ERR_NOMEM = -4,
  XIVO_HIP_ERR_UNSUPPORTED = -5, /* size outside what the kernels are built for */
  XIVO_HIP_ERR_FULL = -6         /* the trajectory / landmark / innovation log holds T_max frames */
};

/* flags for xivo_hip_create / stacking */
enum {
  XIVO_HIP_FLAG_NONE = 0u,
  /* Feature::FillJacobianBlock writes the group-translation block over the
   * group-rotation block (src/feature.cpp:675-676). Default = reproduce it;
   * this flag gives the evidently intended full row (as src/update.cpp:326). */
  XIVO_HIP_FLAG_FIX_GROUP_BLOCK = 1u,
  /* record HIP events around every kernel launch (per-stage timing) */
  XIVO_HIP_FLAG_PROFILE = 2u,
  /* By default the update exploits the row sparsity of H: when every row pair of every filter of the
   * call has at most 16 columns shared by most pairs + 12 private non-zero columns (true for the stacked
   * in-state Jacobians of src/update.cpp:129-138: 21 per pair), H P, S and the H-products of the
   * covariance stage skip the structural zeros (exact: the skipped terms are 0 * x), and the covariance stage
   * evaluates the Joseph expression in its whitened form, P+ = P - (W - D)^T (W + D). An H that does not
   * compress (dense rows, arbitrary input) keeps the same evaluation on dense products for H P and S. This flag forces the
   * AS-CODED sequence of src/estimator.cpp:1259-1287 on dense products for any H: A = K H - I, T = A P,
   * P+ = T A^T + K R K^T (the pure-GEMM variant; 3 x the flops). */
  XIVO_HIP_FLAG_DENSE_H = 64u,
  /* Symmetric ("square-root") form of the gain and covariance: S = L L^T, W = L^-1 (H P) by forward substitution only,
   *   dx = W^T (L^-1 inn),   P+ = P - W^T W
   * - what the Joseph expression of src/estimator.cpp:1276-1287 evaluates to for the optimal gain K = P H^T S^-1 (its
   * correction term (K S - P H^T) K^T vanishes identically), without the backward substitution, the gain residual and
   * the second N x N x M product: about 80 % of the device time of the default. The result is symmetric by
   * construction and its rounding error scales with cond(L) = sqrt(cond(S)). Opt-in: the reference codes the Joseph
   * form and the default reproduces that expression; parity of this mode against the reference is tested to the same
   * tolerances (1e-6 on P, 1e-8 on dx), including an ill-conditioned S. */
  XIVO_HIP_FLAG_SYMMETRIC_FORM = 256u,
  /* Sparse-H pipeline: by default the covariance update is the whitened Joseph expression on the gain still in the solve
   * kernel's registers (or, for wider shapes, on the whitened outputs of the solve) - T and G never reach memory. This flag
   * selects the re-associated tail from stand-alone kernels instead: T = K(HP) - P, G = T H^T + K R, P+ = G K^T - T
   * (= T (KH - I)^T + K R K^T, exact for any gain like the Joseph form it is) - 0.8 x the speed, 5 x closer to the as-coded
   * fp64 result (both lose digits in proportion to cond(S) and meet the 1e-6 / 1e-8 tolerances by orders of magnitude). */
  XIVO_HIP_FLAG_STANDALONE_TAIL = 512u,
  /* Opt-in (round 4; BASELINE config 4 "fp32 MFMA with stated tolerance"), shapes whose covariance product runs outside the
   * solve kernel (N > 256 or M > 176): the whitened outputs V^T = (W - D)^T and Y^T = (W + D)^T leave the fp64 solve as
   * FLOAT and P+ = P - V^T Y runs on v_mfma_f32_16x16x4_f32 (fp32 accumulation over M, subtracted from P in fp64): half
   * the operand bytes of a product that is HBM-bound, twice the matrix rate. Everything else (S, the factorisation, both
   * substitutions, dx) stays fp64: dx is unchanged, P+ carries the rounding of the float operands, <= 5e-5 relative
   * Frobenius (measured ~1e-7 .. 3e-6 per update). Shapes the in-solve update holds are not affected, at any batch size.
   * Over a CHAIN of updates on the resident covariance (tests/test_variants_gpu.py::test_fp32_whitened_chain, 25 updates):
   * P stays within 5e-5 of the all-fp64 chain (measured 2.6e-5); dx of each update is bit-identical to the fp64 path given
   * the same prior, but against the fp64 chain a later dx deviates by up to 5e-2 relative (measured 2.3e-2; <= 0.05 posterior
   * standard deviations): P - V^T Y cancels in the directions earlier measurements shrank, and floats resolve 6e-8 |P| there.
   * Use it where that is acceptable; the default stays all fp64. */
  XIVO_HIP_FLAG_FP32_WHITENED = 16384u,
  /* By default a filter whose innovation covariance the un-pivoted Cholesky cannot factor (S indefinite / not positive
   * definite) is updated the reference's way after all: Eigen's diagonally pivoted L D L^T solve (src/estimator.cpp:1266)
   * and the as-coded Joseph form, on that filter only (ldlt_fallback.hip); xivo_hip_get_ldlt_used tells which filters took
   * that route and their status reads 0. With this flag such a filter keeps its prior covariance bit for bit, absorbs
   * nothing, and xivo_hip_get_status reports it (the behaviour of rounds 1-2). */
  XIVO_HIP_FLAG_NO_LDLT_FALLBACK = 4096u,
  /* By default an update of at most 64 filters (one estimator is the reference's own use) takes the latency route of the
   * default pipeline: the solve on 128-column workgroups of the streamed kernel, the covariance product P - V^T Y on
   * 64 x 64 tiles - the same whitened Joseph evaluation spread over tens of CUs instead of one CU per filter (B = 1,
   * N = 250, M = 160: solve + product 0.07 instead of 0.13 ms). With this flag every batch size runs the kernels sized for
   * thousands of filters (one workgroup per filter, whole update inside the solve kernel). */
  XIVO_HIP_FLAG_THROUGHPUT_ROUTE = 8192u,
  /* The reference's USE_INVDEPTH build (src/CMakeLists.txt:10): a feature's local state is (X/Z, Y/Z, 1/Z) instead of
   * (X/Z, Y/Z, log Z) - Feature::Xc goes through unproject_invz (src/feature.cpp:98-105, common/project.h:31-56) and
   * Feature::z is 1 / x(2) (:120-126). Every kernel that unprojects a feature (in-state Jacobians, depth sub-filter and its
   * candidate depth test, loop-closure rows) follows the flag; the Jacobian block d/dx changes accordingly. */
  XIVO_HIP_FLAG_INVDEPTH = 32768u,
  /* Round 6: shapes one workgroup holds end to end (M <= 64 with N <= 256 - the TUM-VI build; M <= 112 with N <= 192 -
   * BASELINE config 2) run the WHOLE update - P H^T, S, the MH gate, the factorisation, both substitutions, dx and the
   * covariance product - in one kernel per filter (fused_update.hip): nothing but P, P+ and the compressed rows crosses HBM.
   * Same algebra as the multi-kernel pipeline (whitened Joseph evaluation, same gate expressions). This flag keeps such a
   * shape on the multi-kernel pipeline (A/B, and the route-against-route parity tests). */
  XIVO_HIP_FLAG_MULTI_KERNEL = 65536u
};

/* camera models implemented on device (common/camera_pinhole.h,
 * common/camera_equidist.h, common/camera_radtan.h, common/camera_atan.h) */
enum { XIVO_CAM_PINHOLE = 0, XIVO_CAM_ATAN = 1, XIVO_CAM_RADTAN = 2, XIVO_CAM_EQUI = 3 };

/* Error-state layout (src/core.h:40-105). N is a run-time value here
 * (kFullSize is a compile-time constant in the reference). */
typedef struct {
  int N;              /* kFullSize                                           */
  int group_begin;    /* kGroupBegin  (23 in the default build)              */
  int n_groups;       /* kMaxGroup                                           */
  int feature_begin;  /* kFeatureBegin = group_begin + 6*n_groups            */
  int n_features;     /* kMaxFeature                                         */
} xivo_layout;

typedef struct {
  int model;          /* XIVO_CAM_*                                          */
  int rows, cols;
  double fx, fy, cx, cy;
  double d[5];        /* EQUI: k0..k3 ; RADTAN: p1,p2,k1,k2,k3(order of the
                         reference ctor) ; ATAN: w                            */
} xivo_cam;

/* Nominal poses one filter needs for Feature::ComputeJacobian
 * (src/update.cpp:24-32 passes X_.Rsb, X_.Tsb, X_.Rbc, X_.Tbc). 3x3 matrices
 * are column-major. */
typedef struct {
  double Rsb[9], Tsb[3];
  double Rbc[9], Tbc[3];
  /* rest of the nominal motion state (src/core.h:117-130): not read by the Jacobians, but
   * retracted by xivo_hip_absorb_error so the whole State can stay device resident */
  double Vsb[3], bg[3], ba[3];
  double Rsg[9];
} xivo_pose_in;

/* One group anchor (src/group.h:41-107): pose + state slot `sind`. */
typedef struct {
  double Rsb[9], Tsb[3];
} xivo_group_in;

/* One in-state feature (src/feature.h:74-232). */
typedef struct {
  double x[3];        /* (X/Z, Y/Z, log Z) in the reference camera frame, feature.h:258-262 */
  double xp[2];       /* last tracked pixel, Feature::back()                 */
  int ref_sind;       /* ref_->sind(): slot of the reference group           */
  int sind;           /* feature slot; -1 = absent entry: contributes no rows, is never an inlier
                         (filters of one batch may hold different numbers of features)      */
} xivo_feat_in;

/* One out-of-state (MSCKF) feature with k observations from in-state groups
 * (src/oos.cpp:8-89). */
#define XIVO_OOS_MAX_OBS 16
typedef struct {
  double Xs[3];                       /* cache_.Xs, src/oos.cpp:17           */
  int n_obs;
  int group_sind[XIVO_OOS_MAX_OBS];   /* obs.g->sind()                       */
  double xp[XIVO_OOS_MAX_OBS][2];     /* obs.xp                              */
} xivo_oos_in;

/* ---- lifetime -------------------------------------------------------- */
int xivo_hip_create(xivo_hip_ctx** out, int device, int N, int M_max, int batch_max, unsigned flags);
void xivo_hip_destroy(xivo_hip_ctx* ctx);
const char* xivo_hip_strerror(int status);
int xivo_hip_sync(xivo_hip_ctx* ctx);
/* number of visible HIP devices (0 if none / on error) */
int xivo_hip_device_count(void);
/* NUMA node of the host cores / memory closest to `device` (from the sysfs entry of its PCI function), -1 if unknown.
 * The reference runs one estimator per process (src/estimator.cpp:26); with one process per GPU the launcher uses this to
 * keep each rank's host side (hand-over staging, BatchEstimator's OpenMP team) on its GPU's socket. */
int xivo_hip_device_numa_node(int device);
int xivo_hip_set_flags(xivo_hip_ctx* ctx, unsigned flags);

/* ---- covariance residency (Estimator::P_, src/estimator.h:423; a17) --- */
/* P: nb column-major N x N matrices, `stride` elements apart, leading dimension ld. The LOWER triangle of each uploaded
 * matrix is authoritative: the device state is its exact mirror (every pipeline treats P as symmetric; the reference never
 * re-symmetrises P_, src/estimator.cpp:1280-1287, so its triangles differ by rounding - a symmetric matrix round-trips bit
 * for bit, a rounding-level asymmetry stays inside the parity tolerances, tests/test_robustness_gpu.py). */
int xivo_hip_upload_P(xivo_hip_ctx* ctx, int b0, int nb, const double* P, long stride, int ld);
int xivo_hip_download_P(xivo_hip_ctx* ctx, int b0, int nb, double* P, long stride, int ld);
/* BackupState / RestoreState P part (src/estimator.cpp:1413-1414,1434-1435) */
int xivo_hip_snapshot_P(xivo_hip_ctx* ctx);
int xivo_hip_restore_P(xivo_hip_ctx* ctx);
/* P.block(off,0,len,N)=0; P.block(0,off,N,len)=0 (src/estimator.cpp:757-759,781-783,1476-1477; src/update.cpp:299-315) */
int xivo_hip_p_zero_rc(xivo_hip_ctx* ctx, int b, int off, int len);
/* copy rows+cols [src,src+len) onto [dst,dst+len) (AddGroupToState, src/estimator.cpp:808-816) */
int xivo_hip_p_copy_rc(xivo_hip_ctx* ctx, int b, int dst, int src, int len);
/* P.block<3,3>(off,off) = P3 (Feature::FillCovarianceBlock, src/feature.cpp:753-760) */
int xivo_hip_p_set_block3(xivo_hip_ctx* ctx, int b, int off, const double* P3);
/* diag(P) (FindNewRefGroup reads it, src/estimator.cpp:1394-1407) */
int xivo_hip_p_diag(xivo_hip_ctx* ctx, int b, double* diag_out);

/* ---- S-level: dense H / inn / diagR given (Estimator::H_, inn_, diagR_) -- */
/* stage measurements of filters [b0,b0+nb): H is M x N (ldh), inn and diagR
 * have M entries. M may differ between calls, M <= M_max. */
int xivo_hip_set_measurements(xivo_hip_ctx* ctx, int b0, int nb, int M,
                              const double* H, long strideH, int ldh,
                              const double* inn, long strideInn,
                              const double* diagR, long strideR);
/* The same hand-over for measurements that are already in device memory (a device-side producer, or a caller that
 * keeps its Eigen buffers in pinned / managed memory): dH is M x N column-major per filter (leading dimension ldh,
 * filters strideH elements apart), dInn / dR have M entries. This is the per-frame device work of the S-level
 * boundary - H_ changes with every camera frame (src/update.cpp:129-138): one batched launch builds the row-pair
 * compressed rows (each element of H read once); padded dense copies are materialised only for filters whose rows
 * do not fit the compressed form. The device buffers are read during the call only. */
int xivo_hip_set_measurements_device(xivo_hip_ctx* ctx, int b0, int nb, int M,
                                     const double* dH, long strideH, int ldh,
                                     const double* dInn, long strideInn,
                                     const double* dR, long strideR);
/* Estimator::UpdateJosephForm (src/estimator.cpp:1257-1288) for filters [0,B):
 * S = HPH^T + R, K^T = S^-1 HP, dx = K inn, P <- (KH-I)P(KH-I)^T + K R K^T,
 * on the resident P with the staged measurements. Asynchronous on the
 * context's stream. */
int xivo_hip_update_joseph(xivo_hip_ctx* ctx, int B);
/* err_ (dx) of filters [b0,b0+nb) after the update (before AbsorbError) */
int xivo_hip_get_err(xivo_hip_ctx* ctx, int b0, int nb, double* err, long stride);
/* per-filter factorisation status of the last update (0 = ok) ; returns
 * XIVO_HIP_ERR_NOT_SPD if any is non-zero */
int xivo_hip_get_status(xivo_hip_ctx* ctx, int b0, int nb, int* status);
/* used[i] = 1 if the last update of filter b0 + i ran the pivoted L D L^T fallback (S was not positive definite; the
 * reference's S.ldlt().solve, src/estimator.cpp:1266, handles that case silently), 0 otherwise */
int xivo_hip_get_ldlt_used(xivo_hip_ctx* ctx, int b0, int nb, int* used);
/* Estimator::UpdateJosephForm() AS THE REFERENCE CALLS IT (src/estimator.cpp:1257-1288; callers src/update.cpp:141 and
 * :332): one filter whose members live in pageable host memory - P_ (N x N, in-out), H_ (M x N), inn_, diagR_ (M) in,
 * err_ (N) out - in ONE call with ONE host synchronisation. Replaces the sequence upload_P / set_measurements /
 * update_joseph / get_status / get_err / download_P (four synchronisations, three staged copies) for the drop-in binding
 * of INTEGRATION.md section 3. The dense H_ is scanned once on the host while it is staged and crosses PCIe as row-pair
 * compressed rows (the same rows the batched hand-over builds on the device, bit for bit); an H_ without XIVO's row
 * structure takes the general entry points inside this call (same results). P_ crosses through the context's page-locked
 * block (one host copy each way; the boundary kernels address the block directly). Returns XIVO_HIP_ERR_NOT_SPD exactly when
 * xivo_hip_get_status would: with XIVO_HIP_FLAG_NO_LDLT_FALLBACK for any S the Cholesky cannot factor, and without it when the
 * pivoted L D L^T fallback met non-finite arithmetic (a NaN / Inf in P_, H_ or diagR_); P is then the prior, err_out zero.
 * The context's staged row count becomes M.
 *   mode: XIVO_HIP_HOST_P_RESIDENT  the device copy of P (filter b) is current - P_ is not uploaded (no host edit since
 *                                   the last upload / download; P may be NULL when KEEP_P is set too)
 *         XIVO_HIP_HOST_KEEP_P      P+ stays on the device only (resident mode through the same call; read it back later
 *                                   with xivo_hip_download_P) */
#define XIVO_HIP_HOST_P_RESIDENT 1u
#define XIVO_HIP_HOST_KEEP_P 2u
int xivo_hip_update_joseph_host(xivo_hip_ctx* ctx, int b, int M, const double* H, int ldh, const double* inn,
                                const double* diagR, double* P, int ldp, double* err_out, unsigned mode);
/* Test hook (needs neither a device nor a context): the host-side row-pair compression xivo_hip_update_joseph_host applies
 * to H_ while staging it - idx [pairs_clear][28] / val [pairs_clear][28][2] in the layout of the batched hand-over
 * (xivo_hip_set_measurements_device), *nc common slots, *pw private slots; returns 1 when the rows do not fit, else 0. */
/* Host-only check of the tables that say which wave of the one-kernel update (csrc/fused_update.hip) forms which tile of
 * P+ at 10 / 13 column blocks: every block pair exactly once, the counts the kernel's dispatch assumes, per_simd[4] (optional)
 * the tiles per SIMD. 0 = consistent, -1 = no table for that size. No GPU needed. */
int xivo_hip_selftest_fused_tiles(int column_blocks, int* per_simd);
/* Host-only check of the one-kernel update's admission test for a padded shape (Mp, Np multiples of 16) and pw private
 * slots: -1 when the shape takes the multi-kernel pipeline; else the kernel label that would run is written to label[n]
 * (optional) and the return value is a bitmask of broken invariants - 1 more block rows of the factor than waves
 * (Mp > Np), 2 LDS map beyond 160 KB, 4 no column block per product phase, 8 gather staging past the coefficients,
 * 16 more waves than the instantiation's workgroup. 0 = all hold. No GPU needed. */
int xivo_hip_selftest_fused_shape(int Mp, int Np, int pw, char* label, int n);
int xivo_hip_selftest_host_compress(const double* H, int ldh, int M, int N, int pairs_clear, int* idx, double* val, int* nc, int* pw);
/* Host-only answer to "which kernel would this shape launch" for the feature-level and propagation kernels whose launch picks
 * by size (csrc/gate_kernels.hip, csrc/glevel_kernels.hip, csrc/propagate_kernels.hip; the launch calls the same function). label[n] (optional) receives the stage label that
 * xivo_hip_stage_kernel reports for that launch. No GPU needed.
 *   XIVO_HIP_LAUNCH_GATE          a = filters in the call, b = F, c = online-calibration build (0 / 1): returns the threads per
 *                                 filter of gate_sparse_kernel; label "gate_sparse_kernel@<threads>".
 *   XIVO_HIP_LAUNCH_OOS_COMPRESS  a = n_groups, b = the largest OOS row count of the call: returns 0 <36,1>, 1 <64,1>,
 *                                 2 <36,2>, -1 when none is built (xivo_hip_compress_oos leaves the rows as they are; label "").
 *   XIVO_HIP_LAUNCH_PROP_TAIL     a = nm, b = N: returns the passes of 256 tail columns over N - nm (0 when N = nm), -1 when
 *                                 nm is outside 1..40 or above N (refused); label "propagate_cov_fixed_kernel<23>" or
 *                                 "propagate_cov_kernel". */
#define XIVO_HIP_LAUNCH_GATE 0
#define XIVO_HIP_LAUNCH_OOS_COMPRESS 1
#define XIVO_HIP_LAUNCH_PROP_TAIL 2
int xivo_hip_selftest_glevel_launch(int kind, int a, int b, int c, char* label, int n);
/* Test hook: the device blocks the context owns right now - *live their number, *bytes their total size (either may be
 * null). Memory handed out by xivo_hip_dev_alloc belongs to the caller and is not counted. */
int xivo_hip_selftest_ctx_allocs(xivo_hip_ctx* ctx, int* live, unsigned long long* bytes);
/* Estimator::MHGating numeric core on dense rows (src/update.cpp:60-96):
 * rows 2f,2f+1 of the staged H are feature f's J. Writes the inlier mask and
 * Mahalanobis distances; rejected rows are then neutralised in the staged
 * measurements so that a following xivo_hip_update_joseph equals the
 * reference's FilterUpdate over the inliers only. */
int xivo_hip_mh_gate_dense(xivo_hip_ctx* ctx, int B, int F, double R, double mh_thresh,
                           double mh_mult, int min_inliers,
                           unsigned char* inlier_mask_out, double* mh_dist_out);

/* FilterUpdate on dense candidate rows in one pass: HP = H P once, Mahalanobis gating of
 * features 0..F-1 from (HP)_f H_f^T + R (skipped when F <= min_inliers, src/manager.cpp:635),
 * rejected rows neutralised, then UpdateJosephForm. xivo_hip_get_gate returns the mask /
 * distances of that pass ([B x F]). */
int xivo_hip_update_dense_gated(xivo_hip_ctx* ctx, int B, int F, double R, double mh_thresh,
                                double mh_mult, int min_inliers);
int xivo_hip_get_gate(xivo_hip_ctx* ctx, int B, int F, unsigned char* inlier_mask_out, double* mh_dist_out);

/* ---- G-level: features + poses given, Jacobians built on device -------- */
int xivo_hip_set_layout(xivo_hip_ctx* ctx, const xivo_layout* layout, const xivo_cam* cam);
int xivo_hip_set_scene(xivo_hip_ctx* ctx, int b0, int nb, int F,
                       const xivo_pose_in* poses, const xivo_group_in* groups /* nb x n_groups */,
                       const xivo_feat_in* feats /* nb x F */);
/* Estimator::ComputeInstateJacobians (src/update.cpp:24-32) =
 * Feature::ComputeJacobian x F (src/feature.cpp:542-656) */
int xivo_hip_jacobians_instate(xivo_hip_ctx* ctx, int B);
/* compact per-feature result: J blocks 2x21 ([Wsb Tsb Wbc Tbc Wg Tg x], row-major 2 x 21) + inn (2) */
int xivo_hip_get_jacobians(xivo_hip_ctx* ctx, int b0, int nb, double* J2x21, double* inn2);
/* ---- online-calibration builds (measurement side) ---------------------------------------------------------------
 * The reference's USE_ONLINE_TEMPORAL_CALIB / USE_ONLINE_IMU_CALIB / USE_ONLINE_CAMERA_CALIB builds (src/CMakeLists.txt:13-15)
 * put a camera-IMU time offset td, the gyro calibration Cg (9) / accel calibration Ca (6) and up to 9 camera intrinsics
 * into the state (src/core.h:49-83) and give Feature::ComputeJacobian four more blocks (src/feature.cpp:592-609, :611-618,
 * :632-651): d/dtd (2 x 1), d/dCg (2 x 9), d/dbg (2 x 3, at Index::bg) and d/d(intrinsics) (2 x Camera::dim()), which
 * Feature::FillJacobianBlock stacks as well (:664-670, :679-683). xivo_hip_set_calib switches those blocks on for the
 * context: xivo_hip_jacobians_instate then also fills them (xivo_hip_get_jacobians_calib), xivo_hip_stack /
 * xivo_hip_filter_update stack them. Such a row pair has up to 34 columns that every feature shares - more than the 16
 * common slots of the row-pair compressed form - but all of them lie in the leading 48 state columns: the stacking is the
 * default build's compressed rows + a dense [M x 48] block of the calibration columns, and the update takes the sparse
 * pipeline with two skinny products on top (round 5; xivo_hip_last_path 1). MH gating uses the whole row as the reference's
 * f->J() does (43 columns in the compact gate). Where the calibration columns do not fit the leading 48 (cam_begin + 9 > 48),
 * under XIVO_HIP_FLAG_DENSE_H / _SYMMETRIC_FORM / _STANDALONE_TAIL, and whenever dense rows are needed after all (OOS rows appended, xivo_hip_update_dense_gated,
 * xivo_hip_get_H - which therefore sends the NEXT update of that stacking down the dense pipeline) the rows are (re-)stacked
 * as dense rows and gate / update through the dense pipeline (round 4). Same results within the stated tolerances either way.
 * Slots as the reference's Index enum / kCameraBegin would number them
 * (the caller's xivo_layout already counts them in N, group_begin, feature_begin); -1 / 0 = that block is not in the build.
 * Motion side of those builds: xivo_hip_propagate_calib (below, next to xivo_hip_propagate) integrates the
 * kMotionSize = 24 / 38 / 39-dimensional motion block with the Cg / Ca columns of ComputeMotionJacobianAt
 * (src/estimator.cpp:626-638, :674-688) and imu_.Cg() / imu_.Ca() in ComposeMotion (:603-604); xivo_hip_absorb_error
 * then also retracts td, Cg, Ca and the intrinsics (src/core.h:150-152, src/estimator.cpp:879-890, src/imu.cpp:7-21,
 * common/camera_autocalib.h) of the resident per-filter calibration state below. */
typedef struct {
  int td;         /* Index::td, or -1 (no USE_ONLINE_TEMPORAL_CALIB: then neither the td, nor the Cg, nor the bg block exists) */
  int Cg;         /* Index::Cg (9 columns; Ca's 6 follow at Cg + 9), or -1 (no USE_ONLINE_IMU_CALIB); the measurement-side
                     Cg / bg blocks need td >= 0 (they are nested in the temporal block, src/feature.cpp:592-609)              */
  int cam_begin;  /* kCameraBegin                                                                                              */
  int cam_dim;    /* Camera::dim(): 4 pinhole (fx fy cx cy), 5 atan (+ w), 9 radtan (+ p1 p2 k1 k2 k3), 8 equidistant
                     (+ k0..k3); 0 = no USE_ONLINE_CAMERA_CALIB                                                               */
} xivo_calib_layout;
typedef struct {   /* per filter: what Estimator::ComputeInstateJacobians hands down (src/update.cpp:27-28) + the rest of the
                      calibration state that AbsorbError retracts */
  double gyro[3];  /* last_gyro_ (raw measurement)        */
  double Cg[9];    /* imu_.Cg(), column-major             */
  double td;       /* X_.td                               */
  double Ca[9];    /* imu_.Ca(), column-major (upper triangular, src/imu.cpp:24); identity when the build has no Ca */
  double intr[9];  /* camera intrinsics in the order of the state slots: fx fy cx cy, then xivo_cam.d[0..4]. With
                      cam_dim > 0 every kernel that projects (Jacobians, OOS rows, depth sub-filter) takes the filter's
                      intrinsics from here - the context's xivo_cam only names the model; cam_dim = 0: not read */
} xivo_calib_in;
/* layout == NULL switches the calibration blocks off again (default build) */
int xivo_hip_set_calib(xivo_hip_ctx* ctx, const xivo_calib_layout* layout);
int xivo_hip_set_calib_state(xivo_hip_ctx* ctx, int b0, int nb, const xivo_calib_in* calib /* nb */);
int xivo_hip_get_calib_state(xivo_hip_ctx* ctx, int b0, int nb, xivo_calib_in* calib_out /* nb */);
/* only last_gyro_ of every filter (what changes from frame to frame; td / Cg / Ca / intr are state and stay as AbsorbError
 * left them): gyro3 = nb x 3 doubles */
int xivo_hip_set_calib_gyro(xivo_hip_ctx* ctx, int b0, int nb, const double* gyro3);
/* the calibration blocks of the last xivo_hip_jacobians_instate, per feature 2 x 22 row-major:
 * [ td (1) | Cg (9) | bg (3) | intrinsics (9, the first cam_dim in use) ]; blocks that are switched off read 0 */
int xivo_hip_get_jacobians_calib(xivo_hip_ctx* ctx, int b0, int nb, double* Jc2x22);
/* Estimator::MHGating (src/update.cpp:50-116) on the compact Jacobians (full
 * J row, as the reference gates with f->J()). */
int xivo_hip_mh_gate(xivo_hip_ctx* ctx, int B, double R, double mh_thresh, double mh_mult,
                     int min_inliers, unsigned char* inlier_mask_out, double* mh_dist_out);
/* Estimator::FilterUpdate stacking (src/update.cpp:129-138) through
 * Feature::FillJacobianBlock (src/feature.cpp:658-684): in-state inlier rows
 * first, then any OOS rows appended by xivo_hip_oos_project. */
int xivo_hip_stack(xivo_hip_ctx* ctx, int B, double R);
/* Feature::ComputeOOSJacobian (src/oos.cpp:8-89) + SlowGivens
 * (src/helpers.cpp:13-23): per feature (2k-3) projected rows appended after
 * the in-state rows with diagR = Roos. rows_out[b] = total OOS rows. feats == NULL projects the list of the
 * previous call again (it stays resident; same nb and n_oos) - for a caller that re-linearises without new tracks.
 * The 2k-3 rows are a reservation for rank(Hf) = 3. When Hf has rank r < 3 (all k observing groups at one pose - a platform
 * that has not moved - gives r = 2) the kernel of Hf^T has 2k-r vectors and the reference projects onto all of them; here the
 * feature still gets 2k-3 rows: the FIRST 2k-3 columns of Eigen's kernel basis A (A[:, :2k-3]^T Hx, A[:, :2k-3]^T r,
 * diagR = Roos), the last 3-r kernel vectors are dropped. Every row written is a null-space row of Hf; the update uses less
 * information than the reference's, never wrong information. rows_out counts 2k-3 per feature whatever the rank. A group
 * slot may be listed more than once in group_sind (its block accumulates).
 * Camera-calibration builds (cam_dim > 0): the observations are projected with the filter's own intrinsics, and - as the
 * reference codes ComputeOOSJacobianInternal (src/oos.cpp:39-89 writes the group / Wbc / Tbc blocks only) - the rows carry NO
 * intrinsics block; of the row builders in that file only ComputeLCJacobian has one (:125-142, xivo_hip_close_loop_stack). */
int xivo_hip_oos_project(xivo_hip_ctx* ctx, int b0, int nb, int n_oos, const xivo_oos_in* feats,
                         double Roos, int* rows_out);
/* The same with options. XIVO_HIP_OOS_WHOLE_BUFFER reproduces src/oos.cpp:28 AS CODED: SlowGivens is handed the whole
 * 2 * kMaxGroup-row buffers of the feature (src/jac.h:12-16), not the 2k rows ComputeOOSJacobianInternal filled, so every
 * feature contributes 2 * kMaxGroup - 3 rows (kMaxGroup = the layout's n_groups) however many groups saw it. What the
 * reference leaves in the rows behind 2k is unspecified (the buffers are Eigen::resize'd, never cleared); this mode defines
 * them as zero, for which FullPivLU::kernel appends one unit vector per such row: the first 2k - 3 rows are those of the
 * default call (at rank(Hf) < 3 truncated as described there), the others are H = 0, inn = 0, diagR = Roos - they change M
 * and S, not K, dx or P+. options = 0 is
 * xivo_hip_oos_project (SURVEY 8 a9's specification: the top 2k rows). feats == NULL re-projects with the options of the
 * call that uploaded the list. */
#define XIVO_HIP_OOS_WHOLE_BUFFER 1u
int xivo_hip_oos_project_ex(xivo_hip_ctx* ctx, int b0, int nb, int n_oos, const xivo_oos_in* feats,
                            double Roos, int* rows_out, unsigned options);
/* One loop-closure match (Estimator::CloseLoopInternal, src/update.cpp:171-212; the mapper that FINDS matches is out of
 * scope): an in-state feature ("old_feature") re-observed by the group in slot group_sind (Graph::LastAddedGroup) at pixel xp
 * (the observation of the new feature that was matched to it). */
typedef struct {
  int feat;        /* position of the old feature in the resident feature list (xivo_hip_set_scene / xivo_hip_edit_batch);
                      its state and anchor group give Xs = Feature::Xs(gbc), src/feature.cpp:107-118; -1 = absent match */
  int group_sind;  /* obs.g->sind()                                                                                      */
  double xp[2];    /* obs.xp                                                                                             */
} xivo_lc_match;
/* Feature::ComputeLCJacobian (src/oos.cpp:92-145) for the n matches of each filter in [b0, b0 + nb) + the stacking of
 * CloseLoopInternal (src/update.cpp:183-196: H_.setZero(2n, N), row pair 2i from match i, diagR_ = Rlc): the staged
 * measurement of those filters becomes the 2n loop-closure rows - d xp / d (group pose, Wbc, Tbc) and, for a context with
 * camera calibration on (xivo_hip_set_calib, cam_dim > 0), the intrinsics block of :125-142. xivo_hip_update_joseph +
 * xivo_hip_absorb_error then complete CloseLoopInternal (:207-208). matches: host, [nb x n]. */
int xivo_hip_close_loop_stack(xivo_hip_ctx* ctx, int b0, int nb, int n, const xivo_lc_match* matches, double Rlc);
/* Measurement compression (use_compression_ / compression_trigger_ratio_, src/estimator.h:399-402 - parsed by the
 * reference, src/estimator.cpp:115-117, but never acted on; xivo::QR, src/helpers.cpp:77-101 "QR-based measurement
 * compression"): call after xivo_hip_oos_project. For every filter whose OOS block has more than trigger_ratio (>= 1;
 * reference default 1.5) times as many rows as non-zero columns, the block is replaced by the triangular factor of its
 * QR decomposition (Householder reflections on the device; the rows only touch the extrinsics and group columns, so
 * the 2k-3 rows of every OOS feature collapse to at most 6 + 6 n_groups rows in total). Orthogonal row operations with
 * isotropic noise leave S^-1-weighted quantities - K, dx, P+ - unchanged to rounding. rows_out[b] (host, may be NULL) =
 * OOS rows of filter b afterwards; the stacked row count M shrinks to in-state rows + the largest of them. Any call that
 * stages new rows after the projection (xivo_hip_set_measurements*, xivo_hip_stack, xivo_hip_close_loop_stack, the one-filter
 * call) ends the OOS block: XIVO_HIP_ERR_INVALID until the next xivo_hip_oos_project. */
int xivo_hip_compress_oos(xivo_hip_ctx* ctx, int B, double trigger_ratio, int* rows_out);
/* Estimator::OnePointRANSAC (src/update.cpp:213-393) for filters [0,B) on the resident state; call after
 * xivo_hip_jacobians_instate + xivo_hip_mh_gate (the MH inliers are the input set, as OutlierRejection hands them over,
 * src/manager.cpp:629-650). Low-innovation set {|inn| < ransac_thresh} (the hypothesis loop of :238-258 never uses its
 * random index), BackupState on the device, P rows/cols of non-members zeroed (+ a temporary reference group when
 * gauge_group[b] holds no low-innovation inlier, FindNewRefGroup), partial UpdateJosephForm on the full rows J() +
 * AbsorbError, Jacobians at the updated state, chi-square rescue with ransac_chi2, RestoreState, Jacobians at the
 * original state. The resulting inlier set REPLACES the MH mask: a following xivo_hip_stack / xivo_hip_update_joseph /
 * xivo_hip_absorb_error runs on it.
 *   gauge_group   host [B]: slot of gauge_group_ptr_, -1 = none (NULL: none for every filter)
 *   absorb_groups host [B]: bit g = group slot g is in instate_groups_ when the partial update is absorbed (that list is
 *                 the previous frame's, src/manager.cpp:103); NULL = every slot
 *   inlier_mask_out / chi2_out [B x F], n_rejected_out [B]: host, any may be NULL. chi2 is 0 for features not tested.
 * Online-calibration builds (xivo_hip_set_calib): the calibration state is backed up and restored with X_
 * (src/estimator.cpp:1421-1427, :1442-1448), the partial update runs on the whole rows J() with their td / Cg / bg / intrinsics
 * blocks, AbsorbError retracts td / Cg / Ca / the intrinsics, and the rescue test is the whole-row chi-square of :350-356. */
int xivo_hip_one_point_ransac(xivo_hip_ctx* ctx, int B, double R, double ransac_thresh, double ransac_chi2,
                              const int* gauge_group, const unsigned long long* absorb_groups,
                              unsigned char* inlier_mask_out, double* chi2_out, int* n_rejected_out);
/* jac -> gate -> stack -> UpdateJosephForm in one call (Estimator::UpdateStep's
 * numeric core, src/manager.cpp:72-104) */
int xivo_hip_filter_update(xivo_hip_ctx* ctx, int B, double R, double mh_thresh, double mh_mult,
                           int min_inliers, int use_gating);
int xivo_hip_get_H(xivo_hip_ctx* ctx, int b, int* M_out, double* H, int ldh, double* inn, double* diagR);
/* ---- the step just before the path - depth sub-filter + candidate scoring ----
 * Feature::SubfilterUpdate (src/feature.cpp:246-297): one 3x3 EKF step per feature that is tracked but not
 * in the state yet, against the resident sensor pose / anchor groups (xivo_hip_set_scene), followed by
 * Criteria::Candidate / CandidateStrict (src/options.cpp:10-33) and Feature::score (src/feature.cpp:133-142),
 * which decide who is moved into the state. Embarrassingly parallel: one thread per (filter, feature). */
enum { XIVO_FEAT_INITIALIZING = 0, XIVO_FEAT_READY = 1 };
typedef struct {
  double x[3];            /* in/out: (X/Z, Y/Z, log Z) in the anchor camera frame (src/feature.h:258-262) */
  double P[9];            /* in/out: 3x3 covariance, column-major */
  double xp[2];           /* in: tracked pixel in the current frame */
  double outlier_counter; /* in/out */
  double score;           /* out: -P(2,2) */
  int ref_sind;           /* in: anchor group slot */
  int status;             /* in/out: XIVO_FEAT_INITIALIZING / XIVO_FEAT_READY */
  int init_counter;       /* in/out */
  int candidate;          /* out: bit 0 Criteria::Candidate, bit 1 Criteria::CandidateStrict */
} xivo_subfilter_feat;
typedef struct {
  double Rtri, MH_thresh;           /* SubfilterOptions (src/options.h:25-32): 3.5, 5.991 */
  int ready_steps;                  /* 5 */
  double min_depth, max_depth;      /* cfg min_depth / max_depth: 0.05, 5.0 */
  double max_subfilter_outlier;     /* 0.01 */
} xivo_subfilter_opts;
/* feats: host array [nb x n] (filter-major), updated in place */
int xivo_hip_subfilter_update(xivo_hip_ctx* ctx, int b0, int nb, int n, xivo_subfilter_feat* feats,
                              const xivo_subfilter_opts* opts);

/* Criteria::CandidateComparison (src/options.cpp:34-61): the order in which candidates enter the state
 * (std::sort of src/manager.cpp:375-376,420-421,499-500). feats [nb x n] as returned by xivo_hip_subfilter_update;
 * strict = 0: Criteria::Candidate passes, 1: Criteria::CandidateStrict. order_out [nb x n]: indices of the passing
 * candidates of each filter, best first, padded with -1; n_out [nb] their number. The comparison is reproduced AS
 * CODED: FeatureStatus first (READY before INITIALIZING), then Feature::score() = -P(2,2) - the value it computes from
 * `comparison_score_type` is never used (:41-60). score_out (optional, [nb x n]) returns that value anyway:
 * score_type 0 "DepthUncertainty" -P(2,2); 1 "CovarianceDiagNorm" -|diag P|; 2 "CovarianceDiagNormPlusOutlierCount"
 * -(|diag P| + outlier_counter). Host arithmetic only. */
int xivo_hip_candidate_order(const xivo_subfilter_feat* feats, int nb, int n, int strict, int score_type,
                             int* order_out, int* n_out, double* score_out);

/* ---- resident out-of-state feature pool: the reference's life cycle of a new track (src/manager.cpp:18-130) ----
 * Per filter, a pool of `pool_max` entries - features that are tracked but not in the state yet, each running the depth
 * sub-filter above - and a table of `anchor_max` anchors, the groups those features are anchored to (Group::Create from
 * the frame's pose, src/manager.cpp:121-126). An anchor is either linked to an in-state group slot (its pose is then that
 * slot's resident pose) or unlinked with a frozen pose of its own (a group that is not, or no longer, in the state). The
 * entries' data never leave the device; only the selection order (and which entries are still live) comes back.
 * pool_max <= XIVO_POOL_MAX_ENTRIES (the per-filter ordering sorts in one workgroup's LDS), else XIVO_HIP_ERR_UNSUPPORTED.
 * Calling xivo_hip_pool_config again re-allocates and empties everything. */
#define XIVO_POOL_MAX_ENTRIES 512
int xivo_hip_pool_config(xivo_hip_ctx* ctx, int pool_max, int anchor_max, const xivo_subfilter_opts* opts,
                         double remove_outlier_counter);
/* Group::Create(X_.Rsb, X_.Tsb): anchor slot[b] of filter b0 + b <- that filter's current resident pose, unlinked */
int xivo_hip_pool_anchor(xivo_hip_ctx* ctx, int b0, int nb, const int* slot /* nb; -1 = none for that filter */);
/* Feature::Initialize (src/feature.cpp:144-160) of new tracks: x = (UnProject(xp), log z0) - 1 / z0 under
 * XIVO_HIP_FLAG_INVDEPTH -, P = diag(std_xyz)^2, status INITIALIZING, counters 0, anchored at `anchor`. Camera::UnProject
 * runs on the device for every model (common/camera_{pinhole,atan,radtan,equidist}.h; radtan / equidistant with the
 * reference's default max_iter = 15 iterations and no early exit), with the filter's own intrinsics when the context has
 * camera calibration on (cam_dim > 0). Records of one call must name distinct (b, entry) pairs. */
typedef struct {
  int b;              /* filter */
  int entry;          /* pool entry (overwritten if live) */
  int anchor;         /* anchor the feature is anchored to */
  int reserved;
  double xp[2];       /* first pixel (Feature::back()) */
  double z0;          /* initial depth (initial_z, or the simulator's depth) */
  double std_xyz[3];  /* initial std of (x, y, depth coordinate) */
} xivo_pool_new;
int xivo_hip_pool_add(xivo_hip_ctx* ctx, int n, const xivo_pool_new* recs);
/* The out-of-state branch of ProcessTracks (src/manager.cpp:171-250) for every live entry of filters [0, B):
 * xp [B][pool_max][2] is the frame's pixel of each entry; NaN = the track was dropped: the entry is freed. Otherwise
 * Feature::SubfilterUpdate against the current pose and the anchor's pose (same device code and arithmetic as
 * xivo_hip_subfilter_update), then outlier_counter > remove_outlier_counter frees the entry. Then Criteria::Candidate
 * (strict = 0) / CandidateStrict (strict = 1) and the CandidateComparison order of the passing entries, exactly as
 * xivo_hip_candidate_order returns it for the pool as one [B x pool_max] array: order_out [B][pool_max] (entry indices, best
 * first, padded with -1), n_out [B], live_out [B][pool_max] (1 = entry still live). */
int xivo_hip_pool_step(xivo_hip_ctx* ctx, int B, const double* xp, int strict, int* order_out, int* n_out,
                       unsigned char* live_out);
/* download the pool / anchors of filters [b0, b0 + nb) (tests, diagnostics): entries as xivo_subfilter_feat with ref_sind =
 * the entry's anchor (-1: free entry); anchors as their frozen pose and linked slot (-1: unlinked). Either pointer may be NULL. */
int xivo_hip_pool_get(xivo_hip_ctx* ctx, int b0, int nb, xivo_subfilter_feat* entries /* nb x pool_max */,
                      xivo_group_in* anchor_poses /* nb x anchor_max */, int* anchor_slots /* nb x anchor_max */);

/* ---- depth initialisation of new tracks: pre-sub-filter triangulation and AdaptInitialDepth ----
 * Two-view triangulation (Feature::Triangulate, src/feature.cpp:686-751) with the five triangulators of src/helpers.cpp:103-371.
 * Frame 1 is the anchor camera, frame 2 the current camera; g12 = (anchor gsb * gbc)^-1 (gsb * gbc) maps frame-2 points into
 * frame 1, X is returned in frame 1. The reference's float narrowing is reproduced AS CODED: a0 / a1 (L1), lambda0 / lambda1
 * (check_cheirality), theta0 / theta1 / beta (check_angular_reprojection / check_parallax) and both thresholds are float,
 * everything else fp64. DIRECT_LINEAR_TRANSFORM_SVD takes the null vector of the 4x4 A from a one-sided Jacobi SVD (fixed
 * sweep count) and returns X = V(0:3,3) / V(3,3), as coded; L2_ANGULAR takes V.col(1) of the 2x3 B in closed form (B t^ = 0:
 * the minor eigenvector of B^T B in the plane perpendicular to t^; its sign does not enter the result). The depth range is
 * tested as zmin <= z <= zmax, so a NaN depth counts as a bad triangulation. */
enum {
  XIVO_TRI_OFF = 0,
  XIVO_TRI_DLT_SVD = 1,   /* "direct_linear_transform_svd" */
  XIVO_TRI_DLT_AVG = 2,   /* "direct_linear_transform_avg" */
  XIVO_TRI_L1 = 3,        /* "l1_angular" (the reference default, src/estimator.cpp:159) */
  XIVO_TRI_L2 = 4,        /* "l2_angular"   */
  XIVO_TRI_LINF = 5       /* "linf_angular" */
};
typedef struct {
  int struct_size;          /* sizeof(xivo_triangulate_opts) */
  int method;               /* XIVO_TRI_* */
  double zmin, zmax;        /* cfg triangulation zmin / zmax (0.05, 5.0) */
  double max_theta_thresh;  /* radians: the caller converts the cfg's degrees (src/estimator.cpp:163-164); used as float */
  double beta_thresh;       /* radians (cfg key "beta_thesh"); used as float */
} xivo_triangulate_opts;
typedef struct {
  double R12[9];   /* rotation of g12, column-major */
  double t12[3];   /* translation of g12 */
  double xc1[2];   /* UnProject(front()): normalised coordinates in the anchor camera */
  double xc2[2];   /* UnProject(back()): normalised coordinates in the current camera */
} xivo_tri_in;
typedef struct {
  double X[3];     /* the triangulated point in frame 1 (written whatever the return value, as the reference does) */
  int ret;         /* the triangulator's return value */
  int good;        /* ret && zmin <= X[2] <= zmax: Feature::Triangulate would set x = (X/z, Y/z, log z) */
} xivo_tri_out;
/* Stand-alone, batched: n problems from host arrays, one device thread each */
int xivo_hip_triangulate(xivo_hip_ctx* ctx, int n, const xivo_tri_in* in, xivo_tri_out* out, const xivo_triangulate_opts* opts);
/* triangulate_pre_subfilter for the pool (xivo_hip_pool_config): opts NULL or method XIVO_TRI_OFF disables it, the state
 * after xivo_hip_pool_config. While enabled, xivo_hip_pool_step triangulates every live entry at its first step (init_counter
 * == 0, the reference's f->size() == 2; src/manager.cpp:227-231) with this frame's pixel, before the sub-filter step (a
 * kernel of its own, launched only while enabled, ahead of the step): g12 from the entry's anchor pose and the filter's
 * current pose, xc1 = x[0:2], xc2 = UnProject(current pixel) with the filter's own intrinsics under camera calibration. x[0:2] equals UnProject(front()) at that point because only the
 * sub-filter step, which also increments init_counter, writes x after xivo_hip_pool_add; the kernel checks init_counter == 0
 * itself. A good triangulation sets x = (X/z, Y/z, log z) - 1/z under XIVO_HIP_FLAG_INVDEPTH -, P is left as it is. */
int xivo_hip_pool_triangulation(xivo_hip_ctx* ctx, const xivo_triangulate_opts* opts);
/* num_good_triangulations_ / num_bad_triangulations_ summed per filter over [b0, b0 + nb) since xivo_hip_pool_config; either
 * pointer may be NULL */
int xivo_hip_pool_tri_counts(xivo_hip_ctx* ctx, int b0, int nb, int* good_out, int* bad_out);
/* AdaptInitialDepth (src/manager.cpp:255-278). Each filter keeps a resident init_z, set to initial_z for every filter by
 * xivo_hip_pool_adapt_depth_config (and by xivo_hip_pool_config, to 0: unset). */
typedef struct {
  int struct_size;            /* sizeof(xivo_adapt_depth_opts) */
  int min_feature_lifetime;   /* cfg adaptive_initial_depth.minimum_feature_lifetime (5) */
  double initial_z;           /* cfg initial_z */
  double median_weight;       /* cfg adaptive_initial_depth.median_weight (0.99) */
  double min_z, max_z;        /* cfg min_depth / max_depth */
} xivo_adapt_depth_opts;
int xivo_hip_pool_adapt_depth_config(xivo_hip_ctx* ctx, const xivo_adapt_depth_opts* opts);
/* One workgroup per filter of [0, B). The depth set is the in-state features of the resident feature list (sind >= 0, z from
 * x[2]: exp, or 1/x under XIVO_HIP_FLAG_INVDEPTH) and the live READY pool entries whose lifetime exceeds
 * min_feature_lifetime. An entry's lifetime is its init_counter: the pool frees an entry in the first frame it is not
 * tracked, so the number of frames it lived through after its first is the number of sub-filter steps it took. Non-finite
 * depths are left out of the set (the reference would place a NaN wherever its iteration order puts it). m = the order
 * statistic of rank floor(n / 2); min_z <= m <= max_z: init_z <- (1 - beta) init_z + beta m, otherwise (or n = 0) init_z
 * stays. DEVIATION: the reference takes depth[n >> 1] in std::unordered_map iteration order, unsorted - an order that is not
 * a property of the input; this is the median the code names. init_z_out (host [B], may be NULL): init_z afterwards. */
int xivo_hip_pool_adapt_depth(xivo_hip_ctx* ctx, int B, double* init_z_out);
/* The resident init_z of filters [b0, b0 + nb) as it is, without an AdaptInitialDepth step (the device pool life cycle runs that
 * step itself and copies nothing out). Needs xivo_hip_pool_adapt_depth_config. Synchronises. */
int xivo_hip_pool_get_init_z(xivo_hip_ctx* ctx, int b0, int nb, double* init_z_out);
/* xivo_hip_pool_add with options: XIVO_POOL_ADD_ADAPTIVE_Z takes z0 from the filter's resident init_z instead of the record
 * (the record's z0 is then ignored; xivo_hip_pool_adapt_depth_config must have run). options = 0 is xivo_hip_pool_add. */
#define XIVO_POOL_ADD_ADAPTIVE_Z 1u
int xivo_hip_pool_add_ex(xivo_hip_ctx* ctx, int n, const xivo_pool_new* recs, unsigned options);

/* ---- Estimator::Propagate on the device-resident state ----
 * For filters [b0, b0 + nb): integrates the nominal motion state (Rsb, Tsb, Vsb, bg, ba, Rsg of the resident
 * xivo_pose_in, xivo_hip_set_scene) over dt with RK4Step (src/rk4.cpp:35-103) or PrinceDormandStep
 * (src/princedormand.cpp:85-221) under the fixed sub-stepping of src/rk4.cpp:13-32 (stepsize < 0: one step),
 * ComposeMotion (src/estimator.cpp:598-613) and ComputeMotionJacobianAt (src/estimator.cpp:615-704, default build:
 * no online IMU calibration), accumulates the sub-step transitions, then applies the covariance tail
 * (src/rk4.cpp:92-102) and P_mm += Qmodel (src/estimator.cpp:590) to the resident P. The IMU sample is modelled as
 * the reference does between two messages: value at the start + slope * t (src/estimator.cpp:556-575). */
typedef struct {
  double gyro[3], accel[3];              /* last_gyro_, last_accel_ */
  double slope_gyro[3], slope_accel[3];  /* (curr - last) / dt */
  double dt;
} xivo_imu_in;
typedef struct {
  double Qimu[144];    /* 12 x 12, column-major (gyro, accel, gyro-bias, accel-bias noise) */
  double Qmodel[529];  /* 23 x 23, column-major */
  double g[3];         /* gravity in the spatial frame before Rsg */
  int method;          /* 0: RK4, 1: PrinceDormand */
  double stepsize;     /* cfg integration stepsize (0.002); < 0: a single step of length dt */
  /* cfg_["PrinceDormand"] of the step-size-controlled branch (src/princedormand.cpp:17-22, :26-60; off in every shipped
   * configuration). control_stepsize != 0 (method 1 only, stepsize > 0) runs that branch AS CODED: PrinceDormandStep returns
   * 0 - its error estimate is commented out (:216-220) - so every step is followed by h *= max_scale_factor, clipped to the
   * end of the sample with the half-step rule (:53-58); a step starts from gyro0 + slope * total_step (:38-39), and the
   * current step h is carried from one sample - and one call - to the next as the reference's function-local static does
   * (:13; per filter here, (re)started at `stepsize` by the first controlled call of a context or a call with another
   * stepsize). tolerance / min_scale_factor only enter through the dead err != 0 arm; attempts is read and never used (:19).
   * All zero (the value-initialised struct of a caller that predates them): the fixed-step branch. */
  int control_stepsize;
  int attempts;
  double tolerance, min_scale_factor, max_scale_factor;
} xivo_prop_opts;
/* imu: [nb][n_imu] - the n_imu samples of each filter since its last call (one Estimator::Propagate each, in order);
 * their transitions are accumulated on chip and the O(23 N) cross-covariance tail is applied once.
 * Refused (XIVO_HIP_ERR_INVALID) before anything is uploaded or launched - P, the poses and the carried steps unchanged:
 *  - a dt that is not positive and finite (NaN, <= 0, +inf: `while (total_step < dt)` would not end);
 *  - a stepsize that is NaN, or in [0, 1e-6);
 *  - under control_stepsize: method != 1, stepsize not > 0, or max_scale_factor not >= 1 (NaN included). As coded every
 *    controlled step is followed by h *= max_scale_factor; below 1 the steps form a convergent series, and where its sum
 *    stays under dt the step underflows to 0 and the loop never ends - in the reference as here.
 * There is no cap on the number of sub-steps, as in the reference: a finite dt / stepsize ratio is the caller's budget. */
int xivo_hip_propagate(xivo_hip_ctx* ctx, int b0, int nb, int n_imu, const xivo_imu_in* imu, const xivo_prop_opts* opts);
/* The same for an online-calibration build (xivo_hip_set_calib with td >= 0 or Cg >= 0): kMotionSize = Index::End
 * (src/core.h:40-75) = Cg + 15, or td + 1 without the IMU calibration; ComposeMotion with the resident imu_.Cg() / imu_.Ca()
 * (xivo_calib_in), the motion Jacobian with the dWsb/dCg and dVsb/dCa blocks (src/estimator.cpp:626-638, :674-688), the tail
 * over motion_size rows / columns. Qmodel: motion_size x motion_size, column-major (opts->Qmodel is not read).
 * opts->control_stepsize works as in xivo_hip_propagate (the step a filter carries is shared by the two entry points).
 * xivo_hip_propagate itself refuses such a context (XIVO_HIP_ERR_UNSUPPORTED): its motion block is the default build's 23. */
int xivo_hip_propagate_calib(xivo_hip_ctx* ctx, int b0, int nb, int n_imu, const xivo_imu_in* imu, const xivo_prop_opts* opts,
                             const double* Qmodel);

/* ---- orthonormal Givens elimination and QR measurement compression ----
 * Batched xivo::Givens (src/helpers.cpp:48-75) and xivo::QR (src/helpers.cpp:78-101) on host arrays, nb
 * independent problems of identical shape, column-major, leading dimension = rows.
 *  Givens: eliminates Hf [rows x nf] with the rotations of G&VL Alg. 5.1.3 (the reference's givens(), eps guard
 *          1e-4f), rotates x and - as the reference codes it, helpers.cpp:64 - only the first nf columns of
 *          Hx [rows x nx]; then strips the first nf rows. rows_out[b] = rows - nf.
 *  QR:     triangularises Hx [rows x nx] (all columns rotated), rotates x; rows_out[b] = rows (the caller keeps
 *          the top block). effective_rows = -1: all rows. */
int xivo_hip_givens(xivo_hip_ctx* ctx, int nb, int rows, int nx, int nf, double* x, double* Hx, double* Hf,
                    int effective_rows, int* rows_out);
int xivo_hip_qr(xivo_hip_ctx* ctx, int nb, int rows, int nx, double* x, double* Hx, int effective_rows, int* rows_out);

/* Estimator::AbsorbError (src/estimator.cpp:875-921) on the device-resident nominal state of filters
 * [0,B): X += dx via State::operator+= (src/core.h:135-165: SO3 exp on Rsb, Rbc, Rsg), every group slot
 * += dx segment (src/group.h:25-29), every feature that was an inlier of the last gating / stacking pass
 * x += dx segment (src/feature.h:220); then dx = 0. (no host round trip of the state.) */
int xivo_hip_absorb_error(xivo_hip_ctx* ctx, int B);
/* download the resident scene (any pointer may be NULL) */
int xivo_hip_get_scene(xivo_hip_ctx* ctx, int b0, int nb, xivo_pose_in* poses, xivo_group_in* groups,
                       xivo_feat_in* feats);

/* ---- trajectory log: each frame's estimate and marginal covariance, recorded on the device ----
 * A sequence driver keeps thousands of filters resident; what it wants out per camera frame is each filter's motion state
 * and the covariance of a few error-state columns - not the scene (xivo_hip_get_scene) or the N x N covariance
 * (xivo_hip_download_P) of every filter. The log is device memory [T_max][batch_max] that one kernel launch per frame
 * appends to; it is read back in one copy at the end, or in slices of frames and filters. Nothing is allocated until
 * xivo_hip_traj_config. */
#define XIVO_TRAJ_MAX_COLS 32
typedef struct {
  int T_max;                     /* frames the log holds; 0 releases it                                     */
  int n_cols;                    /* 1 .. XIVO_TRAJ_MAX_COLS                                                  */
  int cols[XIVO_TRAJ_MAX_COLS];  /* error-state columns in [0, N), distinct, any order                      */
} xivo_traj_opts;
/* what one frame keeps of one filter's nominal state (fields as in xivo_pose_in) */
typedef struct {
  double Rsb[9], Tsb[3], Vsb[3], bg[3], ba[3];
  int status;    /* the filter's update status at that point (what xivo_hip_get_status would return for it) */
  int reserved;
} xivo_traj_rec;
/* (Re-)allocates the log through the context's owner and empties it: T_max frames of batch_max records and of batch_max
 * packed covariance blocks of n_cols (n_cols + 1) / 2 doubles. T_max = 0 (n_cols / cols are then not read) releases it. Bad
 * columns, n_cols out of range, or a size that overflows: XIVO_HIP_ERR_INVALID and the log is left as it was. */
int xivo_hip_traj_config(xivo_hip_ctx* ctx, const xivo_traj_opts* opts);
/* Appends one frame for filters [0, B), B <= batch_max (records of the other filters of that frame are undefined): one
 * launch on the context's stream, ordered after everything enqueued before it, no synchronisation. Per filter the record
 * above from the resident xivo_pose_in and the lower triangle of P[cols, cols], packed row by row: the entry of list
 * positions (i, j), i >= j, at i (i + 1) / 2 + j, read from the LOWER triangle of the stored P, P[max(ci, cj), min(ci, cj)].
 * ts_ns is kept on the host. frame_out (may be NULL) receives the frame's index. Log full: XIVO_HIP_ERR_FULL, nothing is
 * written or launched. Not configured (or no scene yet): XIVO_HIP_ERR_INVALID. */
int xivo_hip_traj_record(xivo_hip_ctx* ctx, int B, long long ts_ns, int* frame_out);
/* frames recorded so far (negative: a status) */
int xivo_hip_traj_count(xivo_hip_ctx* ctx);
/* count <- 0; the memory and the configuration are kept */
int xivo_hip_traj_reset(xivo_hip_ctx* ctx);
/* Frames [t0, t0 + nt) (all recorded) of filters [b0, b0 + nb) to host arrays, frame-major: recs [nt][nb],
 * cov [nt][nb][n_cols (n_cols + 1) / 2], ts [nt]. A NULL pointer skips that part. One synchronisation. */
int xivo_hip_traj_read(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, xivo_traj_rec* recs, double* cov, long long* ts);
/* Consistency of the logged poses against ground truth, on the device. gt: host [nt][nb][12], the true Rsb (column-major)
 * then Tsb of every entry of the slice. Columns 0..5 (Wsb, Tsb) must be among the recorded ones, else XIVO_HIP_ERR_INVALID.
 * Per entry: e = (log(Rsb_est^T Rsb_gt), Tsb_gt - Tsb_est) - the error-state vector xivo_hip_absorb_error would need in
 * columns 0..5 to move the estimate onto the truth -, Sigma = the 6 x 6 block of the record on those columns, Sigma = L L^T
 * (un-pivoted Cholesky), nees = |L^-1 e|^2; a Sigma that is not positive definite gives NaN. anees[t] is the mean of the
 * finite nees of frame t0 + t, n_used[t] their number (0: anees NaN); it is summed in a fixed order, so two calls on the same
 * log return the same bits. Outputs (host, any may be NULL): err6 [nt][nb][6], nees [nt][nb], anees [nt], n_used [nt]. */
int xivo_hip_traj_nees(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, const double* gt, double* err6, double* nees,
                       double* anees, int* n_used);

/* ---- trajectory score: aligned ATE and RPE of the logged poses against ground truth, on the device ----
 * The accuracy score of a run next to its consistency score (xivo_hip_traj_nees): what the reference's ComputeATE /
 * ComputeRPE (src/metrics.cpp) give for one trajectory, for every filter of a slice of the log, as one small record per
 * filter. The direction is the reference's: the alignment (R, T) = gYX takes ground truth onto the estimate
 * (metrics.cpp:17, r = Y - gYX X). A frame is used for a filter when all twelve values of its ground-truth entry and the
 * Rsb, Tsb of its record are finite; a pair (t, t + rpe_lag) needs both of its frames used. */
typedef struct {
  int align;     /* 0: score est against gt as they are; 1: rigid SE(3) alignment first (no scale) */
  int rpe_lag;   /* pairs (t, t + rpe_lag) in frames of the slice; 0: no RPE                         */
} xivo_traj_score_opts;
typedef struct {
  double ate;          /* sqrt(mean |Tsb_est - (R Tsb_gt + T)|^2) over the used frames; -1 if none     */
  double ate_raw;      /* the same with R = I, T = 0                                                   */
  double rpe_pos, rpe_rot; /* RMS over the pairs; -1 if there is no pair (or rpe_lag = 0)              */
  double R[9], T[3];   /* the alignment, gt -> est, R column-major; I, 0 when align = 0                */
  double sv[3];        /* singular values of the centred cross-covariance, descending                  */
  int n_used, n_pairs;
  int flags;           /* bit 0: rotation not determined (sv[1] <= 1e-12 sv[0], or n_used < 3)         */
  int reserved;
} xivo_traj_score;
#define XIVO_TRAJ_SCORE_UNDETERMINED 1
/* Frames [t0, t0 + nt) (all recorded) of filters [b0, b0 + nb); gt: host [nt][nb][12] as for xivo_hip_traj_nees; out: host
 * [nb]. Needs no particular columns recorded - it reads only the records. The alignment is the closed-form least-squares
 * optimum (Horn / Kabsch): H = sum (y - ybar)(x - xbar)^T over the used frames, y the estimated and x the true Tsb,
 * H = U diag(sv) V^T, R = U diag(1, 1, det(U V^T)) V^T, T = ybar - R xbar; centroids, H and the residuals are three passes
 * over the frames. RPE (metrics.cpp:110-113): dgX = gX(t)^-1 gX(t + lag), dgY likewise for the estimate, E = dgX^-1 dgY,
 * rpe_pos / rpe_rot = the roots of the means of |trans E|^2 / |log rot E|^2. Time association is the caller's: the lag is
 * in frames. Every sum runs in a fixed order that depends on the slice's frames only - a filter's record does not depend on
 * b0, nb or the other filters, and two calls return the same bits. One upload of gt, launches on the context's stream, one
 * download of nb records, one synchronisation; the staging is the context's. Log not configured, a slice outside the
 * recorded frames, rpe_lag < 0, a NULL ctx / gt / opts / out: XIVO_HIP_ERR_INVALID before any device work. nb = 0:
 * XIVO_HIP_OK, nothing is written; nt = 0: every record is the one of a filter without a used frame. One 64-lane workgroup
 * per filter: a slice of 2^26 filters or more would not fit one launch and is XIVO_HIP_ERR_UNSUPPORTED, also before any
 * device work (a guard on the launch shape - batch_max bounds nb first, and no context of that size exists today). */
int xivo_hip_traj_score(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, const double* gt,
                        const xivo_traj_score_opts* opts, xivo_traj_score* out);

/* ---- landmark log: each frame's in-state features, their world positions and covariances, recorded on the device ----
 * The other half of a frame's answer next to the trajectory log: what Estimator::InstateFeaturePositionsAndCovs
 * (src/estimator_accessors.cpp:308-357) returns for one filter - the in-state features ordered by FeatureCovComparison
 * (src/estimator.cpp:1451-1455: the Frobenius norm of the feature's 3 x 3 block of P_), for the best n the world position Xs,
 * that block, the last pixel - for every filter of the context, without moving the scene or the N x N covariance to the host.
 * The block of P_ is in the feature's local coordinates (X/Z, Y/Z, log Z) of its anchor camera and cannot be compared with a
 * world point; XIVO_MAP_WORLD_COV adds the covariance of Xs itself. Device memory [T_max][batch_max][n_out] that one kernel
 * launch per frame appends to; nothing is allocated until the log is configured. Layouts with more than XIVO_MAP_MAX_OUT
 * feature slots (n_features), or a resident feature list longer than that: XIVO_HIP_ERR_UNSUPPORTED. */
#define XIVO_MAP_MAX_OUT 128
enum { XIVO_MAP_WORLD_COV = 1u };
typedef struct {
  int T_max;        /* frames the log holds; 0 releases it (n_out / flags are then not read)       */
  int n_out;        /* entries kept per filter and frame, 1 .. XIVO_MAP_MAX_OUT                      */
  unsigned flags;   /* XIVO_MAP_*                                                                    */
} xivo_map_opts;
typedef struct {
  double Xs[3];          /* Feature::Xs (src/feature.cpp:107-112): Rsb_g (Rbc Xc(x) + Tbc) + Tsb_g, g = the feature's anchor group */
  double cov_local[6];   /* P block at feature_begin + 3 sind: (0,0),(0,1),(0,2),(1,1),(1,2),(2,2), as the reference packs
                            it; entry (r, c) read from the LOWER triangle of the stored P, P[off + c, off + r]                 */
  double cov_world[6];   /* same packing, J Pcc J^T (below); zeros without XIVO_MAP_WORLD_COV                                  */
  double xp[2];          /* last pixel                                                                                         */
  double score;          /* Frobenius norm of the 3 x 3 local block as stored (all nine entries; FeatureCovComparison's key)   */
  int pos, sind, ref_sind, reserved;   /* position in the resident feature list, feature slot, anchor group slot               */
} xivo_map_pt;
/* (Re-)allocates the log through the context's owner and empties it: T_max frames of batch_max x n_out entries and of
 * batch_max counts. n_out outside 1 .. XIVO_MAP_MAX_OUT, unknown flags, no layout yet or a size that overflows:
 * XIVO_HIP_ERR_INVALID, and the log is left as it was. */
int xivo_hip_map_config(xivo_hip_ctx* ctx, const xivo_map_opts* opts);
/* Appends one frame for filters [0, B), B <= batch_max: one launch on the context's stream, ordered after everything enqueued
 * before it, no synchronisation. Every entry of the resident feature list with sind >= 0 is a candidate, at whatever point of
 * the frame the driver calls this. ORDER: ascending score, ties by ascending pos (a score that is NaN sorts as +infinity).
 * The reference's comparator is `<=`, not a strict order, so what std::sort does with equal keys there is unspecified; this
 * rule is deterministic. The first n_pts = min(count, n_out) entries are kept; the slots behind them are written as zeros
 * with pos = sind = -1, so a read never returns stale memory.
 * With XIVO_MAP_WORLD_COV: c = the 15 error-state columns Xs depends on - Wbc (15..17), Tbc (18..20), the anchor group's six at
 * group_begin + 6 ref_sind (Wsb_g, Tsb_g), the feature's three at feature_begin + 3 sind; the calibration columns of an
 * online-calibration context do not enter Xs. Pcc = P[c, c] from the lower triangle, mirrored. J (3 x 15) = dXs / d(error
 * state) under the retraction the absorb call applies (R <- R exp(w), T <- T + dT, x <- x + dx), with Xb = Rbc Xc + Tbc:
 *   [ -Rsb_g Rbc hat(Xc) | Rsb_g | -Rsb_g hat(Xb) | I | Rsb_g Rbc dXc/dx ]
 * (dXc/dx of (X/Z, Y/Z, log Z), or of (X/Z, Y/Z, 1/Z) under XIVO_HIP_FLAG_INVDEPTH). cov_world = J Pcc J^T.
 * ts_ns is kept on the host. frame_out (may be NULL) receives the frame's index. Log full: XIVO_HIP_ERR_FULL, nothing is
 * written or launched. Not configured, no scene yet, or B out of range: XIVO_HIP_ERR_INVALID. */
int xivo_hip_map_record(xivo_hip_ctx* ctx, int B, long long ts_ns, int* frame_out);
/* frames recorded so far (negative: a status) */
int xivo_hip_map_count(xivo_hip_ctx* ctx);
/* count <- 0; the memory and the configuration are kept */
int xivo_hip_map_reset(xivo_hip_ctx* ctx);
/* Frames [t0, t0 + nt) (all recorded) of filters [b0, b0 + nb) to host arrays, frame-major: pts [nt][nb][n_out],
 * n_pts [nt][nb], ts [nt]. A NULL pointer skips that part. One synchronisation. */
int xivo_hip_map_read(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, xivo_map_pt* pts, int* n_pts, long long* ts);
/* Consistency of the logged landmarks against true world points, on the device; needs a log configured with
 * XIVO_MAP_WORLD_COV (else XIVO_HIP_ERR_INVALID). gt: host [nt][nb][n_out][3], the true point of every slot of the slice; a NaN
 * means no truth for that entry. Per recorded entry with finite truth: e = gt - Xs, Sigma = cov_world = L L^T (un-pivoted 3 x 3
 * Cholesky), nees = |L^-1 e|^2; a Sigma that is not positive definite gives NaN; slots behind n_pts and entries without truth
 * give NaN (err3 too). anees[t] is the mean of the finite nees of frame t0 + t over filters and entries, n_used[t] their
 * number (0: anees NaN); it is summed in a fixed order, so two calls on the same log return the same bits. Outputs (host, any
 * may be NULL): err3 [nt][nb][n_out][3], nees [nt][nb][n_out], anees [nt], n_used [nt]. */
int xivo_hip_map_nees(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, const double* gt, double* err3, double* nees,
                      double* anees, int* n_used);

/* ---- innovation log: each update's normalised innovation squared (NIS), recorded on the device ----
 * The consistency figure that needs no ground truth. With innovation inn and S = H P H^T + R it is inn^T S^-1 inn, to be held
 * against the number of rows. After dx = K inn it needs no factor: r = inn - H dx (the post-fit residual) equals R S^-1 inn, so
 *   nis = sum_i inn_i r_i / R_i,   prefit = sum_i inn_i^2 / R_i,   postfit = sum_i r_i^2 / R_i
 * come out of one pass over the staged rows - in whatever representation the update left them - and the resident dx: nothing
 * is factored, nothing staged is changed. PRICE: nis is what a cancellation leaves of prefit, so the rounding of r is
 * amplified by prefit / nis ~ |S| / R: about 1e-9 relative at a ratio of 1e7, 2e-6 at 1e11. prefit is recorded so that the
 * ratio can be seen. COUNTED ROWS: row i < M is counted when it has a non-zero H entry or inn_i != 0 - pairs a gate
 * neutralised (values 0, inn 0, diagR 1) and absent features drop out; OOS and loop-closure rows count like any other.
 * The record must be taken after the update and before xivo_hip_absorb_error (which zeroes dx): the context keeps a host-side
 * "dx is current" flag PER FILTER that every update call sets for the filters it updates (xivo_hip_update_joseph,
 * _dense_gated, _filter_update: [0, B); xivo_hip_update_joseph_host: its one filter) and xivo_hip_absorb_error, every
 * producer of new rows (a hand-over: for its own range), xivo_hip_one_point_ransac and xivo_hip_restore_P clear; a record of
 * filters [0, B) needs the flag of every one of them. Device memory [T_max][batch_max] records that one kernel launch per frame appends to; nothing
 * is allocated until the log is configured, and nothing outside xivo_hip_innov_config allocates for it. */
enum { XIVO_INNOV_FAILED = 1, XIVO_INNOV_LDLT = 2 };
typedef struct { int T_max; } xivo_innov_opts;   /* frames the log holds; 0 releases it */
typedef struct {                  /* 64 bytes */
  double nis, prefit, postfit;    /* as above; NaN when flags has XIVO_INNOV_FAILED                                      */
  double inn_max;                 /* max_i |inn_i| over the counted rows (0 if none; NaN if one of them is NaN)           */
  double dx_max;                  /* max_k |dx_k|, k < N (NaN if an entry is NaN)                                         */
  int dof;                        /* counted rows                                                                         */
  int rows;                       /* staged row count M of the context at that point                                      */
  int flags;                      /* XIVO_INNOV_FAILED: update status != 0 (prior kept, dx = 0); XIVO_INNOV_LDLT: the
                                     pivoted L D L^T fallback produced this update                                        */
  int reserved;
  double reserved2;
} xivo_innov_rec;
/* (Re-)allocates the log through the context's owner and empties it: T_max frames of batch_max records and the staging of
 * xivo_hip_innov_stats. A size that overflows: XIVO_HIP_ERR_INVALID and the log is left as it was. */
int xivo_hip_innov_config(xivo_hip_ctx* ctx, const xivo_innov_opts* opts);
/* Appends one frame for filters [0, B), B <= batch_max: one launch on the context's stream, no synchronisation. dx not
 * current for one of them (see above), not configured, nothing staged, or B out of range: XIVO_HIP_ERR_INVALID; log full:
 * XIVO_HIP_ERR_FULL; a state too wide for the kernel's LDS copy of dx (8 (N + M) + 4 M bytes over 48 KiB, N + M beyond about
 * 6000): XIVO_HIP_ERR_UNSUPPORTED; nothing is written or launched in any of these cases. ts_ns is kept on the host; frame_out (may be NULL) gets the frame's index. */
int xivo_hip_innov_record(xivo_hip_ctx* ctx, int B, long long ts_ns, int* frame_out);
/* frames recorded so far (negative: a status) */
int xivo_hip_innov_count(xivo_hip_ctx* ctx);
/* count <- 0; the memory and the configuration are kept */
int xivo_hip_innov_reset(xivo_hip_ctx* ctx);
/* Frames [t0, t0 + nt) (all recorded) of filters [b0, b0 + nb) to host arrays, frame-major: recs [nt][nb], ts [nt]. A NULL
 * pointer skips that part. One synchronisation. */
int xivo_hip_innov_read(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, xivo_innov_rec* recs, long long* ts);
/* Sums of the slice on the device: per frame over the slice's filters (frame_* [nt]) and per filter over the slice's frames
 * (filt_* [nb]); any output may be NULL. Records with flags != 0 or a non-finite nis are left out; *_used counts those that
 * went in. frame_nis[t] / frame_dof[t] is the figure to hold against 1. Fixed-shape strided partial sums and a tree, no
 * atomics: two calls on the same log return the same bits, and a filter's sums depend on (t0, nt) only - not on b0, nb. */
int xivo_hip_innov_stats(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, double* frame_nis, long long* frame_dof,
                         int* frame_used, double* filt_nis, long long* filt_dof, int* filt_used);

/* ---- resident state edits between updates, batched over filters ----
 * The reference edits X_/P_ one filter at a time on the host (the functions cited per kind). A sequence driver that
 * keeps thousands of filters resident cannot afford one launch per edit, so a whole frame's edits of all filters go
 * down in one call: ops must be grouped by filter with non-decreasing `b`; the ops of one filter are applied in
 * array order by one workgroup, different filters run concurrently. Offsets are error-state indices. */
enum {
  XIVO_EDIT_P_ZERO_RC = 0,     /* i0 = off, i1 = len             : as xivo_hip_p_zero_rc                              */
  XIVO_EDIT_P_COPY_RC = 1,     /* i0 = dst, i1 = src, i2 = len   : as xivo_hip_p_copy_rc                              */
  XIVO_EDIT_P_SET_BLOCK3 = 2,  /* i0 = off, v[0..8] = P3         : as xivo_hip_p_set_block3                           */
  /* Estimator::AddGroupToState (src/estimator.cpp:801-816), i0 = group slot: resident group[i0] <- current (Rsb,Tsb),
   * P rows then columns of the slot <- those of Wsb, then of Tsb */
  XIVO_EDIT_ADD_GROUP = 3,
  /* Estimator::RemoveGroupFromState (src/estimator.cpp:745-759), i0 = group slot */
  XIVO_EDIT_REMOVE_GROUP = 4,
  /* Estimator::AddFeatureToState (src/estimator.cpp:820-846) + Feature::FillCovarianceBlock (src/feature.cpp:753-760):
   * i0 = position j in the resident feature list, i1 = feature slot sind, i2 = anchor group slot,
   * v[0..2] = x, v[3..4] = xp, v[5..13] = the feature's own 3x3 covariance (column-major) */
  XIVO_EDIT_ADD_FEATURE = 5,
  /* Estimator::RemoveFeatureFromState (src/estimator.cpp:762-783), i0 = position j: its slot's rows/cols are zeroed
   * and the entry becomes absent (sind = -1) */
  XIVO_EDIT_REMOVE_FEATURE = 6,
  /* new tracked pixel of the feature at position i0 (Feature::back()), v[0..1] = xp */
  XIVO_EDIT_SET_XP = 7,
  /* feature pool (xivo_hip_pool_config): AddGroupToState (src/estimator.cpp:801-816) of the group behind anchor i1 into
   * group slot i0 - the group keeps its own creation pose (the anchor's), P rows then columns of the slot <- those of Wsb,
   * then of Tsb; the anchor is linked to the slot. XIVO_EDIT_REMOVE_GROUP of a slot an anchor links to first copies the
   * slot's resident pose into the anchor and unlinks it (the Group outlives its slot with its last pose). */
  XIVO_EDIT_ADD_GROUP_ANCHOR = 8,
  /* feature pool: AddFeatureToState + FillCovarianceBlock (as XIVO_EDIT_ADD_FEATURE) from pool entry i2's x / P / xp, at list
   * position i0 and feature slot i1, anchored at the slot its anchor links to; the entry is freed. The launch fails
   * (XIVO_HIP_ERR_INVALID) if the anchor is unlinked at that point of the op list. */
  XIVO_EDIT_ADMIT_POOL = 9
};
typedef struct {
  int b;             /* filter */
  int kind;          /* XIVO_EDIT_* */
  int i0, i1, i2;
  int reserved;
  double v[14];
} xivo_edit_op;
/* F = length of the resident feature list the ops index (positions 0..F-1; entries never written are absent).
 * F <= M_max / 2. Sets the list length used by the following Jacobian / gating / update calls. */
int xivo_hip_edit_batch(xivo_hip_ctx* ctx, int F, int n_ops, const xivo_edit_op* ops);

/* New tracked pixels of a whole frame in one dense array (what the tracker hands over per camera frame; replaces one
 * XIVO_EDIT_SET_XP op per feature): xp is [nb][F][2]; a NaN pair leaves that entry's pixel untouched (feature not
 * tracked in this frame / absent entry). Sets the list length F like xivo_hip_edit_batch. */
int xivo_hip_set_pixels(xivo_hip_ctx* ctx, int b0, int nb, int F, const double* xp);

/* ---- device-resident feature life cycle ("immediate" mode; opt-in) -------------------------------------------------------
 * What a sequence driver otherwise decides on the host per filter and frame and sends down as op lists (xivo_hip_edit_batch +
 * xivo_hip_set_pixels): matching the tracker's ids to the in-state slots, removing the features the tracker dropped
 * (ProcessTracks, src/manager.cpp:152-169) or the gate rejected (src/update.cpp:105-113) together with the groups they leave
 * empty (RemoveGroupFromState, src/estimator.cpp:745-759), and admitting new features with a new group
 * (SelectAndAddNewFeatures, src/manager.cpp:332-450; AddGroupToState / AddFeatureToState, src/estimator.cpp:801-846).
 * One workgroup per filter; the slot book lives on the device: feat_id[F_max] (track id held by feature slot j, -1: free; list
 * position j is feature slot j), group_refs[n_groups] (-1: free group slot, else the in-state features anchored there) and
 * six counters per filter. A feature's reference group is the resident feats[j].ref_sind. A frame is
 *   xivo_hip_life_begin -> update (xivo_hip_filter_update, or mh_gate / one_point_ransac / stack / update_joseph)
 *   -> xivo_hip_absorb_error -> xivo_hip_life_end
 * and no call of it synchronises or downloads anything. The results equal those of the op lists bit for bit, except x[2] =
 * log z of a new feature, where the device's log and libm's may differ in the last place. */
#define XIVO_LIFE_MAX_TRACKS 2048   /* tracks per filter and frame the kernels' LDS plan holds (ids 16 KiB + flags 8 KiB) */
#define XIVO_LIFE_MAX_SLOTS 256     /* feature slots / group slots per filter of that plan */
typedef struct {
  int tracks_max;          /* most tracks one filter brings in a frame; 0 releases the book and the staging */
  int min_new_features;    /* admit only with at least this many free feature slots, unless the state is empty */
  double min_depth, max_depth;   /* a candidate's depth lies strictly between them */
  double var_xyz[3];       /* diagonal of a new feature's 3 x 3 covariance (std^2, computed by the host) */
} xivo_life_opts;
typedef struct {
  long long updates;       /* frames in which the filter held a feature at its update */
  long long rejected;      /* features the gate rejected */
  long long dropped;       /* features the tracker dropped */
  long long admitted;      /* features that entered the state */
  long long groups_added;
  long long not_spd;       /* frames whose update status was non-zero */
} xivo_life_stats;
/* (Re-)allocates the book (all slots free, counters 0), the device copy of one frame's tracks and two page-locked staging
 * blocks - everything the frame calls need. Each of the three blocks holds batch_max * tracks_max tracks of 32 bytes (id, u, v,
 * depth) plus batch_max + 1 offsets, whatever a frame then brings: size tracks_max by the frames, not by the cap. XIVO_HIP_ERR_INVALID: a feature pool is configured on the context, no layout is set,
 * tracks_max > XIVO_LIFE_MAX_TRACKS (or negative), min_depth / max_depth / var_xyz not finite; XIVO_HIP_ERR_UNSUPPORTED: a
 * layout with more than XIVO_LIFE_MAX_SLOTS feature or group slots, a camera other than XIVO_CAM_PINHOLE (a new feature is
 * un-projected as ((u - cx) / fx, (v - cy) / fy)). The camera is the context's xivo_cam, the depth parametrisation
 * XIVO_HIP_FLAG_INVDEPTH. */
int xivo_hip_life_config(xivo_hip_ctx* ctx, const xivo_life_opts* opts);
/* Seeds the ids of filters [b0, b0 + nb) for a scene placed with xivo_hip_set_scene: feat_id is [nb][F] with F the resident
 * list length; an id must be >= 0 exactly where the resident entry is present, and a present entry at position j must sit in
 * feature slot j (else XIVO_HIP_ERR_INVALID, nothing changed). group_refs are counted from the resident sind / ref_sind. A
 * set-up call: reads the resident features back and synchronises. */
int xivo_hip_life_set_book(xivo_hip_ctx* ctx, int b0, int nb, const long long* feat_id);
/* The book of filters [b0, b0 + nb): feat_id [nb][F], feat_ref [nb][F] (-1: free), group_refs [nb][n_groups]; any may be
 * NULL. Synchronises. */
int xivo_hip_life_get_book(xivo_hip_ctx* ctx, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs);
/* Before the update. The frame's tracks of filters [0, B): off [B + 1] (off[0] = 0, non-decreasing), ids [n], meas [n][3] =
 * (u, v, depth), n = off[B]. Per filter: an in-state feature whose id is among the tracks gets that track's pixel (an id that
 * occurs twice: the last occurrence's), every other in-state feature leaves the state, groups left empty leave with them;
 * updates[b] is incremented where a feature is left. Sets the list length F (F <= n_features) like xivo_hip_edit_batch.
 * XIVO_HIP_ERR_INVALID before anything is launched or changed: not configured, a pool configured since, a filter with more
 * than tracks_max tracks, a malformed off, life_begin twice without life_end. The host arrays are copied to page-locked
 * staging before the call returns (two buffers: the copy waits only for the upload of the frame before the previous one). */
int xivo_hip_life_begin(xivo_hip_ctx* ctx, int B, int F, const int* off, const long long* ids, const double* meas);
/* After the update and xivo_hip_absorb_error, with the B of life_begin. Reads the resident inlier mask (what xivo_hip_get_gate
 * downloads) and the update status. Per filter, in order: in-state features with a zero mask leave (rejected), their tracks
 * are candidates again; empty groups are discarded; g = lowest free group slot; nothing is admitted without g, or with fewer
 * than min_new_features free slots while the state is not empty; candidates = tracks not in the state with min_depth < depth <
 * max_depth, by ascending id, ties by position; with a candidate, AddGroupToState(g) from the current pose, then the first
 * min(#free, #candidates) enter the free slots in ascending slot order with x = ((u - cx) / fx, (v - cy) / fy, log z or 1 / z),
 * xp = (u, v), P block = diag(var_xyz) after zeroing its rows and columns (as XIVO_EDIT_ADD_FEATURE). */
int xivo_hip_life_end(xivo_hip_ctx* ctx, int B);
/* The counters of filters [b0, b0 + nb). Synchronises. */
int xivo_hip_life_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_life_stats* out);

/* ---- device-resident feature life cycle, "subfilter" mode: the pool life cycle (opt-in) ------------------------------------
 * The reference's own life cycle of a new track (src/manager.cpp:18-130) decided on the device: what a sequence driver
 * otherwise decides per filter on the host around xivo_hip_pool_step and sends down as op lists (XIVO_EDIT_REMOVE_*,
 * XIVO_EDIT_ADD_GROUP_ANCHOR, XIVO_EDIT_ADMIT_POOL), xivo_hip_set_pixels, xivo_hip_pool_anchor and xivo_hip_pool_add. One
 * workgroup per filter. Next to the in-state book of the immediate life cycle (feat_id, group_refs) a filter has a pool book:
 * ent_id[pool_max] (track id held by pool entry e, -1: free), ent_born[pool_max] (frame counter at the entry's creation),
 * anc_used[anchor_max], anc_life[anchor_max] (Group::lifetime). An entry's anchor is the resident entry's ref_sind, an anchor's
 * link the resident anchor's slot (xivo_hip_pool_get). A frame is
 *   xivo_hip_propagate -> xivo_hip_pool_life_begin -> update -> xivo_hip_absorb_error -> xivo_hip_pool_life_end
 * and no call of it synchronises or downloads anything; with the tracks produced on the device (the point-cloud world below)
 *   xivo_hip_propagate -> xivo_hip_pcw_tracks -> xivo_hip_pool_life_begin_tracks -> update -> xivo_hip_absorb_error -> xivo_hip_pool_life_end
 * and frames of the two kinds may alternate on one context. P, the scene, the pool, the anchors and init_z equal those of the op
 * lists bit for bit: both run the same device functions in the same order. Every camera model is supported (a new entry is
 * initialised by the device code of xivo_hip_pool_add). The rules, per filter, in frame order:
 *   begin  - a used anchor's life is incremented, an unused anchor's is 0 (Group::IncrementLifetime, :36-41);
 *          - of a repeated id among the tracks the last occurrence supplies the pixel, for feature slots and pool entries;
 *          - in-state features without a track leave the state, groups left empty leave with them (an anchor linked to such a
 *            slot is frozen at the group's pose and unlinked, as XIVO_EDIT_REMOVE_GROUP does); pool entries without a track
 *            are freed (ProcessTracks, :171-250);
 *          - the pool step (as xivo_hip_pool_step, triangulation included when configured) on the other entries' pixels;
 *          - entries the step did not leave live are freed; the step's order is walked: the walk stops when no feature slot is
 *            free; an entry whose anchor is unlinked takes the lowest free group slot (ADD_GROUP_ANCHOR), and without a free
 *            group slot that entry is skipped and the walk goes on; admission is ADMIT_POOL into the lowest free feature slot
 *            (:332-450); every in-state feature then takes the frame's pixel.
 *   end    - features with a zero inlier mask leave the state (rejected), groups left empty are discarded;
 *          - new tracks are those whose id is in neither the state nor the pool after these removals, by ascending id, ties
 *            by position; of a repeated id among them only the first takes part, the others are ignored and counted nowhere;
 *          - with a new track: without a free anchor all are counted as pool_dropped; else the lowest free anchor is created
 *            from the current pose, unlinked, life 0, the new tracks take the free entries in ascending order
 *            (Feature::Initialize with z0 = initial_z, or the resident init_z with adaptive_z), the surplus is pool_dropped;
 *          - a used, unlinked anchor with life > max_group_lifetime that no live entry references is freed
 *            (EnforceMaxGroupLifetime, :282-304); then AdaptInitialDepth when xivo_hip_pool_adapt_depth_config is on. */
#define XIVO_POOL_LIFE_MAX_ANCHORS 256   /* anchors per filter the kernels' LDS plan holds */
typedef struct {
  int struct_size;         /* sizeof(xivo_pool_life_opts) */
  int tracks_max;          /* most tracks one filter brings in a frame; 0 releases everything the config allocated */
  int max_group_lifetime;  /* EnforceMaxGroupLifetime's bound */
  int adaptive_z;          /* != 0: a new entry's z0 is the filter's resident init_z (needs xivo_hip_pool_adapt_depth_config) */
  double initial_z;        /* z0 of a new entry otherwise */
  double std_xyz[3];       /* initial std of a new entry's (x, y, depth coordinate) */
} xivo_pool_life_opts;
typedef struct {
  long long updates, rejected, dropped, admitted, groups_added, not_spd;   /* as xivo_life_stats */
  long long pool_added;      /* new tracks that took a pool entry */
  long long pool_dropped;    /* new tracks that found no entry or no anchor */
  long long pool_outliers;   /* entries freed because the step did not leave them live (a tracker-dropped entry is not counted) */
  long long anchors_created, anchors_freed;
  long long admit_steps;     /* sum over admitted entries of the frames since the entry was created */
} xivo_pool_life_stats;
/* (Re-)allocates the books (everything free, counters 0, frame counter 0), the step's device xp / order / n / live, and the
 * track block with its two page-locked staging blocks (as xivo_hip_life_config). Needs xivo_hip_pool_config with no live entry
 * and no anchor created since, and a layout; else, or with the immediate device life cycle configured, a wrong struct_size,
 * tracks_max outside [0, XIVO_LIFE_MAX_TRACKS], values that are not finite, initial_z <= 0, or adaptive_z without
 * xivo_hip_pool_adapt_depth_config: XIVO_HIP_ERR_INVALID. More than XIVO_LIFE_MAX_SLOTS feature or group slots or more than
 * XIVO_POOL_LIFE_MAX_ANCHORS anchors: XIVO_HIP_ERR_UNSUPPORTED. While configured, xivo_hip_pool_anchor, xivo_hip_pool_add(_ex),
 * xivo_hip_pool_step and the XIVO_EDIT_ADD_GROUP_ANCHOR / XIVO_EDIT_ADMIT_POOL ops return XIVO_HIP_ERR_INVALID and change
 * nothing (the context's host mirrors of the pool are stale); xivo_hip_pool_get / _tri_counts / _adapt_depth_config work.
 * tracks_max = 0 releases and re-reads the mirrors from the device, after which the host life cycle can go on; so does
 * xivo_hip_pool_config. Every call that releases the track block (tracks_max = 0 on a configured context,
 * xivo_hip_pool_config) releases the resident worlds of xivo_hip_pcw_config with it, as xivo_hip_life_config does: configure
 * them again after the life cycle; a refused call releases nothing. Synchronises. */
int xivo_hip_pool_life_config(xivo_hip_ctx* ctx, const xivo_pool_life_opts* opts);
/* The in-state ids, as xivo_hip_life_set_book / xivo_hip_life_get_book; get_book also returns the pool book: ent_id
 * [nb][pool_max], ent_born [nb][pool_max], anc_used [nb][anchor_max], anc_life [nb][anchor_max]. Any output may be NULL. */
int xivo_hip_pool_life_set_book(xivo_hip_ctx* ctx, int b0, int nb, const long long* feat_id);
int xivo_hip_pool_life_get_book(xivo_hip_ctx* ctx, int b0, int nb, long long* feat_id, int* feat_ref, int* group_refs,
                                long long* ent_id, int* ent_born, int* anc_used, int* anc_life);
/* Before the update: uploads the tracks (off / ids / meas as xivo_hip_life_begin; the depth column is not read), then the begin
 * kernel, triangulation and the pool step, the admit kernel. strict: CandidateStrict (vision_counter >=
 * strict_criteria_timesteps). Increments the frame counter. XIVO_HIP_ERR_INVALID before anything is copied or launched: not
 * configured, a malformed off, a filter above tracks_max, begin twice without end. */
int xivo_hip_pool_life_begin(xivo_hip_ctx* ctx, int B, int F, const int* off, const long long* ids, const double* meas, int strict);
/* xivo_hip_pool_life_begin without the copy and the upload: consumes the tracks the last xivo_hip_pcw_tracks(B) or
 * xivo_hip_pcw_tracks_resident(B) left in the block (once), one row of tracks_max per filter; the same begin kernel,
 * triangulation, pool step and admit kernel follow, the frame counter is incremented and xivo_hip_pool_life_end reads the tracks
 * in the block too. Neither synchronises nor allocates. XIVO_HIP_ERR_INVALID, nothing changed: no tracks were produced for this
 * B since the last begin of either kind, and everything xivo_hip_pool_life_begin refuses (the immediate life cycle's context
 * among it: that one takes xivo_hip_life_begin_tracks, which in turn refuses a pool context). */
int xivo_hip_pool_life_begin_tracks(xivo_hip_ctx* ctx, int B, int F, int strict);
/* After the update and xivo_hip_absorb_error, with the B of begin: the end kernel, then AdaptInitialDepth when configured. */
int xivo_hip_pool_life_end(xivo_hip_ctx* ctx, int B);
/* The counters of filters [b0, b0 + nb). Synchronises. */
int xivo_hip_pool_life_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_pool_life_stats* out);

/* ---- MSCKF update from tracks that end outside the state (opt-in; needs xivo_hip_pool_config) --------------------------------
 * The reference parses use_OOS / OOS_update_min_observations / oos_meas_std and stops with "MSCKF not implemented"
 * (src/estimator.cpp:113-122). Here a pool entry whose track ends while it is READY, with a depth inside (min_depth, max_depth)
 * and at least min_obs observations from anchors whose groups are in the state now, constrains those groups once: its world
 * point Xs = Feature::Xs(gbc) of the resident entry and its anchor's pose goes with the observations (group slot, pixel) into
 * the context's resident OOS list - the one xivo_hip_oos_project(feats == NULL) re-projects -, at most oos_max entries per filter
 * and frame in ascending entry index. The integer rules are pool_lifecycle_device.h's (plife_oos_*, plife_hist_*).
 * Frame order: ... -> xivo_hip_pool_oos_collect -> pool step / admissions -> Jacobians, gate, xivo_hip_stack ->
 * xivo_hip_pool_oos_project -> xivo_hip_pool_oos_gate -> xivo_hip_update_joseph.
 * Two life cycles, one list, byte for byte. Host life cycle: the observation rings are the host's (SequenceRunner's _PoolBook)
 * and xivo_hip_pool_oos_collect hands its decisions down. Device pool life cycle (xivo_hip_pool_life_config first, then
 * xivo_hip_pool_oos_config, before the first frame): the rings live in HBM next to the pool, xivo_hip_pool_life_begin[_tracks]
 * makes the list itself between its begin kernel and the pool step (pool_oos_select_kernel), xivo_hip_pool_life_end records the
 * frame's observations (pool_oos_record_kernel); nothing is uploaded, downloaded or waited for. */
typedef struct {
  int struct_size;   /* sizeof(xivo_pool_oos_opts) */
  int oos_max;       /* OOS features per filter and frame; 0: off, the buffers are released */
  int max_obs;       /* observations per feature, 2 .. XIVO_OOS_MAX_OBS */
  int min_obs;       /* OOS_update_min_observations (5), 2 .. max_obs */
  double Roos;       /* oos_meas_std^2, > 0 */
  double chi2[32];   /* chi2[dof]: gate threshold of a feature with dof = 2k - 3 rows; 0: no gate for that dof */
} xivo_pool_oos_opts;
/* One dropped pool entry as the host life cycle hands it over: its valid observations, oldest first. Records are ordered by
 * (b, entry); n_obs may be anything in 0 .. max_obs (the device decides with the entry's status and depth). */
typedef struct {
  int b, entry, n_obs, reserved;
  int group_sind[XIVO_OOS_MAX_OBS];
  double xp[XIVO_OOS_MAX_OBS][2];
} xivo_pool_oos_cand;
typedef struct {
  long long oos_used;     /* entries put on a frame's list (counted when the list is made; gated ones included) */
  long long oos_gated;    /* of those, gated out by xivo_hip_pool_oos_gate */
  long long oos_surplus;  /* eligible beyond oos_max */
  long long oos_short;    /* READY, dropped, fewer than min_obs valid observations */
} xivo_pool_oos_stats;
/* Every frame then reserves oos_max * (2 max_obs - 3) rows behind the in-state rows (xivo_hip_pool_oos_rows): create the context
 * with that many rows more plus the 16 rows the mixed stacking pads the block with. Zeroes the counters. */
int xivo_hip_pool_oos_config(xivo_hip_ctx* ctx, const xivo_pool_oos_opts* opts);
int xivo_hip_pool_oos_rows(xivo_hip_ctx* ctx);
/* Host life cycle only (the device one makes the list itself). The frame's list of filters [0, B) from the host's decisions: n records, before the pool step of the frame (which frees the
 * dropped entries) and after the frame's group removals are known to the host - group_sind are the slots the observing
 * anchors' groups hold in this frame's update. One wave per filter walks its records in order (plife_oos_decide), computes Xs of
 * the used ones and writes positions [0, used) of the filter's oos_max list positions; the others get n_obs = 0. An observation
 * whose group_sind is outside the layout is dropped. The entries' data never leave the device. Synchronises (cands is borrowed). */
int xivo_hip_pool_oos_collect(xivo_hip_ctx* ctx, int B, int n, const xivo_pool_oos_cand* cands);
/* After xivo_hip_stack: the resident list's rows (oos_kernel, the mixed stacking of xivo_hip_oos_project_ex) into the fixed
 * block; rows no feature fills are H = 0, inn = 0, diagR = Roos - they change M and S but not K, dx or P+
 * (XIVO_HIP_OOS_WHOLE_BUFFER). Neither synchronises nor downloads. XIVO_HIP_ERR_UNSUPPORTED where the mixed stacking does not
 * apply (online calibration, XIVO_HIP_FLAG_DENSE_H, a context without the spare rows). */
int xivo_hip_pool_oos_project(xivo_hip_ctx* ctx, int B);
/* After xivo_hip_pool_oos_project: per (filter, list position) gamma = r^T (H_o P H_o^T + Roos I)^-1 r over the feature's
 * 2k - 3 rows, from the sub-block of P under the Wbc / Tbc and the k observing groups' columns (chol in LDS, one workgroup each).
 * gamma > chi2[2k - 3] (where that is > 0) or a non-positive pivot gates the feature out: its H rows and inn become zero, diagR
 * stays, oos_gated counts it. gamma is kept per feature (-1: non-positive pivot, 0: unused position). No synchronisation. */
int xivo_hip_pool_oos_gate(xivo_hip_ctx* ctx, int B);
/* tests, diagnostics: the resident list [nb][oos_max] and gamma [nb][oos_max] of filters [b0, b0 + nb). Either may be NULL. */
int xivo_hip_pool_oos_get(xivo_hip_ctx* ctx, int b0, int nb, xivo_oos_in* list, double* gamma);
/* ... and the device life cycle's history of filters [b0, b0 + nb): the anchors' creation frames anc_born [nb][anchor_max] and the
 * rings hist_cnt [nb][pool_max] (observations appended since the entry was taken; ring slot = count % max_obs), hist_anchor /
 * hist_born [nb][pool_max][max_obs], hist_xp [nb][pool_max][max_obs][2]. Any pointer may be NULL. XIVO_HIP_ERR_INVALID without the
 * device pool life cycle. */
int xivo_hip_pool_oos_get_rings(xivo_hip_ctx* ctx, int b0, int nb, int* anc_born, int* hist_cnt, int* hist_anchor, int* hist_born,
                                double* hist_xp);
int xivo_hip_pool_oos_get_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_pool_oos_stats* out);

/* ---- point-cloud world: the simulator's tracks produced on the device (opt-in; needs one of the device life cycles) -------
 * What BatchPCW.generate (xivo_amd/pcw.py, after the reference's scripts/point_cloud_world.py:44-131) computes on the host per
 * camera frame: every world point is projected through the frame's ground-truth camera pose, a point in front of the camera
 * whose pixel lies in [0, imw] x [0, imh] is visible, a visible point without a track id takes the world's next one in ascending
 * point order, a point that is not visible loses its id (so a point that returns is a new track), and the visible points - in
 * ascending point order - are the frame's tracks (id, u + noise, v + noise, depth). The worlds stay on the device (points, the id
 * each point holds, the next id of each world); a frame needs the camera poses only, 96 bytes per filter, and is
 *   xivo_hip_propagate -> xivo_hip_pcw_tracks -> xivo_hip_life_begin_tracks -> update -> xivo_hip_absorb_error -> xivo_hip_life_end
 * (the pool life cycle: xivo_hip_pool_life_begin_tracks / xivo_hip_pool_life_end in their place).
 * The tracks are written into the life cycle's device block, one row of tracks_max per filter; frames fed by
 * xivo_hip_life_begin / xivo_hip_pool_life_begin (host tracks) and by the _begin_tracks calls may alternate freely. The evaluation order of the
 * projection and the noise generator (Philox4x32-10 keyed by the seed, counter = point, filter, frame; one Box-Muller pair per
 * point) are specified in xivo_amd/csrc/pcw_device.h; pcw.philox_normal restates the generator for host code. A point's
 * noise depends on (seed, frame, filter, point) only. */
typedef struct {
  int struct_size;         /* sizeof(xivo_pcw_opts) */
  int npts;                /* points per world; 0 releases the worlds */
  double fx, fy, cx, cy;   /* pinhole intrinsics of the simulated camera (one set for all filters; xivo_hip_pcw_camera: any model) */
  double imw, imh;         /* image width and height in pixels; the borders count as inside */
} xivo_pcw_opts;
/* (Re-)allocates the resident worlds of batch_max filters - Xs [batch_max][npts][3], ids [batch_max][npts], next_id and the track
 * count per filter - and two page-locked blocks of batch_max x 12 doubles for the poses. The worlds start empty (points at
 * the origin, no ids, next id 0) until xivo_hip_pcw_set_world. XIVO_HIP_ERR_INVALID, nothing changed: neither device life cycle
 * is configured (xivo_hip_life_config, xivo_hip_pool_life_config), npts > its tracks_max (a filter can then never produce more tracks than its row of the
 * block holds), a value that is not finite, a wrong struct_size, a frame open between a begin and its end of either life cycle.
 * Who releases the worlds besides npts = 0: xivo_hip_life_config (whatever its arguments, unless the pool life cycle is
 * configured - the block and the worlds are then that one's and stay), xivo_hip_pool_life_config and xivo_hip_pool_config
 * whenever they release the pool life cycle's track block, and xivo_hip_destroy: configure the worlds again after the life
 * cycle. Synchronises. */
int xivo_hip_pcw_config(xivo_hip_ctx* ctx, const xivo_pcw_opts* opts);
/* The camera the producer projects through, after xivo_hip_pcw_config (which returns to the pinhole of xivo_pcw_opts, as does
 * cam = NULL here): any XIVO_CAM_* model, the struct the estimator itself takes (xivo_hip_set_layout); the image is cam->cols x
 * cam->rows, borders included. With x = Xc_0 / z, y = Xc_1 / z the normalised camera coordinates of a point, the pixel is that
 * of the estimator's own projection (xivo_amd/csrc/camera_device.h; XIVO_CAM_PINHOLE: (fx Xc_0) / z + cx as without a camera),
 * and a point is visible when it is in front, hypot(x, y) <= max_radius and the pixel lies in the image. max_radius guards
 * against the fold-back of a polynomial distortion far off axis, where points outside the field of view would land inside the
 * image again; +inf: no guard. The evaluation order is specified in xivo_amd/csrc/pcw_device.h, pcw.project_points_cam restates
 * it for host code. Ranks, ids and noise are as without a camera. Takes effect with the next frame call; does not synchronise.
 * XIVO_HIP_ERR_INVALID, nothing changed: no worlds configured, a frame open between a begin and its end, an unknown model,
 * rows or cols <= 0, an intrinsic or a coefficient that is not finite, max_radius NaN or <= 0. */
int xivo_hip_pcw_camera(xivo_hip_ctx* ctx, const xivo_cam* cam, double max_radius);
/* The worlds of filters [b0, b0 + nb): Xs [nb][npts][3]; ids [nb][npts] (NULL: every id -1, no point is tracked); next_id [nb]
 * (NULL: 10000, counter0 of src/feature.h). A set-up call: synchronises. */
int xivo_hip_pcw_set_world(xivo_hip_ctx* ctx, int b0, int nb, const double* Xs, const long long* ids, const long long* next_id);
/* ids [nb][npts] and next_id [nb] as the last frame left them; either may be NULL. Synchronises. */
int xivo_hip_pcw_get_world(xivo_hip_ctx* ctx, int b0, int nb, long long* ids, long long* next_id);
/* One camera frame of filters [0, B): gsc [B][12] is the ground-truth camera pose of each, Rsc row-major then Tsc (a world
 * point X has camera coordinates Rsc^T (X - Tsc)). Copies the poses to page-locked staging, enqueues their upload and the
 * producer; does not synchronise and allocates nothing. noise_px_std: standard deviation of the pixel noise (0: none, bit for
 * bit the projection); seed, frame: the generator's key and the frame's part of its counter. XIVO_HIP_ERR_INVALID, nothing
 * changed: no worlds configured, B out of range, called between a begin and its end of either life cycle. */
int xivo_hip_pcw_tracks(xivo_hip_ctx* ctx, int B, const double* gsc, double noise_px_std, unsigned long long seed,
                        unsigned long long frame);
/* xivo_hip_life_begin without the upload: consumes the tracks the last xivo_hip_pcw_tracks(B) left in the block (once);
 * xivo_hip_life_end then reads them there too. XIVO_HIP_ERR_INVALID, nothing changed: no tracks were produced for this B since
 * the last life_begin of either kind, and everything xivo_hip_life_begin refuses (a pool life cycle's context among it). */
int xivo_hip_life_begin_tracks(xivo_hip_ctx* ctx, int B, int F);
/* Read-back for tests and debugging of what the last xivo_hip_pcw_tracks left for filters [b0, b0 + nb) (within its B; gone
 * after a host-track xivo_hip_life_begin): cnt [nb], ids [nb][tracks_max], meas [nb][tracks_max][3]; entries behind cnt[b]
 * read -1 / 0. Any may be NULL. Synchronises. */
int xivo_hip_pcw_get_tracks(xivo_hip_ctx* ctx, int b0, int nb, int* cnt, long long* ids, double* meas);

/* ---- track faults of the point-cloud world's producer (opt-in) ---------------------------------------------------------------
 * Random track loss, gross outliers (one frame, or sticky: a bias the track keeps until it ends) and heavy-tailed noise, drawn
 * on the device from two more counters of the pixel noise's generator, with a ground-truth flag byte beside every track and a
 * device-side score of the gate's decisions against the flags. The rules, the two draws and the flag bits are specified in
 * xivo_amd/csrc/pcw_device.h ("Track faults"); pcw.fault_draw and BatchPCW.generate(faults=...) restate them for host code bit
 * for bit. Off (never configured, or released) every call computes what it computes without this section. */
typedef struct {
  int struct_size;                        /* sizeof(xivo_pcw_fault_opts) */
  int sticky;                             /* 0: an outlier lasts one frame; 1: its offset stays on the track until the track ends */
  double p_drop, p_outlier, p_tail;       /* per visible point and frame, each in [0, 1], their sum <= 1 */
  double outlier_min_px, outlier_max_px;  /* each component of an outlier's offset is +-[min, max] px, 0 <= min <= max */
  double tail_scale;                      /* a tail event multiplies noise_px_std by this (>= 1) */
} xivo_pcw_fault_opts;
/* per filter, summed over the frames since xivo_hip_pcw_fault_config. The producer's: tracks written, visible points dropped,
 * outlier events, tail events, tracks that carried an earlier outlier's bias. The score's, over the in-state features whose
 * track the frame held: faulty (flag & 5) or nominal against rejected (inlier mask 0) or kept. */
typedef struct {
  long long tracks, dropped, outlier_events, tail_events, biased;
  long long outlier_rejected, outlier_kept, nominal_rejected, nominal_kept;
} xivo_pcw_fault_stats;
/* Turns the fault path of xivo_hip_pcw_tracks / _tracks_resident on (opts) or off (NULL: releases). Allocates the resident bias
 * [batch_max][npts][2], the flag row [batch_max][tracks_max] and the counters [batch_max], all zero. XIVO_HIP_ERR_INVALID,
 * nothing changed: no worlds configured; a frame open between a begin and its end; a wrong struct_size; a probability outside
 * [0, 1] or their sum (p_drop + p_outlier) + p_tail > 1; outlier_min_px < 0 or > outlier_max_px; tail_scale < 1; any value that
 * is not finite; sticky outside {0, 1}. xivo_hip_pcw_set_world zeroes the bias of the filters it sets; whatever releases the
 * worlds releases these with them. Synchronises. */
int xivo_hip_pcw_fault_config(xivo_hip_ctx* ctx, const xivo_pcw_fault_opts* opts);
/* W > 0: the filter word of the pixel-noise and fault counters is b % W from the next frame call on, so that filters w, w + W,
 * w + 2 W, ... draw the same words (T tunings over W worlds); 0: every filter its own stream. The trajectory producer's IMU
 * stream is not touched. XIVO_HIP_ERR_INVALID: no worlds configured, W < 0, a frame open. Does not synchronise. */
int xivo_hip_pcw_stream_share(xivo_hip_ctx* ctx, int W);
/* Between the update and the life_end / pool_life_end of a frame of B filters that was begun on the producer's tracks
 * (xivo_hip_life_begin_tracks / xivo_hip_pool_life_begin_tracks): for every feature slot of the book that holds an id, the
 * frame's track with that id (the last one on a repeated id), its flag byte and the update's inlier mask entry add one to one
 * of the four cells of the filter's counters. Enqueues only. XIVO_HIP_ERR_INVALID, nothing changed: faults off; no frame of B
 * filters open; the open frame's tracks did not come from the producer; called twice in a frame; no update has left a mask. */
int xivo_hip_pcw_fault_score(xivo_hip_ctx* ctx, int B);
/* the counters of filters [b0, b0 + nb). Synchronises. */
int xivo_hip_pcw_fault_get_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_pcw_fault_stats* out);
/* flags [nb][tracks_max]: the flag byte of every track the last frame call left, parallel to xivo_hip_pcw_get_tracks' ids (0
 * behind a filter's count). XIVO_HIP_ERR_INVALID as xivo_hip_pcw_get_tracks, and with faults off. Synchronises. */
int xivo_hip_pcw_fault_get_flags(xivo_hip_ctx* ctx, int b0, int nb, unsigned char* flags);

/* ---- trajectory producer: the simulator's IMU records and ground-truth poses produced on the device (opt-in) --------------
 * What BatchTrajectorySim (xivo_amd/pcw.py) and ImuFeeder.imu (xivo_amd/sequence.py) compute on the host between two camera
 * frames: every filter follows a closed-form curve (Lissajous or trefoil, at its own rate) with one orientation profile for
 * all, its IMU reports accel = Rsb^T (a_s - grav_s) + noise and gyro = Jr wd + noise at t_k = k imu_dt, and the feeder turns
 * samples k - 1, k into the record of sample k (the value at k - 1, the slope to k, dt_k = t_k - t_{k-1}). With the worlds
 * resident too (xivo_hip_pcw_config) a camera frame of all filters needs no host data and no host wait:
 *   xivo_hip_trajsim_frame -> xivo_hip_propagate_resident -> xivo_hip_pcw_tracks_resident -> xivo_hip_life_begin_tracks ->
 *   update -> xivo_hip_absorb_error -> xivo_hip_life_end
 * (or xivo_hip_pool_life_begin_tracks / xivo_hip_pool_life_end: these calls ask only whether a frame of either life cycle is open).
 * Camera stamps coincide with IMU stamps and a frame covers a whole number of samples. The evaluation order and the noise
 * generator (Philox4x32-10 keyed by the seed, counter = pair, filter, sample) are specified in xivo_amd/csrc/trajsim_device.h;
 * a sample's noise depends on (seed, k, filter) only. The pixel noise of xivo_hip_pcw_tracks draws from the same generator:
 * given the same seed the two streams share words, so give them different seeds. Online-calibration contexts
 * (xivo_hip_set_calib with a motion side) are not supported: XIVO_HIP_ERR_UNSUPPORTED from config, frame and
 * propagate_resident. */
typedef struct {
  int struct_size;             /* sizeof(xivo_trajsim_opts) */
  int n_max;                   /* most samples one frame may cover; 0 releases everything */
  int T_max;                   /* frames of the ground-truth log */
  int reserved;
  double imu_dt;               /* > 0 */
  double rot_amp, rot_w[3];    /* orientation profile: rotation vector rot_amp sin(rot_w t), per component */
  double noise_accel, noise_gyro;   /* standard deviations (>= 0); 0: that sensor draws nothing */
  double grav_s[3];            /* gravity in the spatial frame */
  double Rbc[9], Tbc[3];       /* body-to-camera, Rbc ROW-major (only the camera pose reads them) */
  unsigned long long seed;     /* the IMU noise generator's key */
} xivo_trajsim_opts;
/* (Re-)allocates everything the frame calls use: records [batch_max][n_max], curve and rate per filter, the camera poses
 * [batch_max][12] (the module's own block, with or without worlds configured: xivo_hip_pcw_tracks_resident hands it to the
 * track producer), the ground-truth log [T_max][batch_max][12], the device copy of the propagation options and the propagate
 * staging at its final size. Every filter starts as a Lissajous curve of rate 0 (stationary). XIVO_HIP_ERR_INVALID, nothing
 * changed: wrong struct_size, n_max < 0, (n_max > 0:) T_max <= 0, imu_dt not > 0, a value that is not finite, a negative
 * noise, a frame open between life_begin and life_end, a size that overflows. Synchronises. */
int xivo_hip_trajsim_config(xivo_hip_ctx* ctx, const xivo_trajsim_opts* opts);
/* Curve (0 Lissajous, 1 trefoil) and rate of filters [b0, b0 + nb). A set-up call: synchronises. */
int xivo_hip_trajsim_set(xivo_hip_ctx* ctx, int b0, int nb, const int* motion, const double* rate);
/* One frame of filters [0, B): records k0 + 1 .. k0 + n, the poses at t_{k0 + n}, one more frame of the ground-truth log.
 * n = 0 (the frame at t = 0) writes poses only and leaves no records. Enqueues one kernel; allocates nothing and does not
 * synchronise. Refused with nothing changed: n < 0 or n > n_max, a sample index at which dt_k is not positive or t_k not finite
 * (xivo_hip_propagate_resident cannot read the records it is handed: their dt is vouched for here), B out
 * of range, a frame open between life_begin and life_end, not configured (XIVO_HIP_ERR_INVALID); the log holds T_max frames
 * (XIVO_HIP_ERR_FULL). */
int xivo_hip_trajsim_frame(xivo_hip_ctx* ctx, int B, unsigned long long k0, int n);
/* xivo_hip_propagate of filters [0, B) over the records the last xivo_hip_trajsim_frame(B, ., n > 0) left, which it consumes
 * (once). Same kernels, same arguments; does not synchronise: Qimu / Qmodel are cached on the device and uploaded again only
 * when opts differs from the context's copy (a synchronous copy, since opts is borrowed). control_stepsize works as in
 * xivo_hip_propagate. XIVO_HIP_ERR_INVALID, nothing changed: no fresh records for this B, and what xivo_hip_propagate refuses. */
int xivo_hip_propagate_resident(xivo_hip_ctx* ctx, int B, const xivo_prop_opts* opts);
/* xivo_hip_pcw_tracks without the upload: reads the camera poses the last xivo_hip_trajsim_frame(B) left (they stay, a second
 * call reads them again). XIVO_HIP_ERR_INVALID, nothing changed: no pose for this B, and what xivo_hip_pcw_tracks refuses. */
int xivo_hip_pcw_tracks_resident(xivo_hip_ctx* ctx, int B, double noise_px_std, unsigned long long seed, unsigned long long frame);
/* Read-back for tests and a host arm of what the last xivo_hip_trajsim_frame left for filters [b0, b0 + nb) (within its B):
 * recs [nb][n] (n: that frame's, also written to n_out; consumed records can still be read), gsc [nb][12]. Any may be NULL.
 * Synchronises. */
int xivo_hip_trajsim_get(xivo_hip_ctx* ctx, int b0, int nb, xivo_imu_in* recs, double* gsc, int* n_out);
/* The ground-truth log: frames [t0, t0 + nt) (all written) of filters [b0, b0 + nb), frame-major gt [nt][nb][12] (Rsb
 * column-major, then Tsb: what xivo_hip_traj_score and xivo_hip_traj_nees take). Synchronises. */
int xivo_hip_trajsim_get_gt(xivo_hip_ctx* ctx, int b0, int nb, int t0, int nt, double* gt);
int xivo_hip_trajsim_count(xivo_hip_ctx* ctx);   /* frames in the log; 0 when not configured */
int xivo_hip_trajsim_reset(xivo_hip_ctx* ctx);   /* empties the log (and forgets the last frame's records and poses) */

/* ---- loop closure on the device: the resident landmark map ------------------------------------------------------------
 * What Estimator::CloseLoop needs around the rows of xivo_hip_close_loop_stack: a per-filter map of world points that
 * outlives the features' stay in the state (DiscardFeatures -> Mapper::AddFeature, src/mapper.cpp:158-222), the matcher
 * against it and the verification before the update (Mapper::DetectLoopClosures, src/mapper.cpp:335-418), all resident.
 * What stands in for what: `key` is the caller's stand-in for the descriptor word - two observations with the same
 * non-negative key are the mapper's descriptor match at distance 0 (a point-cloud world supplies its world-point index, a
 * front end its own match id; a negative key matches nothing); a chi-square gate of every match on the filter's own
 * covariance stands in for pnp_ransac's inlier test. The stored point is treated as exact, as the reference treats it (xivo_hip_lcmap_cov_config gives it a covariance). No
 * merging (merge_features = false, mapper.cpp:189-191: the first estimate of a point is kept), no eviction, no pose graph.
 * Off until configured; refused on a context with online calibration. */
#define XIVO_LCMAP_MAX_ENTRIES 4096
#define XIVO_LCMAP_MAX_MATCHES 64
typedef struct {
  int struct_size;        /* sizeof(xivo_lcmap_opts) */
  int map_max;            /* entries per filter, <= XIVO_LCMAP_MAX_ENTRIES; 0 releases the map and zeroes the counters */
  int lc_max;             /* matches per filter and frame, <= XIVO_LCMAP_MAX_MATCHES; 2 lc_max rows are staged */
  int min_matches;        /* a filter closes with at least this many kept matches (>= 1; the reference's default is 5) */
  double Rlc;             /* variance of the loop-closure pixel (> 0) */
  double chi2;            /* gate of one match (2 degrees of freedom); 0: no gate (a gamma that is not finite is gated all the same) */
  double max_depth_var;   /* an added feature whose P(foff + 2, foff + 2) is above this is dropped; 0: no test */
} xivo_lcmap_opts;
typedef struct { long long key; double Xs[3]; } xivo_lcmap_entry;
typedef struct { int b, feat; long long key; } xivo_lcmap_add_rec;                     /* ordered by b */
typedef struct { int b, group_sind; long long key; double xp[2]; } xivo_lcmap_query;   /* ordered by b */
typedef struct {
  int entry;        /* position in the filter's map; -1: this list position is empty */
  int group_sind;   /* the query's */
  double xp[2];     /* the query's */
  double gamma;     /* r^T (H P H^T + Rlc I)^-1 r of the pair; -1 where a pivot was not positive or the value is not finite
                       (a NaN or inf pixel or stored point): such a match is not kept, whatever chi2 is */
  int kept, reserved;   /* reserved: 1 where the match rested (xivo_hip_lcmap_cov_config, revisit_gap), else 0 */
} xivo_lcmap_match;
typedef struct {
  long long added, dup, full, poor, skipped;   /* add records by outcome */
  long long queries, matched, surplus, gated;  /* queries seen; list positions filled; matches beyond lc_max; gated out */
  long long short_frames, closed_frames;       /* frames with a match and fewer than min_matches kept; frames that closed */
} xivo_lcmap_stats;
/* Refusals: XIVO_HIP_ERR_UNSUPPORTED for map_max > XIVO_LCMAP_MAX_ENTRIES, lc_max > XIVO_LCMAP_MAX_MATCHES or a context with
 * online calibration; XIVO_HIP_ERR_INVALID for 2 lc_max > M_max, lc_max < 1, Rlc <= 0, min_matches < 1, negative or non-finite
 * bounds, no layout. Every other entry point of this section returns XIVO_HIP_ERR_INVALID before a configuration. */
int xivo_hip_lcmap_config(xivo_hip_ctx* ctx, const xivo_lcmap_opts* opts);
/* The in-state features that leave (call it before the edit that removes them): n records of filters [0, B), ordered by b. One
 * workgroup per filter takes its records in order: feat not in the state (sind < 0, ref_sind out of range) or key < 0 -
 * skipped; depth variance above max_depth_var - poor; key stored already, by an earlier call or an earlier record - dup, the
 * stored entry stays; map full - full; else the entry {key, Xs = Feature::Xs(gbc)} goes to position count. Enqueues and
 * returns without waiting (the records are copied first). */
int xivo_hip_lcmap_add(xivo_hip_ctx* ctx, int B, int n, const xivo_lcmap_add_rec* recs);
/* DetectLoopClosures + CloseLoopInternal up to the update, for filters [0, B). Match: a query whose key is in its filter's map
 * matches that entry; the first lc_max matching queries in query order fill the match list, the rest are surplus. Rows: every
 * match gets the row pair of ComputeLCJacobian with the entry's Xs as the old feature's world point, observed by group
 * group_sind or (group_sind = -1) by the body pose itself, whose blocks go to columns 0..5. Verify: gamma of every pair from
 * the sub-block of P under its 12 columns; gamma > chi2, a non-positive pivot or a gamma that is not finite (with chi2 = 0
 * too: NaN is "no match" here as it is "not tracked" elsewhere) gates it out and counts in `gated`. A filter with fewer than
 * min_matches kept matches does not close: all its pairs are neutral (H = 0, inn = 0, diagR = 1); else only the gated and
 * empty ones are. The 2 lc_max rows of every filter replace the staged measurement as those of xivo_hip_close_loop_stack do;
 * xivo_hip_update_joseph + xivo_hip_absorb_error complete the closure. n_closing_out == NULL: always stages, never waits.
 * Else: waits, returns the number of closing filters, and stages nothing when that is 0 (the staged rows stay as they were). */
int xivo_hip_lcmap_close(xivo_hip_ctx* ctx, int B, int n, const xivo_lcmap_query* queries, int* n_closing_out);
/* whole maps of filters [b0, b0 + nb): entries host [nb][map_max], count host [nb] (set: 0 <= count <= map_max, the keys of a
 * filter non-negative and distinct) - a surveyed map, or one carried over from another run */
int xivo_hip_lcmap_set(xivo_hip_ctx* ctx, int b0, int nb, const xivo_lcmap_entry* entries, const int* count);
int xivo_hip_lcmap_get(xivo_hip_ctx* ctx, int b0, int nb, xivo_lcmap_entry* entries, int* count);
/* the match lists of the last close call: host [nb][lc_max]; kept and gamma are valid where entry >= 0 */
int xivo_hip_lcmap_get_matches(xivo_hip_ctx* ctx, int b0, int nb, xivo_lcmap_match* matches);
int xivo_hip_lcmap_get_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_lcmap_stats* stats);
/* Two options on top of a configured map, both off until this call and independent of each other (the structs above keep their
 * sizes: what the options need lives in arrays of its own, next to the entries).
 * point_cov = 1: every entry carries the covariance Sigma of its world point, packed (0,0),(0,1),(0,2),(1,1),(1,2),(2,2) like
 * xivo_map_pt's cov_world. xivo_hip_lcmap_add stores Sigma = J Pcc J^T of an accepted record (J = dXs / d error state over
 * the 15 columns Wbc, Tbc, the anchor group's six and the feature's three, Pcc gathered from the lower triangle of P and
 * mirrored: the arithmetic of the landmark log's cov_world); xivo_hip_lcmap_set zeroes it for the filters it loads. The close
 * call then weighs a match with R_e = Rlc I + H_T Sigma H_T^T, H_T the pair's block for Tsb (d xp / d Xs = -H_T): gamma is
 * r^T (H P H^T + R_e)^-1 r, a match whose R_e has a non-positive pivot is not kept (gamma = -1, counted in bad_cov and in
 * gated), and a pair that takes part is whitened - R_e = L L^T, rows and innovation <- L^-1 times themselves, diagR = 1 - so
 * that the update calls run as they are. No cross-covariance between a stored point and the state is kept.
 * revisit_gap > 0: an entry closes the loop once per visit. Every entry keeps {last_seen, used}; t numbers the close calls
 * since this call, from 1. used_now = (last_seen > 0 && t - last_seen <= revisit_gap) ? used : 0, and a match whose entry is
 * used_now rests: it takes its list position, gets its rows and its gate, a kept one counts towards min_matches (it verifies
 * the place), but its pair is neutral and xivo_lcmap_match.reserved is 1. A frame with min_matches kept matches all of which
 * rest does not close (rested_frames; closing = 0). After the decision every matched entry gets last_seen = t and
 * used = used_now || (the frame closed and the match was kept and did not rest); a key that fills two list positions in one
 * call is used if either position used it, both having seen the state from before the call.
 * Both zero: releases the arrays, every entry point behaves as before this call. Entries already in the map get Sigma = 0 and
 * "never seen". Zeroes the counters below and t. XIVO_HIP_ERR_INVALID: no configured map, a wrong struct_size, point_cov
 * outside {0, 1}, a negative gap. xivo_hip_lcmap_config (a new configuration or a release) drops these options too. */
typedef struct { int struct_size; int point_cov; int revisit_gap; int reserved; } xivo_lcmap_cov_opts;
typedef struct {
  long long resting;         /* kept matches that rested */
  long long rested_frames;   /* frames with min_matches kept matches, every one resting */
  long long bad_cov;         /* matches not kept because a pivot of R_e was not positive */
} xivo_lcmap_cov_stats;
int xivo_hip_lcmap_cov_config(xivo_hip_ctx* ctx, const xivo_lcmap_cov_opts* opts);
/* Sigma of filters [b0, b0 + nb): host [nb][map_max][6]. set refuses non-finite values and negative diagonal entries
 * (XIVO_HIP_ERR_INVALID, nothing changed) and stores everything else as given: whether R_e is definite is the close call's
 * pivot test. Both return XIVO_HIP_ERR_INVALID without point_cov, xivo_hip_lcmap_get_cov_stats while both options are off. */
int xivo_hip_lcmap_set_cov(xivo_hip_ctx* ctx, int b0, int nb, const double* cov);
int xivo_hip_lcmap_get_cov(xivo_hip_ctx* ctx, int b0, int nb, double* cov);
int xivo_hip_lcmap_get_cov_stats(xivo_hip_ctx* ctx, int b0, int nb, xivo_lcmap_cov_stats* stats);

/* ---- loop closure inside the device life cycle ("immediate" mode, xivo_hip_life_*): every track carries a key, the in-state
 * book keeps it per slot, and the add records and the queries of a frame are made where the book is - on the device. A frame:
 *   xivo_hip_life_begin_keys (or _begin, _begin_tracks) -> xivo_hip_lcmap_add_resident -> update -> xivo_hip_absorb_error ->
 *   xivo_hip_lcmap_close_resident -> [xivo_hip_update_joseph -> xivo_hip_absorb_error] -> xivo_hip_life_end
 * The rules - which slot yields a record, which a query, where either lies in its filter's list - are lcmap_life_device.h's;
 * what becomes of a record or a query is decided as xivo_hip_lcmap_add / _close decide it.
 * on = 1 needs xivo_hip_life_config and xivo_hip_lcmap_config, and allocates: a key per track next to the track block (long long
 * [batch_max][tracks_max], in the form the tracks are in) with two page-locked staging blocks of its own, feat_key per feature
 * slot next to the book's feat_id (-1: free slot), the per-filter lists of add records and of queries (one row of n_features
 * per filter with a count: no list position depends on another filter), what the begin call hands to the add call, and a copy of
 * the first update's status. on = 0 releases them; so does every call that releases the track block or the map
 * (xivo_hip_life_config, xivo_hip_pool_life_config, xivo_hip_pool_config, xivo_hip_lcmap_config). Off by default, and while
 * off every other entry point behaves as it did without this call. XIVO_HIP_ERR_INVALID, nothing changed: no life cycle or no map
 * configured, a frame open, on outside {0, 1}. XIVO_HIP_ERR_UNSUPPORTED: the context runs the pool life cycle
 * (xivo_hip_pool_life_config), whose pool book carries no keys. */
int xivo_hip_lcmap_life_config(xivo_hip_ctx* ctx, int on);
/* xivo_hip_life_begin plus keys [off[B]], parallel to ids (negative: the track matches nothing and adds nothing). Needs
 * xivo_hip_lcmap_life_config(1) (else XIVO_HIP_ERR_INVALID, nothing changed). With the option on, xivo_hip_life_begin gives every
 * track the key -1, and xivo_hip_life_begin_tracks takes the keys the track producer left: the world-point index of every track
 * (xivo_hip_pcw_tracks writes them while the option is on).
 * With the option on a begin call of any kind decides but does not edit: the features the tracker dropped leave the book and
 * become the frame's add records {b, slot, feat_key[slot]} in ascending slot order, the tracked ones take their pixel, and P and
 * the scene stay as they were until xivo_hip_lcmap_add_resident - the map reads the leaving features from the state as it was. */
int xivo_hip_life_begin_keys(xivo_hip_ctx* ctx, int B, int F, const int* off, const long long* ids, const double* meas, const long long* keys);
/* xivo_hip_lcmap_add on the records the begin call of the open frame of B filters left on the device, then the removals that
 * begin call decided (the edits xivo_hip_life_begin makes itself while the option is off). Once per frame, before the update.
 * No upload, no host loop; enqueues only. XIVO_HIP_ERR_INVALID: the option is off, no frame of B filters is open, or the frame's
 * records were consumed already. */
int xivo_hip_lcmap_add_resident(xivo_hip_ctx* ctx, int B);
/* xivo_hip_lcmap_close on queries made on the device, behind the frame's update and xivo_hip_absorb_error: one query {b, -1,
 * feat_key[slot], the pixel the begin call stored} per slot that holds a feature, was associated with a track by the begin call
 * and whose entry of the update's inlier mask is not zero, in ascending slot order. It also keeps the update's status of every
 * filter, which xivo_hip_life_end then counts in not_spd instead of the second update's. n_closing_out as xivo_hip_lcmap_close:
 * NULL - always stages, never waits; else waits, and stages nothing when no filter closes. Once per frame. XIVO_HIP_ERR_INVALID:
 * the option is off, no frame of B filters is open, the frame's add call has not run or the close call ran already. */
int xivo_hip_lcmap_close_resident(xivo_hip_ctx* ctx, int B, int* n_closing_out);
/* Read-back for tests: feat_key host [nb][F] (F of the last frame call; -1: free slot). ent_key must be NULL (the pool book
 * carries no keys). Synchronises. */
int xivo_hip_lcmap_life_get_keys(xivo_hip_ctx* ctx, int b0, int nb, long long* feat_key, long long* ent_key);
/* Read-back for tests of the keys the last xivo_hip_pcw_tracks left for filters [b0, b0 + nb), as xivo_hip_pcw_get_tracks reads
 * the ids: keys host [nb][tracks_max], -1 behind the filter's count. Synchronises. */
int xivo_hip_lcmap_life_get_track_keys(xivo_hip_ctx* ctx, int b0, int nb, long long* keys);

/* ---- tuning table: per-filter noise parameters (opt-in) -----------------------------------------------------------------
 * Every call above takes one R, one MH_thresh, one Qimu / Qmodel and one var_xyz for all the filters it touches. A configured
 * table gives every filter of the context its own: T tunings x W worlds = batch_max filters in one context, one run, one score
 * per tuning (xivo_amd/sweep.py). Off by default; without a table every call computes what it computes without this section.
 *
 * The table is device memory of the context, one array per field: R [batch_max], mh_thresh [batch_max], var_xyz [batch_max][3],
 * Qimu [batch_max][144], Qmodel [batch_max][529] (the two matrices as xivo_prop_opts holds them). While it is configured
 *   xivo_hip_mh_gate, xivo_hip_stack, xivo_hip_filter_update   use filter b's R (the in-state gate's R and the stacked rows'
 *       diagR) and mh_thresh; their scalar R / mh_thresh arguments are still validated and otherwise not read. mh_mult,
 *       min_inliers and use_gating stay the call's. A re-stacking of the dense rows (xivo_hip_get_H, the dense pipeline) reads
 *       the table again;
 *   xivo_hip_propagate, xivo_hip_propagate_resident             use filter b's Qimu / Qmodel - for a range [b0, b0 + nb) the
 *       entries of those filters -, not the matrices of xivo_prop_opts (resp. of the trajectory producer);
 *   xivo_hip_life_end                                           gives a new feature of filter b diag(var_xyz[b]).
 * The values enter the same expressions in the same order as the scalar arguments do: a table whose rows all equal the scalar
 * arguments leaves every result bit for bit what it is without a table. What carries an R of its own is untouched: Roos, Rlc,
 * the sub-filter's Rtri; the pool life cycle's std_xyz is not var_xyz and is not tuned.
 * Calls that take one parameter set and would have to apply it silently are refused while a table is configured
 * (XIVO_HIP_ERR_UNSUPPORTED, nothing changed): xivo_hip_one_point_ransac, xivo_hip_mh_gate_dense, xivo_hip_update_dense_gated,
 * xivo_hip_propagate_calib, and xivo_hip_set_calib with a layout. Not tuned: gravity, mh_mult / min_inliers, the RANSAC
 * thresholds, the sub-filter's options. */
typedef struct {
  double R;            /* visual_meas_std^2: the in-state gate's R and the stacked rows' diagR */
  double mh_thresh;    /* MH_thresh */
  double var_xyz[3];   /* a new feature's variances in xivo_hip_life_end */
  double Qimu[144];    /* as xivo_prop_opts */
  double Qmodel[529];
} xivo_tune_in;        /* 5424 bytes */
/* Configure the table with every filter of batch_max = *all (already configured: every row is overwritten), or release it
 * (all = NULL: the scalar arguments are back; synchronises). Allocates the five arrays and two page-locked staging blocks of
 * batch_max entries. XIVO_HIP_ERR_INVALID, nothing changed: an entry xivo_hip_tune_set refuses. XIVO_HIP_ERR_UNSUPPORTED: a
 * context with online calibration (xivo_hip_set_calib). */
int xivo_hip_tune_config(xivo_hip_ctx* ctx, const xivo_tune_in* all);
/* Rows [b0, b0 + nb) <- t [nb]. Stages through page-locked memory and only enqueues: t may be reused at once, the rows take
 * effect for the calls enqueued after this one. XIVO_HIP_ERR_INVALID, nothing changed - not one row of the call: no table, a
 * bad range, a non-finite value anywhere, R or mh_thresh not positive, a negative var_xyz. */
int xivo_hip_tune_set(xivo_hip_ctx* ctx, int b0, int nb, const xivo_tune_in* t);
/* Read-back of rows [b0, b0 + nb). Synchronises. */
int xivo_hip_tune_get(xivo_hip_ctx* ctx, int b0, int nb, xivo_tune_in* t);

/* ---- covariance propagation tail (src/rk4.cpp:92-102, src/estimator.cpp:590) */
/* P_mm <- Pmm_new ; P_ms <- Phi P_ms ; P_sm <- P_sm Phi^T. Phi and Pmm_new
 * are nm x nm (nm = kMotionSize: 23, or up to 40 for the online-calibration builds), one pair per filter. */
int xivo_hip_propagate_cov(xivo_hip_ctx* ctx, int b0, int nb, int nm, const double* Phi,
                           const double* Pmm_new);

/* ---- measurement helpers (bench.py / tests only) ----------------------- */
/* device buffers on the context's GPU for inputs that are "already resident" (what xivo_hip_set_measurements_device is
 * handed): allocate, upload `bytes` from the host and replicate that block until `total_bytes` are filled, free. */
int xivo_hip_dev_alloc(xivo_hip_ctx* ctx, size_t bytes, void** out);
int xivo_hip_dev_free(xivo_hip_ctx* ctx, void* p);
int xivo_hip_dev_upload(xivo_hip_ctx* ctx, void* dst, const void* src, size_t bytes, size_t total_bytes);
int xivo_hip_timer_begin(xivo_hip_ctx* ctx);
int xivo_hip_timer_end(xivo_hip_ctx* ctx, float* ms_out);
/* per-stage accumulated GPU time (ms) and launch counts since the last reset;
 * needs XIVO_HIP_FLAG_PROFILE. names_out[i] points to static strings. */
#define XIVO_HIP_MAX_STAGES 16
int xivo_hip_profile_reset(xivo_hip_ctx* ctx);
int xivo_hip_profile_get(xivo_hip_ctx* ctx, int* n_stages, const char** names_out,
                         float* ms_out, int* launches_out, double* flops_per_launch_out);
/* fp64 MFMA issue-rate microbenchmark of v_mfma_f64_16x16x4_f64; out4 = {TFLOP/s full chip,
 * cycles per MFMA (1 wave/SIMD), sustained clock GHz (lower bound), TFLOP/s 1 wave/SIMD} */
int xivo_hip_bench_mfma_peak(xivo_hip_ctx* ctx, double* out4);
/* tile the batched GEMM picks for an (rows x cols) output (symmetric = lower
 * triangle + mirror mode), for DESIGN.md/tests */
void xivo_hip_gemm_tile(int rows, int cols, int symmetric, int* bm, int* bn);
/* which rows the last update call used: 0 = dense, 1 = row-pair compressed (sparse-H) */
int xivo_hip_last_path(xivo_hip_ctx* ctx);
/* the route the last update pass took (round 6: the one table in capi_update.hip, plan_update): 0 fused (one kernel), 1 sparse rows +
 * in-solve whitened update, 2 sparse rows + whitened outputs + tiled product, 3 sparse symmetric form, 4 sparse stand-alone tail,
 * 5 dense as-coded, 6 dense rows + whitened update, 7 dense symmetric form; xivo_hip_route_name gives the table's name */
int xivo_hip_last_route(xivo_hip_ctx* ctx);
const char* xivo_hip_route_name(int route);
/* kernel instantiation the last launch of profile stage `stage` ran (index as in xivo_hip_profile_get; needs
 * XIVO_HIP_FLAG_PROFILE), spelled as rocprofv3 --kernel-trace prints it minus spaces, template arguments included; "" if none.
 * A kernel whose workgroup size depends on the shape has it appended after an '@' (gate_sparse_kernel@1024). */
const char* xivo_hip_stage_kernel(xivo_hip_ctx* ctx, int stage);
/* algorithmic HBM bytes of that launch: every input and every output of the stage once */
double xivo_hip_stage_bytes(xivo_hip_ctx* ctx, int stage);

#ifdef __cplusplus
}
#endif
#endif /* XIVO_HIP_H_ */
