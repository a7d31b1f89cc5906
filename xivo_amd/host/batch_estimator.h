// xivo::hip::BatchEstimator - the per-message surface of the reference's Estimator (InertialMeas /
// VisualMeasPointCloud, src/estimator.h:89-142) for B independent filters that live on one GPU context.
//
// The reference is one singleton filter per process driven message by message; a GPU wants thousands of filters per
// launch. This class keeps the reference's message semantics per filter - IMU bookkeeping of Estimator::Propagate
// (src/estimator.cpp:548-575), IMU before camera at equal stamps, per camera frame the order of Estimator::UpdateStep
// (src/manager.cpp:30-110): tracker-dropped features out, filter update, MH-rejected features out, new features in -
// and turns one camera frame of all filters into five C-ABI calls on the resident state:
//   xivo_hip_propagate, xivo_hip_edit_batch, xivo_hip_set_pixels, xivo_hip_filter_update (+ get_gate, absorb_error),
//   xivo_hip_edit_batch.
// The life cycle is the simplified one of xivo_amd/sequence.py (which it reproduces decision for decision: the tests
// run both on the same input): features enter with the depth that comes with the track (`InitWithSimDepths`,
// src/manager.cpp:588) anchored to a group created from the current pose; no gauge features, no reference-group
// switching, no sub-filter warm-up. The host side holds only the slot book-keeping (gsel_ / fsel_,
// src/estimator.h:496-503); every number of the filter stays on the device.
// EnableSubfilter switches to the reference's sub-filter life cycle of a new track instead (initial_z, depth sub-filter
// in the device-resident feature pool xivo_hip_pool_*, admission by Criteria::Candidate), decision for decision the
// "subfilter" mode of xivo_amd/sequence.py.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <unordered_map>
#include <vector>

#include "../../include/xivo_hip.h"

namespace xivo {
namespace hip {

struct BatchConfig {
  int n_groups = 15, n_features = 30;              // kMaxGroup, kMaxFeature (src/core.h:95-105)
  xivo_cam cam{};                                   // the immediate life cycle needs a pinhole (it un-projects a new feature on the host)
  double visual_meas_std = 1.0;
  double MH_thresh = 5.991, MH_adjust_factor = 1.1;
  int min_inliers = 5;
  int use_MH_gating = 1;                            // cfg use_MH_gating (src/estimator.cpp:364)
  int use_1pt_RANSAC = 0;                           // cfg use_1pt_RANSAC: OnePointRANSAC between gating and the update
  double ransac_thresh = 5.0, ransac_Chi2 = 5.89;   // 1pt_RANSAC_thresh / 1pt_RANSAC_Chi2 (src/estimator.cpp:132-134)
  double initial_std_x = 1.0, initial_std_y = 1.0, initial_std_z = 0.1;   // pixels, pixels, log-depth (estimator.cpp:349-353)
  double min_depth = 0.05, max_depth = 10.0;
  int min_new_features = 3;                         // open a new group only when this many feature slots are free
  int fix_group_block = 1;                          // XIVO_HIP_FLAG_FIX_GROUP_BLOCK (see xivo_amd/sequence.py)
  int extra_rows = 0;                               // measurement rows the context holds beyond the 2 F in-state ones (EnableOosUpdates: its block + padding)
  int use_invdepth = 0;                             // the reference's USE_INVDEPTH build: features are (X/Z, Y/Z, 1/Z); initial_std_z is then an inverse-depth std
  xivo_prop_opts prop{};                            // Qimu, Qmodel, gravity, integrator, step size
  int N() const { return 23 + 6 * n_groups + 3 * n_features; }
};

class BatchEstimator {
 public:
  // poses0: initial nominal state of every filter; P0: one N x N column-major covariance shared by all
  BatchEstimator(const BatchConfig& cfg, int B, int device, const xivo_pose_in* poses0, const double* P0);
  ~BatchEstimator();
  BatchEstimator(const BatchEstimator&) = delete;
  BatchEstimator& operator=(const BatchEstimator&) = delete;

  // Estimator::InertialMeas for all filters at time t [s]: gyro, accel are [B][3]. The first call only initialises
  // last_gyro_ / last_accel_ (nothing to integrate from yet).
  void InertialMeas(double t, const double* gyro, const double* accel);
  // Estimator::VisualMeasPointCloud for all filters at time t: filter b's tracks are ids[off[b] .. off[b + 1]) with rows
  // (x, y, depth) in xp_and_depths. Runs the whole frame on the device. mask_out (may be null): [B][n_features] inliers.
  void VisualMeasPointCloud(double t, const int* off, const int64_t* ids, const double* xp_and_depths,
                            unsigned char* mask_out);

  void Poses(xivo_pose_in* out);                    // gsb / Vsb / bg / ba ... of every filter (reads the resident state)
  int B() const { return B_; }
  const BatchConfig& cfg() const { return cfg_; }
  xivo_hip_ctx* ctx() { return ctx_; }
  long n_updates() const { return n_updates_ + DeviceCount(0); }
  long n_not_spd() const { return n_not_spd_ + DeviceCount(5); }   // updates skipped because S was not positive definite
  long n_rejected() const { return n_rejected_ + DeviceCount(1); }
  double host_seconds() const { return host_s_; }   // time spent in the host-side life cycle (not in C-ABI calls)

  // the reference's life cycle of a new track on the device-resident feature pool (xivo_hip_pool_*), as
  // xivo_amd/sequence.py runs it with feature_init = "subfilter": new tracks start from initial_z, take the depth sub-filter
  // while out of the state and enter by Criteria::Candidate / CandidateStrict, best first
  struct SubfilterConfig {
    double initial_z = 2.5, remove_outlier_counter = 10.0;   // cfg initial_z, remove_outlier_counter
    int strict_criteria_timesteps = 5, max_group_lifetime = 1;
    xivo_subfilter_opts opts{12.25, 5.991, 5, 0.05, 10.0, 0.01};   // cfg "subfilter" (Rtri = visual_meas_std^2), depths, max_subfilter_outlier
    int pool_max = 200, anchor_max = 64;                     // entries / anchors per filter
  };
  void EnableSubfilter(const SubfilterConfig& sc);   // before the first camera frame
  // the depth initialisation of new tracks in that life cycle (both opt-in), as SequenceConfig.triangulate_pre_subfilter /
  // adaptive_initial_depth: pre-sub-filter triangulation (src/manager.cpp:227-231; new tracks then take the badtri stds,
  // :585-586) and AdaptInitialDepth after the new tracks are added (:131, :255-278)
  struct DepthInitConfig {
    bool triangulate = false;
    xivo_triangulate_opts tri{(int)sizeof(xivo_triangulate_opts), XIVO_TRI_L1, 0.05, 5.0, 0.1 * M_PI / 180, 0.25 * M_PI / 180};
    double std_badtri[3] = {1.0, 1.0, 0.1};          // initial_std_{x,y}_badtri in pixels, initial_std_z_badtri
    bool adaptive = false;
    xivo_adapt_depth_opts adapt{(int)sizeof(xivo_adapt_depth_opts), 5, 2.5, 0.99, 0.05, 10.0};
  };
  void EnableDepthInit(const DepthInitConfig& dc);   // after EnableSubfilter, before the first camera frame
  const std::vector<double>& init_z() const { return init_z_; }   // AdaptInitialDepth's init_z after the last frame
  long n_admitted() const { return n_admitted_ + (device_pool_life_ ? DeviceCount(3) : 0); }
  // the innovation log of the estimator's context (xivo_hip_innov_*): T_max frames, one record per camera frame between the
  // update and AbsorbError, stamped with the frame's time in ns; T_max = 0 releases the log and stops recording. The caller
  // reads it through ctx() (xivo_hip_innov_read / _stats).
  void EnableInnovationLog(int T_max);
  long n_pool_dropped() const { return n_pool_dropped_ + (device_pool_life_ ? DeviceCount(7) : 0); }   // new tracks that found no free pool entry or anchor
  // the sub-filter life cycle's decisions on the device (xivo_hip_pool_life_*): after EnableSubfilter (and EnableDepthInit, whose
  // stds and adaptive depth it takes), before the first camera frame. Both books move to the context; VisualMeasPointCloud
  // hands the frame's tracks down (at most tracks_max per filter) and makes no get_gate / get_status call unless mask_out is
  // given; book(b) and the counters then read the device, init_z() stays as configured (xivo_hip_pool_get_init_z reads the
  // resident one). Throws if EnableSubfilter has not run or the immediate device life cycle is on.
  void EnableDevicePoolLifecycle(int tracks_max);
  // MSCKF update from pool entries whose track ends (xivo_hip_pool_oos_config, a thin pass-through): after
  // EnableDevicePoolLifecycle and before the first frame, on an estimator created with BatchConfig::extra_rows >= the block's
  // oos_max * (2 max_obs - 3) rows rounded up with its 16 rows of padding. The frame's update then appends and gates the block
  // (xivo_hip_pool_oos_project / _gate); the selection and the history are the device life cycle's. Not with EnableInnovationLog.
  void EnableOosUpdates(const xivo_pool_oos_opts& opts);
  bool device_pool_lifecycle() const { return device_pool_life_; }
  // the "immediate" life cycle on the device (xivo_hip_life_*): the slot book moves to the context, VisualMeasPointCloud hands
  // the frame's tracks down (at most tracks_max per filter) and makes no get_gate / get_status call unless mask_out is given;
  // book(b), n_updates(), n_rejected() and n_not_spd() then read the device. The book kept so far is adopted
  // (xivo_hip_life_set_book). tracks_max = 0 switches back: books and counters are read home, the device book is released.
  // Not with EnableSubfilter, in either order (both throw).
  void EnableDeviceLifecycle(int tracks_max);
  bool device_lifecycle() const { return device_life_; }
  // the point-cloud world's tracks from the device (xivo_hip_pcw_*; after EnableDeviceLifecycle or EnableDevicePoolLifecycle,
  // both calls throw with neither):
  // EnableDeviceWorld places one world of npts points per filter (Xs [B][npts][3]; nothing tracked yet, ids from 10000) seen by
  // the pinhole camera in cam (fx .. imh; struct_size and npts are filled in here) - or, when the estimator's own camera is not
  // a pinhole, by that camera (xivo_hip_pcw_camera; a point beyond the normalised radius max_radius is then not visible: the
  // guard against a polynomial distortion's fold-back). npts <= tracks_max; npts = 0 releases the
  // worlds, and so does every EnableDeviceLifecycle call. VisualMeasDeviceWorld is then the camera frame: gsc [B][12] are the
  // ground-truth camera poses (Rsc row-major, Tsc), the tracks are produced on the device (pixel noise of standard deviation
  // noise_px_std from the counter-based generator keyed by seed; the frame counter starts at 0 with EnableDeviceWorld) and the
  // life cycle runs on them as in VisualMeasPointCloud (the pool life cycle counts the frame and computes CandidateStrict
  // there too). Frames of either kind may alternate.
  void EnableDeviceWorld(int npts, const xivo_pcw_opts& cam, const double* Xs, double max_radius = std::numeric_limits<double>::infinity());
  void VisualMeasDeviceWorld(double t, const double* gsc, double noise_px_std, unsigned long long seed, unsigned char* mask_out);
  bool device_world() const { return device_world_; }
  // track faults of the device producer (xivo_hip_pcw_fault_config): set before EnableDeviceWorld, which turns them on with the
  // worlds; VisualMeasDeviceWorld / FrameResident then score every update's gate decisions against the tracks' flags
  // (xivo_hip_pcw_fault_score; the counters: xivo_hip_pcw_fault_get_stats on ctx()). ClearTrackFaults: off from the next
  // EnableDeviceWorld on
  void SetTrackFaults(const xivo_pcw_fault_opts& opts) { faults_ = opts; faults_.struct_size = (int)sizeof(faults_); have_faults_ = true; }
  void ClearTrackFaults() { have_faults_ = false; }
  // the simulated IMU and the ground-truth poses from the device too (xivo_hip_trajsim_*; after EnableDeviceWorld, both calls
  // throw without it): EnableDeviceImu configures the trajectory producer (opts as xivo_hip_trajsim_config takes them;
  // struct_size is filled in here) with curve motion[b] (0 Lissajous, 1 trefoil) and rate[b] per filter; n_max = 0 releases it.
  // FrameResident is then a whole camera frame at sample k0 + n without host data or a host wait: trajsim frame -> resident
  // propagate (n > 0) -> resident tracks -> (pool_)life_begin_tracks -> update -> (pool_)life_end. It takes the place of the InertialMeas
  // calls of samples k0 + 1 .. k0 + n and the VisualMeasDeviceWorld call at t_{k0 + n}; the two kinds of frames do not mix in
  // one run (the host feeder does not see the device's samples).
  void EnableDeviceImu(const xivo_trajsim_opts& opts, const int* motion, const double* rate);
  void FrameResident(unsigned long long k0, int n, double noise_px_std, unsigned long long seed, unsigned char* mask_out);
  bool device_imu() const { return device_imu_; }

  struct Book {                                     // one filter's slots
    std::vector<int> group_refs;                    // -1 free, else number of in-state features anchored there
    std::vector<int64_t> feat_id;                   // -1 free
    std::vector<int> feat_ref;
    std::unordered_map<int64_t, int> id2slot;
  };
  const Book& book(int b) { if (device_life_ || device_pool_life_) ReadBook(b); return books_[b]; }

 private:
  void Check(int rc, const char* what);
  void DropFeature(Book& bk, int j);
  void DiscardEmptyGroups(int b, std::vector<xivo_edit_op>& ops);
  void RunUpdate();
  void FrameOnProducedTracks(unsigned char* mask_out);   // (pool_)life_begin_tracks -> update -> (pool_)life_end (-> mask)
  void NewTrackStd(bool badtri, double sd[3]) const;
  void PropagateToFrame(double t, double& t0);
  void VisualSubfilter(const int* off, const int64_t* ids, const double* meas);
  void ReadBook(int b);                 // device life cycle: books_[b] <- xivo_hip_life_get_book
  long LifeCount(int which) const;      // device life cycle: one of xivo_life_stats' counters summed over the filters
  long PoolLifeCount(int which) const;  // device pool life cycle: counter `which` of xivo_pool_life_stats summed over the filters
  long DeviceCount(int which) const { return device_life_ ? LifeCount(which) : (device_pool_life_ ? PoolLifeCount(which) : 0); }
  bool device_life_ = false, want_mask_ = false, device_world_ = false, device_pool_life_ = false;
  unsigned long long world_frame_ = 0;
  xivo_pcw_fault_opts faults_{}; bool have_faults_ = false, faults_on_ = false;
  bool device_imu_ = false; double device_imu_dt_ = 0.0;

  struct PoolBook {                                 // one filter's feature pool: tracks per entry, anchors and their links
    std::vector<int64_t> ent_id;                    // -1 free
    std::vector<int> ent_anchor, ent_born;
    std::unordered_map<int64_t, int> id2ent;
    std::vector<char> anc_used;
    std::vector<int> anc_life, anc_link;            // Group::lifetime; group slot of the anchor's group (-1: not in the state)
    void FreeEntry(int e) { id2ent.erase(ent_id[e]); ent_id[e] = -1; ent_anchor[e] = -1; }
  };
  bool subfilter_ = false;
  SubfilterConfig sc_;
  DepthInitConfig dc_;
  std::vector<double> init_z_;
  std::vector<PoolBook> pools_;
  int vision_counter_ = 0;
  long n_admitted_ = 0, n_pool_dropped_ = 0;

  BatchConfig cfg_;
  int B_;
  xivo_hip_ctx* ctx_ = nullptr;
  std::vector<Book> books_;
  // Estimator::Propagate's bookkeeping per filter
  bool have_imu_ = false;
  double t_ = 0.0;
  std::vector<double> last_gyro_, last_accel_, slope_gyro_, slope_accel_;   // [B][3]
  std::vector<std::vector<xivo_imu_in>> pending_;   // [message][B]
  long n_updates_ = 0, n_rejected_ = 0, n_not_spd_ = 0;
  std::vector<int> status_;
  bool innov_log_ = false;
  bool oos_ = false;
  double t_visual_ = 0.0;                 // stamp of the camera frame being processed
  double host_s_ = 0.0;
  std::vector<unsigned char> mask_;
  std::vector<double> xp_;
  std::vector<unsigned char> in_state_;   // per track of the current frame: is it an in-state feature
  std::vector<std::vector<xivo_edit_op>> per_;   // per filter: the edit ops of the current phase
  std::vector<int> slot_track_all_;       // [B][F] track index of each in-state feature in the current frame
};

}  // namespace hip
}  // namespace xivo
