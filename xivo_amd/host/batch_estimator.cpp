// See batch_estimator.h. Decision for decision the frame loop of xivo_amd/sequence.py (SequenceRunner.frame, ImuFeeder).
#include "batch_estimator.h"
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <cstdlib>
#include <numeric>
#include <stdexcept>
#include <string>

namespace xivo {
namespace hip {

namespace {
// a microsecond of book-keeping per filter: a handful of threads is all the loop can use (256 made it 8x slower) - and
// with one process per GPU never more than this rank's share of the host cores: the launcher (xivo_amd/shard.py:bind_rank)
// sets OMP_NUM_THREADS = min(8, cores / ranks)
static int team_size() {
  static const int n = [] {
    const char* e = std::getenv("OMP_NUM_THREADS");
    const int v = e ? std::atoi(e) : 8;
    return v < 1 ? 1 : (v > 8 ? 8 : v);
  }();
  return n;
}
#define kThreads team_size()
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
xivo_edit_op make_op(int b, int kind, int i0 = 0, int i1 = 0, int i2 = 0) {
  xivo_edit_op o;
  std::memset(&o, 0, sizeof(o));
  o.b = b; o.kind = kind; o.i0 = i0; o.i1 = i1; o.i2 = i2;
  return o;
}
}  // namespace

void BatchEstimator::Check(int rc, const char* what) {
  // the reference LOG(FATAL)s / throws on these conditions (src/estimator.cpp:121,587,821,844)
  if (rc != XIVO_HIP_OK) throw std::runtime_error(std::string(what) + ": " + xivo_hip_strerror(rc));
}

BatchEstimator::BatchEstimator(const BatchConfig& cfg, int B, int device, const xivo_pose_in* poses0, const double* P0)
    : cfg_(cfg), B_(B) {
  const int N = cfg.N(), F = cfg.n_features;
  Check(xivo_hip_create(&ctx_, device, N, 2 * F + (cfg.extra_rows > 0 ? cfg.extra_rows : 0), B, (cfg.fix_group_block ? XIVO_HIP_FLAG_FIX_GROUP_BLOCK : 0u) |
                                                     (cfg.use_invdepth ? XIVO_HIP_FLAG_INVDEPTH : 0u)), "create");
  xivo_layout lay{N, 23, cfg.n_groups, 23 + 6 * cfg.n_groups, F};
  Check(xivo_hip_set_layout(ctx_, &lay, &cfg.cam), "set_layout");
  for (int b = 0; b < B; ++b) Check(xivo_hip_upload_P(ctx_, b, 1, P0, (long)N * N, N), "upload_P");
  std::vector<xivo_group_in> groups((size_t)B * cfg.n_groups);
  for (auto& g : groups) { std::memset(&g, 0, sizeof(g)); g.Rsb[0] = g.Rsb[4] = g.Rsb[8] = 1.0; }
  std::vector<xivo_feat_in> feats((size_t)B * F);
  for (auto& f : feats) { std::memset(&f, 0, sizeof(f)); f.sind = -1; }
  Check(xivo_hip_set_scene(ctx_, 0, B, F, poses0, groups.data(), feats.data()), "set_scene");
  books_.resize(B);
  for (auto& bk : books_) {
    bk.group_refs.assign(cfg.n_groups, -1);
    bk.feat_id.assign(F, -1);
    bk.feat_ref.assign(F, -1);
  }
  last_gyro_.assign((size_t)B * 3, 0.0); last_accel_ = last_gyro_; slope_gyro_ = last_gyro_; slope_accel_ = last_gyro_;
  mask_.assign((size_t)B * F, 0);
  xp_.assign((size_t)B * F * 2, 0.0);
  slot_track_all_.assign((size_t)B * F, -1);
}

BatchEstimator::~BatchEstimator() {
  if (ctx_) xivo_hip_destroy(ctx_);
}

// Estimator::Propagate, visual_meas == false (src/estimator.cpp:558-567)
void BatchEstimator::InertialMeas(double t, const double* gyro, const double* accel) {
  const double t0 = now_s();
  if (!have_imu_) {
    std::copy(gyro, gyro + (size_t)B_ * 3, last_gyro_.begin());
    std::copy(accel, accel + (size_t)B_ * 3, last_accel_.begin());
    have_imu_ = true; t_ = t;
    host_s_ += now_s() - t0;
    return;
  }
  const double dt = t - t_;
  if (!(dt > 0.0)) {
    // Estimator::Propagate returns on dt == 0 with last_ / slope_ untouched (src/estimator.cpp:550-555); a message from
    // the past is skipped the same way
    if (dt < 0.0) fprintf(stderr, "xivo::hip::BatchEstimator: IMU message older than the filter time skipped\n");
    host_s_ += now_s() - t0;
    return;
  }
  std::vector<xivo_imu_in> rec(B_);
  for (int b = 0; b < B_; ++b) {
    xivo_imu_in& r = rec[b];
    for (int i = 0; i < 3; ++i) {
      const size_t k = (size_t)b * 3 + i;
      slope_gyro_[k] = (gyro[k] - last_gyro_[k]) / dt;
      slope_accel_[k] = (accel[k] - last_accel_[k]) / dt;
      r.gyro[i] = last_gyro_[k]; r.accel[i] = last_accel_[k];
      r.slope_gyro[i] = slope_gyro_[k]; r.slope_accel[i] = slope_accel_[k];
      last_gyro_[k] = gyro[k]; last_accel_[k] = accel[k];
    }
    r.dt = dt;
  }
  pending_.push_back(std::move(rec));
  t_ = t;
  host_s_ += now_s() - t0;
}

void BatchEstimator::DropFeature(Book& bk, int j) {
  bk.id2slot.erase(bk.feat_id[j]);
  bk.group_refs[bk.feat_ref[j]] -= 1;
  bk.feat_id[j] = -1; bk.feat_ref[j] = -1;
}

// Estimator::DiscardAffectedGroups, simplified: a group leaves the state with its last feature
void BatchEstimator::DiscardEmptyGroups(int b, std::vector<xivo_edit_op>& ops) {
  Book& bk = books_[b];
  for (int g = 0; g < cfg_.n_groups; ++g)
    if (bk.group_refs[g] == 0) {
      ops.push_back(make_op(b, XIVO_EDIT_REMOVE_GROUP, g));
      bk.group_refs[g] = -1;
      if (subfilter_)   // the device freezes the anchor of the group at its last pose
        for (int& link : pools_[b].anc_link) if (link == g) link = -1;
    }
}

// FilterUpdate on the tracked in-state features of every filter, the inlier mask into mask_, then AbsorbError
void BatchEstimator::RunUpdate() {
  const int F = cfg_.n_features;
  const double R = cfg_.visual_meas_std * cfg_.visual_meas_std;
  if (oos_) {
    // jacobians -> MH gate -> [RANSAC] -> stack -> the OOS block of the frame's list -> its chi-square gate -> update
    Check(xivo_hip_jacobians_instate(ctx_, B_), "jacobians_instate");
    Check(xivo_hip_mh_gate(ctx_, B_, R, cfg_.MH_thresh, cfg_.MH_adjust_factor, cfg_.use_MH_gating ? cfg_.min_inliers : (1 << 30), nullptr, nullptr), "mh_gate");
    if (cfg_.use_1pt_RANSAC)
      Check(xivo_hip_one_point_ransac(ctx_, B_, R, cfg_.ransac_thresh, cfg_.ransac_Chi2, nullptr, nullptr, nullptr, nullptr, nullptr), "one_point_ransac");
    Check(xivo_hip_stack(ctx_, B_, R), "stack");
    Check(xivo_hip_pool_oos_project(ctx_, B_), "pool_oos_project");
    Check(xivo_hip_pool_oos_gate(ctx_, B_), "pool_oos_gate");
    Check(xivo_hip_update_joseph(ctx_, B_), "update_joseph");
  } else if (cfg_.use_1pt_RANSAC) {
    // Estimator::OutlierRejection with use_1pt_RANSAC (src/manager.cpp:629-650): MH gating, OnePointRANSAC on its inliers,
    // the update on what it keeps. (No gauge group / previous-frame group list in this simplified life cycle.)
    Check(xivo_hip_jacobians_instate(ctx_, B_), "jacobians_instate");
    Check(xivo_hip_mh_gate(ctx_, B_, R, cfg_.MH_thresh, cfg_.MH_adjust_factor, cfg_.use_MH_gating ? cfg_.min_inliers : (1 << 30), nullptr, nullptr), "mh_gate");
    Check(xivo_hip_one_point_ransac(ctx_, B_, R, cfg_.ransac_thresh, cfg_.ransac_Chi2, nullptr, nullptr, nullptr, nullptr, nullptr), "one_point_ransac");
    Check(xivo_hip_stack(ctx_, B_, R), "stack");
    Check(xivo_hip_update_joseph(ctx_, B_), "update_joseph");
  } else {
    Check(xivo_hip_filter_update(ctx_, B_, R, cfg_.MH_thresh, cfg_.MH_adjust_factor, cfg_.min_inliers, cfg_.use_MH_gating), "filter_update");
  }
  const bool on_device = device_life_ || device_pool_life_;   // the life cycle reads the mask and the status where they are
  if (!on_device || want_mask_) Check(xivo_hip_get_gate(ctx_, B_, F, mask_.data(), nullptr), "get_gate");
  // a filter whose S was not positive definite keeps its prior P and absorbs nothing (the device skips both); it is
  // counted and reported here - the reference's pivoted LDL^T cannot fail, so there is no reference behaviour to mirror
  // (device life cycles: xivo_hip_life_end / xivo_hip_pool_life_end count it, nothing is downloaded)
  if (!on_device) {
    status_.resize(B_);
    const int st = xivo_hip_get_status(ctx_, 0, B_, status_.data());
    if (st == XIVO_HIP_ERR_NOT_SPD) { for (int b = 0; b < B_; ++b) n_not_spd_ += status_[b] != 0; }
    else Check(st, "get_status");
  }
  // the update's innovation statistics need the dx AbsorbError is about to consume (Estimator::UpdateStep: between
  // UpdateJosephForm and AbsorbError)
  if (innov_log_) Check(xivo_hip_innov_record(ctx_, B_, (long long)std::llround(t_visual_ * 1e9), nullptr), "innov_record");
  Check(xivo_hip_absorb_error(ctx_, B_), "absorb_error");
}

void BatchEstimator::EnableOosUpdates(const xivo_pool_oos_opts& opts) {
  if (!device_pool_life_) throw std::runtime_error("EnableOosUpdates needs EnableDevicePoolLifecycle first (the history rings are the device life cycle's)");
  if (vision_counter_ > 0 || innov_log_) throw std::runtime_error("EnableOosUpdates comes before the first frame and excludes the innovation log");
  Check(xivo_hip_pool_oos_config(ctx_, &opts), "pool_oos_config");
  oos_ = opts.oos_max > 0;
}

void BatchEstimator::EnableInnovationLog(int T_max) {
  if (oos_ && T_max > 0) throw std::runtime_error("the innovation log excludes EnableOosUpdates (its dof would count the block's empty rows)");
  const xivo_innov_opts o{T_max};
  Check(xivo_hip_innov_config(ctx_, &o), "innov_config");
  innov_log_ = T_max > 0;
}

// the camera frame's share of Estimator::Propagate and the pending IMU records in one xivo_hip_propagate call; t0: where the
// caller's host-time interval started (moved past the call)
void BatchEstimator::PropagateToFrame(double t, double& t0) {
  t_visual_ = t;
  // Estimator::Propagate, visual_meas == true (src/estimator.cpp:568-575): extrapolate along the last slope; dt == 0
  // (IMU and camera stamps coincide, the simulation case) propagates nothing (:550-555)
  if (have_imu_ && t != t_) {
    const double dt = t - t_;
    std::vector<xivo_imu_in> rec(B_);
    for (int b = 0; b < B_; ++b) {
      xivo_imu_in& r = rec[b];
      for (int i = 0; i < 3; ++i) {
        const size_t k = (size_t)b * 3 + i;
        r.gyro[i] = last_gyro_[k]; r.accel[i] = last_accel_[k];
        r.slope_gyro[i] = slope_gyro_[k]; r.slope_accel[i] = slope_accel_[k];
        last_gyro_[k] = last_gyro_[k] + slope_gyro_[k] * dt;
        last_accel_[k] = last_accel_[k] + slope_accel_[k] * dt;
      }
      r.dt = dt;
    }
    pending_.push_back(std::move(rec));
    t_ = t;
  }
  if (!pending_.empty()) {
    const int K = (int)pending_.size();
    std::vector<xivo_imu_in> imu((size_t)B_ * K);
    for (int k = 0; k < K; ++k)
      for (int b = 0; b < B_; ++b) imu[(size_t)b * K + k] = pending_[k][b];
    pending_.clear();
    host_s_ += now_s() - t0;
    Check(xivo_hip_propagate(ctx_, 0, B_, K, imu.data(), &cfg_.prop), "propagate");
    t0 = now_s();
  }
}

void BatchEstimator::VisualMeasPointCloud(double t, const int* off, const int64_t* ids, const double* meas,
                                          unsigned char* mask_out) {
  double t0 = now_s();
  const int F = cfg_.n_features;
  PropagateToFrame(t, t0);
  if (device_pool_life_) {
    // the sub-filter life cycle on the device: the tracks go down as they came in, nothing comes back
    host_s_ += now_s() - t0;
    want_mask_ = mask_out != nullptr;
    ++vision_counter_;
    Check(xivo_hip_pool_life_begin(ctx_, B_, F, off, reinterpret_cast<const long long*>(ids), meas,
                                   vision_counter_ >= sc_.strict_criteria_timesteps ? 1 : 0), "pool_life_begin");
    RunUpdate();
    Check(xivo_hip_pool_life_end(ctx_, B_), "pool_life_end");
    if (mask_out) std::memcpy(mask_out, mask_.data(), mask_.size());
    return;
  }
  if (subfilter_) {
    host_s_ += now_s() - t0;
    VisualSubfilter(off, ids, meas);
    if (mask_out) std::memcpy(mask_out, mask_.data(), mask_.size());
    return;
  }
  if (device_life_) {
    // the whole life cycle on the device: the tracks go down as they came in, nothing comes back
    host_s_ += now_s() - t0;
    want_mask_ = mask_out != nullptr;
    Check(xivo_hip_life_begin(ctx_, B_, F, off, reinterpret_cast<const long long*>(ids), meas), "life_begin");
    RunUpdate();
    Check(xivo_hip_life_end(ctx_, B_), "life_end");
    if (mask_out) std::memcpy(mask_out, mask_.data(), mask_.size());
    return;
  }
  // (the sub-filter life cycles above initialise a new track on the device, through any camera model; this one un-projects here)
  if (cfg_.cam.model != XIVO_CAM_PINHOLE)
    throw std::invalid_argument("the immediate life cycle initialises features with a pinhole un-projection");
  // --- before the update: tracker-dropped features leave (ProcessTracks, src/manager.cpp:152-169), tracked ones get
  // their new pixel
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::fill(xp_.begin(), xp_.end(), nan);
  // which track carries each in-state feature: the <= kMaxFeature in-state ids sorted once per filter, one binary
  // search per track (a frame brings ~10^2 tracks per filter, most of them not in the state)
  in_state_.assign((size_t)off[B_], 0);
  per_.resize(B_);
  // (filters are independent: the per-filter book-keeping runs over the host cores, every filter filling its own op
  // list; the lists are then joined in filter order, which xivo_hip_edit_batch requires anyway)
#pragma omp parallel for schedule(static) num_threads(kThreads) if (B_ >= 512)
  for (int b = 0; b < B_; ++b) {
    std::vector<xivo_edit_op>& ops = per_[b];
    ops.clear();
    std::vector<std::pair<int64_t, int>> instate;      // (id, slot), ascending id
    std::vector<int> slot_track(F);
    Book& bk = books_[b];
    for (int j = 0; j < F; ++j) if (bk.feat_id[j] >= 0) instate.emplace_back(bk.feat_id[j], j);
    std::sort(instate.begin(), instate.end());
    std::fill(slot_track.begin(), slot_track.end(), -1);
    for (int k = off[b]; k < off[b + 1]; ++k) {
      auto it = std::lower_bound(instate.begin(), instate.end(), std::make_pair(ids[k], -1));
      if (it != instate.end() && it->first == ids[k]) { slot_track[it->second] = k; in_state_[k] = 1; }
    }
    for (int j = 0; j < F; ++j) {
      if (bk.feat_id[j] < 0) continue;
      const int k = slot_track[j];
      if (k >= 0) {
        xp_[((size_t)b * F + j) * 2] = meas[(size_t)k * 3];
        xp_[((size_t)b * F + j) * 2 + 1] = meas[(size_t)k * 3 + 1];
      } else {
        ops.push_back(make_op(b, XIVO_EDIT_REMOVE_FEATURE, j));
        DropFeature(bk, j);
      }
    }
    DiscardEmptyGroups(b, ops);
    for (int j = 0; j < F; ++j) slot_track_all_[(size_t)b * F + j] = slot_track[j];
  }
  std::vector<xivo_edit_op> ops;
  for (int b = 0; b < B_; ++b) ops.insert(ops.end(), per_[b].begin(), per_[b].end());
  host_s_ += now_s() - t0;
  Check(xivo_hip_edit_batch(ctx_, F, (int)ops.size(), ops.empty() ? nullptr : ops.data()), "edit_batch");
  Check(xivo_hip_set_pixels(ctx_, 0, B_, F, xp_.data()), "set_pixels");
  // --- measurement update on the tracked in-state features (src/manager.cpp:72-104), ragged over the filters
  RunUpdate();
  t0 = now_s();
  for (int b = 0; b < B_; ++b) n_updates_ += books_[b].id2slot.empty() ? 0 : 1;
  // --- after the update: MH-rejected features leave (src/update.cpp:105-113), new ones enter with a new group
  const double fx = cfg_.cam.fx, fy = cfg_.cam.fy, cx = cfg_.cam.cx, cy = cfg_.cam.cy;
  double sd[3];
  NewTrackStd(false, sd);
  long rejected = 0;
#pragma omp parallel for schedule(static) reduction(+ : rejected) num_threads(kThreads) if (B_ >= 512)
  for (int b = 0; b < B_; ++b) {
    std::vector<xivo_edit_op>& ops = per_[b];
    ops.clear();
    std::vector<int> free_slots, order;
    Book& bk = books_[b];
    for (int j = 0; j < F; ++j)
      if (bk.feat_id[j] >= 0 && !mask_[(size_t)b * F + j]) {
        ops.push_back(make_op(b, XIVO_EDIT_REMOVE_FEATURE, j));
        in_state_[slot_track_all_[(size_t)b * F + j]] = 0;      // its track is a candidate again right away
        DropFeature(bk, j);
        ++rejected;
      }
    DiscardEmptyGroups(b, ops);
    free_slots.clear();
    for (int j = 0; j < F; ++j) if (bk.feat_id[j] < 0) free_slots.push_back(j);
    int g = -1;
    for (int q = 0; q < cfg_.n_groups; ++q) if (bk.group_refs[q] < 0) { g = q; break; }
    if (g < 0 || ((int)free_slots.size() < cfg_.min_new_features && !bk.id2slot.empty())) continue;
    // candidates: tracks not in the state, inside the depth range, by ascending id
    order.clear();
    for (int k = off[b]; k < off[b + 1]; ++k)
      if (!in_state_[k] && cfg_.min_depth < meas[(size_t)k * 3 + 2] && meas[(size_t)k * 3 + 2] < cfg_.max_depth)
        order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a_, int b_) { return ids[a_] < ids[b_]; });
    if (order.empty()) continue;
    ops.push_back(make_op(b, XIVO_EDIT_ADD_GROUP, g));          // Estimator::AddGroupToState (src/estimator.cpp:786-819)
    bk.group_refs[g] = 0;
    const size_t n_new = std::min(free_slots.size(), order.size());
    for (size_t q = 0; q < n_new; ++q) {
      const int j = free_slots[q], k = order[q];
      const double u = meas[(size_t)k * 3], v = meas[(size_t)k * 3 + 1], z = meas[(size_t)k * 3 + 2];
      xivo_edit_op o = make_op(b, XIVO_EDIT_ADD_FEATURE, j, j, g);   // AddFeatureToState + FillCovarianceBlock
      o.v[0] = (u - cx) / fx; o.v[1] = (v - cy) / fy; o.v[2] = cfg_.use_invdepth ? 1.0 / z : std::log(z);   // Feature::Initialize (src/feature.cpp:144-150)
      o.v[3] = u; o.v[4] = v;
      o.v[5] = sd[0] * sd[0]; o.v[9] = sd[1] * sd[1]; o.v[13] = sd[2] * sd[2];   // P_ = diag(std)^2 (:158-159)
      ops.push_back(o);
      bk.feat_id[j] = ids[k]; bk.feat_ref[j] = g; bk.id2slot[ids[k]] = j;
      bk.group_refs[g] += 1;
    }
  }
  n_rejected_ += rejected;
  ops.clear();
  for (int b = 0; b < B_; ++b) ops.insert(ops.end(), per_[b].begin(), per_[b].end());
  host_s_ += now_s() - t0;
  Check(xivo_hip_edit_batch(ctx_, F, (int)ops.size(), ops.empty() ? nullptr : ops.data()), "edit_batch");
  if (mask_out) std::memcpy(mask_out, mask_.data(), mask_.size());
}

// the initial std of a new feature's (x, y, depth): pixels over Camera::GetFocalLength() = 0.5 sqrt(fx^2 + fy^2)
// (src/camera_manager.cpp:56, src/estimator.cpp:351-352). badtri: a new track of the pool is never triangulated yet and takes
// the badtri stds (src/manager.cpp:585-586)
void BatchEstimator::NewTrackStd(bool badtri, double sd[3]) const {
  const double fx = cfg_.cam.fx, fy = cfg_.cam.fy;
  const double fl = 0.5 * std::sqrt(fx * fx + fy * fy);
  const double px[3] = {badtri ? dc_.std_badtri[0] : cfg_.initial_std_x, badtri ? dc_.std_badtri[1] : cfg_.initial_std_y,
                        badtri ? dc_.std_badtri[2] : cfg_.initial_std_z};
  sd[0] = px[0] / fl; sd[1] = px[1] / fl; sd[2] = px[2];
}

void BatchEstimator::EnableSubfilter(const SubfilterConfig& sc) {
  if (device_life_) throw std::runtime_error("the device life cycle runs the immediate mode only");
  if (device_pool_life_) throw std::runtime_error("EnableSubfilter would empty the pool under the device pool life cycle");
  sc_ = sc;
  Check(xivo_hip_pool_config(ctx_, sc.pool_max, sc.anchor_max, &sc.opts, sc.remove_outlier_counter), "pool_config");
  pools_.assign(B_, PoolBook{});
  for (auto& pb : pools_) {
    pb.ent_id.assign(sc.pool_max, -1); pb.ent_anchor.assign(sc.pool_max, -1); pb.ent_born.assign(sc.pool_max, 0);
    pb.anc_used.assign(sc.anchor_max, 0); pb.anc_life.assign(sc.anchor_max, 0); pb.anc_link.assign(sc.anchor_max, -1);
  }
  subfilter_ = true;
}

void BatchEstimator::EnableDeviceLifecycle(int tracks_max) {
  if (subfilter_) throw std::runtime_error("the device life cycle runs the immediate mode only");
  device_world_ = false;   // xivo_hip_life_config releases the resident worlds with the track block
  if (tracks_max <= 0) {
    // back to the host life cycle: the books and the counters come home before the device book is released
    if (device_life_) {
      for (int b = 0; b < B_; ++b) ReadBook(b);
      n_updates_ += LifeCount(0); n_rejected_ += LifeCount(1); n_not_spd_ += LifeCount(5);
    }
    device_life_ = false;
    xivo_life_opts off;
    std::memset(&off, 0, sizeof(off));
    Check(xivo_hip_life_config(ctx_, &off), "life_config");
    return;
  }
  double sd[3];
  NewTrackStd(false, sd);
  xivo_life_opts o;
  std::memset(&o, 0, sizeof(o));
  o.tracks_max = tracks_max; o.min_new_features = cfg_.min_new_features;
  o.min_depth = cfg_.min_depth; o.max_depth = cfg_.max_depth;
  for (int i = 0; i < 3; ++i) o.var_xyz[i] = sd[i] * sd[i];   // P_ = diag(std)^2 (src/feature.cpp:158-159)
  Check(xivo_hip_life_config(ctx_, &o), "life_config");
  // adopt the book kept so far (all free before the first frame)
  const int F = cfg_.n_features;
  std::vector<long long> fid((size_t)B_ * F);
  for (int b = 0; b < B_; ++b)
    for (int j = 0; j < F; ++j) fid[(size_t)b * F + j] = books_[b].feat_id[j];
  Check(xivo_hip_life_set_book(ctx_, 0, B_, fid.data()), "life_set_book");
  device_life_ = true;
}

void BatchEstimator::EnableDevicePoolLifecycle(int tracks_max) {
  if (!subfilter_) throw std::runtime_error("the device pool life cycle needs EnableSubfilter first");
  if (device_life_) throw std::runtime_error("the device pool life cycle excludes the immediate device life cycle");
  if (device_pool_life_ || vision_counter_ > 0) throw std::runtime_error("the device pool life cycle starts on an empty pool, once");
  xivo_pool_life_opts o;
  std::memset(&o, 0, sizeof(o));
  o.struct_size = (int)sizeof(o); o.tracks_max = tracks_max; o.max_group_lifetime = sc_.max_group_lifetime;
  o.adaptive_z = dc_.adaptive ? 1 : 0; o.initial_z = sc_.initial_z;
  NewTrackStd(dc_.triangulate, o.std_xyz);
  if (tracks_max <= 0) throw std::runtime_error("tracks_max must be positive");
  Check(xivo_hip_pool_life_config(ctx_, &o), "pool_life_config");
  device_pool_life_ = true;
}

void BatchEstimator::EnableDeviceWorld(int npts, const xivo_pcw_opts& cam, const double* Xs, double max_radius) {
  if (!device_life_ && !device_pool_life_)
    throw std::runtime_error("the device world needs a device life cycle (EnableDeviceLifecycle or EnableDevicePoolLifecycle)");
  xivo_pcw_opts o = cam;
  o.struct_size = (int)sizeof(o); o.npts = npts;
  Check(xivo_hip_pcw_config(ctx_, &o), "pcw_config");
  device_world_ = npts > 0;
  world_frame_ = 0;
  // the simulated camera is the estimator's: a distorted model goes down whole (cam's pinhole is then not read)
  if (device_world_ && cfg_.cam.model != XIVO_CAM_PINHOLE) Check(xivo_hip_pcw_camera(ctx_, &cfg_.cam, max_radius), "pcw_camera");
  faults_on_ = device_world_ && have_faults_;   // (pcw_config released whatever an earlier call turned on)
  if (faults_on_) Check(xivo_hip_pcw_fault_config(ctx_, &faults_), "pcw_fault_config");
  if (device_world_) Check(xivo_hip_pcw_set_world(ctx_, 0, B_, Xs, nullptr, nullptr), "pcw_set_world");
}

void BatchEstimator::VisualMeasDeviceWorld(double t, const double* gsc, double noise_px_std, unsigned long long seed,
                                           unsigned char* mask_out) {
  if (!(device_life_ || device_pool_life_) || !device_world_)
    throw std::runtime_error("VisualMeasDeviceWorld needs a device life cycle and EnableDeviceWorld");
  double t0 = now_s();
  PropagateToFrame(t, t0);
  host_s_ += now_s() - t0;
  want_mask_ = mask_out != nullptr;
  // the frame's tracks are produced where the life cycle reads them: 96 bytes per filter go down, nothing comes back
  Check(xivo_hip_pcw_tracks(ctx_, B_, gsc, noise_px_std, seed, world_frame_++), "pcw_tracks");
  FrameOnProducedTracks(mask_out);
}

// the rest of a frame whose tracks the producer left in the track block
void BatchEstimator::FrameOnProducedTracks(unsigned char* mask_out) {
  if (device_pool_life_) {
    ++vision_counter_;   // (where VisualMeasPointCloud counts the frame)
    Check(xivo_hip_pool_life_begin_tracks(ctx_, B_, cfg_.n_features, vision_counter_ >= sc_.strict_criteria_timesteps ? 1 : 0),
          "pool_life_begin_tracks");
  } else {
    Check(xivo_hip_life_begin_tracks(ctx_, B_, cfg_.n_features), "life_begin_tracks");
  }
  RunUpdate();
  if (faults_on_) Check(xivo_hip_pcw_fault_score(ctx_, B_), "pcw_fault_score");   // (enqueued: no host wait)
  Check(device_pool_life_ ? xivo_hip_pool_life_end(ctx_, B_) : xivo_hip_life_end(ctx_, B_), device_pool_life_ ? "pool_life_end" : "life_end");
  if (mask_out) std::memcpy(mask_out, mask_.data(), mask_.size());
}

void BatchEstimator::EnableDeviceImu(const xivo_trajsim_opts& opts, const int* motion, const double* rate) {
  if (!(device_life_ || device_pool_life_) || !device_world_)
    throw std::runtime_error("the device IMU needs a device life cycle and EnableDeviceWorld");
  xivo_trajsim_opts o = opts;
  o.struct_size = (int)sizeof(o);
  Check(xivo_hip_trajsim_config(ctx_, &o), "trajsim_config");
  device_imu_ = o.n_max > 0; device_imu_dt_ = o.imu_dt;
  if (device_imu_) Check(xivo_hip_trajsim_set(ctx_, 0, B_, motion, rate), "trajsim_set");
}

void BatchEstimator::FrameResident(unsigned long long k0, int n, double noise_px_std, unsigned long long seed, unsigned char* mask_out) {
  if (!device_imu_ || !device_world_ || !(device_life_ || device_pool_life_)) throw std::runtime_error("FrameResident needs EnableDeviceImu");
  t_visual_ = (double)(k0 + (unsigned long long)n) * device_imu_dt_;
  want_mask_ = mask_out != nullptr;
  Check(xivo_hip_trajsim_frame(ctx_, B_, k0, n), "trajsim_frame");
  if (n > 0) Check(xivo_hip_propagate_resident(ctx_, B_, &cfg_.prop), "propagate_resident");
  Check(xivo_hip_pcw_tracks_resident(ctx_, B_, noise_px_std, seed, world_frame_++), "pcw_tracks_resident");
  FrameOnProducedTracks(mask_out);
}

void BatchEstimator::ReadBook(int b) {
  const int F = cfg_.n_features;
  Book& bk = books_[b];
  std::vector<long long> fid(F);
  if (device_pool_life_)
    Check(xivo_hip_pool_life_get_book(ctx_, b, 1, fid.data(), bk.feat_ref.data(), bk.group_refs.data(), nullptr, nullptr, nullptr,
                                      nullptr), "pool_life_get_book");
  else
    Check(xivo_hip_life_get_book(ctx_, b, 1, fid.data(), bk.feat_ref.data(), bk.group_refs.data()), "life_get_book");
  bk.id2slot.clear();
  for (int j = 0; j < F; ++j) { bk.feat_id[j] = fid[j]; if (fid[j] >= 0) bk.id2slot[fid[j]] = j; }
}

long BatchEstimator::LifeCount(int which) const {
  std::vector<xivo_life_stats> st(B_);
  if (xivo_hip_life_stats(ctx_, 0, B_, st.data()) != XIVO_HIP_OK) throw std::runtime_error("life_stats");
  long n = 0;
  for (const auto& s : st) {
    const long long v[6] = {s.updates, s.rejected, s.dropped, s.admitted, s.groups_added, s.not_spd};
    n += (long)v[which];
  }
  return n;
}

long BatchEstimator::PoolLifeCount(int which) const {
  std::vector<xivo_pool_life_stats> st(B_);
  if (xivo_hip_pool_life_stats(ctx_, 0, B_, st.data()) != XIVO_HIP_OK) throw std::runtime_error("pool_life_stats");
  long n = 0;
  for (const auto& s : st) {
    const long long v[12] = {s.updates, s.rejected, s.dropped, s.admitted, s.groups_added, s.not_spd, s.pool_added,
                             s.pool_dropped, s.pool_outliers, s.anchors_created, s.anchors_freed, s.admit_steps};
    n += (long)v[which];
  }
  return n;
}

void BatchEstimator::EnableDepthInit(const DepthInitConfig& dc) {
  if (device_pool_life_) throw std::runtime_error("EnableDepthInit comes before EnableDevicePoolLifecycle");
  if (!subfilter_) throw std::runtime_error("EnableDepthInit needs EnableSubfilter first");
  Check(xivo_hip_pool_triangulation(ctx_, dc.triangulate ? &dc.tri : nullptr), "pool_triangulation");
  if (dc.adaptive) {
    Check(xivo_hip_pool_adapt_depth_config(ctx_, &dc.adapt), "pool_adapt_depth_config");
    init_z_.assign(B_, dc.adapt.initial_z);
  }
  dc_ = dc;
}

// One camera frame of the "subfilter" life cycle, decision for decision SequenceRunner._frame_subfilter of
// xivo_amd/sequence.py (the order of Estimator::UpdateStep, src/manager.cpp:18-130)
void BatchEstimator::VisualSubfilter(const int* off, const int64_t* ids, const double* meas) {
  const int F = cfg_.n_features, PM = sc_.pool_max, AM = sc_.anchor_max;
  ++vision_counter_;
  for (auto& pb : pools_)                               // Group::IncrementLifetime (:36-41)
    for (int a = 0; a < AM; ++a) pb.anc_life[a] = pb.anc_used[a] ? pb.anc_life[a] + 1 : 0;
  std::vector<std::unordered_map<int64_t, int>> pos(B_);
  for (int b = 0; b < B_; ++b)
    for (int k = off[b]; k < off[b + 1]; ++k) pos[b][ids[k]] = k;
  // --- ProcessTracks (:171-250)
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<xivo_edit_op> ops;
  std::vector<double> xpp((size_t)B_ * PM * 2, nan);
  for (int b = 0; b < B_; ++b) {
    Book& bk = books_[b];
    PoolBook& pb = pools_[b];
    for (int j = 0; j < F; ++j)
      if (bk.feat_id[j] >= 0 && !pos[b].count(bk.feat_id[j])) {
        ops.push_back(make_op(b, XIVO_EDIT_REMOVE_FEATURE, j));
        DropFeature(bk, j);
      }
    DiscardEmptyGroups(b, ops);
    for (int e = 0; e < PM; ++e) {
      if (pb.ent_id[e] < 0) continue;
      auto it = pos[b].find(pb.ent_id[e]);
      if (it != pos[b].end()) {
        xpp[((size_t)b * PM + e) * 2] = meas[(size_t)it->second * 3];
        xpp[((size_t)b * PM + e) * 2 + 1] = meas[(size_t)it->second * 3 + 1];
      } else {
        pb.FreeEntry(e);
      }
    }
  }
  std::vector<int> order((size_t)B_ * PM), n_cand(B_);
  std::vector<unsigned char> live((size_t)B_ * PM);
  Check(xivo_hip_pool_step(ctx_, B_, xpp.data(), vision_counter_ >= sc_.strict_criteria_timesteps ? 1 : 0, order.data(),
                           n_cand.data(), live.data()), "pool_step");
  // --- SelectAndAddNewFeatures / ZeroGaugeXYAddFeatures (:332-450): candidates in device order into free slots
  for (int b = 0; b < B_; ++b) {
    Book& bk = books_[b];
    PoolBook& pb = pools_[b];
    for (int e = 0; e < PM; ++e)
      if (pb.ent_id[e] >= 0 && !live[(size_t)b * PM + e]) pb.FreeEntry(e);    // sub-filter outlier (:236-240)
    std::vector<int> free_slots, gfree;
    for (int j = 0; j < F; ++j) if (bk.feat_id[j] < 0) free_slots.push_back(j);
    for (int g = 0; g < cfg_.n_groups; ++g) if (bk.group_refs[g] < 0) gfree.push_back(g);
    size_t fq = 0, gq = 0;
    for (int q = 0; q < n_cand[b] && fq < free_slots.size(); ++q) {
      const int e = order[(size_t)b * PM + q], a = pb.ent_anchor[e];
      if (pb.anc_link[a] < 0) {
        if (gq >= gfree.size()) continue;                 // its group would need a free slot (:437-441)
        const int g = gfree[gq++];
        ops.push_back(make_op(b, XIVO_EDIT_ADD_GROUP_ANCHOR, g, a));
        pb.anc_link[a] = g;
        bk.group_refs[g] = 0;
      }
      const int g = pb.anc_link[a], j = free_slots[fq++];
      const int64_t fid = pb.ent_id[e];
      ops.push_back(make_op(b, XIVO_EDIT_ADMIT_POOL, j, j, e));
      bk.feat_id[j] = fid; bk.feat_ref[j] = g; bk.id2slot[fid] = j;
      bk.group_refs[g] += 1;
      pb.FreeEntry(e);
      ++n_admitted_;
    }
  }
  // xivo_hip_edit_batch takes the ops grouped by filter (each filter's in the order they were made)
  std::stable_sort(ops.begin(), ops.end(), [](const xivo_edit_op& x, const xivo_edit_op& y) { return x.b < y.b; });
  Check(xivo_hip_edit_batch(ctx_, F, (int)ops.size(), ops.empty() ? nullptr : ops.data()), "edit_batch");
  std::fill(xp_.begin(), xp_.end(), nan);
  for (int b = 0; b < B_; ++b)
    for (int j = 0; j < F; ++j)
      if (books_[b].feat_id[j] >= 0) {
        const int k = pos[b][books_[b].feat_id[j]];
        xp_[((size_t)b * F + j) * 2] = meas[(size_t)k * 3];
        xp_[((size_t)b * F + j) * 2 + 1] = meas[(size_t)k * 3 + 1];
      }
  Check(xivo_hip_set_pixels(ctx_, 0, B_, F, xp_.data()), "set_pixels");
  // --- OutlierRejection + FilterUpdate, then DiscardAffectedGroups
  RunUpdate();
  for (int b = 0; b < B_; ++b) n_updates_ += books_[b].id2slot.empty() ? 0 : 1;
  ops.clear();
  for (int b = 0; b < B_; ++b) {
    Book& bk = books_[b];
    for (int j = 0; j < F; ++j)
      if (bk.feat_id[j] >= 0 && !mask_[(size_t)b * F + j]) {
        ops.push_back(make_op(b, XIVO_EDIT_REMOVE_FEATURE, j));
        DropFeature(bk, j);
        ++n_rejected_;
      }
    DiscardEmptyGroups(b, ops);
  }
  Check(xivo_hip_edit_batch(ctx_, F, (int)ops.size(), ops.empty() ? nullptr : ops.data()), "edit_batch");
  // --- Group::Create(X_.Rsb, X_.Tsb) from the updated pose + InitializeJustCreatedTracks (:121-126, :575-600)
  double new_std[3];
  NewTrackStd(dc_.triangulate, new_std);
  std::vector<int> slots(B_, -1);
  std::vector<xivo_pool_new> recs;
  for (int b = 0; b < B_; ++b) {
    Book& bk = books_[b];
    PoolBook& pb = pools_[b];
    std::vector<int> fresh;
    for (int k = off[b]; k < off[b + 1]; ++k)
      if (!bk.id2slot.count(ids[k]) && !pb.id2ent.count(ids[k])) fresh.push_back(k);
    if (fresh.empty()) continue;
    std::stable_sort(fresh.begin(), fresh.end(), [&](int a_, int b_) { return ids[a_] < ids[b_]; });
    int a = -1;
    for (int q = 0; q < AM; ++q) if (!pb.anc_used[q]) { a = q; break; }
    if (a < 0) { n_pool_dropped_ += (long)fresh.size(); continue; }
    slots[b] = a;
    pb.anc_used[a] = 1; pb.anc_life[a] = 0; pb.anc_link[a] = -1;
    size_t q = 0;
    for (int e = 0; e < PM && q < fresh.size(); ++e) {
      if (pb.ent_id[e] >= 0) continue;
      const int k = fresh[q++];
      xivo_pool_new r;
      std::memset(&r, 0, sizeof(r));
      r.b = b; r.entry = e; r.anchor = a;
      r.xp[0] = meas[(size_t)k * 3]; r.xp[1] = meas[(size_t)k * 3 + 1];
      r.z0 = sc_.initial_z;   // (ignored under adaptive_initial_depth: the device's resident init_z)
      for (int i = 0; i < 3; ++i) r.std_xyz[i] = new_std[i];
      recs.push_back(r);
      pb.ent_id[e] = ids[k]; pb.ent_anchor[e] = a; pb.ent_born[e] = vision_counter_; pb.id2ent[ids[k]] = e;
    }
    n_pool_dropped_ += (long)(fresh.size() - q);
  }
  if (std::any_of(slots.begin(), slots.end(), [](int v) { return v >= 0; }))
    Check(xivo_hip_pool_anchor(ctx_, 0, B_, slots.data()), "pool_anchor");
  if (!recs.empty())
    Check(xivo_hip_pool_add_ex(ctx_, (int)recs.size(), recs.data(), dc_.adaptive ? XIVO_POOL_ADD_ADAPTIVE_Z : 0u), "pool_add");
  // --- AdaptInitialDepth (:131)
  if (dc_.adaptive) Check(xivo_hip_pool_adapt_depth(ctx_, B_, init_z_.data()), "pool_adapt_depth");
  // --- EnforceMaxGroupLifetime (:282-304)
  for (auto& pb : pools_) {
    std::vector<char> held(AM, 0);
    for (int e = 0; e < PM; ++e) if (pb.ent_id[e] >= 0) held[pb.ent_anchor[e]] = 1;
    for (int a = 0; a < AM; ++a)
      if (pb.anc_used[a] && pb.anc_link[a] < 0 && pb.anc_life[a] > sc_.max_group_lifetime && !held[a]) pb.anc_used[a] = 0;
  }
}

void BatchEstimator::Poses(xivo_pose_in* out) {
  Check(xivo_hip_get_scene(ctx_, 0, B_, out, nullptr, nullptr), "get_scene");
}

}  // namespace hip
}  // namespace xivo

// ---- C entry points for the Python tests / scripts (ctypes) ------------------------------------------------------
extern "C" {

struct xivo_batch_cfg {   // flat mirror of xivo::hip::BatchConfig
  int n_groups, n_features;
  xivo_cam cam;
  double visual_meas_std, MH_thresh, MH_adjust_factor;
  int min_inliers, min_new_features, fix_group_block, disable_MH_gating;   // cfg use_MH_gating = false
  double initial_std_x, initial_std_y, initial_std_z, min_depth, max_depth;
  xivo_prop_opts prop;
  int use_1pt_RANSAC, use_invdepth;                  // cfg use_1pt_RANSAC, 1pt_RANSAC_thresh, 1pt_RANSAC_Chi2 (src/estimator.cpp:130-134)
  double ransac_thresh, ransac_Chi2;
};

int xivo_batch_create_rows(const xivo_batch_cfg* c, int B, int device, const xivo_pose_in* poses0, const double* P0, int extra_rows,
                           void** out);
int xivo_batch_create(const xivo_batch_cfg* c, int B, int device, const xivo_pose_in* poses0, const double* P0, void** out) {
  return xivo_batch_create_rows(c, B, device, poses0, P0, 0, out);
}
int xivo_batch_enable_oos(void* h, const xivo_pool_oos_opts* o) {
  if (!h || !o) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableOosUpdates(*o); return 0; } catch (const std::exception&) { return -1; }
}
// xivo_batch_create with room for extra_rows measurement rows behind the in-state ones (EnableOosUpdates)
int xivo_batch_create_rows(const xivo_batch_cfg* c, int B, int device, const xivo_pose_in* poses0, const double* P0, int extra_rows,
                           void** out) {
  try {
    xivo::hip::BatchConfig cfg;
    cfg.n_groups = c->n_groups; cfg.n_features = c->n_features; cfg.cam = c->cam;
    cfg.visual_meas_std = c->visual_meas_std; cfg.MH_thresh = c->MH_thresh; cfg.MH_adjust_factor = c->MH_adjust_factor;
    cfg.min_inliers = c->min_inliers; cfg.min_new_features = c->min_new_features; cfg.fix_group_block = c->fix_group_block;
    cfg.use_MH_gating = c->disable_MH_gating ? 0 : 1;
    cfg.use_1pt_RANSAC = c->use_1pt_RANSAC; cfg.ransac_thresh = c->ransac_thresh; cfg.ransac_Chi2 = c->ransac_Chi2;
    cfg.use_invdepth = c->use_invdepth; cfg.extra_rows = extra_rows;
    cfg.initial_std_x = c->initial_std_x; cfg.initial_std_y = c->initial_std_y; cfg.initial_std_z = c->initial_std_z;
    cfg.min_depth = c->min_depth; cfg.max_depth = c->max_depth; cfg.prop = c->prop;
    *out = new xivo::hip::BatchEstimator(cfg, B, device, poses0, P0);
    return 0;
  } catch (const std::exception&) { return -1; }
}
void xivo_batch_destroy(void* h) { delete static_cast<xivo::hip::BatchEstimator*>(h); }
int xivo_batch_imu(void* h, double t, const double* gyro, const double* accel) {
  try { static_cast<xivo::hip::BatchEstimator*>(h)->InertialMeas(t, gyro, accel); return 0; } catch (const std::exception&) { return -1; }
}
int xivo_batch_visual(void* h, double t, const int* off, const long long* ids, const double* meas, unsigned char* mask_out) {
  try {
    static_cast<xivo::hip::BatchEstimator*>(h)->VisualMeasPointCloud(t, off, reinterpret_cast<const int64_t*>(ids), meas, mask_out);
    return 0;
  } catch (const std::exception&) { return -1; }
}
int xivo_batch_poses(void* h, xivo_pose_in* out) {
  try { static_cast<xivo::hip::BatchEstimator*>(h)->Poses(out); return 0; } catch (const std::exception&) { return -1; }
}
int xivo_batch_book(void* h, int b, long long* feat_id, int* feat_ref, int* group_refs) {
  auto* e = static_cast<xivo::hip::BatchEstimator*>(h);
  if (b < 0 || b >= e->B()) return -1;
  try {
    const auto& bk = e->book(b);   // (device life cycle: read from the device)
    for (size_t j = 0; j < bk.feat_id.size(); ++j) { feat_id[j] = bk.feat_id[j]; feat_ref[j] = bk.feat_ref[j]; }
    for (size_t g = 0; g < bk.group_refs.size(); ++g) group_refs[g] = bk.group_refs[g];
    return 0;
  } catch (const std::exception&) { return -1; }
}
void xivo_batch_stats(void* h, long* n_updates, long* n_rejected, double* host_seconds) {
  auto* e = static_cast<xivo::hip::BatchEstimator*>(h);
  *host_seconds = e->host_seconds();
  try { *n_updates = e->n_updates(); *n_rejected = e->n_rejected(); }   // (device life cycle: read from the device)
  catch (const std::exception&) { *n_updates = -1; *n_rejected = -1; }
}
int xivo_batch_cfg_size(void) { return (int)sizeof(xivo_batch_cfg); }   // checked against the ctypes mirror (tests)
struct xivo_batch_subfilter_cfg {   // flat mirror of xivo::hip::BatchEstimator::SubfilterConfig
  double initial_z, remove_outlier_counter;
  int strict_criteria_timesteps, max_group_lifetime;
  xivo_subfilter_opts opts;
  int pool_max, anchor_max;
};
int xivo_batch_enable_subfilter(void* h, const xivo_batch_subfilter_cfg* c) {
  try {
    xivo::hip::BatchEstimator::SubfilterConfig sc;
    sc.initial_z = c->initial_z; sc.remove_outlier_counter = c->remove_outlier_counter;
    sc.strict_criteria_timesteps = c->strict_criteria_timesteps; sc.max_group_lifetime = c->max_group_lifetime;
    sc.opts = c->opts; sc.pool_max = c->pool_max; sc.anchor_max = c->anchor_max;
    static_cast<xivo::hip::BatchEstimator*>(h)->EnableSubfilter(sc);
    return 0;
  } catch (const std::exception&) { return -1; }
}
int xivo_batch_subfilter_cfg_size(void) { return (int)sizeof(xivo_batch_subfilter_cfg); }
struct xivo_batch_depth_init_cfg {   // flat mirror of xivo::hip::BatchEstimator::DepthInitConfig
  int triangulate, adaptive;
  xivo_triangulate_opts tri;
  double std_badtri[3];
  xivo_adapt_depth_opts adapt;
};
int xivo_batch_enable_depth_init(void* h, const xivo_batch_depth_init_cfg* c) {
  if (!h || !c) return -1;
  try {
    xivo::hip::BatchEstimator::DepthInitConfig dc;
    dc.triangulate = c->triangulate != 0; dc.adaptive = c->adaptive != 0;
    dc.tri = c->tri; dc.adapt = c->adapt;
    for (int i = 0; i < 3; ++i) dc.std_badtri[i] = c->std_badtri[i];
    static_cast<xivo::hip::BatchEstimator*>(h)->EnableDepthInit(dc);
    return 0;
  } catch (const std::exception&) { return -1; }
}
int xivo_batch_depth_init_cfg_size(void) { return (int)sizeof(xivo_batch_depth_init_cfg); }
// AdaptInitialDepth's init_z [B] after the last frame; -1 while adaptive_initial_depth is off
int xivo_batch_init_z(void* h, double* out) {
  const auto& z = static_cast<xivo::hip::BatchEstimator*>(h)->init_z();
  if (z.empty()) return -1;
  std::copy(z.begin(), z.end(), out);
  return 0;
}
void xivo_batch_pool_stats(void* h, long* admitted, long* dropped) {
  auto* e = static_cast<xivo::hip::BatchEstimator*>(h);
  try { *admitted = e->n_admitted(); *dropped = e->n_pool_dropped(); }   // (device pool life cycle: read from the device)
  catch (const std::exception&) { *admitted = -1; *dropped = -1; }
}
int xivo_batch_innov_log(void* h, int T_max) {
  if (!h) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableInnovationLog(T_max); return 0; } catch (const std::exception&) { return -1; }
}
int xivo_batch_enable_device_lifecycle(void* h, int tracks_max) {
  if (!h) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableDeviceLifecycle(tracks_max); return 0; } catch (const std::exception&) { return -1; }
}
int xivo_batch_enable_device_pool_lifecycle(void* h, int tracks_max) {
  if (!h) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableDevicePoolLifecycle(tracks_max); return 0; } catch (const std::exception&) { return -1; }
}
long xivo_batch_not_spd(void* h) {
  try { return static_cast<xivo::hip::BatchEstimator*>(h)->n_not_spd(); } catch (const std::exception&) { return -1; }
}
int xivo_batch_enable_device_world(void* h, int npts, const xivo_pcw_opts* cam, const double* Xs, double max_radius) {
  if (!h || !cam) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableDeviceWorld(npts, *cam, Xs, max_radius); return 0; }
  catch (const std::exception&) { return -1; }
}
int xivo_batch_set_track_faults(void* h, const xivo_pcw_fault_opts* opts) {
  if (!h) return -1;
  auto* e = static_cast<xivo::hip::BatchEstimator*>(h);
  if (opts) e->SetTrackFaults(*opts); else e->ClearTrackFaults();
  return 0;
}
int xivo_batch_visual_world(void* h, double t, const double* gsc, double noise_px_std, unsigned long long seed, unsigned char* mask_out) {
  if (!h) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->VisualMeasDeviceWorld(t, gsc, noise_px_std, seed, mask_out); return 0; }
  catch (const std::exception&) { return -1; }
}
int xivo_batch_enable_device_imu(void* h, const xivo_trajsim_opts* opts, const int* motion, const double* rate) {
  if (!h || !opts) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->EnableDeviceImu(*opts, motion, rate); return 0; } catch (const std::exception&) { return -1; }
}
int xivo_batch_frame_resident(void* h, unsigned long long k0, int n, double noise_px_std, unsigned long long seed, unsigned char* mask_out) {
  if (!h) return -1;
  try { static_cast<xivo::hip::BatchEstimator*>(h)->FrameResident(k0, n, noise_px_std, seed, mask_out); return 0; }
  catch (const std::exception&) { return -1; }
}
void* xivo_batch_ctx(void* h) { return static_cast<xivo::hip::BatchEstimator*>(h)->ctx(); }

}  // extern "C"
