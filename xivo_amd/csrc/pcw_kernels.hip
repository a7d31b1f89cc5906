// The point-cloud world's track producer on the device (gfx950): what BatchPCW.generate (xivo_amd/pcw.py, after the reference's
// scripts/point_cloud_world.py:44-131) computes per camera frame on the host and the frame call would otherwise upload. The
// worlds are resident - points, the track id each point holds, the next id of each world - and a frame needs the ground-truth
// camera poses only. One workgroup of 256 threads (four waves) per filter walks its points in chunks of 256 consecutive
// points; the rules and the arithmetic are the functions of pcw_device.h.
//
// Track ids and track positions are order preserving: the k-th visible point of a world, in point order, is track k of the
// filter's row, and the k-th new one takes next_id + k. Both ranks are exclusive prefix counts over the chunk - the wave's
// ballot and the population count of the lanes below, the four wave totals through LDS - plus the totals of the chunks before,
// which every thread carries in registers. Nothing crosses workgroups and no atomic is used: a filter's world, its row of the
// track block and its two counters belong to its own workgroup.
//
// The kernel is a template on the camera: kModel = -1 is the pinhole of xivo_pcw_opts (today's kernel, instruction for
// instruction), kModel = XIVO_CAM_* projects through the xivo_cam of xivo_hip_pcw_camera, which arrives by value in the kernel
// arguments. One instance per model, because a single kernel that branched on the model would hold the equidistant model's
// atan2 / sin / cos registers on every path: 147 VGPRs, 27 SGPR spills, 3 waves per SIMD for the pinhole too, against 94 / 0 / 5.
//
// For the same reason the fault path (pcw_device.h "Track faults": track loss, outliers, heavy tails, the shared stream) is a
// second template parameter: kFault = false is the kernel above, statement for statement, and reads none of the fault fields;
// kFault = true draws the events, ranks on the effective visibility, writes the flag byte of every track and counts the
// producer's five counters with four more ballots through the same wave totals.
#include "ekf_kernels.h"
#include "lifecycle_tracks_device.h"
#include "pcw_device.h"

namespace xivo_hip {

namespace {

constexpr int kPcwThreads = 256, kPcwWaves = kPcwThreads / 64;

template <int kModel, bool kFault>
__global__ __launch_bounds__(kPcwThreads) void pcw_tracks_kernel(PcwArgs a) {
  // wave totals (visible, new; the fault path: dropped, outlier, tail, biased too) of a chunk, two sets taken in turn: a wave
  // may write the next chunk's while another still reads this one's, and the barrier of the next chunk keeps it from going further
  constexpr int kTot = kFault ? 6 : 2;
  __shared__ int tot[2][kTot][kPcwWaves];
  __shared__ double g[12];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, npts = a.npts;
  if (tid < 12) g[tid] = a.gsc[(long)b * 12 + tid];
  __syncthreads();
  const PcwCam cam{a.fx, a.fy, a.cx, a.cy, a.imw, a.imh};
  xivo_cam lens = a.cam;
  lens.model = kModel;   // (known at compile time: camera_project keeps this model's statements alone)
  const double* Xs = a.Xs + (long)b * npts * 3;
  long long* ids = a.ids + (long)b * npts;
  long long* tid_out = a.track_ids + (long)b * a.track_ld;
  double* meas_out = a.track_meas + 3 * (long)b * a.track_ld;
  const long long next_id = a.next_id[b];
  const unsigned long long below = (1ull << lane) - 1ull;
  // the fault path: the rules' parameters and the filter word of this filter's counters
  const PcwFault fault{a.t1, a.t2, a.t3, a.outlier_min_px, a.outlier_max_px, a.tail_scale, a.sticky};
  const int bw = kFault ? pcw_stream_filter(b, a.stream_mod) : b;
  int base_vis = 0, base_new = 0;
  int n_drop = 0, n_out = 0, n_tail = 0, n_bias = 0;   // (kFault only)
  for (int p0 = 0, c = 0; p0 < npts; p0 += kPcwThreads, ++c) {
    const int p = p0 + tid;
    const bool in = p < npts;
    double uvz[3] = {0.0, 0.0, 0.0};
    long long id = -1;
    bool vis = false;
    if (in) {
      const double X[3] = {Xs[3 * (long)p], Xs[3 * (long)p + 1], Xs[3 * (long)p + 2]};
      id = ids[p];
      vis = kModel < 0 ? pcw_project(X, g, cam, uvz) : pcw_project(X, g, lens, a.max_radius, uvz);
    }
    double off[2] = {0.0, 0.0}, scale = 1.0;
    unsigned char flag = 0;
    bool dropped = false;
    if constexpr (kFault) {
      if (in) {   // from here on vis is vis_eff
        int ev;
        const bool geo = vis;
        double* bias = fault.sticky ? a.bias + 2 * ((long)b * npts + p) : nullptr;   // (no block without sticky faults)
        vis = pcw_fault_point(fault, a.seed, a.frame, bw, p, geo, bias, off, &scale, &flag, &ev);
        dropped = geo && !vis;
      }
    }
    const bool is_new = pcw_is_new(vis, id);
    const unsigned long long m_vis = __ballot(vis), m_new = __ballot(is_new);
    if (lane == 0) { tot[c & 1][0][wave] = __popcll(m_vis); tot[c & 1][1][wave] = __popcll(m_new); }
    if constexpr (kFault) {
      const unsigned long long m_drop = __ballot(dropped), m_out = __ballot((flag & PCW_FLAG_OUTLIER) != 0),
                               m_tail = __ballot((flag & PCW_FLAG_TAIL) != 0), m_bias = __ballot((flag & PCW_FLAG_BIASED) != 0);
      if (lane == 0) {
        tot[c & 1][2][wave] = __popcll(m_drop); tot[c & 1][3][wave] = __popcll(m_out);
        tot[c & 1][4][wave] = __popcll(m_tail); tot[c & 1][5][wave] = __popcll(m_bias);
      }
    }
    __syncthreads();
    int r_vis = base_vis + __popcll(m_vis & below), r_new = base_new + __popcll(m_new & below);
    for (int w = 0; w < kPcwWaves; ++w) {
      const int tv = tot[c & 1][0][w], tn = tot[c & 1][1][w];
      if (w < wave) { r_vis += tv; r_new += tn; }
      base_vis += tv; base_new += tn;
      if constexpr (kFault) {
        n_drop += tot[c & 1][2][w]; n_out += tot[c & 1][3][w]; n_tail += tot[c & 1][4][w]; n_bias += tot[c & 1][5][w];
      }
    }
    if (in) {
      const long long id_after = pcw_id_after(vis, id, next_id, r_new);
      if (id_after != id) ids[p] = id_after;
      if (vis) {   // r_vis < number of visible points <= npts <= track_ld (xivo_hip_pcw_config)
        double nu = 0.0, nv = 0.0;
        if (a.noise_px_std != 0.0) pcw_normal_pair(a.seed, a.frame, bw, p, &nu, &nv);
        tid_out[r_vis] = id_after;
        if (a.track_keys) a.track_keys[(long)b * a.track_ld + r_vis] = p;   // the track's key: its world point (BatchPCW's last_point_index)
        if constexpr (kFault) {
          const double std_eff = pcw_fault_std(a.noise_px_std, scale);
          meas_out[3 * (long)r_vis] = pcw_fault_pixel(uvz[0], off[0], std_eff, nu);
          meas_out[3 * (long)r_vis + 1] = pcw_fault_pixel(uvz[1], off[1], std_eff, nv);
          if (a.flags) a.flags[(long)b * a.track_ld + r_vis] = flag;
        } else {
          meas_out[3 * (long)r_vis] = pcw_noisy(uvz[0], a.noise_px_std, nu);
          meas_out[3 * (long)r_vis + 1] = pcw_noisy(uvz[1], a.noise_px_std, nv);
        }
        meas_out[3 * (long)r_vis + 2] = uvz[2];
      }
    }
  }
  if (tid == 0) {
    a.next_id[b] = next_id + base_new; a.cnt[b] = base_vis;
    if constexpr (kFault) {
      if (a.fstats) {   // the filter's own record: nothing crosses workgroups
        xivo_pcw_fault_stats& s = a.fstats[b];
        s.tracks += base_vis; s.dropped += n_drop; s.outlier_events += n_out; s.tail_events += n_tail; s.biased += n_bias;
      }
    }
  }
}

// The gate's decisions against the producer's labels, one workgroup per filter: every feature slot of the book that holds an id
// looks its track up by id among the frame's tracks (the last occurrence wins, as the association has it) and adds one to the
// cell pcw_fault_cell names. It matches by id, so it reads the book but none of the life cycles' LDS plan. The four sums go
// through LDS; thread 0 adds them to the filter's own record.
__global__ __launch_bounds__(kPcwThreads) void pcw_fault_score_kernel(PcwScoreArgs a) {
  __shared__ int cell[4];
  const LifeArgs& l = a.life;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 4) cell[tid] = 0;
  __syncthreads();
  const int k0 = life_track_begin(l, b), n = life_track_count(l, b);
  for (int j = tid; j < l.F; j += kPcwThreads) {
    const long long id = l.feat_id[(long)b * l.slot_ld + j];
    if (id < 0) continue;
    int hit = -1;
    for (int k = 0; k < n; ++k) if (l.ids[k0 + k] == id) hit = k;
    if (hit < 0) continue;
    atomicAdd(&cell[pcw_fault_cell(l.mask[(long)b * l.mask_ld + j], a.flags[(long)b * l.track_ld + hit])], 1);   // (LDS)
  }
  __syncthreads();
  if (tid == 0) {
    xivo_pcw_fault_stats& s = a.stats[b];
    s.outlier_rejected += cell[PCW_CELL_OUTLIER_REJECTED]; s.outlier_kept += cell[PCW_CELL_OUTLIER_KEPT];
    s.nominal_rejected += cell[PCW_CELL_NOMINAL_REJECTED]; s.nominal_kept += cell[PCW_CELL_NOMINAL_KEPT];
  }
}

template <bool kFault>
int launch_pcw_tracks_path(const PcwArgs& a, int batch, hipStream_t s) {
  const dim3 grid(batch), block(kPcwThreads);
  if (!a.use_cam) hipLaunchKernelGGL((pcw_tracks_kernel<-1, kFault>), grid, block, 0, s, a);
  else if (a.cam.model == XIVO_CAM_PINHOLE) hipLaunchKernelGGL((pcw_tracks_kernel<XIVO_CAM_PINHOLE, kFault>), grid, block, 0, s, a);
  else if (a.cam.model == XIVO_CAM_ATAN) hipLaunchKernelGGL((pcw_tracks_kernel<XIVO_CAM_ATAN, kFault>), grid, block, 0, s, a);
  else if (a.cam.model == XIVO_CAM_RADTAN) hipLaunchKernelGGL((pcw_tracks_kernel<XIVO_CAM_RADTAN, kFault>), grid, block, 0, s, a);
  else if (a.cam.model == XIVO_CAM_EQUI) hipLaunchKernelGGL((pcw_tracks_kernel<XIVO_CAM_EQUI, kFault>), grid, block, 0, s, a);
  else return 1;   // (xivo_hip_pcw_camera refuses any other model)
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

int launch_pcw_tracks(const PcwArgs& a, int batch, hipStream_t s) {
  return a.fault_path ? launch_pcw_tracks_path<true>(a, batch, s) : launch_pcw_tracks_path<false>(a, batch, s);
}

int launch_pcw_fault_score(const PcwScoreArgs& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL(pcw_fault_score_kernel, dim3(batch), dim3(kPcwThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace xivo_hip
