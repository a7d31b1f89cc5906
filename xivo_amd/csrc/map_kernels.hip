// Landmark log (xivo_hip_map_*, capi_map.hip): the per-frame record of every filter's in-state features - ordered by the
// norm of their local covariance block (FeatureCovComparison, src/estimator.cpp:1451-1455), with the world position Xs
// (Feature::Xs, src/feature.cpp:107-112), the local block, the covariance of Xs itself and the last pixel - and the
// consistency score of the logged points against true world points. Plain fp64 C++; no atomics - the order is a sorting
// network on (score, pos), the ensemble mean a fixed-shape tree, so both are reproducible.
#include <hip/hip_runtime.h>

#include "ekf_kernels.h"
#include "geometry_device.h"

namespace xivo_hip {

namespace {

constexpr int MAP_KEYS = XIVO_MAP_MAX_OUT;    // keys the sorting network holds: a power of two
constexpr int MAP_THREADS = 256, MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_PT_WORDS = (int)(sizeof(xivo_map_pt) / sizeof(double));
constexpr int MAP_ABSENT = 1 << 20;           // added to pos in the key of an absent entry: behind every present one
static_assert((MAP_KEYS & (MAP_KEYS - 1)) == 0 && MAP_KEYS <= MAP_THREADS, "one key per thread, bitonic network");
static_assert(sizeof(xivo_map_pt) == 20 * sizeof(double) && offsetof(xivo_map_pt, pos) == 18 * sizeof(double),
              "xivo_map_pt is 18 doubles and four ints");

// the packing of a symmetric 3 x 3: (0,0),(0,1),(0,2),(1,1),(1,2),(2,2)
__device__ __forceinline__ int sym6_row(int k) { return k < 3 ? 0 : (k < 5 ? 1 : 2); }
__device__ __forceinline__ int sym6_col(int k) { return k < 3 ? k : (k < 5 ? k - 2 : 2); }
// packed lower triangle of the 15 x 15 gather, row by row
__device__ __forceinline__ int tri_row15(int k) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= k) ++i;
  return i;
}

// (score, pos) keys: ascending score, ties by ascending pos. The score in a key is never NaN (a NaN score is keyed as +inf),
// so this is a strict total order on distinct pos.
__device__ __forceinline__ bool key_less(double sa, int pa, double sb, int pb) { return sa < sb || (sa == sb && pa < pb); }

// error-state column k of the 15 that Xs depends on: Wbc, Tbc (Index::Wbc = 15, Index::Tbc = 18, where jac_instate_kernel and
// absorb_error_kernel take them), the anchor group's six, the feature's three
__device__ __forceinline__ int map_col(int k, int goff, int foff) { return k < 6 ? 15 + k : (k < 12 ? goff + (k - 6) : foff + (k - 12)); }

// One workgroup of four waves per filter.
//  pass 1: thread = entry of the resident feature list: the score from the nine stored entries of its block, key to LDS
//  sort:   bitonic network over MAP_KEYS keys
//  pass 2: one wave per kept entry, four at a time; every phase ends in a workgroup barrier (the trip count is uniform)
__global__ __launch_bounds__(MAP_THREADS) void map_record_kernel(MapRecordArgs a) {
  __shared__ double kScore[MAP_KEYS];
  __shared__ int kPos[MAP_KEYS];
  __shared__ double sScore[MAP_KEYS];              // the score as computed (NaN stays NaN), by list position
  __shared__ int sCount;
  __shared__ double sJ[MAP_WAVES][3][15];
  __shared__ double sP[MAP_WAVES][15][15];
  __shared__ double sT[MAP_WAVES][3][15];
  __shared__ double sRec[MAP_WAVES][MAP_PT_WORDS];

  const int filt = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double* P = a.P + (long)filt * a.strideP;
  const xivo_feat_in* feats = a.feats + (long)filt * a.Fmax;
  const long ldp = a.ldp;

  // ---- pass 1
  if (tid == 0) sCount = 0;
  if (tid < MAP_KEYS) {
    double key = INFINITY;
    int pos = MAP_ABSENT + tid;
    if (tid < a.F) {
      const int sind = feats[tid].sind;
      if (sind >= 0 && sind < a.lay.n_features) {
        const double* B = P + (a.lay.feature_begin + 3 * sind) * (ldp + 1);
        double q[9];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int r = 0; r < 3; ++r) { const double v = B[r + c * ldp]; q[r + 3 * c] = v * v; }
        // a fixed pairwise tree: five roundings on the longest path, the square root's on top
        const double s = sqrt((((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) + q[8]);
        sScore[tid] = s;
        key = s != s ? INFINITY : s;
        pos = tid;
      }
    }
    kScore[tid] = key; kPos[tid] = pos;
  }
  __syncthreads();

  // ---- bitonic sort, ascending
  for (int k = 2; k <= MAP_KEYS; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < MAP_KEYS) {
        const int o = tid ^ j;
        if (o > tid) {
          const double s0 = kScore[tid], s1 = kScore[o];
          const int p0 = kPos[tid], p1 = kPos[o];
          const bool up = (tid & k) == 0;
          if (up ? key_less(s1, p1, s0, p0) : key_less(s0, p0, s1, p1)) {
            kScore[tid] = s1; kPos[tid] = p1; kScore[o] = s0; kPos[o] = p0;
          }
        }
      }
      __syncthreads();
    }
  }
  // the present entries are a prefix of the sorted keys; its last member publishes the count
  if (tid < MAP_KEYS && kPos[tid] < MAP_ABSENT && (tid == MAP_KEYS - 1 || kPos[tid + 1] >= MAP_ABSENT)) sCount = tid + 1;
  __syncthreads();
  const int count = sCount;
  const int n_pts = count < a.n_out ? count : a.n_out;
  xivo_map_pt* out = a.pts + (long)filt * a.n_out;
  if (tid == 0) a.n_pts[filt] = n_pts;

  // ---- the tail behind n_pts: zeros with pos = sind = -1
  {
    double* tail = reinterpret_cast<double*>(out + n_pts);
    const int words = (a.n_out - n_pts) * MAP_PT_WORDS;
    for (int w = tid; w < words; w += MAP_THREADS) {
      if (w % MAP_PT_WORDS == MAP_PT_WORDS - 2) {
        int2 v; v.x = -1; v.y = -1;
        *reinterpret_cast<int2*>(tail + w) = v;
      } else {
        tail[w] = 0.0;
      }
    }
  }

  // ---- pass 2
  const xivo_pose_in& X = a.poses[filt];
  for (int e0 = 0; e0 < n_pts; e0 += MAP_WAVES) {
    const int e = e0 + wave;
    const bool on = e < n_pts;
    int pos = 0, sind = 0, ref = 0, goff = 0, foff = 0;
    if (on) {
      pos = kPos[e];
      sind = feats[pos].sind; ref = feats[pos].ref_sind;
      if (ref < 0 || ref >= a.lay.n_groups) ref = 0;       // (set_scene / the edits never store such an anchor)
      goff = a.lay.group_begin + 6 * ref; foff = a.lay.feature_begin + 3 * sind;
    }
    // phase A: the geometry (every lane, registers), J by columns (lanes 0..14), the gather of Pcc (all lanes)
    if (on) {
      const xivo_feat_in& ft = feats[pos];
      const xivo_group_in& G = a.groups[(long)filt * a.lay.n_groups + ref];
      const M3 Rg = m3_from_colmajor(G.Rsb), Rbc = m3_from_colmajor(X.Rbc);
      M3 dXc_dx;
      const V3 Xc = feature_unproject(ft.x, a.invdepth, dXc_dx);
      const V3 RX = m3_mulv(Rbc, Xc);
      const V3 Xb{{RX.v[0] + X.Tbc[0], RX.v[1] + X.Tbc[1], RX.v[2] + X.Tbc[2]}};
      const V3 RXb = m3_mulv(Rg, Xb);
      if (lane < 3) sRec[wave][lane] = (lane == 0 ? RXb.v[0] : (lane == 1 ? RXb.v[1] : RXb.v[2])) + G.Tsb[lane];   // Xs
      if (lane >= 3 && lane < 5) sRec[wave][15 + lane - 3] = ft.xp[lane - 3];
      if (lane == 5) sRec[wave][17] = sScore[pos];
      if (lane == 6) {
        int* w = reinterpret_cast<int*>(&sRec[wave][18]);
        w[0] = pos; w[1] = sind; w[2] = feats[pos].ref_sind; w[3] = 0;
      }
      if (a.world) {
        if (lane < 15) {
          // column `lane` of J = [ -Rg Rbc hat(Xc) | Rg | -Rg hat(Xb) | I | Rg Rbc dXc/dx ]; hat(v) e_c = v x e_c
          const int blk = lane / 3, c = lane - 3 * blk;
          const V3 ec{{c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0}};
          const M3 Rgc = m3_mul(Rg, Rbc);
          V3 col;
          if (blk == 0 || blk == 2) {
            const V3 v = blk == 0 ? Xc : Xb;
            const V3 n{{-(v.v[1] * ec.v[2] - v.v[2] * ec.v[1]), -(v.v[2] * ec.v[0] - v.v[0] * ec.v[2]),
                        -(v.v[0] * ec.v[1] - v.v[1] * ec.v[0])}};
            col = m3_mulv(blk == 0 ? Rgc : Rg, n);
          } else if (blk == 1) {
            col = m3_mulv(Rg, ec);
          } else if (blk == 3) {
            col = ec;
          } else {
            col = m3_mulv(Rgc, m3_mulv(dXc_dx, ec));
          }
          sJ[wave][0][lane] = col.v[0]; sJ[wave][1][lane] = col.v[1]; sJ[wave][2][lane] = col.v[2];
        }
        for (int k = lane; k < 120; k += 64) {               // the 120 distinct entries of Pcc, lower triangle of P, mirrored
          const int i = tri_row15(k), j = k - i * (i + 1) / 2;
          const int ci = map_col(i, goff, foff), cj = map_col(j, goff, foff);
          const int r = ci > cj ? ci : cj, c = ci > cj ? cj : ci;
          const double v = P[r + c * ldp];
          sP[wave][i][j] = v; sP[wave][j][i] = v;
        }
      } else {
        if (lane < 6) {                                       // the local block alone: (r, c), r <= c, from P[off + c, off + r]
          const int r = sym6_row(lane), c = sym6_col(lane);
          sRec[wave][3 + lane] = P[(foff + c) + (foff + r) * ldp];
          sRec[wave][9 + lane] = 0.0;
        }
      }
    }
    __syncthreads();
    // phase B: T = J Pcc, 45 dot products of length 15; the local block out of the gather
    if (on && a.world) {
      if (lane < 45) {
        const int i = lane / 15, k = lane - 15 * i;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 15; ++m) s += sJ[wave][i][m] * sP[wave][m][k];
        sT[wave][i][k] = s;
      }
      if (lane >= 48 && lane < 54) {
        const int r = sym6_row(lane - 48), c = sym6_col(lane - 48);
        sRec[wave][3 + lane - 48] = sP[wave][12 + c][12 + r];
      }
    }
    __syncthreads();
    // phase C: the six entries of T J^T
    if (on && a.world && lane < 6) {
      const int r = sym6_row(lane), c = sym6_col(lane);
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 15; ++k) s += sT[wave][r][k] * sJ[wave][c][k];
      sRec[wave][9 + lane] = s;
    }
    __syncthreads();
    // phase D: the record, consecutive lanes on consecutive words
    if (on && lane < MAP_PT_WORDS) reinterpret_cast<double*>(out + e)[lane] = sRec[wave][lane];
    __syncthreads();
  }
}

// One thread per (frame, filter, slot) of the slice: e = gt - Xs, Sigma = cov_world = L L^T in registers, nees = |L^-1 e|^2
// (NaN when the un-pivoted factorisation meets a pivot that is not positive, for a slot behind n_pts, without truth).
__global__ __launch_bounds__(256) void map_nees_kernel(MapNeesArgs a) {
  const long per = (long)a.nb * a.n_out, n = (long)a.nt * per;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int t = (int)(id / per), b = (int)((id % per) / a.n_out), s = (int)(id % a.n_out);
  const long at = (long)(a.t0 + t) * a.Bmax + a.b0 + b;
  const double* g = a.gt + id * 3;
  double e[3] = {NAN, NAN, NAN};
  double nees = NAN;
  if (s < a.n_pts[at] && fabs(g[0]) < INFINITY && fabs(g[1]) < INFINITY && fabs(g[2]) < INFINITY) {
    const xivo_map_pt& p = a.pts[at * a.n_out + s];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = g[i] - p.Xs[i];
    const double* S = p.cov_world;                      // (0,0),(0,1),(0,2),(1,1),(1,2),(2,2)
    bool ok = true;
    const double d0 = S[0];
    ok = ok && d0 > 0.0 && d0 < INFINITY;               // (a NaN pivot fails the first comparison)
    const double l00 = sqrt(d0), l10 = S[1] / l00, l20 = S[2] / l00;
    const double d1 = S[3] - l10 * l10;
    ok = ok && d1 > 0.0 && d1 < INFINITY;
    const double l11 = sqrt(d1), l21 = (S[4] - l20 * l10) / l11;
    const double d2 = S[5] - l20 * l20 - l21 * l21;
    ok = ok && d2 > 0.0 && d2 < INFINITY;
    const double l22 = sqrt(d2);
    const double y0 = e[0] / l00, y1 = (e[1] - l10 * y0) / l11, y2 = (e[2] - l20 * y0 - l21 * y1) / l22;
    nees = ok ? y0 * y0 + y1 * y1 + y2 * y2 : NAN;
  }
  if (a.err3) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.err3[id * 3 + i] = e[i];
  }
  a.nees[id] = nees;
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_map_record(const MapRecordArgs& a, int batch, hipStream_t s) {
  if (batch <= 0) return 0;
  if (a.F < 0 || a.F > MAP_KEYS || a.n_out < 1 || a.n_out > MAP_KEYS) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(map_record_kernel, dim3(batch), dim3(MAP_THREADS), 0, s, a);
  CHECK_LAUNCH();
}

int launch_map_nees(const MapNeesArgs& a, hipStream_t s) {
  const long n = (long)a.nt * a.nb * a.n_out;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(map_nees_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return (int)hipErrorLaunchFailure;
  return launch_frame_anees(a.nees, (long)a.nb * a.n_out, a.nt, a.anees, a.n_used, s);   // (traj_kernels.hip)
}

}  // namespace xivo_hip
