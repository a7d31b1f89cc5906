// The resident landmark map (gfx950), driven by capi_lcmap.hip: loop closure without a round trip to the host.
//
//  lcmap_add_kernel     DiscardFeatures -> Mapper::AddFeature (src/mapper.cpp:158-222, merge_features = false): the in-state
//                       features that leave become map entries {key, Xs = Feature::Xs(gbc)}
//  lcmap_match_kernel   Mapper::DetectLoopClosures (src/mapper.cpp:335-418), the matching: the frame's queries against the map,
//                       the first lc_max matching ones in query order fill the filter's match list
//  lcmap_close_kernel   the stacking of Estimator::CloseLoopInternal (src/update.cpp:183-196) on that list: the row pair of every
//                       match (lc_row_pair, geometry_device.h - lc_rows_kernel's arithmetic), its gate on the filter's covariance
//                       (the stand-in for pnp_ransac), whether the filter closes, neutral pairs for what does not take part
// xivo_hip_lcmap_cov_config's options - a covariance per stored point, one use of a point per visit - are the second
// instantiation of the add and the close kernel; without them the first one runs, which holds none of their code.
// One workgroup of one wave per filter in all three: a filter's map is only ever touched by its own workgroup, so the order of
// the records decides (never a race) and the counters are plain sums - no global atomics. The integer rules are
// lcmap_device.h's, which a host program tests; the kernels only evaluate them.
// The records and the queries come packed behind offsets, as the host uploads them, or (cnt non-null) one row per filter with a
// count, as the device life cycle leaves them (xivo_hip_lcmap_add_resident / _close_resident): lc_list_begin / lc_list_end are
// the only place that tells the two apart. lclife_query_kernel makes that life cycle's queries (lcmap_life_device.h's rules).
#include "ekf_kernels.h"
#include "gate_device.h"
#include "geometry_device.h"
#include "lcmap_device.h"
#include "lcmap_life_device.h"

namespace xivo_hip {

namespace {

constexpr long kKeyStride = sizeof(xivo_lcmap_entry) / sizeof(long long);   // entry to entry, in keys
static_assert(sizeof(xivo_lcmap_entry) == 32 && sizeof(xivo_lcmap_entry) % sizeof(long long) == 0, "lcmap_find walks the keys");

// where filter filt's records / queries start and end, in either form of the list (ekf_kernels.h)
template <class Args> __device__ __forceinline__ int lc_list_begin(const Args& a, int filt) {
  return a.cnt ? (int)lclife_list_pos(filt, a.row, 0) : a.off[filt];
}
template <class Args> __device__ __forceinline__ int lc_list_end(const Args& a, int filt) {
  return a.cnt ? (int)lclife_list_pos(filt, a.row, lclife_list_count(a.cnt[filt], a.row)) : a.off[filt + 1];
}

__device__ __forceinline__ int lcmap_count(const LcMapBuffers& m, int filt) {
  const int n = m.count[filt];
  return n < 0 ? 0 : (n > m.map_max ? m.map_max : n);
}

// The covariance of an in-state feature's world point (xivo_hip_lcmap_cov_config, point_cov): Sigma = J Pcc J^T over the 15
// error-state columns Xs depends on - the arithmetic of map_record_kernel's pass 2 (map_kernels.hip), written a second time so
// that kernel stays as it is. The packing of a symmetric 3 x 3 is (0,0),(0,1),(0,2),(1,1),(1,2),(2,2).
__device__ __forceinline__ int lc_sym6_row(int k) { return k < 3 ? 0 : (k < 5 ? 1 : 2); }
__device__ __forceinline__ int lc_sym6_col(int k) { return k < 3 ? k : (k < 5 ? k - 2 : 2); }
__device__ __forceinline__ int lc_tri_row15(int k) {   // packed lower triangle of the 15 x 15 gather, row by row
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= k) ++i;
  return i;
}
// column k of the 15: Wbc, Tbc (15..20), the anchor group's six, the feature's three
__device__ __forceinline__ int lc_cov_col(int k, int goff, int foff) { return k < 6 ? 15 + k : (k < 12 ? goff + (k - 6) : foff + (k - 12)); }

struct LcCovLds { double J[3][15], P[15][15], T[3][15]; };   // 2520 bytes

// One wave, every lane calls it (two barriers inside): lanes 0..14 a column of
// J = [ -Rg Rbc hat(Xc) | Rg | -Rg hat(Xb) | I | Rg Rbc dXc/dx ], all lanes the 120 distinct entries of Pcc from the lower
// triangle of P, lanes 0..44 T = J Pcc, lanes 0..5 the six entries of T J^T to out[0..5]
__device__ __forceinline__ void lc_point_cov(const xivo_pose_in& pose, const xivo_feat_in& ft, const xivo_group_in& gref, int invdepth,
                                             const double* P, long ldp, int goff, int foff, LcCovLds& s, int lane, double* out) {
  if (lane < 15) {
    const M3 Rg = m3_from_colmajor(gref.Rsb), Rbc = m3_from_colmajor(pose.Rbc);
    M3 dXc_dx;
    const V3 Xc = feature_unproject(ft.x, invdepth, dXc_dx);
    const V3 RX = m3_mulv(Rbc, Xc);
    const V3 Xb{{RX.v[0] + pose.Tbc[0], RX.v[1] + pose.Tbc[1], RX.v[2] + pose.Tbc[2]}};
    const int blk = lane / 3, c = lane - 3 * blk;
    const V3 ec{{c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0}};   // hat(v) e_c = v x e_c
    const M3 Rgc = m3_mul(Rg, Rbc);
    V3 col;
    if (blk == 0 || blk == 2) {
      const V3 v = blk == 0 ? Xc : Xb;
      const V3 n{{-(v.v[1] * ec.v[2] - v.v[2] * ec.v[1]), -(v.v[2] * ec.v[0] - v.v[0] * ec.v[2]), -(v.v[0] * ec.v[1] - v.v[1] * ec.v[0])}};
      col = m3_mulv(blk == 0 ? Rgc : Rg, n);
    } else if (blk == 1) {
      col = m3_mulv(Rg, ec);
    } else if (blk == 3) {
      col = ec;
    } else {
      col = m3_mulv(Rgc, m3_mulv(dXc_dx, ec));
    }
    s.J[0][lane] = col.v[0]; s.J[1][lane] = col.v[1]; s.J[2][lane] = col.v[2];
  }
  for (int k = lane; k < 120; k += 64) {
    const int i = lc_tri_row15(k), j = k - i * (i + 1) / 2;
    const int ci = lc_cov_col(i, goff, foff), cj = lc_cov_col(j, goff, foff);
    const int r = ci > cj ? ci : cj, c = ci > cj ? cj : ci;
    const double v = P[r + c * ldp];
    s.P[i][j] = v; s.P[j][i] = v;
  }
  __syncthreads();
  if (lane < 45) {
    const int i = lane / 15, k = lane - 15 * i;
    double t = 0.0;
#pragma unroll
    for (int m = 0; m < 15; ++m) t += s.J[i][m] * s.P[m][k];
    s.T[i][k] = t;
  }
  __syncthreads();
  if (lane < 6) {
    const int r = lc_sym6_row(lane), c = lc_sym6_col(lane);
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) t += s.T[r][k] * s.J[c][k];
    out[lane] = t;
  }
}

// The records of a filter in order. The lanes share the search for the key among the stored entries, lane 0 writes the entry
// a record becomes; the barrier behind an accepted record makes it visible to the search of the next one. EXT: the
// instantiation that also stores the point's covariance (a.ext.cov; the branch around its barriers is uniform); without the
// options of xivo_hip_lcmap_cov_config the first one runs, whose code is what it was before they existed.
template <bool EXT>
__global__ __launch_bounds__(64) void lcmap_add_kernel(LcMapAddArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  xivo_lcmap_entry* ent = a.map.entries + (long)filt * a.map.map_max;
  const double* P = a.P + (long)filt * a.strideP;
  const xivo_pose_in& pose = a.poses[filt];
  int count = lcmap_count(a.map, filt);
  long long n_add = 0, n_skip = 0, n_poor = 0, n_dup = 0, n_full = 0;
  const int r0 = lc_list_begin(a, filt), r1 = lc_list_end(a, filt);
  for (int i = r0; i < r1; ++i) {                        // (every lane walks the same records: the branches are uniform)
    const xivo_lcmap_add_rec r = a.recs[i];
    int in_state = 0, poor = 0, ref = 0;
    const xivo_feat_in* ft = nullptr;
    if (r.key >= 0 && r.feat >= 0 && r.feat < a.F) {
      ft = a.feats + (long)filt * a.Fmax + r.feat;
      ref = ft->ref_sind;
      const int foff = a.lay.feature_begin + 3 * ft->sind;
      in_state = ft->sind >= 0 && ft->sind < a.lay.n_features && foff + 2 < a.lay.N && ref >= 0 && ref < a.lay.n_groups;
      if (in_state) poor = lcmap_poor(P[(foff + 2) + (long)(foff + 2) * a.ldp], a.max_depth_var);
    }
    int hit = 0;
    if (in_state && !poor)
      for (int e = lane; e < count; e += 64) hit |= ent[e].key == r.key ? 1 : 0;
    const int dup = __ballot(hit) != 0ull;
    const int d = lcmap_add_decide(in_state, poor, dup, count, a.map.map_max);
    n_add += d == LCMAP_ADD_ACCEPT; n_skip += d == LCMAP_ADD_SKIPPED; n_poor += d == LCMAP_ADD_POOR;
    n_dup += d == LCMAP_ADD_DUP; n_full += d == LCMAP_ADD_FULL;
    if (d == LCMAP_ADD_ACCEPT) {
      if (lane == 0) {
        const V3 Xs = lc_world_point(pose, *ft, a.groups[(long)filt * a.lay.n_groups + ref], a.invdepth);
        xivo_lcmap_entry& o = ent[count];
        o.key = r.key; o.Xs[0] = Xs.v[0]; o.Xs[1] = Xs.v[1]; o.Xs[2] = Xs.v[2];
      }
      if constexpr (EXT) {
        if (a.ext.cov) {
          __shared__ LcCovLds sCov;
          lc_point_cov(pose, *ft, a.groups[(long)filt * a.lay.n_groups + ref], a.invdepth, P, a.ldp, a.lay.group_begin + 6 * ref,
                       a.lay.feature_begin + 3 * ft->sind, sCov, lane, a.ext.cov + ((long)filt * a.map.map_max + count) * 6);
        }
      }
      ++count;
      __syncthreads();
    }
  }
  if (lane == 0) {
    a.map.count[filt] = count;
    xivo_lcmap_stats& st = a.map.stats[filt];
    st.added += n_add; st.skipped += n_skip; st.poor += n_poor; st.dup += n_dup; st.full += n_full;
  }
}

// the 12 columns a row pair touches: the observing pose's six from goff, then Wbc Tbc (15..20)
__device__ __forceinline__ int lc_col(int k, int goff) { return k < 6 ? goff + k : 15 + (k - 6); }

// match: 64 queries at a time, one lane each; a matching query's rank is the number of matching queries before it, counted in
// LDS (as the life-cycle kernels rank their candidates)
__global__ __launch_bounds__(64) void lcmap_match_kernel(LcMapCloseArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sFlag[64];
  const xivo_lcmap_entry* ent = a.map.entries + (long)filt * a.map.map_max;
  const int count = lcmap_count(a.map, filt);
  xivo_lcmap_match* list = a.matches + (long)filt * a.lc_max;
  const int q0 = lc_list_begin(a, filt), q1 = lc_list_end(a, filt);
  int base = 0;
  for (int c0 = q0; c0 < q1; c0 += 64) {
    const int q = c0 + lane;
    const int e = q < q1 ? lcmap_find(&ent[0].key, kKeyStride, count, a.queries[q].key) : -1;
    sFlag[lane] = e >= 0 ? 1 : 0;
    __syncthreads();
    int rank = base, tot = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) { tot += sFlag[j]; rank += sFlag[j] & ((j - lane) >> 31); }   // (the mask: all ones for j < lane)
    const int slot = e >= 0 ? lcmap_match_slot(rank, a.lc_max) : -1;
    if (slot >= 0) {
      const xivo_lcmap_query& qu = a.queries[q];
      xivo_lcmap_match& o = list[slot];
      o.entry = e; o.group_sind = qu.group_sind; o.xp[0] = qu.xp[0]; o.xp[1] = qu.xp[1]; o.gamma = 0.0; o.kept = 0; o.reserved = 0;
    }
    base += tot;
    __syncthreads();
  }
  const int n_matched = base < a.lc_max ? base : a.lc_max;
  if (lane < a.lc_max && lane >= n_matched) {
    xivo_lcmap_match& o = list[lane];
    o.entry = -1; o.group_sind = 0; o.xp[0] = 0.0; o.xp[1] = 0.0; o.gamma = 0.0; o.kept = 0; o.reserved = 0;
  }
  if (lane == 0) {
    xivo_lcmap_stats& st = a.map.stats[filt];
    st.queries += q1 - q0; st.matched += n_matched; st.surplus += base - n_matched;
  }
}

// rows, verify and the filter's decision: one lane per list position (the filled ones are the leading n_matched). EXT: the
// instantiation for the options of xivo_hip_lcmap_cov_config - the point's covariance in the gate and the whitening of the
// pairs that take part (a.ext.cov), one use per visit (a.ext.visit); either may be null. It starts from what lc_row_pair has
// stored, as the gate does. Without the options the first instantiation runs, whose code is what it was before they existed.
template <bool EXT>
__global__ __launch_bounds__(64) void lcmap_close_kernel(LcMapCloseArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sKept[64];
  int *sFresh = nullptr, *sEntry = nullptr, *sUsed = nullptr;
  if constexpr (EXT) {
    __shared__ int sExt[3][64];
    sFresh = sExt[0]; sEntry = sExt[1]; sUsed = sExt[2];
  }
  __shared__ double sH[64][25];                          // (odd row length: the lanes' rows fall in different banks)
  const xivo_lcmap_entry* ent = a.map.entries + (long)filt * a.map.map_max;
  const int count = lcmap_count(a.map, filt);
  xivo_lcmap_match* list = a.matches + (long)filt * a.lc_max;
  const int my_entry = lane < a.lc_max ? list[lane].entry : -1;
  const int n_matched = __popcll(__ballot(my_entry >= 0 && my_entry < count));
  double* H = a.H + (long)filt * a.strideH;
  double* inn = a.inn + (long)filt * a.strideV;
  double* dR = a.diagR + (long)filt * a.strideV;
  const int r0 = 2 * lane;
  int kept = 0, goff = 0;
  int used_now = 0, resting = 0, bad_cov = 0, filled = 0;   // (EXT)
  double w00 = 1.0, w10 = 0.0, w11 = 1.0;                    // (EXT) R_e = L L^T, L = [w00 0; w10 w11]
  if (lane < n_matched && my_entry >= 0 && my_entry < count) {   // (the second test: a list never has a gap, but is an address)
    const xivo_lcmap_match mt = list[lane];
    const xivo_pose_in& pose = a.poses[filt];
    const xivo_lcmap_entry& en = ent[mt.entry];
    const V3 Xs{{en.Xs[0], en.Xs[1], en.Xs[2]}};
    const bool body = mt.group_sind < 0;                 // observed by the body pose itself: columns 0..5 (Wsb, Tsb)
    const double *gR = pose.Rsb, *gT = pose.Tsb;
    if (!body) {
      const xivo_group_in& g = a.groups[(long)filt * a.lay.n_groups + mt.group_sind];
      gR = g.Rsb; gT = g.Tsb; goff = a.lay.group_begin + 6 * mt.group_sind;
    }
    lc_row_pair(Xs, gR, gT, goff, pose, a.cam, a.cl.cam_begin, a.cl.cam_dim, mt.xp, a.Rlc, H, a.ldh, r0, inn, dR);
    // gamma = r^T (H_i P H_i^T + Rlc I)^-1 r over the 12 columns of the pair (Estimator::MHGating's 2 x 2 Cholesky)
    const double* P = a.P + (long)filt * a.strideP;
    double* h = sH[lane];                                // the pair's 2 x 12 block, row-major (LDS: indexed by a loop counter)
#pragma unroll 1
    for (int k = 0; k < 12; ++k) {
      const long c = lc_col(k, goff);
      h[k] = H[r0 + c * a.ldh]; h[12 + k] = H[r0 + 1 + c * a.ldh];
    }
    double s00 = 0.0, s10 = 0.0, s11 = 0.0;
#pragma unroll 1
    for (int j = 0; j < 12; ++j) {                       // column j of the sub-block of P under the pair's columns
      const double* Pc = P + (long)lc_col(j, goff) * a.ldp;
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const double p = Pc[lc_col(k, goff)];
        t0 += h[k] * p; t1 += h[12 + k] * p;
      }
      s00 += t0 * h[j]; s10 += t1 * h[j]; s11 += t1 * h[12 + j];
    }
    int ok_cov = 1;
    if constexpr (EXT) {
      filled = 1;
      if (a.ext.visit) {
        const int* v = a.ext.visit + ((long)filt * a.map.map_max + mt.entry) * 2;
        used_now = lcmap_used_now(v[0], v[1], a.ext.t, a.ext.gap);
        resting = lcmap_resting(a.ext.gap, used_now);
      }
    }
    if (EXT && a.ext.cov) {
      // R_e = Rlc I + H_T Sigma H_T^T, H_T = d xp / d Tsb: positions 3..5 of the pair's block (d xp / d Xs = -H_T)
      const double* sg = a.ext.cov + ((long)filt * a.map.map_max + mt.entry) * 6;
      // (each entry rounded once, lcmap_quad3: a plain sum of the nine products loses what kappa_2(R_e) then multiplies)
      const double C[3][3] = {{sg[0], sg[1], sg[2]}, {sg[1], sg[3], sg[4]}, {sg[2], sg[4], sg[5]}};
      const double ha[3] = {h[3], h[4], h[5]}, hb[3] = {h[15], h[16], h[17]};
      const double e00 = a.Rlc + lcmap_quad3(C, ha, ha), e10 = lcmap_quad3(C, ha, hb), e11 = a.Rlc + lcmap_quad3(C, hb, hb);
      w00 = sqrt(e00); w10 = e10 / w00;
      const double d11 = e11 - w10 * w10;
      w11 = sqrt(d11);
      ok_cov = e00 > 0.0 && d11 > 0.0;                   // (a pair that fails is not kept: its factors are never used)
      bad_cov = !ok_cov;
      s00 += e00; s10 += e10; s11 += e11;
    } else {
      s00 += a.Rlc; s11 += a.Rlc;
    }
    const double l10 = s10 / sqrt(s00);
    const int ok = s00 > 0.0 && (s11 - l10 * l10) > 0.0 && ok_cov;
    double gamma = ok ? mh_dist_2x2(s00, s10, s11, inn[r0], inn[r0 + 1]) : -1.0;
    kept = lcmap_kept(ok, gamma, a.chi2);
    if (!lcmap_gamma_finite(gamma)) gamma = -1.0;        // (a NaN or inf pixel: shown as a failed pivot is)
    list[lane].gamma = gamma; list[lane].kept = kept;
    if constexpr (EXT) list[lane].reserved = resting;
  }
  sKept[lane] = kept;
  if constexpr (EXT) { sFresh[lane] = kept && !resting; sEntry[lane] = filled ? my_entry : -1; }
  __syncthreads();
  int n_kept = 0;
  for (int j = 0; j < n_matched; ++j) n_kept += sKept[j];
  int frame, neutral;
  if constexpr (EXT) {
    int n_fresh = 0;
    for (int j = 0; j < n_matched; ++j) n_fresh += sFresh[j];
    frame = lcmap_frame_decide_visit(n_matched, n_kept, n_fresh, a.min_matches);
    neutral = lcmap_pair_neutral_visit(frame, lane, n_matched, kept, resting);
    if (a.ext.cov && filled && !neutral) {               // the pair takes part: L^-1 times its rows and innovation, diagR = 1
#pragma unroll 1
      for (int k = 0; k < 12; ++k) {
        const long c = lc_col(k, goff);
        const double x0 = H[r0 + c * a.ldh] / w00;
        H[r0 + c * a.ldh] = x0; H[r0 + 1 + c * a.ldh] = (H[r0 + 1 + c * a.ldh] - w10 * x0) / w11;
      }
      const double y0 = inn[r0] / w00;
      inn[r0] = y0; inn[r0 + 1] = (inn[r0 + 1] - w10 * y0) / w11;
      dR[r0] = 1.0; dR[r0 + 1] = 1.0;
    }
    if (a.ext.visit) {                                   // (a uniform branch around the barrier)
      sUsed[lane] = filled ? lcmap_used_next(used_now, frame, kept, resting) : 0;
      __syncthreads();
      if (filled) {                                      // a key that fills several positions: used if any of them used it
        int used = 0, first = 1;
        for (int j = 0; j < n_matched; ++j)
          if (sEntry[j] == my_entry) { used |= sUsed[j]; first &= j >= lane; }
        if (first) {
          int* v = a.ext.visit + ((long)filt * a.map.map_max + my_entry) * 2;
          v[0] = a.ext.t; v[1] = used;
        }
      }
    }
    const int n_bad = __popcll(__ballot(bad_cov));
    if (lane == 0) {
      xivo_lcmap_cov_stats& cs = a.ext.stats[filt];
      cs.resting += n_kept - n_fresh; cs.rested_frames += frame == LCMAP_FRAME_RESTED ? 1 : 0; cs.bad_cov += n_bad;
    }
  } else {
    frame = lcmap_frame_decide(n_matched, n_kept, a.min_matches);
    neutral = lcmap_pair_neutral(frame, lane, n_matched, kept);
  }
  if (lane < a.lc_max && neutral) {
    if (lane < n_matched) {
#pragma unroll 1
      for (int k = 0; k < 12; ++k) {
        const long c = lc_col(k, goff);
        H[r0 + c * a.ldh] = 0.0; H[r0 + 1 + c * a.ldh] = 0.0;
      }
    }
    inn[r0] = 0.0; inn[r0 + 1] = 0.0; dR[r0] = 1.0; dR[r0 + 1] = 1.0;
  }
  if (lane == 0) {
    a.closing[filt] = frame == LCMAP_FRAME_CLOSED ? 1 : 0;
    xivo_lcmap_stats& st = a.map.stats[filt];
    st.gated += n_matched - n_kept;
    st.short_frames += frame == LCMAP_FRAME_SHORT ? 1 : 0; st.closed_frames += frame == LCMAP_FRAME_CLOSED ? 1 : 0;
  }
}

// The queries of a frame of the device life cycle (SequenceRunner._lc_close on the host): 64 slots at a time, one lane each; a
// yielding slot's rank is the number of yielding slots before it, counted in LDS as lcmap_match_kernel ranks its matches. Lane 0
// also copies the filter's update status to where the second update does not write.
__global__ __launch_bounds__(64) void lclife_query_kernel(LcLifeQueryArgs a) {
  const int filt = blockIdx.x, lane = threadIdx.x;
  if (filt >= a.batch) return;
  __shared__ int sFlag[64];
  const long long* fid = a.feat_id + (long)filt * a.slot_ld;
  const long long* key = a.feat_key + (long)filt * a.slot_ld;
  const unsigned char* tracked = a.tracked + (long)filt * a.slot_ld;
  const unsigned char* mask = a.mask + (long)filt * a.mask_ld;
  const xivo_feat_in* feats = a.feats + (long)filt * a.Fmax;
  int base = 0;
  for (int j0 = 0; j0 < a.F; j0 += 64) {
    const int j = j0 + lane;
    const int yes = j < a.F ? lclife_queries(fid[j], mask[j], tracked[j]) : 0;
    sFlag[lane] = yes;
    __syncthreads();
    int rank = base, tot = 0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) { tot += sFlag[i]; rank += sFlag[i] & ((i - lane) >> 31); }   // (the mask: all ones for i < lane)
    if (yes) {   // rank < the slots before j <= F - 1 < slot_ld: inside the filter's row
      xivo_lcmap_query& q = a.queries[lclife_list_pos(filt, a.slot_ld, rank)];
      q.b = filt; q.group_sind = -1; q.key = key[j]; q.xp[0] = feats[j].xp[0]; q.xp[1] = feats[j].xp[1];
    }
    base += tot;
    __syncthreads();
  }
  if (lane == 0) { a.n_queries[filt] = base; a.status_out[filt] = a.status[filt]; }
}

}  // namespace

#define CHECK_LAUNCH() return (int)hipGetLastError()

int launch_lcmap_add(const LcMapAddArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  if (a.ext.on()) hipLaunchKernelGGL(lcmap_add_kernel<true>, dim3(a.batch), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(lcmap_add_kernel<false>, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_lclife_queries(const LcLifeQueryArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(lclife_query_kernel, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}
int launch_lcmap_close(const LcMapCloseArgs& a, hipStream_t s) {
  if (a.batch <= 0) return 0;
  hipLaunchKernelGGL(lcmap_match_kernel, dim3(a.batch), dim3(64), 0, s, a);
  if (hipError_t e = hipGetLastError()) return (int)e;
  if (a.ext.on()) hipLaunchKernelGGL(lcmap_close_kernel<true>, dim3(a.batch), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(lcmap_close_kernel<false>, dim3(a.batch), dim3(64), 0, s, a);
  CHECK_LAUNCH();
}

}  // namespace xivo_hip
