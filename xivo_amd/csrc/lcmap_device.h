// The integer rules of the resident landmark map (xivo_hip_lcmap_*, include/xivo_hip.h): what becomes of an add record, which
// place a matching query takes in a filter's match list, whether a filter closes - and the one piece of its arithmetic that
// needs care, an entry of H_T Sigma H_T^T (lcmap_quad3). Plain functions of integers and doubles, shared by the
// kernels (lcmap_kernels.hip) and by a host program that holds them against a restatement (tests/lcmap_driver.cpp): this file
// includes no project header and takes HIP's only under __HIPCC__.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LCMAP_HD __host__ __device__ __forceinline__
#else
#define LCMAP_HD inline
#endif

namespace xivo_hip {

// ---- add (DiscardFeatures -> Mapper::AddFeature, src/mapper.cpp:158-222 with merge_features = false, :189-191)
enum { LCMAP_ADD_ACCEPT = 0, LCMAP_ADD_SKIPPED = 1, LCMAP_ADD_POOR = 2, LCMAP_ADD_DUP = 3, LCMAP_ADD_FULL = 4 };

// One record, the tests in this order: not in the state (or a negative key, which no query can ever match) - skipped; depth
// variance above the bound - poor; key stored already (in the map or by an earlier record of the call) - dup, the first
// estimate stays; no room - full, nothing is evicted; else it takes position `count`.
LCMAP_HD int lcmap_add_decide(int in_state, int poor, int dup, int count, int map_max) {
  if (!in_state) return LCMAP_ADD_SKIPPED;
  if (poor) return LCMAP_ADD_POOR;
  if (dup) return LCMAP_ADD_DUP;
  if (count >= map_max) return LCMAP_ADD_FULL;
  return LCMAP_ADD_ACCEPT;
}
// the depth-variance test: var = P(foff + 2, foff + 2); max_depth_var = 0 means no test, equality keeps the record
LCMAP_HD int lcmap_poor(double var, double max_depth_var) { return max_depth_var > 0.0 && var > max_depth_var; }

// the position of `key` among keys[0, count), -1: none (a negative key matches nothing)
LCMAP_HD int lcmap_find(const long long* keys, long stride, int count, long long key) {
  if (key < 0) return -1;
  for (int i = 0; i < count; ++i)
    if (keys[(long)i * stride] == key) return i;
  return -1;
}

// ---- match: the matching query that has `rank` matching queries before it in query order takes list position `rank` while
// there is room, the others are surplus (-1)
LCMAP_HD int lcmap_match_slot(int rank, int lc_max) { return rank < lc_max ? rank : -1; }

// ---- verify (stands in for pnp_ransac's inlier count, src/mapper.cpp:411-415)
// gate of one match: a non-positive pivot of the 2 x 2 Cholesky, a gamma that is not finite (a NaN or inf pixel or stored
// point: whatever chi2 is, 0 included - as everywhere else here NaN is "no candidate"), or gamma above chi2 (0: no gate;
// equality keeps) - not kept. (gamma - gamma is 0 for a finite gamma alone: no <math.h> in this header)
LCMAP_HD int lcmap_gamma_finite(double gamma) { return gamma - gamma == 0.0; }
LCMAP_HD int lcmap_kept(int pivots_ok, double gamma, double chi2) {
  return pivots_ok && lcmap_gamma_finite(gamma) && !(chi2 > 0.0 && gamma > chi2);
}

enum { LCMAP_FRAME_NONE = 0, LCMAP_FRAME_SHORT = 1, LCMAP_FRAME_CLOSED = 2 };
// a filter with n_matched list positions filled of which n_kept passed the gate
LCMAP_HD int lcmap_frame_decide(int n_matched, int n_kept, int min_matches) {
  if (n_kept >= min_matches && n_kept > 0) return LCMAP_FRAME_CLOSED;
  return n_matched > 0 ? LCMAP_FRAME_SHORT : LCMAP_FRAME_NONE;
}
// is the row pair of list position m neutral (H = 0, inn = 0, diagR = 1)?
LCMAP_HD int lcmap_pair_neutral(int frame, int m, int n_matched, int kept) {
  return frame != LCMAP_FRAME_CLOSED || m >= n_matched || !kept;
}

// ---- the point's covariance in the gate and the whitening (xivo_hip_lcmap_cov_config, point_cov): an entry of H_T Sigma H_T^T
// a^T C b for a symmetric 3 x 3 C. The nine products a_j C_ij b_i are of size |C||a||b| and cancel where C is nearly rank one
// and a or b nearly orthogonal to its large direction; summed plainly they leave 8 - 15 ulp in the entry, which kappa_2(R_e)
// multiplies in gamma and in the whitened rows. Here every product is error-free (fma) and the sum runs in two doubles
// (TwoSum): the entry is rounded once. No contraction inside - the roundings are the algorithm.
LCMAP_HD double lcmap_quad3(const double (&C)[3][3], const double (&a)[3], const double (&b)[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double sh = 0.0, sl = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double ph = C[i][j] * a[j], pl = __builtin_fma(C[i][j], a[j], -ph);
      const double qh = ph * b[i], ql = __builtin_fma(ph, b[i], -qh) + pl * b[i];
      const double t = sh + qh, v = t - sh;
      sl += ((sh - (t - v)) + (qh - v)) + ql;
      sh = t;
    }
  return sh + sl;
}

// ---- one use per visit (xivo_hip_lcmap_cov_config, revisit_gap): an entry keeps {last_seen, used}, t numbers the close
// calls from 1. With gap = 0 nothing ever rests and the three rules below are the two above.
enum { LCMAP_FRAME_RESTED = 3 };
// has the entry closed a loop in the visit that call t falls into? A visit ends after gap calls without a match of the entry:
// t - last_seen == gap is still the same visit, gap + 1 a new one; last_seen = 0 is "never seen"
LCMAP_HD int lcmap_used_now(int last_seen, int used, int t, int gap) { return (last_seen > 0 && t - last_seen <= gap) ? used : 0; }
LCMAP_HD int lcmap_resting(int gap, int used_now) { return gap > 0 && used_now; }
// n_kept counts the resting matches too (they verify the place), n_fresh the kept ones that do not rest
LCMAP_HD int lcmap_frame_decide_visit(int n_matched, int n_kept, int n_fresh, int min_matches) {
  const int frame = lcmap_frame_decide(n_matched, n_kept, min_matches);
  return frame == LCMAP_FRAME_CLOSED && n_fresh == 0 ? LCMAP_FRAME_RESTED : frame;
}
LCMAP_HD int lcmap_pair_neutral_visit(int frame, int m, int n_matched, int kept, int resting) {
  return lcmap_pair_neutral(frame, m, n_matched, kept) || resting;
}
// `used` of a matched entry after the call (its last_seen becomes t)
LCMAP_HD int lcmap_used_next(int used_now, int frame, int kept, int resting) {
  return used_now || (frame == LCMAP_FRAME_CLOSED && kept && !resting);
}

}  // namespace xivo_hip
