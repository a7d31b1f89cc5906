// The closed-form rigid alignment of the trajectory score (score_kernels.hip): the rotation R that maximises trace(R^T H) for a
// 3 x 3 cross-covariance H (Horn / Kabsch), through a register SVD. Plain fp64 C++ on fixed-size arrays, host and device: a
// host compiler takes the header alone, and tests/score_kabsch_driver.cpp (tests/test_score_kabsch_cpu.py) runs its
// degenerate branches - H = 0, rank 1, a non-finite H, the axis fallback of score_orth_unit - without a GPU.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XIVO_SCORE_HD __host__ __device__ __forceinline__
#else
#define XIVO_SCORE_HD inline
#endif

namespace xivo_hip {

constexpr int kScoreJacobiSweeps = 12;        // a 3 x 3 converges in four or five; the skip test makes the rest free
constexpr double kScoreRankTol = 1e-12;       // sv[1] <= tol sv[0]: the rotation about the first axis is not determined

XIVO_SCORE_HD void score_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
XIVO_SCORE_HD double score_dot(const double a[3], const double b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
// a <- a / |a|; false (a untouched) when |a| is zero or not finite
XIVO_SCORE_HD bool score_unit(double a[3]) {
  const double n = sqrt(score_dot(a, a));
  if (!(n > 0.0 && n < INFINITY)) return false;
  a[0] /= n; a[1] /= n; a[2] /= n;
  return true;
}
// b <- the unit vector of b - (a . b) a for a unit a; when nothing is left of b, of the coordinate axis a is furthest from
XIVO_SCORE_HD void score_orth_unit(const double a[3], double b[3]) {
  for (int pass = 0; pass < 2; ++pass) {       // twice is enough (Kahan): the second pass removes what the first one's rounding left
    const double d = score_dot(a, b);
    b[0] -= d * a[0]; b[1] -= d * a[1]; b[2] -= d * a[2];
    if (pass == 0 && !score_unit(b)) break;
  }
  if (score_unit(b) && fabs(score_dot(a, b)) < 0x1p-40) return;
  const int k = fabs(a[0]) <= fabs(a[1]) ? (fabs(a[0]) <= fabs(a[2]) ? 0 : 2) : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
  b[0] = b[1] = b[2] = 0.0; b[k] = 1.0;
  const double d = a[k];
  b[0] -= d * a[0]; b[1] -= d * a[1]; b[2] -= d * a[2];
  score_unit(b);
}

// H (row-major h[i][j]) = U diag(sv) V^T by one-sided (Hestenes) Jacobi on the columns of H V - no H^T H is formed, so small
// singular values keep their relative accuracy. sv descending. R = U diag(1, 1, det(U V^T)) V^T, written without the third
// columns: with u2' = u0 x u1 and v2' = v0 x v1 the corrected product is u0 v0^T + u1 v1^T + u2' v2'^T whatever the two
// determinants are, so the column of the smallest singular value - the one without a direction when the points are coplanar -
// is never normalised. Rank <= 1 (returns 1, the flag of xivo_traj_score): u1 is whatever unit vector the data leave, or an
// axis; R is a rotation either way. H = 0: R = I.
XIVO_SCORE_HD int score_kabsch(const double h[3][3], double R[3][3], double sv[3]) {
  double A[3][3], V[3][3];
  double mx = 0.0;
  bool finite = true;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { mx = fmax(mx, fabs(h[i][j])); finite = finite && fabs(h[i][j]) < INFINITY; }
  int e = 0;
  if (finite && mx > 0.0) frexp(mx, &e);       // an exact power-of-two scaling: the squared column norms neither overflow nor vanish
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { A[i][j] = finite ? ldexp(h[i][j], -e) : 0.0; V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < kScoreJacobiSweeps; ++sweep) {
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < 3; ++i) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
        if (!(fabs(ga) > 1e-300 && fabs(ga) > 1e-18 * sqrt(al * be))) continue;   // orthogonal to working precision
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
        for (int i = 0; i < 3; ++i) {
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
  }
  // columns by descending norm: a fixed three-exchange network on (norm, column of A, column of V)
  double nr[3];
  for (int j = 0; j < 3; ++j) nr[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  const int net[3][2] = {{0, 1}, {1, 2}, {0, 1}};
  for (int k = 0; k < 3; ++k) {
    const int p = net[k][0], q = net[k][1];
    if (nr[p] >= nr[q]) continue;
    double t = nr[p]; nr[p] = nr[q]; nr[q] = t;
    for (int i = 0; i < 3; ++i) {
      t = A[i][p]; A[i][p] = A[i][q]; A[i][q] = t;
      t = V[i][p]; V[i][p] = V[i][q]; V[i][q] = t;
    }
  }
  for (int j = 0; j < 3; ++j) sv[j] = ldexp(nr[j], e);
  const int undetermined = !(nr[1] > kScoreRankTol * nr[0]);
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
  for (int i = 0; i < 3; ++i) { u0[i] = A[i][0]; u1[i] = A[i][1]; v0[i] = V[i][0]; v1[i] = V[i][1]; }
  score_unit(v0);                              // V is a product of plane rotations: orthonormal to a few eps; made so to one
  score_orth_unit(v0, v1);
  if (!score_unit(u0)) { for (int i = 0; i < 3; ++i) { u0[i] = v0[i]; u1[i] = v1[i]; } }   // H = 0: R = I
  else score_orth_unit(u0, u1);
  score_cross(u0, u1, u2);
  score_cross(v0, v1, v2);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = u0[i] * v0[j] + u1[i] * v1[j] + u2[i] * v2[j];
  // the six normalisations above leave R^T R - I = E of a few eps; one Newton step of the polar iteration, R <- R (I - E / 2),
  // with E from fused multiply-adds (one rounding per entry), takes it to the rounding of R's own entries
  double E[3][3], P[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[i][j] = fma(R[0][i], R[0][j], fma(R[1][i], R[1][j], fma(R[2][i], R[2][j], i == j ? -1.0 : 0.0)));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) P[i][j] = R[i][j] - 0.5 * (R[i][0] * E[0][j] + R[i][1] * E[1][j] + R[i][2] * E[2][j]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = P[i][j];
  return undetermined;
}

}  // namespace xivo_hip
