// Two-view triangulation of one track (Feature::Triangulate, src/feature.cpp:686-751) with the five triangulators of
// src/helpers.cpp:103-371 (paths relative to the reference tree), for pool_kernels.hip. fp64 throughout, rounded to float at
// exactly the points where the reference holds a float: a0 / a1 (L1Angular), lambda0 / lambda1 (check_cheirality), theta0 /
// theta1 / beta (check_angular_reprojection / check_parallax) and the two thresholds; those comparisons are made in float.
// Vector arithmetic follows Eigen's association order (dot = (a0 b0 + a1 b1) + a2 b2, cross, normalize = v / sqrt(|v|^2)),
// without contraction into fused multiply-adds: the branch decisions hang on last bits (L1Angular's unmodified ray gives
// acos of 1 +- 1 ulp, NaN or 0, and std::max lets a NaN theta0 pass), so the device computes the plain IEEE sequence a
// restatement can follow (every function opens with the pragma: it holds for its own body only).
#pragma once
#include "xivo_hip.h"

namespace xivo_hip {
namespace tri {

struct T3 { double v[3]; };

__device__ __forceinline__ T3 t3(double a, double b, double c) {
#pragma clang fp contract(off)
  return T3{{a, b, c}};
}
__device__ __forceinline__ double dot(const T3& a, const T3& b) {
#pragma clang fp contract(off)
  return (a.v[0] * b.v[0] + a.v[1] * b.v[1]) + a.v[2] * b.v[2];
}
__device__ __forceinline__ double norm(const T3& a) {
#pragma clang fp contract(off)
  return sqrt(dot(a, a));
}
__device__ __forceinline__ T3 cross(const T3& a, const T3& b) {
#pragma clang fp contract(off)
  return t3(a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]);
}
__device__ __forceinline__ T3 scale(const T3& a, double s) {
#pragma clang fp contract(off)
  return t3(a.v[0] * s, a.v[1] * s, a.v[2] * s);
}
__device__ __forceinline__ T3 divs(const T3& a, double s) {
#pragma clang fp contract(off)
  return t3(a.v[0] / s, a.v[1] / s, a.v[2] / s);
}
__device__ __forceinline__ T3 add(const T3& a, const T3& b) {
#pragma clang fp contract(off)
  return t3(a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]);
}
__device__ __forceinline__ T3 sub(const T3& a, const T3& b) {
#pragma clang fp contract(off)
  return t3(a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]);
}
// Eigen normalize(): divide by the norm when the squared norm is > 0
__device__ __forceinline__ T3 normalized(const T3& a) {
#pragma clang fp contract(off)
  const double z = dot(a, a);
  return z > 0.0 ? divs(a, sqrt(z)) : a;
}
// R (column-major 9) times x, R^T times x
__device__ __forceinline__ T3 mulv(const double* R, const T3& x) {
#pragma clang fp contract(off)
  return t3((R[0] * x.v[0] + R[3] * x.v[1]) + R[6] * x.v[2], (R[1] * x.v[0] + R[4] * x.v[1]) + R[7] * x.v[2],
            (R[2] * x.v[0] + R[5] * x.v[1]) + R[8] * x.v[2]);
}
__device__ __forceinline__ T3 mulvt(const double* R, const T3& x) {
#pragma clang fp contract(off)
  return t3((R[0] * x.v[0] + R[1] * x.v[1]) + R[2] * x.v[2], (R[3] * x.v[0] + R[4] * x.v[1]) + R[5] * x.v[2],
            (R[6] * x.v[0] + R[7] * x.v[1]) + R[8] * x.v[2]);
}

// check_cheirality (helpers.cpp:327-341)
__device__ __forceinline__ bool check_cheirality(const T3& z, const T3& t, const T3& f1p, const T3& Rf0p) {
#pragma clang fp contract(off)
  const double zn = norm(z), zz = zn * zn;   // pow(z.norm(), 2)
  const float lambda0 = (float)(dot(z, cross(t, f1p)) / zz);
  const float lambda1 = (float)(dot(z, cross(t, Rf0p)) / zz);
  return !(lambda0 <= 0.0f || lambda1 <= 0.0f);
}
// check_angular_reprojection (helpers.cpp:344-357); std::max(theta0, theta1) = theta0 < theta1 ? theta1 : theta0
__device__ __forceinline__ bool check_angular_reprojection(const T3& Rf0, const T3& Rf0p, const T3& f1, const T3& f1p,
                                                           float thresh) {
#pragma clang fp contract(off)
  const float theta0 = (float)acos(dot(Rf0, Rf0p) / (norm(Rf0) * norm(Rf0p)));
  const float theta1 = (float)acos(dot(f1, f1p) / (norm(f1) * norm(f1p)));
  const float max_theta = theta0 < theta1 ? theta1 : theta0;
  return !(max_theta > thresh);
}
// check_parallax (helpers.cpp:359-371)
__device__ __forceinline__ bool check_parallax(const T3& Rf0p, const T3& f1p, float thresh) {
#pragma clang fp contract(off)
  const float beta = (float)acos(dot(f1p, Rf0p) / (norm(f1p) * norm(Rf0p)));
  return !(beta < thresh);
}

// The common tail of the three angular methods (helpers.cpp:206-222 and the same lines of L2 / Linf): the point from the
// corrected rays m0' (= Rf0'), m1' (= f1'), back into frame 0, then the three checks
__device__ __forceinline__ bool angular_tail(const double* R01, const T3& t01, const T3& t10, const T3& m0, const T3& m1,
                                             const T3& m0p, const T3& m1p, float max_theta, float beta, double X[3]) {
#pragma clang fp contract(off)
  const T3 z = cross(m1p, m0p);
  const double zn = norm(z);
  const T3 Xl = scale(m1p, dot(z, cross(t10, m0p)) / (zn * zn));
  const T3 Xw = add(mulv(R01, Xl), t01);
  X[0] = Xw.v[0]; X[1] = Xw.v[1]; X[2] = Xw.v[2];
  return check_cheirality(z, t10, m1p, m0p) && check_angular_reprojection(m0, m0p, m1, m1p, max_theta) &&
         check_parallax(m0p, m1p, beta);
}

// direct_linear_transform_svd (helpers.cpp:103-131): the right singular vector of the smallest singular value of the 4x4 A
// by one-sided (Hestenes) Jacobi: column pairs of A V are rotated until orthogonal; V accumulates the rotations.
constexpr int kJacobiSweeps = 10;
__device__ __forceinline__ bool dlt_svd(const double* R, const T3& t, const T3& f1, const T3& f2, double X[3]) {
#pragma clang fp contract(off)
  // P1 = [I | 0], P2 = [R^T | -R^T t]; rows of A (row-major here) as coded
  double P2[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) P2[i][j] = R[i * 3 + j];    // R^T(i, j) = R(j, i)
  }
  const T3 Rtt = mulvt(R, t);
  P2[0][3] = -Rtt.v[0]; P2[1][3] = -Rtt.v[1]; P2[2][3] = -Rtt.v[2];
  const double P1[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
  double A[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[0][j] = f1.v[0] * P1[2][j] - f1.v[2] * P1[0][j];
    A[1][j] = f1.v[1] * P1[2][j] - f1.v[2] * P1[1][j];
    A[2][j] = f2.v[0] * P2[2][j] - f2.v[2] * P2[0][j];
    A[3][j] = f2.v[1] * P2[2][j] - f2.v[2] * P2[1][j];
  }
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
        if (!(fabs(ga) > 1e-300 && fabs(ga) > 1e-18 * sqrt(al * be))) continue;   // already orthogonal to working precision
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
  }
  // the column of A V with the smallest norm is sigma_min u_min: its V column is the null vector (V(:, 3) of Eigen's order)
  int k = 0;
  double best = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s2 += A[i][j] * A[i][j];
    if (j == 0 || s2 < best) { best = s2; k = j; }
  }
  double v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = V[i][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (k == j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = V[i][j];
    }
  X[0] = v[0] / v[3]; X[1] = v[1] / v[3]; X[2] = v[2] / v[3];
  return true;
}

// direct_linear_transform_avg (helpers.cpp:133-158); Eigen's closed-form 2x2 inverse
__device__ __forceinline__ bool dlt_avg(const double* R, const T3& t, const T3& f1, const T3& f2, double X[3]) {
#pragma clang fp contract(off)
  const T3 f2u = mulv(R, f2);
  const double b0 = dot(t, f1), b1 = dot(t, f2u);
  const double a00 = dot(f1, f1), a10 = dot(f1, f2u), a01 = -a10, a11 = -dot(f2u, f2u);
  const double idet = 1.0 / (a00 * a11 - a10 * a01);
  const double i00 = a11 * idet, i10 = -a10 * idet, i01 = -a01 * idet, i11 = a00 * idet;
  const double l0 = i00 * b0 + i01 * b1, l1 = i10 * b0 + i11 * b1;
  const T3 xm = scale(f1, l0), xn = add(t, scale(f2u, l1));
  const T3 s = add(xm, xn);
  X[0] = s.v[0] / 2.0; X[1] = s.v[1] / 2.0; X[2] = s.v[2] / 2.0;
  return true;
}

// L2Angular's n' = V.col(1) of B = A^T (I - t^ t^T) (helpers.cpp:248-261). B t^ = 0, so B's right singular vectors for its two
// non-zero singular values lie in the plane perpendicular to t^: with an orthonormal basis (e1, e2) of that plane, V.col(1) is
// the minor eigenvector of the 2x2 C = (B e_i . B e_j). Its sign is free: only n' n'^T enters m0' and m1'.
__device__ __forceinline__ T3 l2_normal(const T3& m0h, const T3& m1h, const T3& t) {
#pragma clang fp contract(off)
  const T3 th = divs(t, norm(t));
  double M[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = (i == j ? 1.0 : 0.0) - th.v[i] * th.v[j];
  T3 b0, b1;   // rows of B
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    b0.v[j] = (m0h.v[0] * M[0][j] + m0h.v[1] * M[1][j]) + m0h.v[2] * M[2][j];
    b1.v[j] = (m1h.v[0] * M[0][j] + m1h.v[1] * M[1][j]) + m1h.v[2] * M[2][j];
  }
  const double n0 = norm(b0), n1 = norm(b1);
  T3 e1;
  if (n0 >= n1 && n0 > 0.0) e1 = divs(b0, n0);
  else if (n1 > 0.0) e1 = divs(b1, n1);
  else {   // B = 0: every vector perpendicular to t^ is a right singular vector; take one
    const int i = fabs(th.v[0]) <= fabs(th.v[1]) ? (fabs(th.v[0]) <= fabs(th.v[2]) ? 0 : 2) : (fabs(th.v[1]) <= fabs(th.v[2]) ? 1 : 2);
    T3 u = t3(0.0, 0.0, 0.0);
    u.v[i] = 1.0;
    e1 = normalized(cross(th, u));
  }
  const T3 e2 = normalized(cross(th, e1));
  const double c01 = dot(b0, e1), c02 = dot(b0, e2), c11 = dot(b1, e1), c12 = dot(b1, e2);
  const double p = c01 * c01 + c11 * c11, q = c01 * c02 + c11 * c12, r = c02 * c02 + c12 * c12;
  const double th2 = 0.5 * atan2(2.0 * q, p - r);   // major direction (cos, sin); the minor one is (-sin, cos)
  const double cs = cos(th2), sn = sin(th2);
  return add(scale(e1, -sn), scale(e2, cs));
}

// One problem: returns the triangulator's value; X as the reference leaves it
__device__ __forceinline__ bool triangulate_one(const double* R12, const double* t12v, const double* xc1, const double* xc2,
                                                int method, float max_theta, float beta, double X[3]) {
#pragma clang fp contract(off)
  const T3 t12 = t3(t12v[0], t12v[1], t12v[2]);
  const T3 f0 = normalized(t3(xc1[0], xc1[1], 1.0)), f1 = normalized(t3(xc2[0], xc2[1], 1.0));
  if (method == XIVO_TRI_DLT_SVD) return dlt_svd(R12, t12, f0, f1, X);
  if (method == XIVO_TRI_DLT_AVG) return dlt_avg(R12, t12, f0, f1, X);
  // the angular methods (helpers.cpp:161-325): frame 0 = xc1's camera, R10 = R01^T, t10 = -R01^T t01
  const T3 Rtt = mulvt(R12, t12);
  const T3 t10 = t3(-Rtt.v[0], -Rtt.v[1], -Rtt.v[2]);
  const T3 m0 = mulvt(R12, f0), m1 = f1;
  T3 m0p, m1p;
  if (method == XIVO_TRI_L1) {
    const float a0 = (float)norm(cross(divs(m0, norm(m0)), t10));
    const float a1 = (float)norm(cross(divs(m1, norm(m1)), t10));
    if (a0 <= a1) {
      const T3 n1 = cross(m1, t10), nh = divs(n1, norm(n1));
      m0p = sub(m0, scale(nh, dot(m0, nh))); m1p = m1;
    } else {
      const T3 n0 = cross(m0, t10), nh = divs(n0, norm(n0));
      m0p = m0; m1p = sub(m1, scale(nh, dot(m1, nh)));
    }
  } else {
    const T3 m0h = divs(m0, norm(m0)), m1h = divs(m1, norm(m1));
    T3 np;
    if (method == XIVO_TRI_L2) {
      np = l2_normal(m0h, m1h, t10);
    } else {   // Linf: n' is NOT normalised, as coded (helpers.cpp:293-296)
      const T3 na = cross(add(m0h, m1h), t10), nb = cross(sub(m0h, m1h), t10);
      np = norm(na) >= norm(nb) ? na : nb;
    }
    m0p = sub(m0, scale(np, dot(m0, np))); m1p = sub(m1, scale(np, dot(m1, np)));
  }
  return angular_tail(R12, t12, t10, m0, m1, m0p, m1p, max_theta, beta, X);
}

// Feature::Triangulate's acceptance: the method's value and zmin <= z <= zmax (a NaN depth is rejected)
__device__ __forceinline__ bool triangulation_good(bool ret, const double X[3], const xivo_triangulate_opts& o) {
#pragma clang fp contract(off)
  return ret && X[2] >= o.zmin && X[2] <= o.zmax;
}

}  // namespace tri
}  // namespace xivo_hip
