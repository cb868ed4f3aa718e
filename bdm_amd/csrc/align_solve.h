// The closed-form similarity alignment of two paired point sets from their integer moments (align.hip, bdm_hip.h section 18): the
// fixed-point scale, the float64 moments, Horn's quaternion rotation through a cyclic Jacobi on the 4 x 4 matrix, scale,
// translation and the analytic mean squared residual.  Plain C++ (host and device) like normals_eig.h, so a host program can
// exercise the same arithmetic.  Everything is float64, one operation at a time: the file is compiled without FMA contraction, and
// float64 division and square root are correctly rounded on both sides, so tests/align_ref.py restates it bit for bit.
//
// Sweeps.  The Jacobi runs ALIGN_JACOBI_SWEEPS = 10 cyclic sweeps over the six pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  On the
// host test's cases (random, planar, collinear, single pair, near reflection) the off-diagonal norm is below 1e-17 of the largest
// eigenvalue after six to eight sweeps (quadratic convergence; a rotation whose a_pq is already zero is skipped); ten leaves two spare
// and costs nothing beside the search.  A fixed count keeps the result a function of the moments alone.
//
// mse is ANALYTIC: the mean squared residual of the pairs under the new transform written in the moments,
// s^2 Xvar - 2 s tr + Yvar, clamped at zero -- not a second pass over the points.  It is what pytorch3d calls rmse (no root is taken).
// On clouds whose residual is zero it is rounding noise of the order 1e-16 of the variance, of either sign before the clamp.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BDM_ALIGN_HD __host__ __device__ __forceinline__
#else
#define BDM_ALIGN_HD inline
#endif

namespace bdm {

constexpr int ALIGN_JACOBI_SWEEPS = 10;
constexpr int ALIGN_MOMENTS = 18;   // W, Sx[3], Sy[3], Sxy[9] (a-major), Sxx, Syy

// 2^k as a double, -1022 <= k <= 1023
BDM_ALIGN_HD double align_pow2(int k) {
  const uint64_t u = (uint64_t)(1023 + k) << 52;
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}

// smallest k with 2^k >= n (n >= 1)
BDM_ALIGN_HD int align_ceil_log2(long long n) {
  int k = 0;
  while ((1ll << k) < n) ++k;
  return k;
}

// the fixed-point exponent e of an entry: amax_bits = the float bits of the largest |coordinate| of its finite rows, p = its source count
BDM_ALIGN_HD int align_scale_exp(unsigned int amax_bits, long long p) {
  const int field = (int)((amax_bits >> 23) & 0xffu);
  const int E = (field < 1 ? 1 : field) - 127;   // zero and denormals: -126
  const int half = (62 - align_ceil_log2(p < 1 ? 1 : p)) / 2;
  const int bits = half < 24 ? half : 24;
  return bits - 1 - E;
}

// q(c) = rint(c 2^e) as an integer; c finite, |c| <= amax, so |q| <= 2^bits
BDM_ALIGN_HD long long align_quantise(float c, double two_e) { return (long long)rint((double)c * two_e); }

struct AlignSolution {
  double R[9], T[3], s, mse;
};

// One rotation in the (p, q) plane that zeroes a[p][q]: jacobi_rotate's formulas (normals_eig.h) in float64 on a 4 x 4.
BDM_ALIGN_HD void align_jacobi_rotate(double (&a)[4][4], double (&v)[4][4], const int p, const int q) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r) {
    if (r == p || r == q) continue;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
    a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 4; ++i) {
    const double vip = v[i][p], viq = v[i][q];
    v[i][p] = vip - s * (viq + tau * vip);
    v[i][q] = viq + s * (vip - tau * viq);
  }
}

// m: the 18 integer moments of the matched pairs (m[0] = W >= 1), e: the entry's fixed-point exponent.
BDM_ALIGN_HD void align_solve(const long long (&m)[ALIGN_MOMENTS], const int e, const bool estimate_scale, const double eps,
                              AlignSolution &out) {
  const double inv1 = align_pow2(-e), inv2 = align_pow2(-2 * e), W = (double)m[0];
  double mx[3], my[3], M[3][3];
  for (int a = 0; a < 3; ++a) {
    mx[a] = ((double)m[1 + a] * inv1) / W;
    my[a] = ((double)m[4 + a] * inv1) / W;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[a][b] = ((double)m[7 + 3 * a + b] * inv2) / W - mx[a] * my[b];
  const double xvar = ((double)m[16] * inv2) / W - ((mx[0] * mx[0] + mx[1] * mx[1]) + mx[2] * mx[2]);
  const double yvar = ((double)m[17] * inv2) / W - ((my[0] * my[0] + my[1] * my[1]) + my[2] * my[2]);

  double n[4][4], v[4][4];
  n[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  n[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  n[2][2] = (M[1][1] - M[0][0]) - M[2][2];
  n[3][3] = (M[2][2] - M[0][0]) - M[1][1];
  n[0][1] = n[1][0] = M[1][2] - M[2][1];
  n[0][2] = n[2][0] = M[2][0] - M[0][2];
  n[0][3] = n[3][0] = M[0][1] - M[1][0];
  n[1][2] = n[2][1] = M[0][1] + M[1][0];
  n[1][3] = n[3][1] = M[2][0] + M[0][2];
  n[2][3] = n[3][2] = M[1][2] + M[2][1];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ALIGN_JACOBI_SWEEPS; ++sweep) {
    align_jacobi_rotate(n, v, 0, 1);
    align_jacobi_rotate(n, v, 0, 2);
    align_jacobi_rotate(n, v, 0, 3);
    align_jacobi_rotate(n, v, 1, 2);
    align_jacobi_rotate(n, v, 1, 3);
    align_jacobi_rotate(n, v, 2, 3);
  }
  // the column of the largest eigenvalue, the lowest column among equals; chosen without indexing by a run-time value
  double best = n[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
  if (n[1][1] > best) best = n[1][1], qw = v[0][1], qx = v[1][1], qy = v[2][1], qz = v[3][1];
  if (n[2][2] > best) best = n[2][2], qw = v[0][2], qx = v[1][2], qy = v[2][2], qz = v[3][2];
  if (n[3][3] > best) best = n[3][3], qw = v[0][3], qx = v[1][3], qy = v[2][3], qz = v[3][3];
  const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw = qw / len, qx = qx / len, qy = qy / len, qz = qz / len;
  const double ww = qw * qw, xx = qx * qx, yy = qy * qy, zz = qz * qz;
  const double xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
  // Rc (column-vector convention, y ~ Rc x) from the quaternion; R = Rc^T serves xt = x @ R
  double *R = out.R;
  R[0] = ((ww + xx) - yy) - zz, R[3] = 2.0 * (xy - wz), R[6] = 2.0 * (xz + wy);
  R[1] = 2.0 * (xy + wz), R[4] = ((ww - xx) + yy) - zz, R[7] = 2.0 * (yz - wx);
  R[2] = 2.0 * (xz - wy), R[5] = 2.0 * (yz + wx), R[8] = ((ww - xx) - yy) + zz;
  double tr = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double t = R[3 * a + b] * M[a][b];
      tr = (a == 0 && b == 0) ? t : tr + t;
    }
  const double s = estimate_scale ? tr / (xvar > eps ? xvar : eps) : 1.0;
  for (int b = 0; b < 3; ++b) out.T[b] = my[b] - s * ((mx[0] * R[b] + mx[1] * R[3 + b]) + mx[2] * R[6 + b]);
  const double res = ((s * s) * xvar - (2.0 * s) * tr) + yvar;
  out.s = s;
  out.mse = res > 0.0 ? res : 0.0;   // a NaN (overflowed moments) becomes 0 as well
}

}  // namespace bdm
