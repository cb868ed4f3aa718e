// Eigen-decomposition of a symmetric 3 x 3 float32 matrix for normals.hip: cyclic Jacobi, a fixed number of sweeps, on the
// trace-scaled matrix.  Plain C++ (host and device), so the arithmetic can be exercised by a host program as well.  No FMA
// contraction is assumed either way: the rotations are orthogonal to a rounding each, which is all the accuracy argument needs.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define BDM_HD __host__ __device__ __forceinline__
#else
#define BDM_HD inline
#endif

namespace bdm {

constexpr int NORMALS_JACOBI_SWEEPS = 6;  // 3 x 3: the off-diagonal norm is below 2^-24 of the trace after 4; two spare

// One Jacobi rotation in the (p, q) plane that zeroes a[p][q]; r is the third index.  v accumulates the rotations by columns.
BDM_HD void jacobi_rotate(float (&a)[3][3], float (&v)[3][3], const int p, const int q, const int r) {
  const float apq = a[p][q];
  if (apq == 0.0f) return;
  const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
  // the root of t^2 + 2 t theta - 1 of smaller magnitude (|t| <= 1: the rotation of at most 45 degrees); theta^2 = inf gives t = 0
  const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c, tau = s / (1.0f + c);
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0f;
  const float arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
  a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
  for (int i = 0; i < 3; ++i) {
    const float vip = v[i][p], viq = v[i][q];
    v[i][p] = vip - s * (viq + tau * vip);
    v[i][q] = viq + s * (vip - tau * viq);
  }
}

// c: xx, xy, xz, yy, yz, zz  ->  lambda[3] ascending and the unit eigenvector of lambda[0].  A zero matrix gives (0, 0, 0) and
// the x axis; a non-finite one gives NaN.
BDM_HD void sym3_eigen(const float (&c)[6], float (&lambda)[3], float (&nrm)[3]) {
  const float trace = (c[0] + c[3]) + c[5];
  const float scale = trace > 0.0f ? 1.0f / trace : (trace == 0.0f ? 0.0f : trace * 0.0f /* NaN or inf -> NaN */);
  float a[3][3] = {{c[0] * scale, c[1] * scale, c[2] * scale},
                   {c[1] * scale, c[3] * scale, c[4] * scale},
                   {c[2] * scale, c[4] * scale, c[5] * scale}};
  float v[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
  for (int sweep = 0; sweep < NORMALS_JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate(a, v, 0, 1, 2);
    jacobi_rotate(a, v, 0, 2, 1);
    jacobi_rotate(a, v, 1, 2, 0);
  }
  const float d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
  // ascending order without indexing the arrays by a run-time value (that would put them in scratch)
  const int lo = (d0 <= d1 && d0 <= d2) ? 0 : (d1 <= d2 ? 1 : 2);
  const float x0 = lo == 0 ? d1 : d0, x1 = lo == 2 ? d1 : d2;   // the other two, in index order
  lambda[0] = (lo == 0 ? d0 : (lo == 1 ? d1 : d2)) * trace;
  lambda[1] = fminf(x0, x1) * trace;
  lambda[2] = fmaxf(x0, x1) * trace;
  float nx = lo == 0 ? v[0][0] : (lo == 1 ? v[0][1] : v[0][2]);
  float ny = lo == 0 ? v[1][0] : (lo == 1 ? v[1][1] : v[1][2]);
  float nz = lo == 0 ? v[2][0] : (lo == 1 ? v[2][1] : v[2][2]);
  const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
  nrm[0] = nx * inv, nrm[1] = ny * inv, nrm[2] = nz * inv;
}

}  // namespace bdm
