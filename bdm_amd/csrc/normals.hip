// Point-cloud normals (section 10 of bdm_hip.h): K nearest neighbours of every point within its own cloud, the covariance of the
// neighbourhood, its eigen-decomposition and the sign of the normal, in ONE kernel.  DESIGN.md section 14.
//
// One wave owns NRM_QPW query points; a workgroup of four waves streams the cloud through LDS in tiles of NRM_TILE points (x, y, z
// planes), so a tile is read from global memory once per 4 * NRM_QPW queries and from LDS once per NRM_QPW.  Per step each lane
// holds one candidate j and tests it against every query of its wave: d2 is the unfused fp32 squared distance of the header, its
// bit pattern (d2 >= +0, so the pattern orders like the value) is compared with the query's current k-th key, and a ballot
// collects the lanes that beat it.  The rare accepted candidate is inserted into the query's sorted list, which lives one entry
// per lane (lane l = l-th nearest so far, hence k <= 64): the lanes behind the insertion point take their left neighbour's entry
// through a DPP wave shift.  Candidates arrive in ascending j and the accepted lanes of a step are inserted in ascending lane
// order, so "strictly below the k-th key" and "behind every equal key" order the list by (d2, j) without j taking part in a
// comparison.  A non-finite point is stored as NaN: its d2 is NaN against every query, and a NaN pattern is above the list's
// initial key 0x7f800001 in the unsigned comparison, while +inf (a finite pair whose distance overflows) is below it.
// The key and the list step are knn_list.h's, shared with the two-set search of knn.hip.
//
// Then, per query, lane l fetches neighbour l, the wave forms the mean difference and the six central second moments with
// fixed-order wave sums (no atomics: the bits do not depend on the batch or the launch), and every lane runs the same Jacobi
// iteration (normals_eig.h).  The file is compiled with -ffp-contract=off (Makefile): the distance arithmetic defines indices.
#include "common.h"
#include "bdm_hip.h"
#include "knn_list.h"
#include "normals_eig.h"

namespace bdm {

constexpr int NRM_THREADS = 256;
constexpr int NRM_WAVES = NRM_THREADS / 64;
constexpr int NRM_QPW = 4;                        // queries per wave
constexpr int NRM_QPB = NRM_WAVES * NRM_QPW;      // queries per workgroup
constexpr int NRM_TILE = 1024;                    // candidates per LDS tile: 3 planes of 4 KiB
constexpr unsigned int NRM_EMPTY = KNN_EMPTY;     // key of an unused list entry (knn_list.h, shared with knn.hip)

__global__ __launch_bounds__(NRM_THREADS) void estimate_normals_kernel(int n, int k, int orient, int blocks_per_cloud,
                                                                       const float *__restrict__ points,
                                                                       const float *__restrict__ viewpoints,
                                                                       int *__restrict__ knn_idx, float *__restrict__ normals,
                                                                       float *__restrict__ curvatures) {
  __shared__ float sx[NRM_TILE], sy[NRM_TILE], sz[NRM_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cloud = blockIdx.x / blocks_per_cloud, q0 = ((blockIdx.x % blocks_per_cloud) * NRM_WAVES + wave) * NRM_QPW;
  const float *pts = points + (size_t)cloud * n * 3;
  const float nan = __builtin_nanf("");

  float qx[NRM_QPW], qy[NRM_QPW], qz[NRM_QPW];
  unsigned int lkey[NRM_QPW], thr[NRM_QPW];
  int lidx[NRM_QPW];
#pragma unroll
  for (int q = 0; q < NRM_QPW; ++q) {
    const int qi = min(q0 + q, n - 1);  // a wave's queries past the cloud's end repeat the last point and are not written
    qx[q] = pts[3 * (size_t)qi], qy[q] = pts[3 * (size_t)qi + 1], qz[q] = pts[3 * (size_t)qi + 2];
    if (!(fabsf(qx[q]) < INFINITY && fabsf(qy[q]) < INFINITY && fabsf(qz[q]) < INFINITY)) qx[q] = nan;  // accepts nobody
    lkey[q] = thr[q] = NRM_EMPTY;
    lidx[q] = -1;
  }

  for (int base = 0; base < n; base += NRM_TILE) {
    __syncthreads();  // the previous tile has been consumed
    for (int t = tid; t < NRM_TILE; t += NRM_THREADS) {
      float x = nan, y = nan, z = nan;
      if (base + t < n) {
        const float *p = pts + 3 * (size_t)(base + t);
        x = p[0], y = p[1], z = p[2];
        if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) x = nan;  // nobody's neighbour
      }
      sx[t] = x, sy[t] = y, sz[t] = z;
    }
    __syncthreads();
    const int cnt = min(NRM_TILE, n - base);
    for (int s = 0; s < cnt; s += 64) {  // s + lane < NRM_TILE: the tile is a multiple of 64 and padded with NaN
      const float cx = sx[s + lane], cy = sy[s + lane], cz = sz[s + lane];
#pragma unroll
      for (int q = 0; q < NRM_QPW; ++q) {
        knn_list_step(knn_key(cx, cy, cz, qx[q], qy[q], qz[q]), base + s, k, lane, lkey[q], lidx[q], thr[q]);  // knn_list.h
      }
    }
  }

  const float inv_k = 1.0f / (float)k;
#pragma unroll
  for (int q = 0; q < NRM_QPW; ++q) {
    const int qi = q0 + q;
    if (qi >= n) break;  // wave-uniform
    const bool ok = thr[q] != NRM_EMPTY;  // k finite neighbours were found (the query itself is finite then)
    const bool mine = lane < k;
    const int j = ok && mine ? lidx[q] : qi;  // in [0, n)
    float ex = pts[3 * (size_t)j] - qx[q], ey = pts[3 * (size_t)j + 1] - qy[q], ez = pts[3 * (size_t)j + 2] - qz[q];
    if (!mine) ex = ey = ez = 0.0f;
    const float mx = wave_sum(ex) * inv_k, my = wave_sum(ey) * inv_k, mz = wave_sum(ez) * inv_k;
    const float fx = mine ? ex - mx : 0.0f, fy = mine ? ey - my : 0.0f, fz = mine ? ez - mz : 0.0f;
    const float c[6] = {wave_sum(fx * fx) * inv_k, wave_sum(fx * fy) * inv_k, wave_sum(fx * fz) * inv_k,
                        wave_sum(fy * fy) * inv_k, wave_sum(fy * fz) * inv_k, wave_sum(fz * fz) * inv_k};
    float lambda[3], nrm[3];
    sym3_eigen(c, lambda, nrm);
    bool flip;
    if (orient == 0) {  // the component of largest magnitude is positive, the lowest axis among equals
      const float ax = fabsf(nrm[0]), ay = fabsf(nrm[1]), az = fabsf(nrm[2]);
      flip = (ax >= ay && ax >= az ? nrm[0] : (ay >= az ? nrm[1] : nrm[2])) < 0.0f;
    } else if (orient == 1) {  // the majority of the neighbours lies on the positive side
      const float proj = (ex * nrm[0] + ey * nrm[1]) + ez * nrm[2];
      flip = 2 * __popcll(__ballot(mine && proj > 0.0f)) < k;
    } else {  // towards the viewpoint
      const float *vp = viewpoints + 3 * (size_t)cloud;
      flip = ((vp[0] - qx[q]) * nrm[0] + (vp[1] - qy[q]) * nrm[1]) + (vp[2] - qz[q]) * nrm[2] < 0.0f;
    }
    const size_t row = (size_t)cloud * n + qi;
    if (knn_idx && mine) knn_idx[row * k + lane] = ok ? lidx[q] : -1;
    if (lane < 3) {
      const float v = lane == 0 ? nrm[0] : (lane == 1 ? nrm[1] : nrm[2]);
      normals[row * 3 + lane] = ok ? (flip ? -v : v) : nan;
      if (curvatures) curvatures[row * 3 + lane] = ok ? (lane == 0 ? lambda[0] : (lane == 1 ? lambda[1] : lambda[2])) : nan;
    }
  }
}

}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_estimate_normals_workspace_bytes(int b, int n, int k) {
  (void)b, (void)n, (void)k;
  return 0;  // the neighbour lists live in registers
}

extern "C" int bdm_estimate_normals(int b, int n, int k, int orient, const float *points, const float *viewpoints, int *knn_idx,
                                    float *normals, float *curvatures, void *workspace, void *stream) {
  (void)workspace;
  BDM_REQUIRE(k >= 3 && k <= 64, "estimate_normals: k=%d outside 3..64 (the neighbour list holds one entry per lane)", k);
  BDM_REQUIRE(b >= 0 && n > k, "estimate_normals: bad sizes b=%d n=%d k=%d (n must exceed k)", b, n, k);
  BDM_REQUIRE(orient >= 0 && orient <= 2, "estimate_normals: orient=%d is not 0, 1 or 2", orient);
  BDM_REQUIRE((viewpoints != nullptr) == (orient == 2), "estimate_normals: viewpoints go with orient == 2 and with nothing else");
  BDM_REQUIRE((long long)b * n * k < (1ll << 31), "estimate_normals: b n k = %lld exceeds int", (long long)b * n * k);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(points && normals, "estimate_normals: null points or normals");
  const int blocks_per_cloud = cdiv(n, NRM_QPB);
  BDM_REQUIRE((long long)b * blocks_per_cloud < (1ll << 31), "estimate_normals: grid too large");
  hipLaunchKernelGGL(estimate_normals_kernel, dim3((unsigned)(b * blocks_per_cloud)), dim3(NRM_THREADS), 0, (hipStream_t)stream, n, k,
                     orient, blocks_per_cloud, points, viewpoints, knn_idx, normals, curvatures);
  return launch_status("estimate_normals");
}
