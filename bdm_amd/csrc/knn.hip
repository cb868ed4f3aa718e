// K nearest neighbours between two different point sets over ragged batches, and the transfer of per-point attributes through the
// neighbour lists (section 15 of bdm_hip.h; restates pytorch3d's knn_points from its published behaviour).  DESIGN.md section 19.
//
// knn_points_kernel is estimate_normals_kernel's search (normals.hip) without the covariance: one wave owns KNN_QPW queries, a
// workgroup of four waves streams the entry's reference rows through LDS in tiles of KNN_TILE (x, y, z planes; a non-finite row and
// the tail are stored as NaN), each lane holds one candidate per step and the neighbour list lives one entry per lane (knn_list.h).
// blockIdx.y is the batch entry; the starts and lengths of its two sets come from the offset arrays, which travel as launch
// arguments into the workspace (send_offsets, ragged.h).  A workgroup whose first query lies past its entry's end leaves as a whole
// before the first barrier; inside a live workgroup the waves past the end clamp their queries and write nothing, so no barrier sits
// under a divergent condition.
//
// knn_interpolate_kernel: one thread per (query row, channel) of an entry.  Neighbouring threads hold neighbouring channels of one
// row, so the gathers of attr rows and the stores are contiguous; the k indices and keys of the row are re-read by its c threads
// (from cache) and every thread forms the same weights in the same order, so no LDS and no array in registers is needed.
#include "common.h"
#include "bdm_hip.h"
#include "knn_list.h"
#include "ragged.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace bdm {

constexpr int KNN_THREADS = 256;
constexpr int KNN_WAVES = KNN_THREADS / 64;
constexpr int KNN_QPW = 4;                        // queries per wave
constexpr int KNN_QPB = KNN_WAVES * KNN_QPW;      // queries per workgroup
constexpr int KNN_TILE = 1024;                    // candidates per LDS tile: 3 planes of 4 KiB
constexpr int KNN_MAX_B = 65535;                  // gridDim.y
constexpr int KNN_MAX_C = 16;

namespace {

__global__ __launch_bounds__(KNN_THREADS) void knn_points_kernel(int k, const float *__restrict__ queries,
                                                                 const float *__restrict__ refs,
                                                                 const long long *__restrict__ q_first,
                                                                 const long long *__restrict__ r_first, int *__restrict__ idx,
                                                                 float *__restrict__ d2) {
  __shared__ float sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE];
  const int entry = blockIdx.y;
  const long long qs = q_first[entry], rs = r_first[entry];
  const int np = (int)(q_first[entry + 1] - qs), nr = (int)(r_first[entry + 1] - rs);   // both < 2^31
  if ((long long)blockIdx.x * KNN_QPB >= np) return;  // the whole workgroup, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = ((int)blockIdx.x * KNN_WAVES + wave) * KNN_QPW;   // < np + KNN_QPB
  const float *qp = queries + 3 * (size_t)qs, *rp = refs + 3 * (size_t)rs;
  const float nan = __builtin_nanf("");

  float qx[KNN_QPW], qy[KNN_QPW], qz[KNN_QPW];
  unsigned int lkey[KNN_QPW], thr[KNN_QPW];
  int lidx[KNN_QPW];
#pragma unroll
  for (int q = 0; q < KNN_QPW; ++q) {
    const int qi = min(q0 + q, np - 1);  // a wave's queries past the entry's end repeat the last query and are not written
    qx[q] = qp[3 * (size_t)qi], qy[q] = qp[3 * (size_t)qi + 1], qz[q] = qp[3 * (size_t)qi + 2];
    if (!finite3(qx[q], qy[q], qz[q])) qx[q] = nan;  // accepts nobody
    lkey[q] = thr[q] = KNN_EMPTY;
    lidx[q] = -1;
  }

  for (int base = 0; base < nr; base += KNN_TILE) {   // uniform over the workgroup: nr is the entry's
    __syncthreads();  // the previous tile has been consumed
    for (int t = tid; t < KNN_TILE; t += KNN_THREADS) {
      float x = nan, y = nan, z = nan;
      if (t < nr - base) {
        const float *p = rp + 3 * (size_t)(base + t);
        x = p[0], y = p[1], z = p[2];
        if (!finite3(x, y, z)) x = nan;  // nobody's neighbour
      }
      sx[t] = x, sy[t] = y, sz[t] = z;
    }
    __syncthreads();
    const int cnt = min(KNN_TILE, nr - base);
    for (int s = 0; s < cnt; s += 64) {  // s + lane < KNN_TILE: the tile is a multiple of 64 and padded with NaN
      const float cx = sx[s + lane], cy = sy[s + lane], cz = sz[s + lane];
#pragma unroll
      for (int q = 0; q < KNN_QPW; ++q)
        knn_list_step(knn_key(cx, cy, cz, qx[q], qy[q], qz[q]), base + s, k, lane, lkey[q], lidx[q], thr[q]);
    }
  }

  if (lane >= k) return;  // no barrier follows
#pragma unroll
  for (int q = 0; q < KNN_QPW; ++q) {
    const int qi = q0 + q;
    if (qi >= np) break;  // wave-uniform
    const size_t o = (size_t)(qs + qi) * k + lane;   // < sum P * k < 2^31
    const bool used = lkey[q] != KNN_EMPTY;
    if (idx) idx[o] = used ? lidx[q] : -1;
    if (d2) d2[o] = used ? __uint_as_float(lkey[q]) : INFINITY;
  }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_interpolate_kernel(int k, int c, int mode, float eps, float fill,
                                                                      const float *__restrict__ attr, const int *__restrict__ idx,
                                                                      const float *__restrict__ d2,
                                                                      const long long *__restrict__ q_first,
                                                                      const long long *__restrict__ r_first, float *__restrict__ out) {
  const int entry = blockIdx.y;
  const long long qs = q_first[entry], rs = r_first[entry];
  const long long np = q_first[entry + 1] - qs, nr = r_first[entry + 1] - rs;
  const long long t = (long long)blockIdx.x * KNN_THREADS + threadIdx.x;   // 64-bit: np * c may pass 2^31
  if (t >= np * c) return;
  const long long row = qs + t / c;
  const int ch = (int)(t % c);
  const int *ri = idx + (size_t)row * k;
  const float *rd = d2 + (size_t)row * k;
  const float *a = attr + (size_t)rs * c + ch;
  float num = 0.f, den = 0.f, first = fill;
  int m = 0;
  for (int l = 0; l < k; ++l) {   // ascending: the sums are sequential
    const int j = ri[l];
    if (j < 0 || j >= nr) continue;   // an empty entry (or an index no search of this entry wrote): takes no part
    const float v = a[(size_t)j * c];
    if (mode == 0) {
      first = v;
      m = 1;
      break;
    }
    const float w = 1.0f / (rd[l] + eps);   // +inf gives 0
    const float wv = w * v;
    num = m ? num + wv : wv;
    den = m ? den + w : w;
    ++m;
  }
  out[(size_t)row * c + ch] = m == 0 ? fill : (mode == 0 ? first : num / den);
}

// the checks on the offset arrays both entry points share -> 0, or 1 with the error set; max_p = the largest query count
int knn_check_offsets(const char *what, int b, const long long *q_first, const long long *r_first, long long &max_p) {
  long long max_r = 0;
  if (check_first(what, "entry", b, q_first, &max_p) != BDM_OK || check_first(what, "entry", b, r_first, &max_r) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(q_first[b] <= INT_MAX && r_first[b] <= INT_MAX, "%s: %lld queries or %lld reference rows reach 2^31", what, q_first[b],
              r_first[b]);
  return BDM_OK;
}

}  // namespace
}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_knn_points_workspace_bytes(int b, long long sum_p, int k) {
  if (b < 0 || b > KNN_MAX_B || k < 1 || k > 64 || sum_p < 0 || sum_p > INT_MAX || sum_p * k > INT_MAX) return 0;
  return offsets_bytes(b);
}

extern "C" int bdm_knn_points(int b, int k, const float *queries, const float *refs, const long long *q_first,
                              const long long *r_first, int *idx, float *d2, void *workspace, void *stream) {
  BDM_REQUIRE(k >= 1 && k <= 64, "knn_points: k=%d outside 1..64 (the neighbour list holds one entry per lane)", k);
  BDM_REQUIRE(b >= 0 && b <= KNN_MAX_B, "knn_points: batch size %d outside 0 .. %d", b, KNN_MAX_B);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(q_first && r_first, "knn_points: an offset array is NULL");
  long long max_p = 0;
  if (knn_check_offsets("knn_points", b, q_first, r_first, max_p) != BDM_OK) return BDM_ERR_ARG;
  const long long sum_p = q_first[b], sum_r = r_first[b];
  BDM_REQUIRE(sum_p * k <= INT_MAX, "knn_points: %lld queries of %d neighbours reach 2^31", sum_p, k);
  if (sum_p == 0) return BDM_OK;
  BDM_REQUIRE(queries && refs && workspace, "knn_points: the queries, the reference rows or the workspace is NULL");
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "knn_points: the workspace is not 16-byte aligned");
  const size_t n = (size_t)sum_p * k;
  const Range in[2] = {{queries, 12 * (size_t)sum_p}, {refs, 12 * (size_t)sum_r}};
  const Range out[3] = {{idx, 4 * n}, {d2, 4 * n}, {workspace, offsets_bytes(b)}};
  if (check_overlap("knn_points", in, 2, out, 3) != BDM_OK) return BDM_ERR_ARG;
  if (!idx && !d2) return BDM_OK;  // nothing to write
  hipStream_t st = (hipStream_t)stream;
  long long *dev_q = (long long *)workspace, *dev_r = dev_q + (b + 1);
  send_offsets(b, q_first, r_first, dev_q, dev_r, st);
  hipLaunchKernelGGL(knn_points_kernel, dim3((unsigned)cdivll(max_p, KNN_QPB), (unsigned)b), dim3(KNN_THREADS), 0, st, k, queries, refs,
                     dev_q, dev_r, idx, d2);
  return launch_status("knn_points");
}

extern "C" size_t bdm_knn_interpolate_workspace_bytes(int b) {
  if (b < 0 || b > KNN_MAX_B) return 0;
  return offsets_bytes(b);
}

extern "C" int bdm_knn_interpolate(int b, int k, int c, int mode, float eps, float fill, const float *attr, const int *idx,
                                   const float *d2, const long long *q_first, const long long *r_first, float *out,
                                   void *workspace, void *stream) {
  BDM_REQUIRE(k >= 1 && k <= 64, "knn_interpolate: k=%d outside 1..64", k);
  BDM_REQUIRE(c >= 1 && c <= KNN_MAX_C, "knn_interpolate: c=%d outside 1..%d", c, KNN_MAX_C);
  BDM_REQUIRE(mode == 0 || mode == 1, "knn_interpolate: mode %d is neither 0 (nearest) nor 1 (inverse squared distance)", mode);
  BDM_REQUIRE(mode == 0 || (eps > 0.f && eps < INFINITY), "knn_interpolate: eps must be positive and finite");
  BDM_REQUIRE(b >= 0 && b <= KNN_MAX_B, "knn_interpolate: batch size %d outside 0 .. %d", b, KNN_MAX_B);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(q_first && r_first, "knn_interpolate: an offset array is NULL");
  long long max_p = 0;
  if (knn_check_offsets("knn_interpolate", b, q_first, r_first, max_p) != BDM_OK) return BDM_ERR_ARG;
  const long long sum_p = q_first[b], sum_r = r_first[b];
  BDM_REQUIRE(sum_p * k <= INT_MAX, "knn_interpolate: %lld queries of %d neighbours reach 2^31", sum_p, k);
  if (sum_p == 0) return BDM_OK;
  BDM_REQUIRE(attr && idx && d2 && out && workspace, "knn_interpolate: an input, the output or the workspace is NULL");
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "knn_interpolate: the workspace is not 16-byte aligned");
  const size_t n = (size_t)sum_p * k;
  const Range in[3] = {{attr, 4 * (size_t)sum_r * c}, {idx, 4 * n}, {d2, 4 * n}};
  const Range outs[2] = {{out, 4 * (size_t)sum_p * c}, {workspace, offsets_bytes(b)}};
  if (check_overlap("knn_interpolate", in, 3, outs, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  long long *dev_q = (long long *)workspace, *dev_r = dev_q + (b + 1);
  send_offsets(b, q_first, r_first, dev_q, dev_r, st);
  hipLaunchKernelGGL(knn_interpolate_kernel, dim3((unsigned)cdivll(max_p * c, KNN_THREADS), (unsigned)b), dim3(KNN_THREADS), 0, st, k, c,
                     mode, eps, fill, attr, idx, d2, dev_q, dev_r, out);
  return launch_status("knn_interpolate");
}
