// Rigid and similarity alignment of point clouds over ragged batches: the similarity transform of a cloud, the match-and-moments
// kernel, the closed-form solve and the ICP iteration (section 18 of bdm_hip.h; restates pytorch3d's iterative_closest_point and
// corresponding_points_alignment from their published behaviour).  DESIGN.md section 22.
//
// align_match_kernel is the hot kernel.  K = 1 needs no neighbour list, so it has nn_sqdist_kernel's shape and not
// knn_points_kernel's: one source point per lane, the entry's target rows streamed through LDS in tiles of ALIGN_TILE (x, y, z
// planes; a non-finite row and the tail are stored as NaN), every lane reading the same candidate (an LDS broadcast, four candidates
// per 16-byte read) and keeping the smallest key with a strict comparison in ascending index, which is the (d2, j) order of
// knn_list.h.  One point per lane alone leaves one wave per SIMD at 16 x 4096 points, so the four waves of a workgroup hold the SAME
// 64 source points and each scans a quarter of every tile; their four minima meet in LDS, where equal keys are decided by the index
// (measured: DESIGN.md section 22).  Wave 0 gathers the partner's coordinates once, quantises the pair (align_solve.h) and sums its
// 18 integer moments over the wave; 18 threads send them with 64-bit integer atomic adds to the entry's state.  Integer sums are exact, so nothing depends on the launch geometry or the order of the atomics.
//
// blockIdx.y is the batch entry.  A workgroup of an entry that is done, or whose first point lies past its entry's end, leaves as a
// whole before the first barrier; inside a live workgroup the lanes past the end carry a NaN query and add zeros, so no barrier sits
// under a divergent condition.  align_solve_kernel (one thread per entry) turns the moments into the next transform in float64
// (align_solve.h), clears them for the next match and applies the stopping rule.
#include "common.h"
#include "bdm_hip.h"
#include "align_solve.h"
#include "knn_list.h"
#include "ragged.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace bdm {

constexpr int ALIGN_THREADS = 256;                 // the match: four waves share 64 source points, each scans a quarter of every tile
constexpr int ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr int ALIGN_QPB = 64;                      // source points per workgroup of the match: 16 x 4096 points are 1024 workgroups
constexpr int ALIGN_TILE = 1024;                   // candidates per LDS tile: 3 planes of 4 KiB
constexpr int ALIGN_PART = ALIGN_TILE / ALIGN_WAVES;   // a wave's share of a tile, a multiple of 4
constexpr int ALIGN_ROW_THREADS = 256;             // the one-thread-per-row kernels
constexpr int ALIGN_MAX_B = 65535;                 // gridDim.y
constexpr long long ALIGN_MAX_N = 1ll << 20;       // points per entry: 21 bits per coordinate are left
constexpr int ALIGN_MAX_ITER = 10000;

namespace {

struct alignas(16) AlignState {
  long long m[ALIGN_MOMENTS];   // the moments of the current match; zero between two matches
  double mse;                   // of the last iteration, NaN before the first
  float tr[13];                 // R (9, row-major), T (3), s
  float mse32;
  unsigned int amax_bits;
  int iter, done, converged;
  int pad[2];
};
static_assert(sizeof(AlignState) % 16 == 0, "AlignState rows stay 16-byte aligned");

// the apply rule of section 18 for output axis b: fl(fl(s d) + T_b), d = fl(fl(fl(x0 R0b) + fl(x1 R1b)) + fl(x2 R2b))
__device__ __forceinline__ float align_apply_axis(const float *t, int b, float x0, float x1, float x2) {
  const float d = __fadd_rn(__fadd_rn(__fmul_rn(x0, t[b]), __fmul_rn(x1, t[3 + b])), __fmul_rn(x2, t[6 + b]));
  return __fadd_rn(__fmul_rn(t[12], d), t[9 + b]);
}

__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_state_init_kernel(int b, const float *__restrict__ start,
                                                                             AlignState *__restrict__ state) {
  const int i = blockIdx.x * ALIGN_ROW_THREADS + threadIdx.x;
  if (i >= b) return;
  AlignState &st = state[i];
  for (int k = 0; k < ALIGN_MOMENTS; ++k) st.m[k] = 0;
  for (int k = 0; k < 13; ++k) st.tr[k] = start ? start[13 * (size_t)i + k] : ((k == 0 || k == 4 || k == 8 || k == 12) ? 1.0f : 0.0f);
  st.mse = __builtin_nan("");
  st.mse32 = __builtin_nanf("");
  st.amax_bits = 0u;
  st.iter = st.done = st.converged = 0;
  st.pad[0] = st.pad[1] = 0;
}

// the largest |coordinate| over the finite rows of both sets: an integer maximum of float bits, as mm_area_kernel's
__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_amax_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                       const long long *__restrict__ x_first,
                                                                       const long long *__restrict__ y_first,
                                                                       AlignState *__restrict__ state) {
  const int entry = blockIdx.y;
  const long long xs = x_first[entry], ys = y_first[entry];
  const long long np = x_first[entry + 1] - xs, nr = y_first[entry + 1] - ys;
  if ((long long)blockIdx.x * ALIGN_ROW_THREADS >= max(np, nr)) return;   // the whole workgroup
  const long long i = (long long)blockIdx.x * ALIGN_ROW_THREADS + threadIdx.x;
  float m = 0.f;
  if (i < np) {
    const float *p = x + 3 * (size_t)(xs + i);
    if (finite3(p[0], p[1], p[2])) m = fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
  }
  if (i < nr) {
    const float *p = y + 3 * (size_t)(ys + i);
    if (finite3(p[0], p[1], p[2])) m = fmaxf(m, fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2])));
  }
  m = wave_max(m);   // every lane of the workgroup is here
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(&state[entry].amax_bits, __float_as_uint(m));   // non-negative floats order like their bits
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool PAIRED>
__global__ __launch_bounds__(ALIGN_THREADS) void align_match_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                    const long long *__restrict__ x_first,
                                                                    const long long *__restrict__ y_first,
                                                                    AlignState *__restrict__ state, int *__restrict__ partner) {
  __shared__ __attribute__((aligned(16))) float sx[ALIGN_TILE];
  __shared__ __attribute__((aligned(16))) float sy[ALIGN_TILE];
  __shared__ __attribute__((aligned(16))) float sz[ALIGN_TILE];
  __shared__ unsigned int skey[ALIGN_WAVES][64];
  __shared__ int sidx[ALIGN_WAVES][64];
  __shared__ long long red[ALIGN_MOMENTS];
  const int entry = blockIdx.y;
  AlignState &st = state[entry];
  if (st.done) return;   // the whole workgroup, before any barrier
  const long long xs = x_first[entry], ys = y_first[entry];
  const int np = (int)(x_first[entry + 1] - xs), nr = (int)(y_first[entry + 1] - ys);   // both <= 2^20
  if ((long long)blockIdx.x * ALIGN_QPB >= np) return;   // likewise
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = (int)blockIdx.x * ALIGN_QPB + lane;   // the same source point in lane l of every wave
  const bool live = i < np;
  const float *xp = x + 3 * (size_t)(xs + min(i, np - 1));   // a lane past the end repeats the last point and adds nothing
  const float *yp = y + 3 * (size_t)ys;
  const float px = xp[0], py = xp[1], pz = xp[2];
  const float nan = __builtin_nanf("");
  int bi = -1;

  if (PAIRED) {
    if (wave == 0 && live && i < nr && finite3(px, py, pz)) {
      const float *c = yp + 3 * (size_t)i;
      if (finite3(c[0], c[1], c[2])) bi = i;
    }
  } else {
    float tr[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) tr[k] = st.tr[k];
    float qx = align_apply_axis(tr, 0, px, py, pz);
    const float qy = align_apply_axis(tr, 1, px, py, pz), qz = align_apply_axis(tr, 2, px, py, pz);
    if (!live || !finite3(qx, qy, qz)) qx = nan;   // accepts nobody (a non-finite source point transforms to a non-finite one)
    unsigned int best = KNN_EMPTY;
    for (int base = 0; base < nr; base += ALIGN_TILE) {   // uniform over the workgroup: nr is the entry's
      __syncthreads();   // the previous tile has been consumed
      const int cnt = min(ALIGN_TILE, nr - base), fill = (cnt + 3) & ~3;   // fill <= ALIGN_TILE
      for (int t = tid; t < fill; t += ALIGN_THREADS) {
        float cx = nan, cy = nan, cz = nan;
        if (t < cnt) {
          const float *p = yp + 3 * (size_t)(base + t);
          cx = p[0], cy = p[1], cz = p[2];
          if (!finite3(cx, cy, cz)) cx = nan;   // nobody's partner
        }
        sx[t] = cx, sy[t] = cy, sz[t] = cz;
      }
      __syncthreads();
      const int hi = min(cnt, (wave + 1) * ALIGN_PART);
      for (int j = wave * ALIGN_PART; j < hi; j += 4) {   // this wave's quarter; j + 3 < fill: the tail of the last four is NaN
        const float4 cx = *reinterpret_cast<const float4 *>(sx + j), cy = *reinterpret_cast<const float4 *>(sy + j),
                     cz = *reinterpret_cast<const float4 *>(sz + j);
        const unsigned int k0 = knn_key(cx.x, cy.x, cz.x, qx, qy, qz), k1 = knn_key(cx.y, cy.y, cz.y, qx, qy, qz);
        const unsigned int k2 = knn_key(cx.z, cy.z, cz.z, qx, qy, qz), k3 = knn_key(cx.w, cy.w, cz.w, qx, qy, qz);
        if (k0 < best) best = k0, bi = base + j;       // strict and ascending: the lowest index among equal distances
        if (k1 < best) best = k1, bi = base + j + 1;
        if (k2 < best) best = k2, bi = base + j + 2;
        if (k3 < best) best = k3, bi = base + j + 3;
      }
    }
    // the four waves' minima of (d2, j) -> wave 0.  A wave's indices ascend, but not from wave to wave across tiles: equal keys
    // are decided by the index itself here.
    skey[wave][lane] = best, sidx[wave][lane] = bi;
    __syncthreads();   // every thread of a live workgroup arrives
    if (wave == 0) {
#pragma unroll
      for (int w = 1; w < ALIGN_WAVES; ++w) {
        const unsigned int k = skey[w][lane];
        const int j = sidx[w][lane];
        if (k < best || (k == best && j >= 0 && j < bi)) best = k, bi = j;
      }
    } else {
      bi = -1;   // waves 1 .. 3 add nothing below
    }
  }
  if (partner && live && wave == 0) partner[xs + i] = bi;

  long long acc[ALIGN_MOMENTS];
#pragma unroll
  for (int k = 0; k < ALIGN_MOMENTS; ++k) acc[k] = 0;
  if (bi >= 0) {   // 0 <= bi < nr
    const double two_e = align_pow2(align_scale_exp(st.amax_bits, np));
    const float *c = yp + 3 * (size_t)bi;
    const long long a[3] = {align_quantise(px, two_e), align_quantise(py, two_e), align_quantise(pz, two_e)};
    const long long g[3] = {align_quantise(c[0], two_e), align_quantise(c[1], two_e), align_quantise(c[2], two_e)};
    acc[0] = 1;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      acc[1 + u] = a[u], acc[4 + u] = g[u];
#pragma unroll
      for (int w = 0; w < 3; ++w) acc[7 + 3 * u + w] = a[u] * g[w];
    }
    acc[16] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    acc[17] = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
  }
#pragma unroll
  for (int k = 0; k < ALIGN_MOMENTS; ++k) {
    const long long s = wave_sum_ll(acc[k]);   // waves 1 .. 3 hold zeros
    if (tid == 0) red[k] = s;
  }
  __syncthreads();   // every thread of a live workgroup arrives
  if (tid < ALIGN_MOMENTS) {
    const long long s = red[tid];
    if (s != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&st.m[tid]), (unsigned long long)s);   // two's complement: exact
  }
}

// one thread per entry: moments -> the next transform, the stopping rule of section 18
__global__ __launch_bounds__(64) void align_solve_kernel(int b, int max_iterations, int estimate_scale, double thr, double eps,
                                                         const long long *__restrict__ x_first, float *__restrict__ history,
                                                         AlignState *__restrict__ state) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  AlignState &st = state[i];
  if (st.done) return;
  long long m[ALIGN_MOMENTS];
  for (int k = 0; k < ALIGN_MOMENTS; ++k) {
    m[k] = st.m[k];
    st.m[k] = 0;
  }
  if (m[0] == 0) {   // nobody matched: the transform and the iteration count stay
    st.done = 1, st.converged = 0;
    st.mse = __builtin_nan("");
    st.mse32 = __builtin_nanf("");
    return;
  }
  AlignSolution sol;
  align_solve(m, align_scale_exp(st.amax_bits, x_first[i + 1] - x_first[i]), estimate_scale != 0, eps, sol);
  const int t = st.iter + 1;
  const double prev = st.mse;
  for (int k = 0; k < 9; ++k) st.tr[k] = (float)sol.R[k];
  for (int k = 0; k < 3; ++k) st.tr[9 + k] = (float)sol.T[k];
  st.tr[12] = (float)sol.s;
  st.mse = sol.mse;
  st.mse32 = (float)sol.mse;
  st.iter = t;
  if (history) {
    float *h = history + 13 * ((size_t)i * max_iterations + (t - 1));   // t <= max_iterations: an entry is done there
    for (int k = 0; k < 13; ++k) h[k] = st.tr[k];
  }
  if (sol.mse == 0.0 || (t >= 2 && (prev - sol.mse) / prev <= thr))
    st.done = 1, st.converged = 1;
  else if (t >= max_iterations)
    st.done = 1, st.converged = 0;
}

__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_active_kernel(int b, const AlignState *__restrict__ state, int *__restrict__ active) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int n = 0;
  for (int i = threadIdx.x; i < b; i += ALIGN_ROW_THREADS) n += state[i].done ? 0 : 1;
  if (n) atomicAdd(&total, n);   // LDS, integers
  __syncthreads();
  if (threadIdx.x == 0) *active = total;
}

// xt = s (x @ R) + T per point; the transform of entry i is the 13 floats at tr + i * stride
__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_apply_kernel(const float *__restrict__ x, const long long *__restrict__ x_first,
                                                                        const float *__restrict__ tr, int stride, float *__restrict__ xt) {
  const int entry = blockIdx.y;
  const long long xs = x_first[entry], np = x_first[entry + 1] - xs;
  const long long i = (long long)blockIdx.x * ALIGN_ROW_THREADS + threadIdx.x;
  if (i >= np) return;
  const float *t = tr + (size_t)entry * stride;
  const float *p = x + 3 * (size_t)(xs + i);
  const float x0 = p[0], x1 = p[1], x2 = p[2];
  float *o = xt + 3 * (size_t)(xs + i);
  o[0] = align_apply_axis(t, 0, x0, x1, x2), o[1] = align_apply_axis(t, 1, x0, x1, x2), o[2] = align_apply_axis(t, 2, x0, x1, x2);
}

// the per-entry outputs; any pointer may be NULL
__global__ __launch_bounds__(ALIGN_ROW_THREADS) void align_out_kernel(int b, const long long *__restrict__ x_first,
                                                                      const AlignState *__restrict__ state, float *__restrict__ transform,
                                                                      float *__restrict__ mse, int *__restrict__ converged,
                                                                      int *__restrict__ iterations, long long *__restrict__ moments,
                                                                      int *__restrict__ exponent) {
  const int i = blockIdx.x * ALIGN_ROW_THREADS + threadIdx.x;
  if (i >= b) return;
  const AlignState &st = state[i];
  if (transform)
    for (int k = 0; k < 13; ++k) transform[13 * (size_t)i + k] = st.tr[k];
  if (mse) mse[i] = st.mse32;
  if (converged) converged[i] = st.converged;
  if (iterations) iterations[i] = st.iter;
  if (moments)
    for (int k = 0; k < ALIGN_MOMENTS; ++k) moments[ALIGN_MOMENTS * (size_t)i + k] = st.m[k];
  if (exponent) exponent[i] = align_scale_exp(st.amax_bits, x_first[i + 1] - x_first[i]);
}

struct AlignWs {
  long long *x_first, *y_first;
  AlignState *state;
  size_t bytes;
};
AlignWs align_ws(void *workspace, int b) {
  AlignWs w;
  w.x_first = (long long *)workspace;
  w.y_first = w.x_first + (b + 1);
  w.state = (AlignState *)((char *)workspace + offsets_bytes(b));
  w.bytes = offsets_bytes(b) + sizeof(AlignState) * (size_t)b;
  return w;
}

// what every entry point checks first -> 0, or 1 with the error set.  nothing: b == 0 or no source point at all.
int align_prologue(const char *what, int b, const long long *x_first, const long long *y_first, const void *workspace, long long &max_p,
                   long long &max_r, bool &nothing) {
  BDM_REQUIRE(b >= 0 && b <= ALIGN_MAX_B, "%s: batch size %d outside 0 .. %d", what, b, ALIGN_MAX_B);
  nothing = b == 0;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(x_first && y_first, "%s: an offset array is NULL", what);
  if (check_first(what, "entry", b, x_first, &max_p) != BDM_OK || check_first(what, "entry", b, y_first, &max_r) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(x_first[b] <= INT_MAX && y_first[b] <= INT_MAX, "%s: %lld source or %lld target rows reach 2^31", what, x_first[b], y_first[b]);
  BDM_REQUIRE(max_p <= ALIGN_MAX_N && max_r <= ALIGN_MAX_N, "%s: an entry of %lld source or %lld target points exceeds 2^20", what, max_p,
              max_r);
  nothing = x_first[b] == 0;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(workspace, "%s: the workspace is NULL", what);
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace is not 16-byte aligned", what);
  return BDM_OK;
}

void align_start(const AlignWs &w, int b, const float *x, const float *y, const long long *x_first, const long long *y_first,
                 const float *start, long long max_p, long long max_r, hipStream_t st) {
  send_offsets(b, x_first, y_first, w.x_first, w.y_first, st);
  hipLaunchKernelGGL(align_state_init_kernel, dim3((unsigned)cdiv(b, ALIGN_ROW_THREADS)), dim3(ALIGN_ROW_THREADS), 0, st, b, start, w.state);
  hipLaunchKernelGGL(align_amax_kernel, dim3((unsigned)cdivll(max_p > max_r ? max_p : max_r, ALIGN_ROW_THREADS), (unsigned)b),
                     dim3(ALIGN_ROW_THREADS), 0, st, x, y, w.x_first, w.y_first, w.state);
}

void align_match(const AlignWs &w, int b, int mode, const float *x, const float *y, long long max_p, int *partner, hipStream_t st) {
  const dim3 grid((unsigned)cdivll(max_p, ALIGN_QPB), (unsigned)b);
  if (mode == 1)
    hipLaunchKernelGGL(align_match_kernel<true>, grid, dim3(ALIGN_THREADS), 0, st, x, y, w.x_first, w.y_first, w.state, partner);
  else
    hipLaunchKernelGGL(align_match_kernel<false>, grid, dim3(ALIGN_THREADS), 0, st, x, y, w.x_first, w.y_first, w.state, partner);
}

int align_check_paired(const char *what, int b, const long long *x_first, const long long *y_first) {
  for (int i = 0; i < b; ++i)
    BDM_REQUIRE(x_first[i + 1] - x_first[i] == y_first[i + 1] - y_first[i], "%s: entry %d pairs %lld source with %lld target points", what, i,
                x_first[i + 1] - x_first[i], y_first[i + 1] - y_first[i]);
  return BDM_OK;
}

}  // namespace
}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_similarity_apply_workspace_bytes(int b) {
  if (b < 0 || b > ALIGN_MAX_B) return 0;
  return offsets_bytes(b);
}

extern "C" int bdm_similarity_apply(int b, const float *x, const long long *x_first, const float *transform, float *xt, void *workspace,
                                    void *stream) {
  BDM_REQUIRE(b >= 0 && b <= ALIGN_MAX_B, "similarity_apply: batch size %d outside 0 .. %d", b, ALIGN_MAX_B);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(x_first, "similarity_apply: the offset array is NULL");
  long long max_p = 0;
  if (check_first("similarity_apply", "entry", b, x_first, &max_p) != BDM_OK) return BDM_ERR_ARG;
  const long long sum_p = x_first[b];
  BDM_REQUIRE(sum_p <= INT_MAX, "similarity_apply: %lld rows reach 2^31", sum_p);
  if (sum_p == 0) return BDM_OK;
  BDM_REQUIRE(x && transform && xt && workspace, "similarity_apply: the points, the transforms, the output or the workspace is NULL");
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "similarity_apply: the workspace is not 16-byte aligned");
  const Range in[2] = {{x, 12 * (size_t)sum_p}, {transform, 52 * (size_t)b}};
  const Range out[2] = {{xt, 12 * (size_t)sum_p}, {workspace, offsets_bytes(b)}};
  if (check_overlap("similarity_apply", in, 2, out, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  long long *dev_x = (long long *)workspace;
  send_offsets(b, x_first, nullptr, dev_x, dev_x + (b + 1), st);
  hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)cdivll(max_p, ALIGN_ROW_THREADS), (unsigned)b), dim3(ALIGN_ROW_THREADS), 0, st, x, dev_x,
                     transform, 13, xt);
  return launch_status("similarity_apply");
}

extern "C" size_t bdm_align_workspace_bytes(int b) {
  if (b < 0 || b > ALIGN_MAX_B) return 0;
  return offsets_bytes(b) + sizeof(AlignState) * (size_t)b;
}

extern "C" int bdm_align_moments(int b, int mode, const float *x, const float *y, const long long *x_first, const long long *y_first,
                                 const float *transform, long long *moments, int *exponent, int *partner, void *workspace, void *stream) {
  BDM_REQUIRE(mode == 0 || mode == 1, "align_moments: mode %d is neither 0 (nearest) nor 1 (paired)", mode);
  long long max_p = 0, max_r = 0;
  bool nothing = false;
  if (align_prologue("align_moments", b, x_first, y_first, workspace, max_p, max_r, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  if (mode == 1 && align_check_paired("align_moments", b, x_first, y_first) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(x && y && moments, "align_moments: the points or the moments are NULL");
  const AlignWs w = align_ws(workspace, b);
  const size_t sum_p = (size_t)x_first[b];
  const Range in[3] = {{x, 12 * sum_p}, {y, 12 * (size_t)y_first[b]}, {transform, 52 * (size_t)b}};
  const Range out[4] = {{moments, 8 * (size_t)ALIGN_MOMENTS * b}, {exponent, 4 * (size_t)b}, {partner, 4 * sum_p}, {workspace, w.bytes}};
  if (check_overlap("align_moments", in, 3, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  align_start(w, b, x, y, x_first, y_first, transform, max_p, max_r, st);
  align_match(w, b, mode, x, y, max_p, partner, st);
  hipLaunchKernelGGL(align_out_kernel, dim3((unsigned)cdiv(b, ALIGN_ROW_THREADS)), dim3(ALIGN_ROW_THREADS), 0, st, b, w.x_first, w.state,
                     (float *)nullptr, (float *)nullptr, (int *)nullptr, (int *)nullptr, moments, exponent);
  return launch_status("align_moments");
}

extern "C" int bdm_corresponding_points_alignment(int b, int estimate_scale, double eps, const float *x, const float *y,
                                                  const long long *x_first, const long long *y_first, float *transform, float *mse,
                                                  void *workspace, void *stream) {
  BDM_REQUIRE(eps >= 0.0 && eps < INFINITY, "corresponding_points_alignment: eps must be finite and not negative");
  long long max_p = 0, max_r = 0;
  bool nothing = false;
  if (align_prologue("corresponding_points_alignment", b, x_first, y_first, workspace, max_p, max_r, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (b > 0 && align_check_paired("corresponding_points_alignment", b, x_first, y_first) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(x && y && transform, "corresponding_points_alignment: the points or the transforms are NULL");
  const AlignWs w = align_ws(workspace, b);
  const Range in[2] = {{x, 12 * (size_t)x_first[b]}, {y, 12 * (size_t)y_first[b]}};
  const Range out[3] = {{transform, 52 * (size_t)b}, {mse, 4 * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap("corresponding_points_alignment", in, 2, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  align_start(w, b, x, y, x_first, y_first, nullptr, max_p, max_r, st);
  align_match(w, b, 1, x, y, max_p, nullptr, st);
  hipLaunchKernelGGL(align_solve_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0, st, b, 1, estimate_scale, 0.0, eps, w.x_first, (float *)nullptr,
                     w.state);
  hipLaunchKernelGGL(align_out_kernel, dim3((unsigned)cdiv(b, ALIGN_ROW_THREADS)), dim3(ALIGN_ROW_THREADS), 0, st, b, w.x_first, w.state, transform,
                     mse, (int *)nullptr, (int *)nullptr, (long long *)nullptr, (int *)nullptr);
  return launch_status("corresponding_points_alignment");
}

extern "C" int bdm_icp_init(int b, const float *x, const float *y, const long long *x_first, const long long *y_first, const float *start,
                            void *workspace, void *stream) {
  long long max_p = 0, max_r = 0;
  bool nothing = false;
  if (align_prologue("icp_init", b, x_first, y_first, workspace, max_p, max_r, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(x && y, "icp_init: the points are NULL");
  const AlignWs w = align_ws(workspace, b);
  const Range in[3] = {{x, 12 * (size_t)x_first[b]}, {y, 12 * (size_t)y_first[b]}, {start, 52 * (size_t)b}};
  const Range out[1] = {{workspace, w.bytes}};
  if (check_overlap("icp_init", in, 3, out, 1) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  align_start(w, b, x, y, x_first, y_first, start, max_p, max_r, st);
  return launch_status("icp_init");
}

extern "C" int bdm_icp_rounds(int b, int rounds, int max_iterations, int estimate_scale, double relative_rmse_thr, double eps, const float *x,
                              const float *y, const long long *x_first, const long long *y_first, float *history, int *active,
                              void *workspace, void *stream) {
  BDM_REQUIRE(rounds >= 1, "icp_rounds: rounds=%d is not positive", rounds);
  BDM_REQUIRE(max_iterations >= 1 && max_iterations <= ALIGN_MAX_ITER, "icp_rounds: max_iterations=%d outside 1 .. %d", max_iterations,
              ALIGN_MAX_ITER);
  BDM_REQUIRE(eps >= 0.0 && eps < INFINITY, "icp_rounds: eps must be finite and not negative");
  BDM_REQUIRE(relative_rmse_thr == relative_rmse_thr, "icp_rounds: relative_rmse_thr is NaN");
  long long max_p = 0, max_r = 0;
  bool nothing = false;
  if (align_prologue("icp_rounds", b, x_first, y_first, workspace, max_p, max_r, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(x && y && active, "icp_rounds: the points or the counter are NULL");
  BDM_REQUIRE(!history || 13ll * b * max_iterations <= INT_MAX, "icp_rounds: a history of %d x %d transforms reaches 2^31 floats", b,
              max_iterations);
  const AlignWs w = align_ws(workspace, b);
  const Range in[2] = {{x, 12 * (size_t)x_first[b]}, {y, 12 * (size_t)y_first[b]}};
  const Range out[3] = {{history, 52 * (size_t)b * max_iterations}, {active, 4}, {workspace, w.bytes}};
  if (check_overlap("icp_rounds", in, 2, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  for (int r = 0; r < rounds; ++r) {
    align_match(w, b, 0, x, y, max_p, nullptr, st);
    hipLaunchKernelGGL(align_solve_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0, st, b, max_iterations, estimate_scale, relative_rmse_thr, eps,
                       w.x_first, history, w.state);
  }
  hipLaunchKernelGGL(align_active_kernel, dim3(1), dim3(ALIGN_ROW_THREADS), 0, st, b, w.state, active);
  return launch_status("icp_rounds");
}

extern "C" int bdm_icp_finish(int b, const float *x, const long long *x_first, const long long *y_first, float *xt, float *transform,
                              float *mse, int *converged, int *iterations, void *workspace, void *stream) {
  long long max_p = 0, max_r = 0;
  bool nothing = false;
  if (align_prologue("icp_finish", b, x_first, y_first, workspace, max_p, max_r, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  BDM_REQUIRE(x && xt && transform && mse && converged && iterations, "icp_finish: the points or an output is NULL");
  const AlignWs w = align_ws(workspace, b);
  const size_t sum_p = (size_t)x_first[b];
  const Range in[1] = {{x, 12 * sum_p}};
  const Range out[6] = {{xt, 12 * sum_p}, {transform, 52 * (size_t)b}, {mse, 4 * (size_t)b}, {converged, 4 * (size_t)b},
                          {iterations, 4 * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap("icp_finish", in, 1, out, 6) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)cdivll(max_p, ALIGN_ROW_THREADS), (unsigned)b), dim3(ALIGN_ROW_THREADS), 0, st, x,
                     w.x_first, w.state->tr, (int)(sizeof(AlignState) / sizeof(float)), xt);
  hipLaunchKernelGGL(align_out_kernel, dim3((unsigned)cdiv(b, ALIGN_ROW_THREADS)), dim3(ALIGN_ROW_THREADS), 0, st, b, w.x_first, w.state, transform,
                     mse, converged, iterations, (long long *)nullptr, (int *)nullptr);
  return launch_status("icp_finish");
}
