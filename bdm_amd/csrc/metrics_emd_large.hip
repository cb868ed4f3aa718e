// Approximate-match EMD of clouds of ANY size (section 7 of bdm_hip.h: bdm_pairwise_emd_large), beside pairwise_emd_kernel of
// metrics.hip, which holds a pair in one workgroup's LDS and registers and stops at 2048 points.  The same definition (DESIGN.md
// section 10: ten levels, K = v_exp_f32(d^2 * lvl2), difference-form distances, passes 1 - 3 with every term of pass 3 multiplied by
// ratioL), one workgroup per pair, a persistent grid of at most EL_SLABS workgroups that loop over the pairs, no atomics.
//
// A workgroup of 512 threads walks ROW TILES of 2048 owned indices (four per thread: k in passes 1 and 3, l in pass 2) and sweeps the
// OTHER cloud for each tile.  Two forms of that sweep:
//
//   resident   both clouds sit in LDS in the pair layout with their fourth component (32 npad bytes, 128 KB at n = 4096);
//   streamed   the other cloud passes through LDS in stages of 1024 points, each assembled from the shared cloud (xyz) and one of the
//              pair's weight arrays; the four partial sums of every owned index are carried across the stages in registers.
//
// Per-index state (remainL, remainR, the two weight arrays of the streamed form, the per-index cost) lives in the workgroup's slab of
// the caller's workspace: 20 npad bytes, read and written by the owner of the index except for the weight arrays, which the stage
// assembly reads behind a barrier.
//
// ORDER OF ARITHMETIC (what makes both forms, any grid and any tile ownership give the same bits).  For one index, a sum over the
// other cloud runs over that cloud in point order into four partial sums -- point p goes to sum p mod 4 -- and the four are added
// ((0 + 1) + (2 + 3)) after the last point; stages are multiples of 4 points.  The per-index cost is accumulated over the levels in
// float.  The pair's cost is the sum of cost[k] in double: lane t < 256 adds k = t, t + 256, ... in ascending order, then wave_sum,
// then the four waves in order -- a function of n alone.  Contraction is off in the sweep: every fma there is written out.
#include "common.h"
#include "bdm_hip.h"

namespace bdm {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int EL_THREADS = 512;
constexpr int EL_KPT = 4;                       // owned indices per thread and row tile
constexpr int EL_TILE = EL_THREADS * EL_KPT;    // 2048
constexpr int EL_STAGE = 1024;                  // points per LDS stage of the streamed form
constexpr int EL_SLABS = 256;                   // workgroups of the persistent grid = slabs of the workspace (one per CU of an MI355X)
constexpr int EL_RESIDENT_MAX_N = 4096;         // 32 * 4096 bytes = 128 KB of the CU's 160 KB
constexpr int EL_MAX_N = 65536;                 // a pair is never split over workgroups and its time grows with n^2
constexpr int EL_REDUCE = 256;                  // lanes of the final reduction

struct EmdLargeLevels {
  float lvl2[10];  // level * log2(e) for j = 7 .. -2
};

// accumulates, for the KPT owned points, the sums over `npairs` pairs of staged points (a multiple of 2) into the partial sums
// s0 (.x: points 4m, .y: 4m + 1), s1 (4m + 2, 4m + 3): K w, or with COST (K rl) w and, into c0 / c1, the same terms times sqrt(d^2)
template <bool COST>
__device__ __forceinline__ void emd_large_sweep(const float4 *cloud, int npairs, float lvl2, const float (&px)[EL_KPT],
                                                const float (&py)[EL_KPT], const float (&pz)[EL_KPT], const float (&rl)[EL_KPT],
                                                f2 (&s0)[EL_KPT], f2 (&s1)[EL_KPT], f2 (&c0)[EL_KPT], f2 (&c1)[EL_KPT]) {
#pragma clang fp contract(off)
  for (int pr = 0; pr < npairs; pr += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 xy = cloud[2 * (pr + h)], zw = cloud[2 * (pr + h) + 1];
      const f2 qx = {xy.x, xy.y}, qy = {xy.z, xy.w}, qz = {zw.x, zw.y}, w = {zw.z, zw.w};
#pragma unroll
      for (int q = 0; q < EL_KPT; ++q) {
        const f2 dx = qx - px[q], dy = qy - py[q], dz = qz - pz[q];
        f2 d = dx * dx;
        d = __builtin_elementwise_fma(dy, dy, d);
        d = __builtin_elementwise_fma(dz, dz, d);
        const f2 e = d * lvl2;
        const f2 kk = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
        f2 &sa = h ? s1[q] : s0[q];
        if (COST) {
          const f2 kw = (kk * rl[q]) * w;
          const f2 rt = {__builtin_amdgcn_sqrtf(d.x), __builtin_amdgcn_sqrtf(d.y)};
          f2 &ca = h ? c1[q] : c0[q];
          sa = sa + kw;
          ca = __builtin_elementwise_fma(kw, rt, ca);
        } else {
          sa = __builtin_elementwise_fma(kk, w, sa);
        }
      }
    }
  }
}

// float offset of point idx's x in the pair layout: pair q = [2q] (x0, x1, y0, y1), [2q + 1] (z0, z1, w0, w1); y at + 2, z at + 4, w at + 6
__device__ __forceinline__ int el_slot(int idx) { return 8 * (idx >> 1) + (idx & 1); }

// s[q] (and c[q]) of the owned points against the WHOLE other cloud: resident, `lds` is that cloud; streamed, `lds` is the stage
// buffer, filled from the other cloud's coordinates `gother` and the weights `wother` (both of n points; the padding up to npad
// repeats the last point with weight 0).  Called by every thread of the workgroup (the streamed form has barriers).
template <bool RESIDENT, bool COST>
__device__ __forceinline__ void emd_large_rows(float4 *lds, const float *gother, const float *wother, int n, int npad, float lvl2,
                                               const float (&px)[EL_KPT], const float (&py)[EL_KPT], const float (&pz)[EL_KPT],
                                               const float (&rl)[EL_KPT], float (&s)[EL_KPT], float (&c)[EL_KPT]) {
  f2 s0[EL_KPT], s1[EL_KPT], c0[EL_KPT], c1[EL_KPT];
#pragma unroll
  for (int q = 0; q < EL_KPT; ++q) s0[q] = s1[q] = c0[q] = c1[q] = f2{0.0f, 0.0f};
  if (RESIDENT) {
    emd_large_sweep<COST>(lds, npad >> 1, lvl2, px, py, pz, rl, s0, s1, c0, c1);
  } else {
    float *stage = (float *)lds;
    for (int t0 = 0; t0 < npad; t0 += EL_STAGE) {
      const int len = min(EL_STAGE, npad - t0);  // a multiple of 4
      __syncthreads();
      for (int idx = (int)threadIdx.x; idx < len; idx += EL_THREADS) {
        const int p = t0 + idx, src = p < n ? p : n - 1, o = el_slot(idx);
        stage[o] = gother[3 * src], stage[o + 2] = gother[3 * src + 1], stage[o + 4] = gother[3 * src + 2];
        stage[o + 6] = p < n ? wother[p] : 0.0f;
      }
      __syncthreads();
      emd_large_sweep<COST>(lds, len >> 1, lvl2, px, py, pz, rl, s0, s1, c0, c1);
    }
  }
#pragma unroll
  for (int q = 0; q < EL_KPT; ++q) {
    s[q] = (s0[q].x + s0[q].y) + (s1[q].x + s1[q].y);
    c[q] = (c0[q].x + c0[q].y) + (c1[q].x + c1[q].y);
  }
}

// the owned indices of the row tile at r0 and their coordinates in cloud g; a thread without an index computes on point 0 and writes nothing
__device__ __forceinline__ void emd_large_own(const float *g, int r0, int n, int (&idx)[EL_KPT], bool (&own)[EL_KPT],
                                              float (&px)[EL_KPT], float (&py)[EL_KPT], float (&pz)[EL_KPT]) {
#pragma unroll
  for (int q = 0; q < EL_KPT; ++q) {
    idx[q] = r0 + (int)threadIdx.x + q * EL_THREADS;
    own[q] = idx[q] < n;
    const float *p = g + 3 * (own[q] ? idx[q] : 0);
    px[q] = p[0], py[q] = p[1], pz[q] = p[2];
  }
}

// ws: gridDim.x slabs of 5 npad floats: remainL | remainR | ratioL | ratioR | cost (the resident form keeps the two ratios in LDS).
// The slab pointers are deliberately not __restrict__: the stage assembly reads what other threads of the workgroup wrote.
template <bool RESIDENT>
__global__ __launch_bounds__(EL_THREADS) void pairwise_emd_large_kernel(int pairs, int r, int n, int paired, EmdLargeLevels levels,
                                                                        const float *__restrict__ a, const float *__restrict__ b,
                                                                        float *ws, float *__restrict__ out) {
  extern __shared__ float4 el_lds[];  // resident: cloud a (npad float4), cloud b (npad float4); streamed: one stage (EL_STAGE float4)
  __shared__ double wcost[EL_REDUCE / 64];
  const int tid = threadIdx.x;
  const int npad = (n + 3) & ~3;
  float *remL = ws + (size_t)blockIdx.x * 5 * npad, *remR = remL + npad, *wA = remR + npad, *wB = wA + npad, *cost = wB + npad;
  float4 *A = el_lds, *B = RESIDENT ? el_lds + npad : el_lds;
  float *Af = (float *)A, *Bf = (float *)B;

  for (int pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const float *ga = a + (size_t)(paired ? pair : pair / r) * n * 3, *gb = b + (size_t)(paired ? pair : pair % r) * n * 3;
    __syncthreads();  // the previous pair's reduction has read cost and wcost
    for (int idx = tid; idx < npad; idx += EL_THREADS) {
      remL[idx] = remR[idx] = 1.0f, cost[idx] = 0.0f;
      if (RESIDENT) {
        const int src = idx < n ? idx : n - 1, o = el_slot(idx);
        Af[o] = ga[3 * src], Af[o + 2] = ga[3 * src + 1], Af[o + 4] = ga[3 * src + 2], Af[o + 6] = 0.0f;
        Bf[o] = gb[3 * src], Bf[o + 2] = gb[3 * src + 1], Bf[o + 4] = gb[3 * src + 2], Bf[o + 6] = idx < n ? 1.0f : 0.0f;
      }
    }
    __syncthreads();

    int idx[EL_KPT];
    bool own[EL_KPT];
    float px[EL_KPT], py[EL_KPT], pz[EL_KPT], rl[EL_KPT], sum[EL_KPT], csum[EL_KPT];
    for (int lv = 0; lv < 10; ++lv) {
      const float lvl2 = levels.lvl2[lv];
      // pass 1 (k): ratioL = remainL / (1e-9 + sum_l K remainR); b carries remainR
      for (int r0 = 0; r0 < n; r0 += EL_TILE) {
        emd_large_own(ga, r0, n, idx, own, px, py, pz);
#pragma unroll
        for (int q = 0; q < EL_KPT; ++q) rl[q] = 0.0f;
        emd_large_rows<RESIDENT, false>(B, gb, remR, n, npad, lvl2, px, py, pz, rl, sum, csum);
#pragma unroll
        for (int q = 0; q < EL_KPT; ++q)
          if (own[q]) {
            const float ratL = remL[idx[q]] / (1e-9f + sum[q]);
            if (RESIDENT) Af[el_slot(idx[q]) + 6] = ratL;
            else wA[idx[q]] = ratL;
          }
      }
      __syncthreads();
      // pass 2 (l): sumr = remainR sum_k K ratioL; ratioR = remainR min(remainR / (sumr + 1e-9), 1); remainR = max(0, remainR - sumr)
      for (int r0 = 0; r0 < n; r0 += EL_TILE) {
        emd_large_own(gb, r0, n, idx, own, px, py, pz);
        emd_large_rows<RESIDENT, false>(A, ga, wA, n, npad, lvl2, px, py, pz, rl, sum, csum);
#pragma unroll
        for (int q = 0; q < EL_KPT; ++q)
          if (own[q]) {
            const float rr = remR[idx[q]], sumr = rr * sum[q];
            const float ratR = rr * fminf(rr / (sumr + 1e-9f), 1.0f);
            remR[idx[q]] = fmaxf(0.0f, rr - sumr);
            if (RESIDENT) Bf[el_slot(idx[q]) + 6] = ratR;  // pass 2 reads cloud a only
            else wB[idx[q]] = ratR;
          }
      }
      __syncthreads();
      // pass 3 (k): w = K ratioL ratioR; cost += sum_l w sqrt(d^2); remainL = max(0, remainL - sum_l w); b carries ratioR
      for (int r0 = 0; r0 < n; r0 += EL_TILE) {
        emd_large_own(ga, r0, n, idx, own, px, py, pz);
#pragma unroll
        for (int q = 0; q < EL_KPT; ++q) rl[q] = own[q] ? (RESIDENT ? Af[el_slot(idx[q]) + 6] : wA[idx[q]]) : 0.0f;
        emd_large_rows<RESIDENT, true>(B, gb, wB, n, npad, lvl2, px, py, pz, rl, sum, csum);
#pragma unroll
        for (int q = 0; q < EL_KPT; ++q)
          if (own[q]) {
            cost[idx[q]] += csum[q];
            remL[idx[q]] = fmaxf(0.0f, remL[idx[q]] - sum[q]);
          }
      }
      __syncthreads();
      if (RESIDENT) {  // b carries remainR again
        for (int l = tid; l < n; l += EL_THREADS) Bf[el_slot(l) + 6] = remR[l];
        __syncthreads();
      }
    }

    // cost of the pair: lane t < 256 over k = t, t + 256, ... in double, wave_sum, the four waves in order
    if (tid < EL_REDUCE) {  // whole waves
      double t = 0.0;
      for (int k = tid; k < n; k += EL_REDUCE) t += (double)cost[k];
      t = wave_sum(t);
      if ((tid & 63) == 0) wcost[tid >> 6] = t;
    }
    __syncthreads();
    if (tid == 0) out[pair] = (float)((((wcost[0] + wcost[1]) + wcost[2]) + wcost[3]) / (double)n);
  }
}

// mode 0: resident while it fits, else streamed; 1: resident; 2: streamed.  -> BDM_OK and *resident, or the error code
static int emd_large_choose(int n, int mode, int *resident) {
  *resident = 0;
  BDM_REQUIRE(n >= 1 && mode >= 0 && mode <= 2, "pairwise_emd_large: bad n=%d or mode=%d", n, mode);
  if (n > EL_MAX_N) {
    set_error("pairwise_emd_large: n=%d exceeds the limit of %d points per cloud", n, EL_MAX_N);
    return BDM_ERR_UNSUPPORTED;
  }
  if (mode == 1 && n > EL_RESIDENT_MAX_N) {
    set_error("pairwise_emd_large: n=%d does not fit the resident form (at most %d points)", n, EL_RESIDENT_MAX_N);
    return BDM_ERR_UNSUPPORTED;
  }
  *resident = mode == 1 || (mode == 0 && n <= EL_RESIDENT_MAX_N);
  return BDM_OK;
}

static size_t emd_large_ws_bytes(long long pairs, int n) {
  if (pairs < 1 || pairs >= (1ll << 31) || n < 1 || n > EL_MAX_N) return 0;
  const size_t npad = (size_t)((n + 3) & ~3);
  return (size_t)(pairs < EL_SLABS ? pairs : EL_SLABS) * 5 * npad * sizeof(float);
}

}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_pairwise_emd_large_workspace_bytes(int pairs, int n) { return emd_large_ws_bytes(pairs, n); }

extern "C" int bdm_pairwise_emd_large_variant(int n, int mode, int *resident, int *threads, int *kpt, int *stage) {
  int res = 0;
  const int rc = emd_large_choose(n, mode, &res);
  if (resident) *resident = rc == BDM_OK ? res : 0;
  if (threads) *threads = rc == BDM_OK ? EL_THREADS : 0;
  if (kpt) *kpt = rc == BDM_OK ? EL_KPT : 0;
  if (stage) *stage = rc == BDM_OK && !res ? EL_STAGE : 0;
  return rc;
}

extern "C" int bdm_pairwise_emd_large(int s, int r, int n, int paired, int mode, const float *a, const float *b, void *workspace,
                                      size_t workspace_bytes, float *out, void *stream) {
  BDM_REQUIRE(s >= 0 && r >= 0 && n >= 1, "pairwise_emd_large: bad sizes s=%d r=%d n=%d", s, r, n);
  BDM_REQUIRE(paired == 0 || paired == 1, "pairwise_emd_large: paired=%d is neither 0 nor 1", paired);
  BDM_REQUIRE(!paired || s == r, "pairwise_emd_large: paired needs s == r, got %d and %d", s, r);
  int resident = 0;
  const int rc = emd_large_choose(n, mode, &resident);
  if (rc != BDM_OK) return rc;
  if (s == 0 || r == 0) return BDM_OK;
  const long long pairs = paired ? (long long)s : (long long)s * r;
  BDM_REQUIRE(pairs < (1ll << 31), "pairwise_emd_large: %d x %d pairs exceed the grid", s, r);
  BDM_REQUIRE(a && b && out && workspace, "pairwise_emd_large: null pointer");
  const size_t need = emd_large_ws_bytes(pairs, n);
  BDM_REQUIRE(workspace_bytes >= need, "pairwise_emd_large: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  EmdLargeLevels levels;
  for (int lv = 0; lv < 10; ++lv) {
    const int j = 7 - lv;
    double level = 0.0;  // -4^j, 0 at j = -2
    if (j != -2) {
      level = -1.0;
      for (int e = 0; e < (j < 0 ? -j : j); ++e) level = j < 0 ? level / 4.0 : level * 4.0;
    }
    levels.lvl2[lv] = (float)(level * 1.4426950408889634074);
  }
  const int npad = (n + 3) & ~3;
  const dim3 grid((unsigned)(pairs < EL_SLABS ? pairs : EL_SLABS)), block(EL_THREADS);
  if (resident) {
    const size_t lds = (size_t)2 * npad * sizeof(float4);
    BDM_ALLOW_LDS(pairwise_emd_large_kernel<true>, lds);
    hipLaunchKernelGGL(pairwise_emd_large_kernel<true>, grid, block, lds, (hipStream_t)stream, (int)pairs, r, n, paired, levels, a, b,
                       (float *)workspace, out);
  } else {
    hipLaunchKernelGGL(pairwise_emd_large_kernel<false>, grid, block, EL_STAGE * sizeof(float4), (hipStream_t)stream, (int)pairs, r, n,
                       paired, levels, a, b, (float *)workspace, out);
  }
  return launch_status("pairwise_emd_large");
}
