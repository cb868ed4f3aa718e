// Generation metrics (section 7 of bdm_hip.h): the all-pairs cloud-to-cloud distance matrices that MMD, COV and 1-NNA are
// reduced from (bdm_amd/metrics.py).  Two kernels, both without atomics and with a fixed reduction order per matrix entry:
// entry (i, j) of an S x R call carries the bits of the 1 x 1 call on clouds i and j.
//
//   pairwise_chamfer_kernel  one direction of the Chamfer matrix; launched twice with the roles swapped
//   pairwise_emd_kernel      approximate-match EMD (Fan et al.'s approxmatch + matchcost), one workgroup per pair
//
// Both inner loops run on PAIRS of target points: the staged cloud is kept in LDS as (x0, x1, y0, y1) (z0, z1, w0, w1) so that one
// broadcast read feeds two-wide packed fp32 arithmetic (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32).  DESIGN.md section 10.
#include "common.h"
#include "bdm_hip.h"

namespace bdm {

typedef float f2 __attribute__((ext_vector_type(2)));

// -------------------------------------------------------------------------------------
// Chamfer, one direction: out[i * os + j * ot] = mean over the n points p of source cloud i of min over the m points q of
// target cloud j of |p - q|^2 (difference form).  One workgroup owns source cloud i and walks `tj` target clouds; every thread
// keeps P source points in registers; the target cloud passes through LDS in stages of CH_TM points.
// The sum of entry (i, j): per thread over its P points, then wave_sum, then the four waves in order, then the source chunks
// (of 256 P points) in order -- a function of n alone (P is chosen from n), never of s, r or tj.
// -------------------------------------------------------------------------------------
constexpr int CH_THREADS = 256;
constexpr int CH_TM = 1024;    // target points per LDS stage
constexpr int CH_TJ_MAX = 8;   // target clouds per workgroup

template <int P>
__global__ __launch_bounds__(CH_THREADS) void pairwise_chamfer_kernel(int r, int n, int m, int tj, long long os, long long ot,
                                                                      const float *__restrict__ a, const float *__restrict__ b,
                                                                      float *__restrict__ out) {
  __shared__ float4 sxy[CH_TM / 2];  // pair q of the stage: (x0, x1, y0, y1)
  __shared__ float2 sz[CH_TM / 2];   //                      (z0, z1)
  __shared__ float wsum[CH_THREADS / 64];
  __shared__ float acc[CH_TJ_MAX];
  const int tid = threadIdx.x;
  const int ntiles = (r + tj - 1) / tj;
  const int i = blockIdx.x / ntiles, j0 = (blockIdx.x % ntiles) * tj, j1 = min(r, j0 + tj);
  if (tid < CH_TJ_MAX) acc[tid] = 0.0f;

  for (int c0 = 0; c0 < n; c0 += CH_THREADS * P) {
    float px[P], py[P], pz[P];
    bool valid[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int idx = c0 + tid + CH_THREADS * p;
      valid[p] = idx < n;
      const float *s = a + ((size_t)i * n + (valid[p] ? idx : 0)) * 3;
      px[p] = s[0], py[p] = s[1], pz[p] = s[2];
    }
    for (int j = j0; j < j1; ++j) {
      float best[P];
#pragma unroll
      for (int p = 0; p < P; ++p) best[p] = INFINITY;
      for (int t0 = 0; t0 < m; t0 += CH_TM) {
        const int len = min(CH_TM, m - t0), npairs = (len + 1) >> 1;
        __syncthreads();
        for (int q = tid; q < npairs; q += CH_THREADS) {  // an odd tail repeats its last point: the minimum does not change
          const float *t0p = b + ((size_t)j * m + t0 + 2 * q) * 3;
          const float *t1p = (2 * q + 1 < len) ? t0p + 3 : t0p;
          sxy[q] = make_float4(t0p[0], t1p[0], t0p[1], t1p[1]);
          sz[q] = make_float2(t0p[2], t1p[2]);
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < npairs; ++q) {
          const float4 xy = sxy[q];
          const float2 zz = sz[q];
          const f2 qx = {xy.x, xy.y}, qy = {xy.z, xy.w}, qz = {zz.x, zz.y};
#pragma unroll
          for (int p = 0; p < P; ++p) {
            const f2 dx = qx - px[p], dy = qy - py[p], dz = qz - pz[p];
            f2 d = dx * dx;
            d = __builtin_elementwise_fma(dy, dy, d);
            d = __builtin_elementwise_fma(dz, dz, d);
            best[p] = fminf(fminf(best[p], d.x), d.y);  // v_min3_f32
          }
        }
      }
      float sum = 0.0f;
#pragma unroll
      for (int p = 0; p < P; ++p) sum += valid[p] ? best[p] : 0.0f;
      sum = wave_sum(sum);
      if ((tid & 63) == 0) wsum[tid >> 6] = sum;
      __syncthreads();
      if (tid == 0) acc[j - j0] += ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
      // wsum is rewritten only behind the two barriers of the next cloud's first stage (m >= 1)
    }
  }
  __syncthreads();
  if (tid < j1 - j0) out[(size_t)i * os + (size_t)(j0 + tid) * ot] = acc[tid] / (float)n;
}

// the instance one direction runs: P source points per thread from n alone, tj target clouds per workgroup from the grid it leaves
static void chamfer_choose(int s, int r, int n, int *p, int *tj) {
  *p = n <= CH_THREADS ? 1 : n <= 2 * CH_THREADS ? 2 : n <= 4 * CH_THREADS ? 4 : 8;
  int t = CH_TJ_MAX;
  while (t > 1 && (long long)s * cdiv(r, t) < 1024) t >>= 1;  // keep the 256 CUs busy on small matrices
  *tj = t;
}

// one direction for every (source cloud, target cloud)
static int chamfer_one_side(int s, int r, int n, int m, const float *a, const float *b, float *out, long long os, long long ot,
                            hipStream_t stream) {
  int P, tj;
  chamfer_choose(s, r, n, &P, &tj);
  const long long blocks = (long long)s * cdiv(r, tj);
  BDM_REQUIRE(blocks < (1ll << 31), "pairwise_chamfer: %d x %d clouds exceed the grid", s, r);
  const dim3 grid((unsigned)blocks), block(CH_THREADS);
  if (P == 1)
    hipLaunchKernelGGL(pairwise_chamfer_kernel<1>, grid, block, 0, stream, r, n, m, tj, os, ot, a, b, out);
  else if (P == 2)
    hipLaunchKernelGGL(pairwise_chamfer_kernel<2>, grid, block, 0, stream, r, n, m, tj, os, ot, a, b, out);
  else if (P == 4)
    hipLaunchKernelGGL(pairwise_chamfer_kernel<4>, grid, block, 0, stream, r, n, m, tj, os, ot, a, b, out);
  else
    hipLaunchKernelGGL(pairwise_chamfer_kernel<8>, grid, block, 0, stream, r, n, m, tj, os, ot, a, b, out);
  return launch_status("pairwise_chamfer");
}

// -------------------------------------------------------------------------------------
// Approximate-match EMD of one pair per workgroup.  Both clouds sit in LDS in the pair layout with a fourth component per point:
// cloud a carries ratioL, cloud b carries remainR (passes 1) or ratioR (pass 3).  Thread t owns the indices t + q T (q < KPT,
// T = blockDim.x) as k in passes 1 and 3 and as l in pass 2 and keeps remainL[k], remainR[l] and its share of the cost in registers.
// The clouds are padded to a multiple of 4 points with copies of the last point whose fourth component stays 0: they add exact zeros.
// K = exp(level d^2) is v_exp_f32(d^2 * (level log2 e)), the product rounded once on the host.
// -------------------------------------------------------------------------------------
constexpr int EMD_MAX_THREADS = 1024;
constexpr int EMD_MAX_N = 2 * EMD_MAX_THREADS;

// s[k] = sum over the staged cloud of K(k, .) w(.); COST (pass 3): s[k] = sum of (K(k, .) rl[k]) w(.), c[k] = the same terms times sqrt(d^2).
// Four partial sums per k (two pairs in flight).  Pass 3 multiplies every term by ratioL as the definition writes it: with ratioL
// factored out of the two sums instead, one pair of the n = 1000 test case came out 2.2e-5 from the float64 restatement (a CPU
// emulation of the kernel's arithmetic reproduces that figure; this form measures 7.9e-8 on that pair).
template <int KPT, bool COST>
__device__ __forceinline__ void emd_sweep(const float4 *__restrict__ cloud, int npairs, float lvl2, const float (&px)[KPT],
                                          const float (&py)[KPT], const float (&pz)[KPT], const float (&rl)[KPT], float (&s)[KPT],
                                          float (&c)[KPT]) {
  f2 s0[KPT], s1[KPT], c0[KPT], c1[KPT];
#pragma unroll
  for (int q = 0; q < KPT; ++q) s0[q] = s1[q] = c0[q] = c1[q] = f2{0.0f, 0.0f};
  for (int pr = 0; pr < npairs; pr += 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 xy = cloud[2 * (pr + h)], zw = cloud[2 * (pr + h) + 1];
      const f2 qx = {xy.x, xy.y}, qy = {xy.z, xy.w}, qz = {zw.x, zw.y}, w = {zw.z, zw.w};
#pragma unroll
      for (int q = 0; q < KPT; ++q) {
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
          sa += kw;
          ca = __builtin_elementwise_fma(kw, rt, ca);
        } else {
          sa = __builtin_elementwise_fma(kk, w, sa);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    s[q] = (s0[q].x + s0[q].y) + (s1[q].x + s1[q].y);
    c[q] = (c0[q].x + c0[q].y) + (c1[q].x + c1[q].y);
  }
}

struct EmdLevels {
  float lvl2[10];  // level * log2(e) for j = 7 .. -2
};

template <int KPT>
__global__ __launch_bounds__(EMD_MAX_THREADS) void pairwise_emd_kernel(int r, int n, EmdLevels levels, const float *__restrict__ a,
                                                                       const float *__restrict__ b, float *__restrict__ out) {
  extern __shared__ float4 emd_lds[];
  __shared__ double wcost[EMD_MAX_THREADS / 64];
  const int tid = threadIdx.x, T = blockDim.x;
  const int npad = (n + 3) & ~3, npairs = npad >> 1;
  float4 *A = emd_lds, *B = emd_lds + npad;  // pair q: [2q] = (x0, x1, y0, y1), [2q + 1] = (z0, z1, w0, w1)
  float *Af = (float *)A, *Bf = (float *)B;
  const float *ga = a + (size_t)(blockIdx.x / r) * n * 3, *gb = b + (size_t)(blockIdx.x % r) * n * 3;

  for (int idx = tid; idx < npad; idx += T) {
    const int src = idx < n ? idx : n - 1, o = 8 * (idx >> 1) + (idx & 1);
    Af[o] = ga[3 * src], Af[o + 2] = ga[3 * src + 1], Af[o + 4] = ga[3 * src + 2], Af[o + 6] = 0.0f;
    Bf[o] = gb[3 * src], Bf[o + 2] = gb[3 * src + 1], Bf[o + 4] = gb[3 * src + 2], Bf[o + 6] = idx < n ? 1.0f : 0.0f;
  }
  __syncthreads();

  int wslot[KPT];  // float offset of the fourth component of the owned index (the same in both clouds)
  bool own[KPT];
  float ax[KPT], ay[KPT], az[KPT], bx[KPT], by[KPT], bz[KPT], remL[KPT], remR[KPT], ratL[KPT], cost[KPT];
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const int idx = tid + q * T;
    own[q] = idx < n;
    const int o = own[q] ? 8 * (idx >> 1) + (idx & 1) : 0;  // threads without an index compute on point 0 and write nothing
    wslot[q] = o + 6;
    ax[q] = Af[o], ay[q] = Af[o + 2], az[q] = Af[o + 4];
    bx[q] = Bf[o], by[q] = Bf[o + 2], bz[q] = Bf[o + 4];
    remL[q] = remR[q] = 1.0f;
    ratL[q] = cost[q] = 0.0f;
  }

  float sum[KPT], csum[KPT];
  for (int lv = 0; lv < 10; ++lv) {
    const float lvl2 = levels.lvl2[lv];
    // pass 1 (k): ratioL = remainL / (1e-9 + sum_l K remainR)
    emd_sweep<KPT, false>(B, npairs, lvl2, ax, ay, az, ratL, sum, csum);
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      ratL[q] = remL[q] / (1e-9f + sum[q]);
      if (own[q]) Af[wslot[q]] = ratL[q];
    }
    __syncthreads();
    // pass 2 (l): sumr = remainR sum_k K ratioL; ratioR = remainR min(remainR / (sumr + 1e-9), 1); remainR = max(0, remainR - sumr)
    emd_sweep<KPT, false>(A, npairs, lvl2, bx, by, bz, ratL, sum, csum);
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const float sumr = remR[q] * sum[q];
      const float ratR = remR[q] * fminf(remR[q] / (sumr + 1e-9f), 1.0f);
      remR[q] = fmaxf(0.0f, remR[q] - sumr);
      if (own[q]) Bf[wslot[q]] = ratR;
    }
    __syncthreads();
    // pass 3 (k): w = K ratioL ratioR; cost += sum_l w sqrt(d^2); remainL = max(0, remainL - sum_l w)
    emd_sweep<KPT, true>(B, npairs, lvl2, ax, ay, az, ratL, sum, csum);
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      cost[q] += csum[q];
      remL[q] = fmaxf(0.0f, remL[q] - sum[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KPT; ++q)
      if (own[q]) Bf[wslot[q]] = remR[q];
    __syncthreads();
  }

  // cost of the pair: per thread over its indices, wave_sum, then the waves in order (double: the order is fixed either way)
  double total = 0.0;
#pragma unroll
  for (int q = 0; q < KPT; ++q) total += own[q] ? (double)cost[q] : 0.0;
  total = wave_sum(total);
  if ((tid & 63) == 0) wcost[tid >> 6] = total;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < (T >> 6); ++w) t += wcost[w];
    out[blockIdx.x] = (float)(t / (double)n);
  }
}

}  // namespace bdm

using namespace bdm;

extern "C" int bdm_pairwise_chamfer(int s, int r, int n, int m, const float *a, const float *b, float *out_ab, float *out_ba,
                                    void *stream) {
  BDM_REQUIRE(s >= 0 && r >= 0 && n >= 1 && m >= 1, "pairwise_chamfer: bad sizes s=%d r=%d n=%d m=%d", s, r, n, m);
  if (s == 0 || r == 0) return BDM_OK;
  BDM_REQUIRE(a && b, "pairwise_chamfer: null cloud pointer");
  if (out_ab) {
    const int rc = chamfer_one_side(s, r, n, m, a, b, out_ab, r, 1, (hipStream_t)stream);
    if (rc != BDM_OK) return rc;
  }
  if (out_ba) {  // the same kernel with the roles swapped, written transposed: out_ba stays (s, r)
    const int rc = chamfer_one_side(r, s, m, n, b, a, out_ba, 1, r, (hipStream_t)stream);
    if (rc != BDM_OK) return rc;
  }
  return BDM_OK;
}

extern "C" int bdm_pairwise_chamfer_variant(int s, int r, int n, int *p, int *tj) {
  int P = 0, t = 0;
  const bool ok = s >= 1 && r >= 1 && n >= 1;
  if (ok) chamfer_choose(s, r, n, &P, &t);
  if (p) *p = P;
  if (tj) *tj = t;
  BDM_REQUIRE(ok, "pairwise_chamfer_variant: bad sizes s=%d r=%d n=%d", s, r, n);
  return BDM_OK;
}

extern "C" int bdm_pairwise_emd_approx(int s, int r, int n, const float *a, const float *b, float *out, void *stream) {
  BDM_REQUIRE(s >= 0 && r >= 0 && n >= 1, "pairwise_emd_approx: bad sizes s=%d r=%d n=%d", s, r, n);
  if (n > EMD_MAX_N) {
    set_error("pairwise_emd_approx: n=%d exceeds the %d points per cloud one workgroup holds", n, EMD_MAX_N);
    return BDM_ERR_UNSUPPORTED;
  }
  if (s == 0 || r == 0) return BDM_OK;
  BDM_REQUIRE(a && b && out, "pairwise_emd_approx: null pointer");
  BDM_REQUIRE((long long)s * r < (1ll << 31), "pairwise_emd_approx: %d x %d pairs exceed the grid", s, r);
  EmdLevels levels;
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
  const size_t lds = (size_t)2 * npad * sizeof(float4);
  const dim3 grid((unsigned)((long long)s * r));
  if (n <= EMD_MAX_THREADS) {
    BDM_ALLOW_LDS(pairwise_emd_kernel<1>, lds);
    hipLaunchKernelGGL(pairwise_emd_kernel<1>, grid, dim3(cdiv(n, 64) * 64), lds, (hipStream_t)stream, r, n, levels, a, b, out);
  } else {
    BDM_ALLOW_LDS(pairwise_emd_kernel<2>, lds);
    hipLaunchKernelGGL(pairwise_emd_kernel<2>, grid, dim3(EMD_MAX_THREADS), lds, (hipStream_t)stream, r, n, levels, a, b, out);
  }
  return launch_status("pairwise_emd_approx");
}
