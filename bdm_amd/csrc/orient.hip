// Consistent orientation of point-cloud normals by visibility voting (section 11 of bdm_hip.h).
//
// orient_vote_kernel: one workgroup per (cloud, view).  Every workgroup forms the cloud's bounding-box centre c and scale h itself
// (exact minima and maxima, so all views of a cloud agree bit for bit and nothing has to be handed between kernels), keeps the
// r x r z-buffer of depth keys in LDS, splats every finite point into it with integer atomicMin, and after a barrier writes one
// byte per point: 0 = not visible in this view, 2 + sigma = visible with sigma in {-1, 0, +1}.
// orient_decide_kernel: one workgroup per cloud.  It sums the bytes of every point over the views (integer sums: any order gives
// the same bits), keeps the state s of the cloud twice in LDS (one byte per point), runs the Jacobi rounds of the fallback on it
// and writes the normals with their sign.  Every loop is bounded by an argument of the launch; nothing waits on another workgroup.
//
// The file is compiled with -ffp-contract=off and correctly rounded division and sqrt (Makefile): the projection defines integers.
#include "common.h"
#include "bdm_hip.h"

namespace bdm {

constexpr int ORI_THREADS = 1024;
constexpr int ORI_WAVES = ORI_THREADS / 64;
constexpr int ORI_N_MAX = 32768;     // two state buffers of one byte per point in 64 KiB of LDS
constexpr int ORI_R_MAX = 128;       // r x r uint32 depth keys in 64 KiB of LDS
constexpr int ORI_SCRATCH = 8 * ORI_WAVES;   // words of the z-buffer the reductions borrow before it is filled
constexpr unsigned int ORI_FAR = 0xffffffffu;

__device__ __forceinline__ float dot3(float x, float y, float z, float a, float b, float c) {
  return __fadd_rn(__fadd_rn(__fmul_rn(x, a), __fmul_rn(y, b)), __fmul_rn(z, c));
}

// clamp(floor(f), 0, hi) as an integer; NaN -> 0
__device__ __forceinline__ int floor_clamp(float f, int hi) {
  const float g = floorf(f);
  return !(g >= 0.0f) ? 0 : (g >= (float)hi ? hi : (int)g);
}

__device__ __forceinline__ int sgn_f(float f) { return f > 0.0f ? 1 : (f < 0.0f ? -1 : 0); }   // NaN -> 0

__device__ __forceinline__ float wave_min_all(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

__global__ __launch_bounds__(ORI_THREADS) void orient_vote_kernel(int n, int v, int r, int splat, int eps,
                                                                  const float *__restrict__ points,
                                                                  const float *__restrict__ normals,
                                                                  const float *__restrict__ views,
                                                                  unsigned char *__restrict__ codes) {
  extern __shared__ unsigned int zb[];   // max(r * r, 2 * ORI_SCRATCH) words
  float *scratch = reinterpret_cast<float *>(zb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cloud = blockIdx.x / v, view = blockIdx.x % v;
  const float *pts = points + (size_t)cloud * n * 3;
  const float *nrm = normals + (size_t)cloud * n * 3;
  unsigned char *out = codes + ((size_t)cloud * v + view) * n;

  // bounding box of the finite points
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = tid; i < n; i += ORI_THREADS) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (finite3(x, y, z)) {
      lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min_all(lo[a]), hi[a] = wave_max_all(hi[a]);
    if (lane == 0) scratch[wave * 8 + a] = lo[a], scratch[wave * 8 + 3 + a] = hi[a];
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int w = 0; w < ORI_WAVES; ++w) lo[a] = fminf(lo[a], scratch[w * 8 + a]), hi[a] = fmaxf(hi[a], scratch[w * 8 + 3 + a]);
  const bool any_finite = lo[0] <= hi[0];   // false when no point was finite (+inf against -inf)
  const float cx = __fmul_rn(0.5f, __fadd_rn(lo[0], hi[0])), cy = __fmul_rn(0.5f, __fadd_rn(lo[1], hi[1])),
              cz = __fmul_rn(0.5f, __fadd_rn(lo[2], hi[2]));

  // rho = the largest squared distance from the centre (a maximum: exact, any order)
  float rho = 0.0f;
  if (any_finite)
    for (int i = tid; i < n; i += ORI_THREADS) {
      const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
      if (finite3(x, y, z)) {
        const float qx = __fsub_rn(x, cx), qy = __fsub_rn(y, cy), qz = __fsub_rn(z, cz);
        rho = fmaxf(rho, dot3(qx, qy, qz, qx, qy, qz));
      }
    }
  rho = wave_max_all(rho);
  if (lane == 0) scratch[ORI_SCRATCH + wave] = rho;
  __syncthreads();
  for (int w = 0; w < ORI_WAVES; ++w) rho = fmaxf(rho, scratch[ORI_SCRATCH + w]);
  if (!any_finite || !(rho > 0.0f)) {   // uniform over the workgroup: nothing is visible
    for (int i = tid; i < n; i += ORI_THREADS) out[i] = 0;
    return;
  }
  const float h = __fmul_rn(1.02f, __fsqrt_rn(rho));
  const float half_r = 0.5f * (float)r;
  const float *vw = views + 9 * (size_t)view;
  const float ux = vw[0], uy = vw[1], uz = vw[2], wx = vw[3], wy = vw[4], wz = vw[5], dx = vw[6], dy = vw[7], dz = vw[8];

  __syncthreads();   // the scratch words have been read
  for (int p = tid; p < r * r; p += ORI_THREADS) zb[p] = ORI_FAR;
  __syncthreads();

  // pixel and depth key of point i (the same instructions in both passes: the same integers)
  auto project = [&](int i, int &X, int &Y, int &Z) -> bool {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (!finite3(x, y, z)) return false;
    const float qx = __fsub_rn(x, cx), qy = __fsub_rn(y, cy), qz = __fsub_rn(z, cz);
    const float a = dot3(qx, qy, qz, ux, uy, uz), b = dot3(qx, qy, qz, wx, wy, wz), t = dot3(qx, qy, qz, dx, dy, dz);
    X = floor_clamp(__fmul_rn(__fadd_rn(__fdiv_rn(a, h), 1.0f), half_r), r - 1);
    Y = floor_clamp(__fmul_rn(__fadd_rn(__fdiv_rn(b, h), 1.0f), half_r), r - 1);
    Z = floor_clamp(__fmul_rn(__fsub_rn(1.0f, __fdiv_rn(t, h)), 32768.0f), 65535);
    return true;
  };

  for (int i = tid; i < n; i += ORI_THREADS) {
    int X, Y, Z;
    if (!project(i, X, Y, Z)) continue;
    const int x0 = max(X - splat, 0), x1 = min(X + splat, r - 1), y0 = max(Y - splat, 0), y1 = min(Y + splat, r - 1);
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) atomicMin(&zb[x * r + y], (unsigned int)Z);   // x * r + y < r * r: both clamped to [0, r)
  }
  __syncthreads();
  for (int i = tid; i < n; i += ORI_THREADS) {
    int X, Y, Z;
    unsigned char code = 0;
    if (project(i, X, Y, Z) && (unsigned int)Z <= zb[X * r + Y] + (unsigned int)eps)   // zb <= Z <= 65535 here: no wrap
      code = (unsigned char)(2 + sgn_f(dot3(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], dx, dy, dz)));
    out[i] = code;
  }
}

__global__ __launch_bounds__(ORI_THREADS) void orient_decide_kernel(int n, int k, int v, int kg, int rounds,
                                                                    const float *__restrict__ normals_in,
                                                                    const int *__restrict__ knn_idx,
                                                                    const unsigned char *__restrict__ codes,
                                                                    float *__restrict__ normals_out, int *__restrict__ votes,
                                                                    int *__restrict__ seen, int *__restrict__ undecided) {
  extern __shared__ signed char state[];   // two buffers of n_pad bytes
  __shared__ int changed[33], count;
  const int tid = threadIdx.x, cloud = blockIdx.x;
  const int n_pad = (n + 3) & ~3;
  signed char *cur = state, *nxt = state + n_pad;
  const float *nrm = normals_in + (size_t)cloud * n * 3;
  const int *idx = knn_idx + (size_t)cloud * n * k;
  const unsigned char *cd = codes + (size_t)cloud * v * n;

  if (tid < 33) changed[tid] = 0;
  if (tid == 0) count = 0;
  for (int i = tid; i < n; i += ORI_THREADS) {
    int vt = 0, sn = 0;
    for (int w = 0; w < v; ++w) {
      const int c = cd[(size_t)w * n + i];
      vt += c ? c - 2 : 0;
      sn += c != 0;
    }
    if (votes) votes[(size_t)cloud * n + i] = vt;
    if (seen) seen[(size_t)cloud * n + i] = sn;
    cur[i] = (signed char)(vt > 0 ? 1 : (vt < 0 ? -1 : 0));
  }
  __syncthreads();

  for (int round = 0; round < rounds; ++round) {
    for (int i = tid; i < n; i += ORI_THREADS) {
      int s = cur[i];
      if (s == 0) {
        const float nx = nrm[3 * (size_t)i], ny = nrm[3 * (size_t)i + 1], nz = nrm[3 * (size_t)i + 2];
        int t = 0, taken = 0;
        for (int e = 0; e < k && taken < kg; ++e) {
          const int j = idx[(size_t)i * k + e];
          if (j < 0 || j >= n || j == i) continue;   // j >= n cannot come from bdm_estimate_normals: kept out of the address
          ++taken;
          const int sj = cur[j];
          if (sj != 0) t += sj * sgn_f(dot3(nx, ny, nz, nrm[3 * (size_t)j], nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2]));
        }
        s = t > 0 ? 1 : (t < 0 ? -1 : 0);
        if (s != 0) changed[round] = 1;
      }
      nxt[i] = (signed char)s;
    }
    __syncthreads();
    signed char *tmp = cur;
    cur = nxt, nxt = tmp;
    if (!changed[round]) break;   // uniform: written before the barrier, never written again
  }

  int mine = 0;
  for (int i = tid; i < n; i += ORI_THREADS) {
    const int s = cur[i];
    mine += s == 0;
    const unsigned int flip = s < 0 ? 0x80000000u : 0u;
    const size_t row = ((size_t)cloud * n + i) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) normals_out[row + a] = __uint_as_float(__float_as_uint(normals_in[row + a]) ^ flip);
  }
  if (undecided) {
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if (tid == 0) undecided[cloud] = count;
  }
}

static bool orient_sizes_ok(int b, int n, int v) { return b >= 0 && n >= 1 && n <= ORI_N_MAX && v >= 1 && v <= 256; }

}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_orient_normals_workspace_bytes(int b, int n, int v) {
  return orient_sizes_ok(b, n, v) ? (size_t)b * (size_t)n * (size_t)v : 0;
}

extern "C" int bdm_orient_normals(int b, int n, int k, int v, int r, int splat, int eps, int kg, int rounds, const float *points,
                                  const float *normals_in, const int *knn_idx, const float *views, float *normals_out, int *votes,
                                  int *seen, int *undecided, void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0 && n >= 1 && n <= ORI_N_MAX, "orient_normals: bad sizes b=%d n=%d (n in 1..%d: a cloud's state lives in LDS)", b,
              n, ORI_N_MAX);
  BDM_REQUIRE(k >= 1 && (long long)b * n * k < (1ll << 31), "orient_normals: k=%d below 1, or b n k = %lld exceeds int", k,
              (long long)b * n * k);
  BDM_REQUIRE(v >= 1 && v <= 256 && (long long)b * v < (1ll << 31), "orient_normals: v=%d outside 1..256, or b v exceeds int", v);
  BDM_REQUIRE(r >= 1 && r <= ORI_R_MAX, "orient_normals: r=%d outside 1..%d (the z-buffer lives in LDS)", r, ORI_R_MAX);
  BDM_REQUIRE(splat >= 0 && splat <= 4, "orient_normals: splat=%d outside 0..4", splat);
  BDM_REQUIRE(eps >= 0 && eps <= 65535, "orient_normals: eps=%d outside 0..65535", eps);
  BDM_REQUIRE(kg >= 1 && kg <= k, "orient_normals: kg=%d outside 1..k=%d", kg, k);
  BDM_REQUIRE(rounds >= 0 && rounds <= 32, "orient_normals: rounds=%d outside 0..32", rounds);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(points && normals_in && knn_idx && views && normals_out && workspace, "orient_normals: null pointer");
  BDM_REQUIRE(normals_out != normals_in, "orient_normals: normals_out must not alias normals_in");
  unsigned char *codes = (unsigned char *)workspace;
  const int zwords = r * r > 2 * ORI_SCRATCH ? r * r : 2 * ORI_SCRATCH;
  const size_t vote_lds = (size_t)zwords * sizeof(unsigned int), decide_lds = 2 * (size_t)((n + 3) & ~3);
  BDM_ALLOW_LDS(orient_vote_kernel, vote_lds);
  BDM_ALLOW_LDS(orient_decide_kernel, decide_lds);
  hipLaunchKernelGGL(orient_vote_kernel, dim3((unsigned)(b * v)), dim3(ORI_THREADS), vote_lds, (hipStream_t)stream, n, v, r, splat,
                     eps, points, normals_in, views, codes);
  hipLaunchKernelGGL(orient_decide_kernel, dim3((unsigned)b), dim3(ORI_THREADS), decide_lds, (hipStream_t)stream, n, k, v, kg, rounds,
                     normals_in, knn_idx, codes, normals_out, votes, seen, undecided);
  return launch_status("orient_normals");
}
