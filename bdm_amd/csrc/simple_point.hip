// simple_point.hip -- gfx950 kernels of the simple point denoiser (SimplePointModel, simple/simple_model.py:9-34, and the
// first half of PVCNN2PlusPlus): input projection with the positional encoding generated in registers, and ONE kernel per
// gated feed-forward layer that never writes the 512-wide hidden layer.
//
// Layout: the model state x is channel-first (b, 128, n).  A workgroup owns one SLICE of 128 consecutive points of one shape;
// its four waves own 32 points each, the point index on the MFMA column (lane & 31).
//
// Layer algebra (FeedForward with LayerNorm(384) over x_in = [x, max_N x, std_N x], simple_model_utils.py:158-201).  With
// mu_p / sigma_p the per-point LayerNorm statistics over all 384 channels, ms = [max, std] (per shape) and mbar its mean:
//   W . LN(x_in) = (1/sigma_p) [ (W_x diag(g_x)) (x_p - mu_p) + W_ms diag(g_ms) (ms - mbar) + (mbar - mu_p) d ] + W beta
// d = W_ms g_ms.  The first term is a K = 128 GEMM per point on (x_p - mu_p), subtracted before the MFMA; the second is a
// 1024-wide vector per shape (bdm_simple_layer_prep); d and W beta are per-layer constants packed on the host.
// The layer is 0.39 MFLOP per point instead of the plain form's 0.92.
//
// Pooling: every kernel that writes x also leaves, per 128-point slice and channel, max (float) and sum / sum of squares
// (double), reduced in a fixed order.  bdm_simple_layer_prep merges the slices of a shape in slice order: a shape's results
// do not depend on the batch it is run in, nor on the number of workgroups.
//
// All contractions: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).
#include "../../include/bdm_hip.h"
#include "common.h"

using namespace bdm;
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

constexpr int kD = 128;            // model width
constexpr int kHid = 512;          // hidden width (4 * dim)
constexpr int kSlice = 128;        // points per pooling slice = per workgroup
constexpr int kChunks = kHid / 32; // hidden chunks of 32 rows
constexpr int kState = 1296;       // floats per shape: ms[256], msum, Q, (pad to 272), c[1024]
constexpr int kStateC = 272;
constexpr int kFreqs = 10;         // PositionalEncoding(N_freqs=10): 3 + 60 channels

__host__ __device__ inline int n_slices(int n) { return (n + kSlice - 1) / kSlice; }

// row of accumulator register r of a 32x32 tile in lane half h
__device__ inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct Partials {  // [b][slice][channel]
  float *mx;
  double *sum, *sq;
};

__host__ __device__ inline Partials partials_of(void *ws, int b, int n) {
  const size_t cnt = (size_t)b * n_slices(n) * kD;
  Partials p;
  p.mx = (float *)ws;
  p.sum = (double *)((char *)ws + cnt * sizeof(float));
  p.sq = p.sum + cnt;
  return p;
}

// Epilogue shared by the input projection and the layers: store the wave's 32 points x 128 channels (acc[ob][r] is channel
// 32 ob + acc_row(r, h) of point p) and leave the slice's pooling partials.  Fixed order: points in index order within each
// wave's 32, then the four waves in order.
__device__ void store_and_pool(const f32x16 (&acc)[4], float *yb, int n, int p0, int slice, Partials part, int bi, int nsl) {
  __shared__ float tile[64][kSlice + 1];
  __shared__ float rmax[4][64];
  __shared__ double rsum[4][64], rsq[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int pl = wave * 32 + li, p = p0 + pl;
  const int nvalid = min(kSlice, n - p0);
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (p < n) yb[(size_t)(32 * ob + acc_row(r, h)) * n + p] = acc[ob][r];
#pragma unroll
  for (int half = 0; half < 2; ++half) {  // channels [64 half, 64 half + 64)
    __syncthreads();
#pragma unroll
    for (int ob = 2 * half; ob < 2 * half + 2; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[32 * (ob - 2 * half) + acc_row(r, h)][pl] = acc[ob][r];
    __syncthreads();
    const int c = tid & 63, q = tid >> 6;  // channel, quarter of 32 points
    float m = -INFINITY;
    double s = 0.0, s2 = 0.0;
    for (int j = 32 * q; j < min(32 * q + 32, nvalid); ++j) {
      const float v = tile[c][j];
      m = fmaxf(m, v);
      s += (double)v;
      s2 += (double)v * (double)v;
    }
    rmax[q][c] = m;
    rsum[q][c] = s;
    rsq[q][c] = s2;
    __syncthreads();
    if (tid < 64) {
      m = rmax[0][c];
      s = rsum[0][c];
      s2 = rsq[0][c];
      for (int k = 1; k < 4; ++k) {
        m = fmaxf(m, rmax[k][c]);
        s += rsum[k][c];
        s2 += rsq[k][c];
      }
      const size_t o = ((size_t)bi * nsl + slice) * kD + 64 * half + c;
      part.mx[o] = m;
      part.sum[o] = s;
      part.sq[o] = s2;
    }
  }
}

// ---- input projection: y = W_in [x ; posenc(x[0:3])] + bb[b] ------------------------------------------------------------
// A operand packed as wp[s][ob][lane] = W[32 ob + (lane & 31)][2 s + (lane >> 5)] (zero beyond K); the lane's B value is
// feature 2 s + h of its point: an input channel, or a positional-encoding channel computed here (precise sinf / cosf: the
// arguments reach |512 x|).
__global__ __launch_bounds__(256) void input_proj_kernel(int n, int cin, const float *__restrict__ x, const float *__restrict__ freq,
                                                         const float *__restrict__ wp, const float *__restrict__ bb,
                                                         float *__restrict__ y, Partials part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x, bi = blockIdx.y, nsl = gridDim.x;
  const int p0 = slice * kSlice, p = p0 + wave * 32 + li;
  const bool valid = p < n;
  const float *xb = x + (size_t)bi * cin * n;
  float v[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = valid ? xb[(size_t)j * n + p] : 0.f;
  float fr[kFreqs];
#pragma unroll
  for (int f = 0; f < kFreqs; ++f) fr[f] = freq[f];
  const int K = cin + 3 + 6 * kFreqs, steps = (K + 1) / 2;
  f32x16 acc[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ob][r] = 0.f;
  for (int s = 0; s < steps; ++s) {
    const int k = 2 * s + h;
    float b = 0.f;
    if (k < cin) {
      b = valid ? xb[(size_t)k * n + p] : 0.f;
    } else if (k < K) {
      const int q = k - cin;
      if (q < 3) {
        b = v[q];
      } else {
        const int f = (q - 3) / 6, w = (q - 3) % 6;
        float fq = 0.f, vj = 0.f;
#pragma unroll
        for (int j = 0; j < kFreqs; ++j) fq = (j == f) ? fr[j] : fq;
#pragma unroll
        for (int j = 0; j < 3; ++j) vj = (j == w % 3) ? v[j] : vj;
        const float a = fq * vj;
        b = w < 3 ? sinf(a) : cosf(a);
      }
    }
    const float *ws = wp + (size_t)s * 256 + lane;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[64 * ob], b, acc[ob], 0, 0, 0);
  }
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ob][r] += bb[(size_t)bi * kD + 32 * ob + acc_row(r, h)];
  store_and_pool(acc, y + (size_t)bi * kD * n, n, p0, slice, part, bi, nsl);
}

// ---- per-shape prologue of a layer: pooled max / unbiased std, and c = W_ms diag(g_ms) (ms - mbar) ------------------------
// grid (4, b): every block merges the shape's slices (same order, same bits), block x computes rows [256 x, 256 x + 256) of c.
// wms: (1024, 256) row-major = [W1; V][:, 128:384] * g[128:384].
__global__ __launch_bounds__(256) void layer_prep_kernel(int n, int nsl, Partials part, const float *__restrict__ wms,
                                                         float *__restrict__ state) {
  __shared__ float ms[256];
  __shared__ float stat[2];
  const int tid = threadIdx.x, bi = blockIdx.y;
  float *st = state + (size_t)bi * kState;
  if (tid < kD) {
    const size_t o = (size_t)bi * nsl * kD + tid;
    float m = part.mx[o];
    double s = part.sum[o], s2 = part.sq[o];
    for (int t = 1; t < nsl; ++t) {
      m = fmaxf(m, part.mx[o + (size_t)t * kD]);
      s += part.sum[o + (size_t)t * kD];
      s2 += part.sq[o + (size_t)t * kD];
    }
    const double mean = s / n;
    const double var = fmax(s2 - s * mean, 0.0) / (double)(n - 1);  // torch.std: unbiased
    ms[tid] = m;
    ms[kD + tid] = (float)sqrt(var);
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int c = 0; c < 256; ++c) s += (double)ms[c];
    const float msum = (float)s, mbar = (float)(s / 256.0);
    double q = 0.0;
    for (int c = 0; c < 256; ++c) {
      const double d = (double)ms[c] - (double)mbar;
      q += d * d;
    }
    stat[0] = msum;
    stat[1] = (float)q;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    st[tid] = ms[tid];
    if (tid < 2) st[256 + tid] = stat[tid];
  }
  const float mbar = stat[0] / 256.f;
  const int row = 256 * blockIdx.x + tid;
  const float *w = wms + (size_t)row * 256;
  float acc = 0.f;
  for (int c = 0; c < 256; ++c) acc = fmaf(w[c], ms[c] - mbar, acc);
  st[kStateC + row] = acc;
}

// ---- one gated feed-forward layer: y = x + W2 (silu(W1 LN(x_in)) * (V LN(x_in))) ---------------------------------------
// Lane (li, h) holds channels c = s + 64 h (s < 64) of point li as the B operand of k-step s; a1 / av are packed to match:
// a1[ck][s][lane] = W1[32 ck + li][s + 64 h] g[s + 64 h].  The hidden chunk's 32 x 32 result has its point on the lane, so it is
// the B operand of the W2 product directly (k-step r of lane half h = hidden row acc_row(r, h)): a2[ck][ob][r][lane] =
// W2[32 ob + li][32 ck + acc_row(r, h)].  vec = [d1, e1, dv, ev] (4 x 512): d = W_ms g_ms, e = W beta.
__global__ __launch_bounds__(256) void layer_kernel(int n, const float *__restrict__ x, const float *__restrict__ state,
                                                    const float *__restrict__ a1, const float *__restrict__ av,
                                                    const float *__restrict__ a2, const float *__restrict__ vec,
                                                    float *__restrict__ y, Partials part) {
  __shared__ float cs[4][kHid];  // c1 + ... per row: c (shape), d, e for the W1 and V halves
  __shared__ float cv[2][kHid];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x, bi = blockIdx.y, nsl = gridDim.x;
  const int p0 = slice * kSlice, p = p0 + wave * 32 + li;
  const bool valid = p < n;
  const float *st = state + (size_t)bi * kState;
  for (int i = tid; i < kHid; i += 256) {
    cs[0][i] = st[kStateC + i];         // c1
    cs[1][i] = vec[i];                  // d1
    cs[2][i] = vec[kHid + i];           // e1
    cs[3][i] = st[kStateC + kHid + i];  // cv
    cv[0][i] = vec[2 * kHid + i];       // dv
    cv[1][i] = vec[3 * kHid + i];       // ev
  }
  const float msum = st[256], qms = st[257], mbar = msum / 256.f;
  const float *xb = x + (size_t)bi * kD * n;
  float z[64];
  float s1 = 0.f;
#pragma unroll
  for (int s = 0; s < 64; ++s) {
    z[s] = valid ? xb[(size_t)(s + 64 * h) * n + p] : 0.f;
    s1 += z[s];
  }
  float o1 = __shfl_xor(s1, 32);
  const float mu = ((h ? o1 + s1 : s1 + o1) + msum) / 384.f;
  float s2 = 0.f;
#pragma unroll
  for (int s = 0; s < 64; ++s) {
    z[s] -= mu;
    s2 = fmaf(z[s], z[s], s2);
  }
  float o2 = __shfl_xor(s2, 32);
  const float dm = mbar - mu;
  const float var = ((h ? o2 + s2 : s2 + o2) + qms + 256.f * dm * dm) / 384.f;
  const float rs = 1.f / sqrtf(var + 1e-5f);
  __syncthreads();

  f32x16 acc[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ob][r] = 0.f;
  for (int ck = 0; ck < kChunks; ++ck) {
    f32x16 ha, hv;
#pragma unroll
    for (int r = 0; r < 16; ++r) ha[r] = hv[r] = 0.f;
    const float *w1 = a1 + (size_t)ck * 64 * 64 + lane, *wv = av + (size_t)ck * 64 * 64 + lane;
#pragma unroll
    for (int s = 0; s < 64; ++s) {
      ha = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[64 * s], z[s], ha, 0, 0, 0);
      hv = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[64 * s], z[s], hv, 0, 0, 0);
    }
    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * ck + acc_row(r, h);
      const float a = fmaf(ha[r] + cs[0][j] + dm * cs[1][j], rs, cs[2][j]);
      const float v = fmaf(hv[r] + cs[3][j] + dm * cv[0][j], rs, cv[1][j]);
      g[r] = a / (1.f + expf(-a)) * v;  // SiLU(a) * v
    }
    const float *w2 = a2 + (size_t)ck * 4 * 16 * 64 + lane;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[(ob * 16 + r) * 64], g[r], acc[ob], 0, 0, 0);
  }
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ob][r] += valid ? xb[(size_t)(32 * ob + acc_row(r, h)) * n + p] : 0.f;
  store_and_pool(acc, y + (size_t)bi * kD * n, n, p0, slice, part, bi, nsl);
}

// ---- elementwise sum (PVCNN++'s x + PVCNN(x), pvcnn_plus_plus.py:40) --------------------------------------------------------
__global__ __launch_bounds__(256) void add_kernel(long long n, const float *a, const float *b, float *out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = a[i] + b[i];
}

}  // namespace

extern "C" size_t bdm_simple_partials_bytes(int b, int n) {
  return (b <= 0 || n <= 0) ? 0 : (size_t)b * n_slices(n) * kD * (sizeof(float) + 2 * sizeof(double));
}

extern "C" size_t bdm_simple_state_elems(int b) { return b <= 0 ? 0 : (size_t)b * kState; }

extern "C" int bdm_simple_input_proj(int b, int n, int c_in, const float *x, const float *freq, const float *w_packed,
                                     const float *batch_bias, float *y, void *partials, void *stream) {
  BDM_REQUIRE(b >= 0 && n >= 0 && c_in >= 3, "simple_input_proj: bad sizes (b %d, n %d, c_in %d)", b, n, c_in);
  if (b == 0 || n == 0) return BDM_OK;
  BDM_REQUIRE(x && freq && w_packed && batch_bias && y && partials, "simple_input_proj: null pointer");
  BDM_REQUIRE(x != y, "simple_input_proj: y must not alias x");
  input_proj_kernel<<<dim3(n_slices(n), b), 256, 0, (hipStream_t)stream>>>(n, c_in, x, freq, w_packed, batch_bias, y,
                                                                            partials_of(partials, b, n));
  return launch_status("simple_input_proj");
}

extern "C" int bdm_simple_layer_prep(int b, int n, const void *partials, const float *w_ms, float *state, void *stream) {
  BDM_REQUIRE(b >= 0 && n >= 2, "simple_layer_prep: need at least two points per shape (unbiased std), got n %d", n);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(partials && w_ms && state, "simple_layer_prep: null pointer");
  layer_prep_kernel<<<dim3(4, b), 256, 0, (hipStream_t)stream>>>(n, n_slices(n), partials_of((void *)partials, b, n), w_ms, state);
  return launch_status("simple_layer_prep");
}

extern "C" int bdm_simple_layer(int b, int n, const float *x, const float *state, const float *w1_packed, const float *wv_packed,
                                const float *w2_packed, const float *vec, float *y, void *partials, void *stream) {
  BDM_REQUIRE(b >= 0 && n >= 0, "simple_layer: bad sizes (b %d, n %d)", b, n);
  if (b == 0 || n == 0) return BDM_OK;
  BDM_REQUIRE(x && state && w1_packed && wv_packed && w2_packed && vec && y && partials, "simple_layer: null pointer");
  BDM_REQUIRE(x != y, "simple_layer: y must not alias x");
  layer_kernel<<<dim3(n_slices(n), b), 256, 0, (hipStream_t)stream>>>(n, x, state, w1_packed, wv_packed, w2_packed, vec, y,
                                                                       partials_of(partials, b, n));
  return launch_status("simple_layer");
}

extern "C" int bdm_simple_add(long long n, const float *a, const float *b, float *out, void *stream) {
  BDM_REQUIRE(n >= 0, "simple_add: bad size %lld", n);
  if (n == 0) return BDM_OK;
  BDM_REQUIRE(a && b && out, "simple_add: null pointer");
  const long long blocks = (n + 255) / 256;
  add_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, (hipStream_t)stream>>>(n, a, b, out);
  return launch_status("simple_add");
}
