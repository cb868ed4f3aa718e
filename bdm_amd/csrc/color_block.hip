// color_block.hip -- second half of one block of the PC^2 colouring model (PointCloudModelBlock,
// point_cloud_transformer_model.py:56-61 with use_attn = False), fused per point:
//   r = h + p;  y = r + fc2(gelu(fc1(LayerNorm(r))));  then LayerNorm(y) for the next block, or the colour head.
// The 4E-wide hidden vector stays in registers: 32 rows at a time come out of the fc1 MFMAs with the point on the lane, which
// is the B operand layout of the fc2 MFMAs (the scheme of simple_point.hip's layer_kernel).
//
// Layout: tokens channel-first (b, 64, n).  A workgroup owns a tile of 128 consecutive points of one shape, its four waves 32
// points each, the point index on the MFMA column (lane & 31).  Lane (li, h) holds channels s + 32 h (s < 32) of point li.
// No LDS, no atomics, no cross-point reduction: a point's results do not depend on n, b or the tile it falls in.
//
// Arithmetic: fp32 throughout.  LayerNorm is two-pass (mean, then the squared deviations) with the biased variance, GELU is
// the exact erf form, both contractions are v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).
#include "../../include/bdm_hip.h"
#include "common.h"

using namespace bdm;
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

constexpr int kE = 64;              // model width (point_cloud_model_embed_dim)
constexpr int kHid = 4 * kE;        // Mlp hidden width (mlp_ratio = 4)
constexpr int kTile = 128;          // points per workgroup
constexpr int kChunks = kHid / 32;  // hidden chunks of 32 rows
constexpr int kW1 = kChunks * 32 * 64;      // floats of the fc1 record
constexpr int kW2 = kChunks * 2 * 16 * 64;  // floats of the fc2 record

// row of accumulator register r of a 32x32 tile in lane half h
__host__ __device__ inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// sum of a value over the two lane halves that share a point; the same bits in both halves
__device__ inline float pair_sum(float v, int h) {
  const float o = __shfl_xor(v, 32);
  return h ? o + v : v + o;
}

// packed[0 .. kW1)       [ck][s][lane]     = W1[32 ck + (lane & 31)][s + 32 (lane >> 5)]
// packed[kW1 .. kW1+kW2) [ck][ob][r][lane] = W2[32 ob + (lane & 31)][32 ck + acc_row(r, lane >> 5)]
__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ w1, const float *__restrict__ w2,
                                                   float *__restrict__ packed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kW1) {
    const int lane = i & 63, s = (i >> 6) & 31, ck = i >> 11;
    packed[i] = w1[(size_t)(32 * ck + (lane & 31)) * kE + s + 32 * (lane >> 5)];
  } else if (i < kW1 + kW2) {
    const int j = i - kW1, lane = j & 63, r = (j >> 6) & 15, ob = (j >> 10) & 1, ck = j >> 11;
    packed[i] = w2[(size_t)(32 * ob + (lane & 31)) * kHid + 32 * ck + acc_row(r, lane >> 5)];
  }
}

struct TailArgs {
  const float *h, *p, *g2, *be2, *wp, *b1, *b2;
  float *y;
  const float *gn, *ben;  // next block's norm0 (ln_next)
  float *ln_next;
  const float *wo, *bo;   // colour head (colors)
  float *colors;
  float eps2, epsn, cmean, cstd;
};

__global__ __launch_bounds__(256) void tail_kernel(int n, TailArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int bi = blockIdx.y;
  const long long p = (long long)blockIdx.x * kTile + wave * 32 + li;
  const bool valid = p < n;
  const size_t base = (size_t)bi * kE * n;
  const float *hb = a.h + base, *pb = a.p + base;

  // r = h + p, LayerNorm(norm2) over the point's 64 channels: this lane's 32 and its partner's
  float z[32];
  float s1 = 0.f;
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const size_t o = (size_t)(s + 32 * h) * n + p;
    z[s] = valid ? hb[o] + pb[o] : 0.f;
    s1 += z[s];
  }
  const float mu = pair_sum(s1, h) * (1.f / kE);
  float s2 = 0.f;
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    z[s] -= mu;
    s2 = fmaf(z[s], z[s], s2);
  }
  const float rs = 1.f / sqrtf(pair_sum(s2, h) * (1.f / kE) + a.eps2);
#pragma unroll
  for (int s = 0; s < 32; ++s) z[s] = fmaf(z[s] * rs, a.g2[s + 32 * h], a.be2[s + 32 * h]);

  f32x16 acc[2];
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ob][r] = 0.f;
  for (int ck = 0; ck < kChunks; ++ck) {
    f32x16 ha;
#pragma unroll
    for (int r = 0; r < 16; ++r) ha[r] = 0.f;
    const float *w1 = a.wp + (size_t)ck * 32 * 64 + lane;
#pragma unroll
    for (int s = 0; s < 32; ++s) ha = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[64 * s], z[s], ha, 0, 0, 0);
    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = ha[r] + a.b1[32 * ck + acc_row(r, h)];
      g[r] = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));  // exact GELU (nn.GELU())
    }
    const float *w2 = a.wp + kW1 + (size_t)ck * 2 * 16 * 64 + lane;
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[(ob * 16 + r) * 64], g[r], acc[ob], 0, 0, 0);
  }

  // y = r + (fc2 + b2): acc[ob][r] is channel 32 ob + acc_row(r, h) of the point; r is formed again from h and p (same bits)
  float *yb = a.y + base;
  float t1 = 0.f;
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 32 * ob + acc_row(r, h);
      const size_t o = (size_t)c * n + p;
      const float res = valid ? hb[o] + pb[o] : 0.f;
      const float v = res + (acc[ob][r] + a.b2[c]);
      acc[ob][r] = v;
      t1 += v;
      if (valid) yb[o] = v;
    }

  if (a.ln_next) {  // LayerNorm of y with the next block's norm0
    const float m = pair_sum(t1, h) * (1.f / kE);
    float t2 = 0.f;
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[ob][r] -= m;
        t2 = fmaf(acc[ob][r], acc[ob][r], t2);
      }
    const float q = 1.f / sqrtf(pair_sum(t2, h) * (1.f / kE) + a.epsn);
    float *lb = a.ln_next + base;
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * ob + acc_row(r, h);
        if (valid) lb[(size_t)c * n + p] = fmaf(acc[ob][r] * q, a.gn[c], a.ben[c]);
      }
  } else if (a.colors) {  // output_projection + denormalize + clamp, point-major (b, n, 3)
    float d[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * ob + acc_row(r, h);
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = fmaf(a.wo[j * kE + c], acc[ob][r], d[j]);
      }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = fmaf(pair_sum(d[j], h) + a.bo[j], a.cstd, a.cmean);
      if (valid && h == 0) a.colors[((size_t)bi * n + p) * 3 + j] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);  // torch.clamp: NaN stays
    }
  }
}

}  // namespace

extern "C" size_t bdm_color_block_packed_elems(int e) { return e == kE ? (size_t)(kW1 + kW2) : 0; }

extern "C" int bdm_color_block_pack_weights(int e, const float *fc1_w, const float *fc2_w, float *packed, void *stream) {
  if (e != kE) {
    set_error("color_block_pack_weights: built for E = %d, got %d", kE, e);
    return BDM_ERR_UNSUPPORTED;
  }
  BDM_REQUIRE(fc1_w && fc2_w && packed, "color_block_pack_weights: null pointer");
  pack_kernel<<<(kW1 + kW2) / 256, 256, 0, (hipStream_t)stream>>>(fc1_w, fc2_w, packed);
  return launch_status("color_block_pack_weights");
}

extern "C" int bdm_color_block_tail(int b, int e, int n, const float *h, const float *p, const float *norm2_w,
                                    const float *norm2_b, float norm2_eps, const float *w_packed, const float *fc1_b,
                                    const float *fc2_b, float *y, const float *next_w, const float *next_b, float next_eps,
                                    float *ln_next, const float *out_w, const float *out_b, float colors_mean,
                                    float colors_std, float *colors, void *stream) {
  if (e != kE) {
    set_error("color_block_tail: built for E = %d, got %d", kE, e);
    return BDM_ERR_UNSUPPORTED;
  }
  BDM_REQUIRE(b >= 0 && n >= 0 && b <= 65535, "color_block_tail: bad sizes (b %d, n %d)", b, n);
  if (b == 0 || n == 0) return BDM_OK;
  BDM_REQUIRE(h && p && norm2_w && norm2_b && w_packed && fc1_b && fc2_b && y, "color_block_tail: null pointer");
  BDM_REQUIRE(y != h && y != p, "color_block_tail: y must not alias h or p");
  BDM_REQUIRE(!(ln_next && colors), "color_block_tail: at most one of ln_next and colors");
  BDM_REQUIRE(!ln_next || (next_w && next_b && ln_next != h && ln_next != p && ln_next != y),
              "color_block_tail: ln_next needs next_w / next_b and a buffer of its own");
  BDM_REQUIRE(!colors || (out_w && out_b), "color_block_tail: colors needs out_w / out_b");
  TailArgs a{h, p, norm2_w, norm2_b, w_packed, fc1_b, fc2_b, y, next_w, next_b, ln_next, out_w, out_b, colors,
             norm2_eps, next_eps, colors_mean, colors_std};
  tail_kernel<<<dim3((unsigned)((n + kTile - 1) / kTile), b), 256, 0, (hipStream_t)stream>>>(n, a);
  return launch_status("color_block_tail");
}
