// attention_h2.hip -- flash attention on the fp16 matrix cores at fp32-grade accuracy ("fp16x3"), half the matrix work of the
// bf16x6 kernel of attention_s3.hip (same geometry, same online softmax, same register-resident probability tile).
//
// An fp32 operand times a power of two is stored as hi + lo (two fp16 terms, 22 signed bits); a product is
// lo.hi + hi.lo + hi.hi accumulated in fp32 (lo.lo <= 2^-22 relative is dropped).  fp16 has a narrow exponent range, so every
// tensor gets ONE power-of-two scale PER SHAPE from its max |value| (amax[3 s + 0..2] for q, k, v of shape s: left by the projection GEMM's epilogue,
// bdm_pointwise_conv_gn, as bit patterns of non-negative floats -- an integer atomicMax, order independent): the scaled
// operands sit in [2^14, 2^15) at the top, the scales are divided out exactly (q.k scale inside the exponential's constant,
// v and probability scales at the final normalisation).  Probabilities (in [0, 1]) are scaled by 2^14 before their split.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "h2_split.h"
#include <type_traits>

using namespace bdm;

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

namespace {

__device__ __forceinline__ void split2h(float v, unsigned short &h, unsigned short &l) {
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  h = __builtin_bit_cast(unsigned short, hi);
  l = __builtin_bit_cast(unsigned short, lo);
}

__device__ __forceinline__ uint4 pack8(const unsigned short x[8]) {
  return make_uint4(x[0] | (x[1] << 16), x[2] | (x[3] << 16), x[4] | (x[5] << 16), x[6] | (x[7] << 16));
}

__device__ __forceinline__ f16x8 as_f16x8(uint4 u) { return __builtin_bit_cast(f16x8, u); }

}  // namespace

// q or k: (C, L) fp32 rows of stride ld -> records [c8][split][l] of 8 channels x fp16
__global__ void attn_split_qk_h2_kernel(int C, int L, const float *__restrict__ q, const float *__restrict__ k, long long bs,
                                        int ld, const float *__restrict__ amax, uint4 *__restrict__ qs, uint4 *__restrict__ ks) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x, c8 = blockIdx.y, C8 = gridDim.y, bi = blockIdx.z >> 1, which = blockIdx.z & 1;
  if (l >= L) return;
  const float s = act_scale_from_max(amax[bi * 3 + which]);  // per shape
  const float *src = (which ? k : q) + (size_t)bi * bs;
  uint4 *dst = (which ? ks : qs) + ((size_t)bi * C8 + c8) * 2 * (size_t)L;
  unsigned short h[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c8 * 8 + j;
    split2h(c < C ? src[(size_t)c * ld + l] * s : 0.f, h[j], lo[j]);
  }
  dst[l] = pack8(h);
  dst[(size_t)L + l] = pack8(lo);
}

// v: (C, L) fp32 -> planes [split][c][Lp] fp16 with the KEY index contiguous, zero for c >= C and l >= L
__global__ void attn_split_v_h2_kernel(int C, int CP, int L, int Lp, const float *__restrict__ v, long long bs, int ld,
                                       const float *__restrict__ amax, unsigned short *__restrict__ vt) {
  const int l0 = (blockIdx.x * blockDim.x + threadIdx.x) * 8, c = blockIdx.y, bi = blockIdx.z;
  if (l0 >= Lp) return;
  const float s = act_scale_from_max(amax[bi * 3 + 2]);
  unsigned short h[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) split2h((c < C && l0 + j < L) ? v[(size_t)bi * bs + (size_t)c * ld + l0 + j] * s : 0.f, h[j], lo[j]);
  unsigned short *base = vt + (size_t)bi * 2 * CP * Lp;
  *reinterpret_cast<uint4 *>(base + ((size_t)0 * CP + c) * Lp + l0) = pack8(h);
  *reinterpret_cast<uint4 *>(base + ((size_t)1 * CP + c) * Lp + l0) = pack8(lo);
}

#define VROW_H2 36  // fp16 per V row in LDS: 32 keys + 4 pad

// Software-pipelined over the key tiles (round 5).  Iteration t of a wave runs two INDEPENDENT instruction streams:
//   matrix pipe:  O += P(t-1) V(t-1)   and   S(t+1) = K(t+1)^T Q          (24 MFMAs, 768 cycles)
//   vector ALU :  online softmax of S(t) -> P(t), running maximum / sum     (~190 instructions, ~900 cycles)
// In the straight-line form (S, softmax, PV per tile) a wave's matrix phases waited for its own softmax and the matrix pipe was 38 % busy
// (r05_mfma_busy.txt): the waves of a SIMD run the same phases at the same time (two workgroup barriers per tile keep them aligned), so
// other waves did not fill the gaps.  K tiles are double-buffered in LDS, V tiles triple-buffered (V(t-1) is read while tile t + 1 is stored).
template <int CB>  // channel blocks of 32 (C <= 32 * CB)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_flash_h2_kernel(int C, int L, int Lp, int nb, const uint4 *__restrict__ qs,
                                                            const uint4 *__restrict__ ks,
                                                            const unsigned short *__restrict__ vt,
                                                            const float *__restrict__ amax, float *__restrict__ out,
                                                            long long bs_o, int ld_o, int ksplit, float *__restrict__ part_o,
                                                            float *__restrict__ part_ml) {
  constexpr int C8 = 4 * CB, CP = 32 * CB, KT = C8 * 2 * 32, VT = 2 * CP * 4;  // uint4 items per K / V tile
  constexpr int KI = (KT + 255) / 256, VI = (VT + 255) / 256;
  constexpr int VSZ = 2 * CP * VROW_H2;
  __shared__ uint4 Ksh[2][KT];                                 // [buffer][c8][split][key]
  __shared__ __align__(16) unsigned short Vsh[3][VSZ];         // [buffer][split][c][VROW_H2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  // XCD-aware item order: workgroup ids are dealt round-robin to the 8 XCDs; XCD x takes the contiguous (shape, query tile) items
  // [x * per, (x + 1) * per), so a shape's K / V stay in ONE XCD's L2 (they were fetched by all eight: 272 MB per launch at B = 16, PMC)
  // ksplit > 1 (few shapes: the (shape, query tile) items alone cannot fill the chip, and an item is a chain of L / 32 dependent key tiles):
  // an item is (shape, query tile, KEY RANGE); it leaves its unnormalised accumulator, exponent offset and row sum, and
  // attn_combine_kernel merges the ranges (the order of the sum over keys changes: a different, equally valid rounding)
  const int qtiles = (L + 127) / 128, total = qtiles * nb * ksplit, per = (total + 7) >> 3;
  const int item0 = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (item0 >= total) return;
  const int split = item0 % ksplit, item = item0 / ksplit;
  const int bi = item / qtiles;
  const int i0 = ((item - bi * qtiles) * 4 + wave) * 32;  // this wave's first query
  const uint4 *qb = qs + (size_t)bi * C8 * 2 * L, *kb = ks + (size_t)bi * C8 * 2 * L;
  const unsigned short *vb = vt + (size_t)bi * 2 * CP * Lp;
  const float sq = act_scale_from_max(amax[bi * 3]), sk = act_scale_from_max(amax[bi * 3 + 1]), sv = act_scale_from_max(amax[bi * 3 + 2]);
  // exp(x) = 2^(x log2 e): the q.k scale (a power of two, exact) is divided out inside the constant
  const float ec = 1.44269504088896340736f / (sq * sk);

  f16x8 qreg[2 * CB][2];
#pragma unroll
  for (int s = 0; s < 2 * CB; ++s)
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) qreg[s][sp] = as_f16x8(qb[((size_t)(2 * s + lh) * 2 + sp) * L + min(i0 + li, L - 1)]);
  f32x16 o[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
  float run_max = -INFINITY, run_sum = 0.f, run_mneg = INFINITY;

  typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
  u32x4v kr[KI], vr[VI];
  auto load_tile = [&](int j0) {
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int e = tid + i * 256, key = e & 31, cs = min(e >> 5, KT / 32 - 1);
      kr[i] = *reinterpret_cast<const u32x4v *>(&kb[(size_t)cs * L + min(j0 + key, L - 1)]);
    }
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const int e = tid + i * 256, piece = e & 3, rowi = min(e >> 2, VT / 4 - 1);
      vr[i] = *reinterpret_cast<const u32x4v *>(vb + ((size_t)rowi * Lp + min(j0 + piece * 8, Lp - 8)));
    }
  };
  auto store_tile = [&](uint4 *kdst, unsigned short *vdst) {
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int e = tid + i * 256;
      if (e < KT) *reinterpret_cast<u32x4v *>(&kdst[e]) = kr[i];
    }
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const int e = tid + i * 256, piece = e & 3, rowi = e >> 2;
      if (e < VT) {
        uint2 *d = reinterpret_cast<uint2 *>(vdst + rowi * VROW_H2 + piece * 8);
        d[0] = make_uint2(vr[i].x, vr[i].y);
        d[1] = make_uint2(vr[i].z, vr[i].w);
      }
    }
  };
  // S^T[j][i] = sum_c k[c][j] q[c][i]  (scaled by sq * sk); two accumulators: even / odd 16-channel steps
  // (ONE accumulator chain: the MFMAs are spaced by the softmax's vector instructions, so a dependent successor finds its predecessor done;
  // the two-chain form cost 16 registers and 8 packed adds per tile)
  auto scores = [&](const uint4 *kt, f32x16 &st) {
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 2 * CB; ++s) {
      const f16x8 ah = as_f16x8(kt[((2 * s + lh) * 2 + 0) * 32 + li]), al = as_f16x8(kt[((2 * s + lh) * 2 + 1) * 32 + li]);
      st = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qreg[s][0], st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qreg[s][1], st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qreg[s][0], st, 0, 0, 0);
    }
  };

  const int T_all = (L + 31) / 32, t_per = (T_all + ksplit - 1) / ksplit;
  const int tb = min(split * t_per, T_all), T = min(tb + t_per, T_all);   // this item's key tiles [tb, T); buffers are indexed by the absolute tile
  if (tb >= T) {   // (an empty range: only when ksplit does not divide the tile count) -- contributes nothing
    if (ksplit > 1 && i0 + li < L && lh == 0) {
      float *ml = part_ml + (((size_t)split * nb + bi) * L + i0 + li) * 2;
      ml[0] = INFINITY; ml[1] = 0.f;
    }
    return;
  }
  load_tile(tb * 32);
  store_tile(Ksh[tb & 1], Vsh[tb % 3]);
  __syncthreads();
  if (T - tb > 1) load_tile((tb + 1) * 32);
  f32x16 s_cur;
  scores(Ksh[tb & 1], s_cur);
  f16x8 p_prev[2][2];     // P(t-1) x 2^14 as B operand (hi, lo), registers 8jj .. 8jj+7 -> the 8 k-slots of MFMA jj
  float corr_prev = 1.0f; // rescale of O that P(t-1)'s tile asked for
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) p_prev[jj][sp] = as_f16x8(make_uint4(0u, 0u, 0u, 0u));

  // One iteration; the flags are compile-time so that the steady state (all true, no tail mask) is ONE basic block in which the
  // scheduler interleaves the two streams (sched_group_barrier: one MFMA, then a few vector instructions, ...): a wave issues in order, so
  // 24 MFMAs in a row would hold its softmax back for the 768 cycles they take to issue.
  auto iteration = [&](int t, auto has_prev, auto has_next, auto has_cur, auto tail) {
    constexpr bool HP = decltype(has_prev)::value, HN = decltype(has_next)::value, HC = decltype(has_cur)::value, TAIL = decltype(tail)::value;
    __syncthreads();                                   // every wave has finished iteration t - 1 (its reads of K(t), V(t-2))
    if (HN) store_tile(Ksh[(t + 1) & 1], Vsh[(t + 1) % 3]);
    __syncthreads();
    if (HN) load_tile((t + 2) * 32);                   // (clamped addresses: a tile beyond the last one re-reads valid memory, never stored)
    if (HP) {
      if (__any(corr_prev != 1.0f)) {                  // the running maximum moves in the first few tiles only
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[cb][r] *= corr_prev;
      }
    }
    // ---- matrix stream: O += P(t-1) V(t-1);  S(t+1) ----------------------------------------------------------------------------
    f32x16 s_next;
    if (HP) {
      const unsigned short *vtile = Vsh[(t - 1) % 3];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        f32x16 acc = o[cb];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          f16x8 a[2];
#pragma unroll
          for (int sp = 0; sp < 2; ++sp) {
            const unsigned short *rowp = vtile + (sp * CP + cb * 32 + li) * VROW_H2 + 16 * jj + 4 * lh;
            const uint2 p0 = *reinterpret_cast<const uint2 *>(rowp), p1 = *reinterpret_cast<const uint2 *>(rowp + 8);
            a[sp] = as_f16x8(make_uint4(p0.x, p0.y, p1.x, p1.y));
          }
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1], p_prev[jj][0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], p_prev[jj][1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], p_prev[jj][0], acc, 0, 0, 0);
        }
        o[cb] = acc;
      }
    }
    if (HN) scores(Ksh[(t + 1) & 1], s_next);
    // ---- vector stream: online softmax of S(t) ------------------------------------------------------------------------------------
    if (HC) {
      const int j0 = t * 32;
      f32x16 st = s_cur;
      if (TAIL) {         // only the last tile can hold keys beyond L
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (j0 + (r & 3) + 8 * (r >> 2) + 4 * lh >= L) st[r] = -INFINITY;
      }
      float tile_max = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tile_max = fmaxf(tile_max, st[r]);
      tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, 64));
      const float new_max = fmaxf(run_max, tile_max);
      // exponent offset of this tile, ROUNDED once; the rescale of what was accumulated under the previous offset uses the difference of
      // the two rounded offsets, so every probability of a query carries the same factor 2^(rounding error) and it cancels in the
      // normalisation (an offset recomputed per tile from the running maximum would not: measured 7.1e-7 -> 8.3e-7 vs float64)
      float mneg = -new_max * ec;
      asm("" : "+v"(mneg));   // opaque: contracted into the subtraction below, the product would not be the ROUNDED value the exponentials use
      const float corr = __builtin_amdgcn_exp2f(mneg - run_mneg);  // exp2(-inf) = 0 on the first tile (run_mneg = +inf)
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], ec, mneg));   // one rounding of the argument (was subtract, then multiply)
        psum += st[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      run_sum = run_sum * corr + psum;
      run_max = new_max;
      run_mneg = mneg;
      corr_prev = corr;
      // P x 2^14 split into fp16 pairs, written as ELEMENTS of the operand vectors: the compiler converts with v_fma_mixlo / mixhi_f16
      // straight into the two halves of a register (the unsigned-short form packed every pair with a shift and an or: 32 instructions a tile)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        f16x8 hv, lv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = st[8 * jj + i] * 16384.f;
          const _Float16 hi = (_Float16)v;
          hv[i] = hi;
          lv[i] = (_Float16)(v - (float)hi);
        }
        p_prev[jj][0] = hv;
        p_prev[jj][1] = lv;
      }
    }
    if (HP && HN && HC && !TAIL) {
      // steady state: 24 MFMAs against ~200 vector instructions
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);   // eight vector-ALU instructions
      }
    }
    if (HN) s_cur = s_next;
  };
  using yes = std::integral_constant<bool, true>;
  using no = std::integral_constant<bool, false>;
  const bool tail = (L & 31) != 0 && T == T_all;   // (keys beyond L live in the last tile of the whole range only)
  if (T - tb == 1) {
    if (tail) iteration(tb, no{}, no{}, yes{}, yes{}); else iteration(tb, no{}, no{}, yes{}, no{});
  } else {
    iteration(tb, no{}, yes{}, yes{}, no{});
    for (int t = tb + 1; t + 1 < T; ++t) iteration(t, yes{}, yes{}, yes{}, no{});
    if (tail) iteration(T - 1, yes{}, no{}, yes{}, yes{}); else iteration(T - 1, yes{}, no{}, yes{}, no{});
  }
  iteration(T, yes{}, no{}, no{}, no{});
  if (ksplit > 1) {   // partial result of this key range: O (unnormalised, under the offset run_mneg), the offset and the row sum
    if (i0 + li < L) {
      float *po = part_o + ((size_t)split * nb + bi) * CP * (size_t)L;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) po[(size_t)(cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * L + i0 + li] = o[cb][r];
      if (lh == 0) {
        float *ml = part_ml + (((size_t)split * nb + bi) * L + i0 + li) * 2;
        ml[0] = run_mneg; ml[1] = run_sum;
      }
    }
    return;
  }
  const float inv = 1.0f / (run_sum * 16384.f * sv);  // sv and 2^14 are powers of two
  float *ob = out + (size_t)bi * bs_o;
  if (i0 + li < L) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (c < C) ob[(size_t)c * ld_o + i0 + li] = o[cb][r] * inv;
      }
  }
}

// out[c][l] = sum_s O_s[c][l] 2^(m - m_s) / (sum_s l_s 2^(m - m_s)) / (2^14 sv),  m = min_s m_s (the offset of the largest running maximum):
// the key ranges of a query in ascending order -- a fixed order, deterministic
__global__ void attn_combine_kernel(int C, int CP, int L, int nb, int ksplit, const float *__restrict__ part_o,
                                    const float *__restrict__ part_ml, const float *__restrict__ amax, float *__restrict__ out,
                                    long long bs_o, int ld_o) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x, bi = blockIdx.z;
  if (l >= L) return;
  float m = INFINITY;
  for (int s = 0; s < ksplit; ++s) m = fminf(m, part_ml[(((size_t)s * nb + bi) * L + l) * 2]);
  float f[8], den = 0.f;   // ksplit <= 8
  for (int s = 0; s < ksplit; ++s) {
    const float *ml = part_ml + (((size_t)s * nb + bi) * L + l) * 2;
    f[s] = ml[1] > 0.f ? __builtin_amdgcn_exp2f(m - ml[0]) : 0.f;
    den += ml[1] * f[s];
  }
  const float sv = act_scale_from_max(amax[bi * 3 + 2]);
  const float inv = 1.0f / (den * 16384.f * sv);
  for (int c = blockIdx.y; c < C; c += gridDim.y) {
    float acc = 0.f;
    for (int s = 0; s < ksplit; ++s)
      if (f[s] != 0.f) acc += part_o[(((size_t)s * nb + bi) * CP + c) * (size_t)L + l] * f[s];
    out[(size_t)bi * bs_o + (size_t)c * ld_o + l] = acc * inv;
  }
}

// key ranges per (shape, query tile) the library RECOMMENDS: 1 when those items fill the chip; a function of the sizes only (the same for 1 .. 3
// shapes of 4096 positions, so the small-batch equality tests compare like with like).  The count a launch USES is the caller's argument
// (no environment look-up here -- the workspace size and the launch can no longer disagree, and a caller that wants a shape's bits
// independent of its launch's batch passes a fixed count).
static inline int attn_ksplit(int b, int l) {
  const long long items = (long long)b * ((l + 127) / 128);
  // measured at l = 4096, 64 channels (us per call, 1 / 2 / 4 / 8 ranges): 1 shape 131 / 82 / 60 / 59, 3 shapes 140 / 96 / 87 / 90, 8 shapes 165 / 149 / 158 / 174
  return l < 1024 ? 1 : (items < 128 ? 4 : (items < 512 ? 2 : 1));
}
extern "C" int bdm_attention_h2_key_slices(int b, int l) { return attn_ksplit(b, l); }
static inline int attn_cp(int c) { return c <= 32 ? 32 : 64; }
static inline int attn_lp(int l) { return (l + 7) / 8 * 8; }

extern "C" size_t bdm_attention_h2_workspace_bytes(int b, int c, int l, int key_slices) {
  if (l <= 64 || c > 64) return 0;
  const size_t cp = attn_cp(c), qk = (size_t)(cp / 8) * 2 * l * 16, v = 2 * cp * (size_t)attn_lp(l) * 2;
  const int ks = key_slices < 1 ? 1 : key_slices;   // + the partial results of the key ranges (none for one range)
  return (size_t)b * (2 * qk + v) + 64 + (ks > 1 ? (size_t)ks * b * (cp + 2) * l * sizeof(float) + 64 : 0);
}

// out (b, c, l) = softmax_keys(q^T k) applied to v, for q, k, v (b, c, l) rows of stride ld_qkv; amax[3 s + 0..2] = max |q|, |k|, |v| of
// shape s (bit patterns of non-negative floats, e.g. from bdm_pointwise_conv_gn's amax output).  64 < l, c <= 64.
extern "C" int bdm_attention_core_h2(int b, int c, int l, const float *q, const float *k, const float *v, long long bs_qkv,
                                     int ld_qkv, const float *amax, float *out, long long bs_o, int ld_o, void *workspace,
                                     size_t workspace_bytes, int key_slices, void *stream) {
  BDM_REQUIRE(b >= 0 && c >= 1 && c <= 64 && l > 64 && amax != nullptr && workspace != nullptr, "attention_core_h2: bad arguments");
  BDM_REQUIRE(key_slices >= 1 && key_slices <= 8, "attention_core_h2: key_slices = %d (1 .. 8; bdm_attention_h2_key_slices recommends one)", key_slices);
  BDM_REQUIRE(workspace_bytes >= bdm_attention_h2_workspace_bytes(b, c, l, key_slices),
              "attention_core_h2: workspace of %zu bytes, %zu needed for %d key ranges", workspace_bytes,
              bdm_attention_h2_workspace_bytes(b, c, l, key_slices), key_slices);
  if (b == 0) return BDM_OK;
  hipStream_t s = (hipStream_t)stream;
  const int cp = attn_cp(c), c8 = cp / 8, lp = attn_lp(l);
  const size_t qk_rec = (size_t)b * c8 * 2 * l;
  uint4 *qs = reinterpret_cast<uint4 *>((reinterpret_cast<size_t>(workspace) + 15) & ~(size_t)15);
  uint4 *ks = qs + qk_rec;
  unsigned short *vt = reinterpret_cast<unsigned short *>(ks + qk_rec);
  hipLaunchKernelGGL(attn_split_qk_h2_kernel, dim3(cdiv(l, 128), c8, 2 * b), dim3(128), 0, s, c, l, q, k, bs_qkv, ld_qkv, amax, qs, ks);
  hipLaunchKernelGGL(attn_split_v_h2_kernel, dim3(cdiv(lp / 8, 64), cp, b), dim3(64), 0, s, c, cp, l, lp, v, bs_qkv, ld_qkv, amax, vt);
  const int ksplit = key_slices;
  const long long total = (long long)cdiv(l, 128) * b * ksplit;
  BDM_REQUIRE(total < (1ll << 28), "attention_core_h2: too many workgroups");
  float *part_o = reinterpret_cast<float *>((reinterpret_cast<size_t>(vt + (size_t)b * 2 * cp * lp) + 63) & ~(size_t)63);
  float *part_ml = part_o + (size_t)ksplit * b * cp * l;
  dim3 grid((unsigned)(8 * ((total + 7) / 8)));
  if (cp == 32)
    hipLaunchKernelGGL(attn_flash_h2_kernel<1>, grid, dim3(256), 0, s, c, l, lp, b, (const uint4 *)qs, (const uint4 *)ks, vt, amax, out,
                       bs_o, ld_o, ksplit, part_o, part_ml);
  else
    hipLaunchKernelGGL(attn_flash_h2_kernel<2>, grid, dim3(256), 0, s, c, l, lp, b, (const uint4 *)qs, (const uint4 *)ks, vt, amax, out,
                       bs_o, ld_o, ksplit, part_o, part_ml);
  if (ksplit > 1)
    hipLaunchKernelGGL(attn_combine_kernel, dim3(cdiv(l, 256), 8, b), dim3(256), 0, s, c, cp, l, b, ksplit, part_o, part_ml, amax, out, bs_o, ld_o);
  return launch_status("attention_core_h2");
}
