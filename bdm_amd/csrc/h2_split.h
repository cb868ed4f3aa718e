// h2_split.h -- the one definition of the two-term fp16 split ("H2") shared by every kernel that writes fp16x3 operands (conv3d_h2.hip,
// pvconv_compact.hip, the sparse first convolution through sparse_h2_common.h, experimental/sparse_gather_h2_small.hip):
//   v = hi + lo  with hi = RN_11(v), lo = RN_11(v - hi) (the remainder is exact in fp32), v saturated at +-65504 instead of overflowing
//   to inf.  A record is 8 consecutive channels of one position = 8 fp16 = 16 bytes per term.
// With it: the power-of-two activation scale derived from a maximum, the host-side check that a caller's scale IS a power of two, and
// the launcher of the per-output-channel weight scale (the kernel lives in conv3d_h2.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace bdm {

__device__ __forceinline__ void split2(float v, unsigned short &h, unsigned short &l) {
  v = fminf(fmaxf(v, -65504.f), 65504.f);         // saturate instead of overflowing to inf
  const _Float16 hi = (_Float16)v;                // round to nearest even
  const _Float16 lo = (_Float16)(v - (float)hi);  // the remainder is exact in fp32
  h = __builtin_bit_cast(unsigned short, hi);
  l = __builtin_bit_cast(unsigned short, lo);
}

// eight values -> the (hi, lo) records
__device__ __forceinline__ void split2_record(const float v[8], uint4 &ph, uint4 &pl) {
  unsigned short h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) split2(v[j], h[j], l[j]);
  ph.x = h[0] | (h[1] << 16); ph.y = h[2] | (h[3] << 16); ph.z = h[4] | (h[5] << 16); ph.w = h[6] | (h[7] << 16);
  pl.x = l[0] | (l[1] << 16); pl.y = l[2] | (l[3] << 16); pl.z = l[4] | (l[5] << 16); pl.w = l[6] | (l[7] << 16);
}

// power of two s with amax * s in [2^14, 2^15)  (1 when amax is 0 / not finite)
__device__ __forceinline__ float act_scale_from_max(float amax) {
  if (!(amax > 0.f) || !(amax < INFINITY)) return 1.f;
  int ex;
  (void)frexpf(amax, &ex);  // amax = f * 2^ex, f in [0.5, 1)
  return ldexpf(1.f, 15 - ex);
}

// host: a caller-chosen activation scale must be a finite positive power of two (it is divided out exactly in the epilogue)
inline bool h2_scale_is_pow2(float act_scale) {
  int ex = 0;
  return act_scale > 0.f && act_scale < INFINITY && frexpf(act_scale, &ex) == 0.5f;
}

// host: scale[co] = 2^e with max |w[co]| * 2^e in [2^9, 2^10), inv_scale[co] = 2^-e  (h2_weight_scale_kernel, conv3d_h2.hip)
void h2_weight_scale(int cout, int cin, const float *w, float *scale, float *inv_scale, hipStream_t s);

}  // namespace bdm
