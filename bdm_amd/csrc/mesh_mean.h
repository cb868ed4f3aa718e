// mesh_mean.h -- the order-free fixed-point mean that mesh_decimate.hip (clusters) and mesh_qem.hip (the vertices an edge collapse
// merged) share: bdm_hip.h section 19 rule 5.  A value v of a set whose largest finite magnitude has the bits amax_bits is quantised to
// rint(v 2^e) as a 64-bit integer, the integers are summed in any order, and the mean is one float64 division rounded once to float32.
#pragma once
#include "common.h"

namespace bdm {

namespace {

#if defined(__HIPCC__)
// the exponent e of the fixed point: every finite |value| <= amax quantises to rint(value 2^e) below 2^40 in magnitude
__device__ __forceinline__ int mean_scale_exp(unsigned amax_bits) {
  const int field = (int)((amax_bits >> 23) & 0xffu);
  return 39 - ((field < 1 ? 1 : field) - 127);
}

// S 2^-e / n in float64, rounded once to float32
__device__ __forceinline__ float mean_of_sum(long long s, double inv, double n) { return (float)(((double)s * inv) / n); }
#endif

}  // namespace

}  // namespace bdm
