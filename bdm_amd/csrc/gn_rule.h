// gn_rule.h -- the one definition of GroupNorm's finalisation: fp64 (sum, sum of squares) of a group -> fp32 (mean, rstd), and the
// per-channel affine form (a, b) with a*v + b.  Every kernel that normalises takes it from here, so a group has the same statistics
// whichever launch finalises them.  The summation that feeds it stays in each kernel (its order is that kernel's own), and so does the
// unfolded application (v - mean) * rstd * gamma + beta, which rounds differently from a*v + b and is never converted into it.
// No contraction pragma: no caller finalises under one, and the fp64 lines contract the same way in every translation unit.
#pragma once
#include <hip/hip_runtime.h>

namespace bdm {

__device__ __forceinline__ float gn_rstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }

__device__ __forceinline__ void gn_mean_rstd(double sum, double sumsq, double cnt, float eps, float &mean, float &rstd) {
  const double m = sum / cnt;
  double var = sumsq / cnt - m * m;
  if (var < 0) var = 0;
  mean = (float)m;
  rstd = gn_rstd(var, eps);
}

// x -> a x + b with a = gamma * rstd, b = beta - mean * a  (arguments in the order the two expressions read them)
__device__ __forceinline__ float2 gn_affine(float gamma, float rstd, float beta, float mean) {
  const float a = gamma * rstd;
  return make_float2(a, beta - mean * a);
}

}  // namespace bdm
