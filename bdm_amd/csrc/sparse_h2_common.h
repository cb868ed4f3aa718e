// sparse_h2_common.h -- what the sparse first convolution's fp16x3 GEMMs (sparse_conv_h2.hip, sparse_conv_os.hip, pvconv_small.hip, and
// the experimental one-kernel form experimental/sparse_conv_fused.hip) share beyond h2_split.h: the scaled split of a record held as two
// float4 into MFMA operands, and the LDS-only barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "h2_split.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
namespace {

__device__ __forceinline__ void split_record(const float4 &p, const float4 &q, float s, f16x8 &hi, f16x8 &lo) {
  const float v[8] = {p.x * s, p.y * s, p.z * s, p.w * s, q.x * s, q.y * s, q.z * s, q.w * s};
  uint4 ph, pl;
  bdm::split2_record(v, ph, pl);
  hi = *reinterpret_cast<const f16x8 *>(&ph);
  lo = *reinterpret_cast<const f16x8 *>(&pl);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter (vmcnt(0)), i.e.
// it waits for the global loads issued as PREFETCH for later steps and so exposes their whole latency at every barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace
