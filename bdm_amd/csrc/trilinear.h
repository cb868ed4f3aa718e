// trilinear.h -- the one definition of the trilinear devoxelisation's arithmetic (trilinear_devox.cu:64-75), shared by every kernel
// that gathers from a voxel grid (devox_kernel in pvcnn_ops.hip, devox_train_kernel in backward_ops.hip, the folded forms of
// dense_ops.hip, pvconv_small.hip and pvconv_compact.hip), so that the forms agree bit for bit by construction:
//   the eight corner weights and indices of a point, the left-to-right sum over the corners, and the cell value of a folded
//   GroupNorm-2 + Swish + SE gate.
// The weights define which cells a point reads and the sums are compared with torch.equal: every body is written unfused and carries
// `#pragma clang fp contract(off)` itself -- the flag travels with the inlined instructions, whatever the caller's scope or flags.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace bdm {

// corners in the order 000, 001, 010, 011, 100, 101, 110, 111 (z fastest)
struct TrilinearCorners {
  float w[8];
  int i[8];
};

// (x, y, z) in voxel units inside an r^3 grid.  The +1 neighbour on an axis is addressed only when the fractional part is > 0: a
// corner of weight 0 aliases an in-grid cell (its value is finite and multiplies 0).
__device__ __forceinline__ TrilinearCorners trilinear_corners(float x, float y, float z, int r) {
#pragma clang fp contract(off)
  TrilinearCorners t;
  const int r2 = r * r;
  const float xl = floorf(x), yl = floorf(y), zl = floorf(z);
  const float x1 = x - xl, y1 = y - yl, z1 = z - zl;
  const float x0 = 1.0f - x1, y0 = 1.0f - y1, z0 = 1.0f - z1;
  t.w[0] = x0 * y0 * z0; t.w[1] = x0 * y0 * z1; t.w[2] = x0 * y1 * z0; t.w[3] = x0 * y1 * z1;
  t.w[4] = x1 * y0 * z0; t.w[5] = x1 * y0 * z1; t.w[6] = x1 * y1 * z0; t.w[7] = x1 * y1 * z1;
  const int sx = x1 > 0 ? r2 : 0, sy = y1 > 0 ? r : 0, sz = z1 > 0 ? 1 : 0;
  const int i000 = (int)xl * r2 + (int)yl * r + (int)zl;
  const int i010 = i000 + sy, i100 = i000 + sx, i110 = i100 + sy;
  t.i[0] = i000; t.i[1] = i000 + sz; t.i[2] = i010; t.i[3] = i010 + sz;
  t.i[4] = i100; t.i[5] = i100 + sz; t.i[6] = i110; t.i[7] = i110 + sz;
  return t;
}

// ((w0 v0 + w1 v1) + w2 v2) + ... + w7 v7, the values given as an array or, evaluated one at a time right before their product,
// as value(k)
template <class F>
__device__ __forceinline__ float trilinear_sum_of(const float (&w)[8], F &&value) {
#pragma clang fp contract(off)
  float acc = w[0] * value(0);
#pragma unroll
  for (int k = 1; k < 8; ++k) acc += w[k] * value(k);
  return acc;
}
__device__ __forceinline__ float trilinear_sum(const float (&w)[8], const float (&v)[8]) {
  return trilinear_sum_of(w, [&](int k) { return v[k]; });
}

// cell value of the folded tail: Swish(GroupNorm-2(g)) * gate, the GroupNorm as the affine form a g + b (gn_rule.h)
__device__ __forceinline__ float gn_swish_gate(float g, float a, float b, float s) {
#pragma clang fp contract(off)
  return swishf(g * a + b) * s;
}
__device__ __forceinline__ float gn_swish_gate(float g, float2 ab, float s) { return gn_swish_gate(g, ab.x, ab.y, s); }
__device__ __forceinline__ float4 gn_swish_gate(float4 g, float2 ab, float s) {
  return make_float4(gn_swish_gate(g.x, ab, s), gn_swish_gate(g.y, ab, s), gn_swish_gate(g.z, ab, s), gn_swish_gate(g.w, ab, s));
}

}  // namespace bdm
