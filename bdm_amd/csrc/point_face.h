// point_face.h -- the one definition of the (point, face) pair rule of bdm_hip.h section 14 and of the 64-byte face record both
// directions of the distance read: mesh_metrics.hip (point to face: a point in registers, records streamed) and face_point.hip (face
// to point, section 17: a record in registers, points streamed).  Every translation unit that includes this is compiled with
// -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: the operations below are rounded one by one, in the order written.
//
// The record of a face, four float4:
//   r0 = (v0x, v0y, v0z, v1x)   r1 = (v1y, v1z, v2x, v2y)   r2 = (v2z, nx, ny, nz)   r3 = (nn, l2_0, l2_1, l2_2)
// nn == 0 marks an invalid face (all sixteen floats are 0 then).
#pragma once
#include "common.h"

#if defined(__HIPCC__)
#pragma clang fp contract(off)

namespace bdm {

__device__ __forceinline__ float mm_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

struct MmFace {
  float v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z;
  float nx, ny, nz, nn;   // nn == 0: invalid
};

// face `row` of the packed array, of a mesh whose vertices start at vbase and number nv.  false (and f.nn = 0) = invalid.
__device__ __forceinline__ bool mm_face_load(const float *__restrict__ verts, const int *__restrict__ faces, long long row,
                                             long long vbase, long long nv, MmFace &f) {
  f.nn = 0.f;
  const int *fp = faces + (size_t)row * 3;
  const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return false;
  const float *a = verts + (size_t)(vbase + i0) * 3, *b = verts + (size_t)(vbase + i1) * 3, *c = verts + (size_t)(vbase + i2) * 3;
  f.v0x = a[0]; f.v0y = a[1]; f.v0z = a[2];
  f.v1x = b[0]; f.v1y = b[1]; f.v1z = b[2];
  f.v2x = c[0]; f.v2y = c[1]; f.v2z = c[2];
  if (!(finite1(f.v0x) && finite1(f.v0y) && finite1(f.v0z) && finite1(f.v1x) && finite1(f.v1y) && finite1(f.v1z) &&
        finite1(f.v2x) && finite1(f.v2y) && finite1(f.v2z)))
    return false;
  const float ex = f.v1x - f.v0x, ey = f.v1y - f.v0y, ez = f.v1z - f.v0z;   // e_0
  const float gx = f.v2x - f.v0x, gy = f.v2y - f.v0y, gz = f.v2z - f.v0z;   // g
  f.nx = ey * gz - ez * gy;
  f.ny = ez * gx - ex * gz;
  f.nz = ex * gy - ey * gx;
  const float nn = mm_dot(f.nx, f.ny, f.nz, f.nx, f.ny, f.nz);
  if (!(nn > 0.f && nn < INFINITY)) return false;
  f.nn = nn;
  return true;
}

// the record of face `row` into r[0 .. 3]; zeros for an invalid face
__device__ __forceinline__ void mm_record_store(const float *__restrict__ verts, const int *__restrict__ faces, long long row,
                                                long long vbase, long long nv, float4 *__restrict__ r) {
  MmFace f;
  if (!mm_face_load(verts, faces, row, vbase, nv, f)) {
    r[0] = r[1] = r[2] = r[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float e0x = f.v1x - f.v0x, e0y = f.v1y - f.v0y, e0z = f.v1z - f.v0z;
  const float e1x = f.v2x - f.v1x, e1y = f.v2y - f.v1y, e1z = f.v2z - f.v1z;
  const float e2x = f.v0x - f.v2x, e2y = f.v0y - f.v2y, e2z = f.v0z - f.v2z;
  r[0] = make_float4(f.v0x, f.v0y, f.v0z, f.v1x);
  r[1] = make_float4(f.v1y, f.v1z, f.v2x, f.v2y);
  r[2] = make_float4(f.v2z, f.nx, f.ny, f.nz);
  r[3] = make_float4(f.nn, mm_dot(e0x, e0y, e0z, e0x, e0y, e0z), mm_dot(e1x, e1y, e1z, e1x, e1y, e1z), mm_dot(e2x, e2y, e2z, e2x, e2y, e2z));
}

// squared distance from x to the segment a + t e, t in [0, 1] (section 14's "Segment")
__device__ __forceinline__ float mm_segment(float x, float y, float z, float ax, float ay, float az, float ex, float ey, float ez, float l2) {
  const float rx = x - ax, ry = y - ay, rz = z - az;
  const float h = mm_dot(ex, ey, ez, rx, ry, rz);
  float t = l2 == 0.f ? 0.f : h / l2;
  t = t > 0.f ? t : 0.f;
  t = t < 1.f ? t : 1.f;
  const float wx = x - (ax + t * ex), wy = y - (ay + t * ey), wz = z - (az + t * ez);
  return mm_dot(wx, wy, wz, wx, wy, wz);
}

// s_i of the inside test: dot(n, cross(e, x - a))
__device__ __forceinline__ float mm_side(float x, float y, float z, float ax, float ay, float az, float ex, float ey, float ez, float nx,
                                         float ny, float nz) {
  const float rx = x - ax, ry = y - ay, rz = z - az;
  return mm_dot(nx, ny, nz, ey * rz - ez * ry, ez * rx - ex * rz, ex * ry - ey * rx);
}

// section 14's d of the pair (point (x, y, z), the VALID face whose record is r0 .. r3).  The nine edge differences depend on the
// record alone: a caller that holds the record in registers across a loop over points has them hoisted out of it.
__device__ __forceinline__ float mm_pair_sqdist(float x, float y, float z, const float4 r0, const float4 r1, const float4 r2,
                                                const float4 r3) {
  const float v0x = r0.x, v0y = r0.y, v0z = r0.z, v1x = r0.w, v1y = r1.x, v1z = r1.y, v2x = r1.z, v2y = r1.w, v2z = r2.x;
  const float nx = r2.y, ny = r2.z, nz = r2.w, nn = r3.x;
  const float e0x = v1x - v0x, e0y = v1y - v0y, e0z = v1z - v0z;
  const float e1x = v2x - v1x, e1y = v2y - v1y, e1z = v2z - v1z;
  const float e2x = v0x - v2x, e2y = v0y - v2y, e2z = v0z - v2z;
  float d = mm_segment(x, y, z, v0x, v0y, v0z, e0x, e0y, e0z, r3.y);
  const float d1 = mm_segment(x, y, z, v1x, v1y, v1z, e1x, e1y, e1z, r3.z);
  const float d2 = mm_segment(x, y, z, v2x, v2y, v2z, e2x, e2y, e2z, r3.w);
  d = d1 < d ? d1 : d;
  d = d2 < d ? d2 : d;
  const float s0 = mm_side(x, y, z, v0x, v0y, v0z, e0x, e0y, e0z, nx, ny, nz);
  const float s1 = mm_side(x, y, z, v1x, v1y, v1z, e1x, e1y, e1z, nx, ny, nz);
  const float s2 = mm_side(x, y, z, v2x, v2y, v2z, e2x, e2y, e2z, nx, ny, nz);
  if (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f) {
    const float kk = mm_dot(nx, ny, nz, x - v0x, y - v0y, z - v0z);
    const float dp = (kk * kk) / nn;
    d = dp < d ? dp : d;
  }
  return d;
}

}  // namespace bdm
#endif
