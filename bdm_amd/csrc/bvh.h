// bvh.h -- what mesh_bvh.hip (the build) and mesh_raycast.hip (the queries) share: the ray rule of bdm_hip.h section 24 (the set-up of
// a ray, the interval of a box, the triangle test), the node record and the layout of the caller-owned hierarchy buffer.  The rule is
// restated by tests/mesh_raycast_ref.py; DESIGN.md section 28 holds the argument that culling by boxes changes no answer.
//
// Both .hip files are compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: every operation below is rounded on
// its own, in the order written.  No function here indexes a per-lane array with a runtime value: axes are picked by selects.
#pragma once
#include "mesh_incidence.h"

#include <limits.h>
#include <math.h>

namespace bdm {

constexpr int BVH_THREADS = MESH_THREADS;
constexpr int BVH_HEAD_INTS = 4;                   // per mesh: used faces n, dropped faces, 0, 0
constexpr long long BVH_DROPPED = 1ll << 30;       // the key bit of a dropped face: it sorts behind the used faces of its mesh
constexpr float BVH_SHRINK = 0.9999847412109375f;  // 1 - 2^-16
constexpr float BVH_GROW = 1.0000152587890625f;    // 1 + 2^-16

// lo, hi of the box, link (internal: left child; leaf: face inside its mesh), skip (the node after the subtree, -1: none)
struct alignas(16) BvhNode {
  float lox, loy, loz, hix, hiy, hiz;
  int link, skip;
};
static_assert(sizeof(BvhNode) == 32, "a node is two 16-byte loads");

// the heads of the b meshes, then 2 sum F nodes: those of mesh m start at node 2 face_first[m]
struct BvhLayout {
  int *head;
  BvhNode *nodes;
  size_t bytes;
};
static inline BvhLayout bvh_layout(void *buf, int b, long long sum_f) {
  Carve c{(char *)buf, 0};
  BvhLayout l;
  l.head = c.take<int>((size_t)BVH_HEAD_INTS * (b > 0 ? b : 1));
  l.nodes = c.take<BvhNode>(2 * (size_t)(sum_f > 0 ? sum_f : 1));
  l.bytes = c.o;
  return l;
}
static inline bool bvh_sizes_ok(int b, long long sum_v, long long sum_f, long long sum_r) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_f >= 0 && sum_r >= 0 && sum_v < INT_MAX && 3 * sum_f < INT_MAX && sum_r < INT_MAX;
}

#if defined(__HIPCC__)
#pragma clang fp contract(off)

__device__ __forceinline__ float bvh_pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

struct BvhRay {
  float ox, oy, oz, tmin, tmax;
  float ix, iy, iz;    // 1 / d per axis: the infinity of its sign for a zero
  float sx, sy, sz;    // the shear and the scale of the triangle test
  int kx, ky, kz;
  bool nx, ny, nz;     // the sign bit of d per axis
  bool valid;
};

__device__ __forceinline__ BvhRay bvh_ray(const float *__restrict__ r) {
  BvhRay q;
  const float dx = r[3], dy = r[4], dz = r[5];
  q.ox = r[0], q.oy = r[1], q.oz = r[2], q.tmin = r[6], q.tmax = r[7];
  q.valid = finite3(q.ox, q.oy, q.oz) && finite3(dx, dy, dz) && finite1(q.tmin) && !(dx == 0.f && dy == 0.f && dz == 0.f) &&
            q.tmax == q.tmax && q.tmin <= q.tmax;
  q.ix = 1.0f / dx, q.iy = 1.0f / dy, q.iz = 1.0f / dz;
  q.nx = signbit(dx), q.ny = signbit(dy), q.nz = signbit(dz);
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  int kz = 0;
  float big = ax;
  if (ay > big) kz = 1, big = ay;
  if (az > big) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dk = bvh_pick(dx, dy, dz, kz);
  if (dk < 0.f) {
    const int s = kx;
    kx = ky, ky = s;
  }
  q.kx = kx, q.ky = ky, q.kz = kz;
  q.sx = bvh_pick(dx, dy, dz, kx) / dk, q.sy = bvh_pick(dx, dy, dz, ky) / dk, q.sz = 1.0f / dk;
  return q;
}

// one axis of rule 4: the widened entry and exit parameters of the slab lo .. hi
__device__ __forceinline__ void bvh_slab(float lo, float hi, float o, float inv, bool neg, float &tn, float &tf) {
  const float a = (lo - o) * inv, b = (hi - o) * inv;
  const float n = neg ? b : a, f = neg ? a : b;
  tn = n >= 0.f ? n * BVH_SHRINK : n * BVH_GROW;
  tf = f >= 0.f ? f * BVH_GROW : f * BVH_SHRINK;
}

// rule 4 for any box: [near, far] with the ray's own tmin and tmax folded in; a NaN constrains nothing
__device__ __forceinline__ void bvh_interval(const BvhRay &q, float lox, float loy, float loz, float hix, float hiy, float hiz, float &near,
                                             float &far) {
  float nx, fx, ny, fy, nz, fz;
  bvh_slab(lox, hix, q.ox, q.ix, q.nx, nx, fx);
  bvh_slab(loy, hiy, q.oy, q.iy, q.ny, ny, fy);
  bvh_slab(loz, hiz, q.oz, q.iz, q.nz, nz, fz);
  near = fmaxf(fmaxf(fmaxf(q.tmin, nx), ny), nz);
  far = fminf(fminf(fminf(q.tmax, fx), fy), fz);
}

struct BvhHit {
  float t, b1, b2;
  bool back;
};

// rules 3 and 4 for one used face with corners a, b, c -> accepted?
__device__ __forceinline__ bool bvh_face(const BvhRay &q, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                         float cz, BvhHit &h) {
  float near, far;
  bvh_interval(q, fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz), fmaxf(fmaxf(ax, bx), cx),
               fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz), near, far);
  if (!(near <= far)) return false;   // implied by the last test: leaves early
  const float pax = ax - q.ox, pay = ay - q.oy, paz = az - q.oz;
  const float pbx = bx - q.ox, pby = by - q.oy, pbz = bz - q.oz;
  const float pcx = cx - q.ox, pcy = cy - q.oy, pcz = cz - q.oz;
  const float akz = bvh_pick(pax, pay, paz, q.kz), bkz = bvh_pick(pbx, pby, pbz, q.kz), ckz = bvh_pick(pcx, pcy, pcz, q.kz);
  const float Ax = bvh_pick(pax, pay, paz, q.kx) - q.sx * akz, Ay = bvh_pick(pax, pay, paz, q.ky) - q.sy * akz;
  const float Bx = bvh_pick(pbx, pby, pbz, q.kx) - q.sx * bkz, By = bvh_pick(pbx, pby, pbz, q.ky) - q.sy * bkz;
  const float Cx = bvh_pick(pcx, pcy, pcz, q.kx) - q.sx * ckz, Cy = bvh_pick(pcx, pcy, pcz, q.ky) - q.sy * ckz;
  float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  double Ud = U, Vd = V, Wd = W;
  if (U == 0.f || V == 0.f || W == 0.f) {
    Ud = (double)Cx * (double)By - (double)Cy * (double)Bx;
    Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
    Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
    U = (float)Ud, V = (float)Vd, W = (float)Wd;
  }
  if ((Ud < 0.0 || Vd < 0.0 || Wd < 0.0) && (Ud > 0.0 || Vd > 0.0 || Wd > 0.0)) return false;
  const float det = (U + V) + W;
  if (det == 0.f) return false;
  const float Az = q.sz * akz, Bz = q.sz * bkz, Cz = q.sz * ckz;
  const float t = ((U * Az + V * Bz) + W * Cz) / det;
  if (!(near <= t && t <= far && fabsf(t) < INFINITY)) return false;   // a NaN fails
  h.t = t, h.b1 = V / det, h.b2 = W / det, h.back = det < 0.f;
  return true;
}

// the corners of face `row` (packed) of a mesh of nv vertices from vbase on, if the face is used (rule 2)
__device__ __forceinline__ bool bvh_load_face(const float *__restrict__ verts, const int *__restrict__ faces, long long row, long long vbase,
                                              long long nv, float (&p)[9]) {
  int idx[3];
  if (!connected_face(faces, row, nv, idx)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float *v = verts + 3 * (size_t)(vbase + idx[c]);
    p[3 * c] = v[0], p[3 * c + 1] = v[1], p[3 * c + 2] = v[2];
  }
  return finite3(p[0], p[1], p[2]) && finite3(p[3], p[4], p[5]) && finite3(p[6], p[7], p[8]);
}
#endif

}  // namespace bdm
