// mesh_raycast.hip -- rays against a packed batch of triangle meshes as gfx950 kernels: the closest hit, the occlusion flag and the
// crossing count under the rule of bdm_hip.h section 24 (bvh.h holds its arithmetic), once over the hierarchy
// of mesh_bvh.hip and once over every face.  One ray per lane in both.
//
//   rc_tree_kernel<MODE>   walks the nodes of the ray's mesh from node 0: an internal node is entered (link) when its interval is not
//                          empty and, for the closest hit, does not begin behind the best t so far (a strict >: an equal t with a
//                          lower face index is still found); otherwise the walk goes to skip.  A leaf runs the face rule.  No stack
//                          and no per-lane array: the state is the node index.  The loop ends after 2 n steps at the latest and at
//                          a link outside 0 .. 2 n - 2, whatever the buffer holds; a face index outside the mesh is not followed.
//   rc_all_kernel<MODE>    the same rule on every face: a workgroup stages 256 faces at a time in LDS (nine floats and a flag each,
//                          10 KiB; every lane reads the same face at the same time: a broadcast, no bank conflict), as the
//                          point-to-face kernel of mesh_metrics.hip does.  Ascending face order and a strict < give the lowest index
//                          on equal t.
// Both sum the ray counts of a workgroup in LDS and add them once; faces used and dropped come from the head of the hierarchy
// (tree) or are counted while staging by workgroup 0 of the mesh (exhaustive).
#include "../../include/bdm_hip.h"
#include "bvh.h"

#pragma clang fp contract(off)

using namespace bdm;

#define RC_COUNTS 5   // per mesh: valid rays, invalid rays, rays with an accepted face, faces used, faces dropped

namespace {

struct RcOut {
  float *t;
  int *face;
  float *bary;
  unsigned char *back, *occluded;
  int *crossings;
};

// what one ray has found so far
struct RcBest {
  float t, b1, b2;
  int face, count;
  bool back;
};

__device__ __forceinline__ RcBest rc_none() { return RcBest{INFINITY, 0.f, 0.f, -1, 0, false}; }

__device__ __forceinline__ void rc_take(RcBest &best, const BvhHit &h, int face) {
  ++best.count;
  if (h.t < best.t || (h.t == best.t && face < best.face)) best.t = h.t, best.b1 = h.b1, best.b2 = h.b2, best.face = face, best.back = h.back;
}

template <int MODE>
__device__ __forceinline__ void rc_write(const RcOut &o, long long row, const RcBest &best) {
  if (MODE == 0) {
    if (o.t) o.t[row] = best.t;
    if (o.face) o.face[row] = best.face;
    if (o.bary) o.bary[2 * row] = best.b1, o.bary[2 * row + 1] = best.b2;
    if (o.back) o.back[row] = best.back ? 1 : 0;
  } else if (MODE == 1) {
    if (o.occluded) o.occluded[row] = best.count > 0 ? 1 : 0;
  } else {
    if (o.crossings) o.crossings[row] = best.count;
  }
}

__device__ __forceinline__ BvhRay rc_load_ray(const float *__restrict__ rays, long long row) {
  const float4 a = *(const float4 *)(rays + 8 * (size_t)row), b = *(const float4 *)(rays + 8 * (size_t)row + 4);
  const float r[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return bvh_ray(r);
}

// part: valid, invalid, with a hit -> one atomic add each per workgroup
__device__ __forceinline__ void rc_tally(int *part, bool live, bool valid, bool hit) {
  const int v = __popcll(__ballot(live && valid)), i = __popcll(__ballot(live && !valid)), h = __popcll(__ballot(live && hit));
  if ((threadIdx.x & 63) == 0) {
    if (v) atomicAdd(part + 0, v);
    if (i) atomicAdd(part + 1, i);
    if (h) atomicAdd(part + 2, h);
  }
}

template <int MODE>
__global__ __launch_bounds__(BVH_THREADS) void rc_tree_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                              const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                              const long long *__restrict__ ray_first, const int *__restrict__ head,
                                                              const BvhNode *__restrict__ nodes, const float *__restrict__ rays, RcOut out,
                                                              int *__restrict__ counts) {
  __shared__ int part[3];
  const int m = blockIdx.y;
  const long long rbase = ray_first[m], nr = ray_first[m + 1] - rbase;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  int n = head[BVH_HEAD_INTS * m];
  n = n < 0 ? 0 : (n > nf ? (int)nf : n);
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[RC_COUNTS * m + 3] = n, counts[RC_COUNTS * m + 4] = (int)nf - n;
  if ((long long)blockIdx.x * BVH_THREADS >= nr) return;   // the whole workgroup
  if (threadIdx.x < 3) part[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  const bool live = i < nr;
  RcBest best = rc_none();
  bool valid = false;
  if (live) {
    const BvhRay q = rc_load_ray(rays, rbase + i);
    valid = q.valid;
    const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
    const BvhNode *nb = nodes + 2 * fbase;
    int node = valid && n > 0 ? 0 : -1;
    for (int step = 0; step < 2 * n && node >= 0 && node < 2 * n - 1; ++step) {
      const float4 a = *(const float4 *)(nb + node), c = *((const float4 *)(nb + node) + 1);
      const int link = __float_as_int(c.z), skip = __float_as_int(c.w);
      if (node >= n - 1) {   // a leaf
        float p[9];
        BvhHit h;
        if (link >= 0 && link < nf && bvh_load_face(verts, faces, fbase + link, vbase, nv, p) &&
            bvh_face(q, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], h))
          rc_take(best, h, link);
        node = (MODE == 1 && best.count > 0) ? -1 : skip;
      } else {
        float near, far;
        bvh_interval(q, a.x, a.y, a.z, a.w, c.x, c.y, near, far);
        bool enter = near <= far;
        if (MODE == 0) enter = enter && !(near > best.t);
        node = enter ? link : skip;
      }
    }
    rc_write<MODE>(out, rbase + i, best);
  }
  rc_tally(part, live, valid, best.count > 0);
  __syncthreads();
  if (threadIdx.x < 3 && part[threadIdx.x]) atomicAdd(counts + RC_COUNTS * m + threadIdx.x, part[threadIdx.x]);
}

template <int MODE>
__global__ __launch_bounds__(BVH_THREADS) void rc_all_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                             const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                             const long long *__restrict__ ray_first, const float *__restrict__ rays, RcOut out,
                                                             int *__restrict__ counts) {
  __shared__ float tri[9][BVH_THREADS];
  __shared__ int used[BVH_THREADS];
  __shared__ int part[4];
  const int m = blockIdx.y;
  const long long rbase = ray_first[m], nr = ray_first[m + 1] - rbase;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  if ((long long)blockIdx.x * BVH_THREADS >= nr && blockIdx.x != 0) return;   // the whole workgroup; workgroup 0 counts the faces
  if (threadIdx.x < 4) part[threadIdx.x] = 0;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  const bool live = i < nr;
  RcBest best = rc_none();
  BvhRay q;
  q.valid = false;
  if (live) q = rc_load_ray(rays, rbase + i);
  const bool valid = live && q.valid;
  for (long long c0 = 0; c0 < nf; c0 += BVH_THREADS) {   // uniform trip count
    __syncthreads();
    float p[9];
    const bool ok = c0 + threadIdx.x < nf && bvh_load_face(verts, faces, fbase + c0 + threadIdx.x, vbase, nv, p);
    used[threadIdx.x] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[k][threadIdx.x] = ok ? p[k] : 0.f;
    if (blockIdx.x == 0) {
      const int u = __popcll(__ballot(ok));
      if ((threadIdx.x & 63) == 0 && u) atomicAdd(part + 3, u);
    }
    __syncthreads();
    const int len = nf - c0 < BVH_THREADS ? (int)(nf - c0) : BVH_THREADS;
    if (valid && !(MODE == 1 && best.count > 0)) {
      for (int k = 0; k < len; ++k) {
        BvhHit h;
        if (used[k] && bvh_face(q, tri[0][k], tri[1][k], tri[2][k], tri[3][k], tri[4][k], tri[5][k], tri[6][k], tri[7][k], tri[8][k], h)) {
          rc_take(best, h, (int)c0 + k);
          if (MODE == 1) break;
        }
      }
    }
  }
  if (live) rc_write<MODE>(out, rbase + i, best);
  __syncthreads();
  rc_tally(part, live, valid, best.count > 0);
  __syncthreads();
  if (threadIdx.x < 3 && part[threadIdx.x]) atomicAdd(counts + RC_COUNTS * m + threadIdx.x, part[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 3) counts[RC_COUNTS * m + 3] = part[3], counts[RC_COUNTS * m + 4] = (int)nf - part[3];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the offsets of the vertices and faces | those of the rays
struct RcWs {
  long long *vert_first, *face_first, *ray_first;
  size_t bytes;
};
RcWs rc_ws(void *ws, int b) {
  Carve c{(char *)ws, 0};
  RcWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.ray_first = c.take_offsets(b);
  w.bytes = c.o;
  return w;
}

int rc_run(const char *what, bool tree, int mode, int b, const float *verts, const int *faces, const long long *vert_first,
           const long long *face_first, const void *bvh, const float *rays, const long long *ray_first, const RcOut &o, int *counts,
           void *workspace, void *stream) {
  long long max_v = 0, max_f = 0, max_r = 0;
  if (check_mesh_batch(what, b, vert_first, face_first, true, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(mode >= 0 && mode <= 2, "%s: mode=%d is none of 0 (closest), 1 (any), 2 (count)", what, mode);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(ray_first, "%s: an offset array is NULL", what);
  if (check_first(what, "mesh", b, ray_first, &max_r) != BDM_OK) return BDM_ERR_ARG;
  const long long sum_v = vert_first[b], sum_f = face_first[b], sum_r = ray_first[b];
  BDM_REQUIRE(sum_v < INT_MAX && 3 * sum_f < INT_MAX && sum_r < INT_MAX, "%s: %lld vertices, %lld faces (three corners each) or %lld rays reach 2^31",
              what, sum_v, sum_f, sum_r);
  BDM_REQUIRE(verts && faces && rays && counts, "%s: an input or the counts are NULL", what);
  BDM_REQUIRE(((uintptr_t)rays & 15) == 0, "%s: the rays are not 16-byte aligned", what);
  BDM_REQUIRE(!tree || (bvh && ((uintptr_t)bvh & 15) == 0), "%s: the hierarchy buffer is NULL or not 16-byte aligned", what);
  if (check_workspace(what, workspace) != BDM_OK) return BDM_ERR_ARG;
  const RcWs w = rc_ws(workspace, b);
  const size_t r = (size_t)sum_r;
  const Range in[4] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {rays, 32 * r}, {bvh, tree ? bvh_layout(nullptr, b, sum_f).bytes : 0}};
  const Range out[8] = {{o.t, 4 * r}, {o.face, 4 * r}, {o.bary, 8 * r}, {o.back, r}, {o.occluded, r}, {o.crossings, 4 * r},
                        {counts, 4 * RC_COUNTS * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap(what, in, 4, out, 8) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  send_offsets(b, ray_first, nullptr, w.ray_first, w.ray_first + (b + 1), st);
  fill_ints(counts, (long long)RC_COUNTS * b, 0, st);
  const dim3 grid((unsigned)(max_r > 0 ? cdivll(max_r, BVH_THREADS) : 1), (unsigned)b), block(BVH_THREADS);
  if (tree) {
    const BvhLayout l = bvh_layout(const_cast<void *>(bvh), b, sum_f);
#define RC_TREE(M) hipLaunchKernelGGL(rc_tree_kernel<M>, grid, block, 0, st, verts, faces, w.vert_first, w.face_first, w.ray_first, l.head, l.nodes, rays, o, counts)
    if (mode == 0) RC_TREE(0); else if (mode == 1) RC_TREE(1); else RC_TREE(2);
#undef RC_TREE
  } else {
#define RC_ALL(M) hipLaunchKernelGGL(rc_all_kernel<M>, grid, block, 0, st, verts, faces, w.vert_first, w.face_first, w.ray_first, rays, o, counts)
    if (mode == 0) RC_ALL(0); else if (mode == 1) RC_ALL(1); else RC_ALL(2);
#undef RC_ALL
  }
  return launch_status(what);
}

}  // namespace

extern "C" size_t bdm_mesh_raycast_workspace_bytes(int b) {
  if (b < 0 || b > MESH_MAX_B) return 0;
  return rc_ws(nullptr, b).bytes;
}

extern "C" int bdm_mesh_raycast(int mode, int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first,
                                const void *bvh, const float *rays, const long long *ray_first, float *t, int *face, float *bary,
                                unsigned char *back, unsigned char *occluded, int *crossings, int *counts, void *workspace, void *stream) {
  return rc_run("mesh_raycast", true, mode, b, verts, faces, vert_first, face_first, bvh, rays, ray_first,
                RcOut{t, face, bary, back, occluded, crossings}, counts, workspace, stream);
}

extern "C" int bdm_mesh_raycast_exhaustive(int mode, int b, const float *verts, const int *faces, const long long *vert_first,
                                           const long long *face_first, const float *rays, const long long *ray_first, float *t, int *face,
                                           float *bary, unsigned char *back, unsigned char *occluded, int *crossings, int *counts,
                                           void *workspace, void *stream) {
  return rc_run("mesh_raycast_exhaustive", false, mode, b, verts, faces, vert_first, face_first, nullptr, rays, ray_first,
                RcOut{t, face, bary, back, occluded, crossings}, counts, workspace, stream);
}
