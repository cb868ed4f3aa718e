// mesh_bvh.hip -- a linear bounding-volume hierarchy over the used faces of every mesh of a packed batch, as gfx950 kernels (bdm_hip.h
// section 24; bvh.h holds the node record and the buffer layout).  Two calls with a stable sort of the caller's
// between them (torch.sort(stable=True) in bdm_amd/mesh_raycast.py, as mesh_metrics.py sorts between two calls):
//
// bdm_mesh_bvh_keys, after send_offsets (ragged.h):
//   bvh_bounds_kernel  one thread per vertex: the box of the finite vertices of its mesh, by integer atomic min / max on the ordered
//                      bits of the floats (LDS first, one global atomic per workgroup and bound): min / max do not depend on order.
//   bvh_keys_kernel    one thread per face: (mesh << 32) | (dropped << 30) | the 30-bit Morton code of its centroid in that box.
// bdm_mesh_bvh_build, given the sorted keys and the permutation:
//   bvh_head_kernel    one thread per sorted slot: the slot after which the dropped faces of a mesh begin gives n, the number of used
//                      faces: the head of the mesh in the buffer and the two counts.
//   bvh_tree_kernel    one thread per internal node i < n - 1: its range, split and children by Karras' search on (key, position), so
//                      that equal keys still split by position and the depth is at most 60; the parent of both children; and
//                      after[split] = the right child: every node whose range ends at `split` is followed by that child in a
//                      depth-first walk, so the skip links need no top-down pass.  Every loop is a bisection of at most 32 steps.
//   bvh_fit_kernel     one thread per leaf j < n: the box of its face, its links, and those of internal node j; then it climbs: at
//                      each parent it adds 1 to the node's arrival counter; the first to arrive leaves, the second reads both
//                      children's boxes (fenced, volatile) and writes the parent's.  Nobody waits: at most 64 steps up.
#include "../../include/bdm_hip.h"
#include "bvh.h"

#include <string.h>

#pragma clang fp contract(off)

using namespace bdm;

namespace {

__device__ __forceinline__ unsigned bvh_ordered(float f) {   // unsigned order = float order (-0 below +0)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bvh_unordered(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// lo: [3 b] ordered bits, filled with 0xffffffff; hi: [3 b], filled with 0
__global__ __launch_bounds__(BVH_THREADS) void bvh_bounds_kernel(const float *__restrict__ verts, const long long *__restrict__ vert_first,
                                                                 unsigned *__restrict__ lo, unsigned *__restrict__ hi) {
  __shared__ unsigned part[6];
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  if ((long long)blockIdx.x * BVH_THREADS >= nv) return;   // the whole workgroup
  if (threadIdx.x < 6) part[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  const long long i = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  if (i < nv) {
    const float *p = verts + 3 * (size_t)(vbase + i);
    const float x = p[0], y = p[1], z = p[2];
    if (finite3(x, y, z)) {
      atomicMin(part + 0, bvh_ordered(x)), atomicMin(part + 1, bvh_ordered(y)), atomicMin(part + 2, bvh_ordered(z));
      atomicMax(part + 3, bvh_ordered(x)), atomicMax(part + 4, bvh_ordered(y)), atomicMax(part + 5, bvh_ordered(z));
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(lo + 3 * m + threadIdx.x, part[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(hi + 3 * m + (threadIdx.x - 3), part[threadIdx.x]);
}

__device__ __forceinline__ unsigned bvh_spread(unsigned v) {   // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__device__ __forceinline__ unsigned bvh_cell(float c, float lo, float hi) {
  const float ext = hi - lo;
  const float s = (ext > 0.f && ext < INFINITY) ? 1024.0f / ext : 0.f;
  return (unsigned)fminf(fmaxf((c - lo) * s, 0.f), 1023.f);   // fmaxf drops a NaN
}

__global__ __launch_bounds__(BVH_THREADS) void bvh_keys_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                               const unsigned *__restrict__ lo, const unsigned *__restrict__ hi,
                                                               long long *__restrict__ keys) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  float p[9];
  long long key = (long long)m << 32;
  if (bvh_load_face(verts, faces, fbase + i, vbase, vert_first[m + 1] - vbase, p)) {
    const float third = 0.333333343267440796f;
    const float cx = ((p[0] + p[3]) + p[6]) * third, cy = ((p[1] + p[4]) + p[7]) * third, cz = ((p[2] + p[5]) + p[8]) * third;
    const unsigned qx = bvh_cell(cx, bvh_unordered(lo[3 * m]), bvh_unordered(hi[3 * m]));
    const unsigned qy = bvh_cell(cy, bvh_unordered(lo[3 * m + 1]), bvh_unordered(hi[3 * m + 1]));
    const unsigned qz = bvh_cell(cz, bvh_unordered(lo[3 * m + 2]), bvh_unordered(hi[3 * m + 2]));
    key |= (long long)((bvh_spread(qx) << 2) | (bvh_spread(qy) << 1) | bvh_spread(qz));
  } else {
    key |= BVH_DROPPED;
  }
  keys[fbase + i] = key;
}

// head: [b][4], zeroed; counts: [b][2], zeroed
__global__ __launch_bounds__(BVH_THREADS) void bvh_head_kernel(const long long *__restrict__ keys, const long long *__restrict__ face_first,
                                                               int *__restrict__ head, int *__restrict__ counts) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  if (i >= nf) return;
  const bool used = !(keys[fbase + i] & BVH_DROPPED), next_used = i + 1 < nf && !(keys[fbase + i + 1] & BVH_DROPPED);
  int n = -1;
  if (used && !next_used) n = (int)(i + 1);
  else if (i == 0 && !used) n = 0;
  if (n >= 0) {   // one thread per mesh when the keys are sorted; any of them otherwise
    head[BVH_HEAD_INTS * m] = n, head[BVH_HEAD_INTS * m + 1] = (int)nf - n;
    counts[2 * m] = n, counts[2 * m + 1] = (int)nf - n;
  }
}

// the number of leading bits that (key, position) of slots i and j of the mesh share; -1 outside the mesh
__device__ __forceinline__ int bvh_delta(const long long *__restrict__ mk, int n, int i, long long j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long x = (unsigned long long)(mk[i] ^ mk[j]);
  return x ? __clzll(x) : 64 + __clz((unsigned)(i ^ (int)j));
}

__global__ __launch_bounds__(BVH_THREADS) void bvh_tree_kernel(const long long *__restrict__ keys, const long long *__restrict__ face_first,
                                                               const int *__restrict__ head, BvhNode *__restrict__ nodes,
                                                               int *__restrict__ parent, int *__restrict__ right, int *__restrict__ last,
                                                               int *__restrict__ after) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m];
  const int n = head[BVH_HEAD_INTS * m];
  const long long t = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  if (t >= n - 1) return;
  const int i = (int)t;
  const long long *mk = keys + fbase;
  const int d = bvh_delta(mk, n, i, (long long)i + 1) - bvh_delta(mk, n, i, (long long)i - 1) < 0 ? -1 : 1;   // never equal: the positions differ
  const int dmin = bvh_delta(mk, n, i, (long long)i - d);
  long long lmax = 2;
  for (int step = 0; step < 32 && bvh_delta(mk, n, i, i + lmax * d) > dmin; ++step) lmax *= 2;
  long long l = 0;
  for (long long s = lmax / 2; s >= 1; s /= 2)   // at most 32 halvings
    if (bvh_delta(mk, n, i, i + (l + s) * d) > dmin) l += s;
  const long long j = i + l * d;
  const int dnode = bvh_delta(mk, n, i, j);
  long long s = 0, step = l;
  for (int it = 0; it < 33; ++it) {
    step = (step + 1) >> 1;
    if (bvh_delta(mk, n, i, i + (s + step) * d) > dnode) s += step;
    if (step <= 1) break;
  }
  const int first = (int)(d > 0 ? i : j), end = (int)(d > 0 ? j : i);
  int split = (int)(i + s * d + (d < 0 ? -1 : 0));   // first <= split < end for sorted keys
  split = split < 0 ? 0 : (split > n - 2 ? n - 2 : split);   // unsorted keys give a wrong tree, never an index outside the mesh
  const int lc = split == first ? n - 1 + split : split, rc = split + 1 == end ? n - 1 + split + 1 : split + 1;
  nodes[2 * fbase + i].link = lc;
  right[fbase + i] = rc, last[fbase + i] = end, after[fbase + split] = rc;
  parent[2 * fbase + lc] = i, parent[2 * fbase + rc] = i;
}

__device__ __forceinline__ void bvh_read_box(const BvhNode *node, float (&b)[6]) {
  const volatile float *p = (const volatile float *)node;
#pragma unroll
  for (int k = 0; k < 6; ++k) b[k] = p[k];
}

// parent: [2 sum F] filled with -1 before bvh_tree_kernel; arrive: [sum F] zeroed
__global__ __launch_bounds__(BVH_THREADS) void bvh_fit_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                              const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                              const long long *__restrict__ order, const int *__restrict__ head,
                                                              BvhNode *__restrict__ nodes, const int *__restrict__ parent,
                                                              const int *__restrict__ right, const int *__restrict__ last,
                                                              const int *__restrict__ after, int *__restrict__ arrive) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const int n = head[BVH_HEAD_INTS * m];
  const long long t = (long long)blockIdx.x * BVH_THREADS + threadIdx.x;
  if (t >= n) return;
  const int j = (int)t;
  BvhNode *nb = nodes + 2 * fbase;
  if (j < n - 1) {
    const int e = last[fbase + j];
    nb[j].skip = e < n - 1 ? after[fbase + e] : -1;
  }
  const long long vbase = vert_first[m];
  const long long row = order[fbase + j];
  float p[9];
  BvhNode leaf;
  leaf.lox = leaf.loy = leaf.loz = INFINITY, leaf.hix = leaf.hiy = leaf.hiz = -INFINITY, leaf.link = -1;
  if (row >= fbase && row < fbase + nf && bvh_load_face(verts, faces, row, vbase, vert_first[m + 1] - vbase, p)) {   // a foreign row: an empty leaf
    leaf.lox = fminf(fminf(p[0], p[3]), p[6]), leaf.loy = fminf(fminf(p[1], p[4]), p[7]), leaf.loz = fminf(fminf(p[2], p[5]), p[8]);
    leaf.hix = fmaxf(fmaxf(p[0], p[3]), p[6]), leaf.hiy = fmaxf(fmaxf(p[1], p[4]), p[7]), leaf.hiz = fmaxf(fmaxf(p[2], p[5]), p[8]);
    leaf.link = (int)(row - fbase);
  }
  leaf.skip = j < n - 1 ? after[fbase + j] : -1;
  nb[n - 1 + j] = leaf;
  int cur = n - 1 + j;
  for (int up = 0; up < 64; ++up) {   // the depth is at most 60: 30 Morton bits and 30 position bits (n < 2^30) can differ inside a mesh
    const int p_ = parent[2 * fbase + cur];
    if (p_ < 0 || p_ >= n - 1) break;   // the root
    __threadfence();                    // this thread's box is visible before its arrival is
    if (atomicAdd(arrive + fbase + p_, 1) != 1) break;   // the first to arrive leaves
    __threadfence();                    // the other child's box is visible after its arrival is
    float a[6], b[6];
    bvh_read_box(nb + nb[p_].link, a);
    bvh_read_box(nb + right[fbase + p_], b);
    BvhNode *q = nb + p_;
    q->lox = fminf(a[0], b[0]), q->loy = fminf(a[1], b[1]), q->loz = fminf(a[2], b[2]);
    q->hix = fmaxf(a[3], b[3]), q->hiy = fmaxf(a[4], b[4]), q->hiz = fmaxf(a[5], b[5]);
    cur = p_;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// offsets | the bounds (6 b) | parent (2 sum F) | right, last, after, arrive (sum F each)
struct BuildWs {
  long long *vert_first, *face_first;
  unsigned *lo, *hi;
  int *parent, *right, *last, *after, *arrive;
  size_t bytes;
};
BuildWs build_ws(void *ws, int b, long long sum_f) {
  Carve c{(char *)ws, 0};
  BuildWs w;
  const size_t f = (size_t)(sum_f > 0 ? sum_f : 1);
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.lo = c.take<unsigned>(6 * (size_t)(b > 0 ? b : 1)), w.hi = w.lo + 3 * (size_t)b;
  w.parent = c.take<int>(2 * f);
  w.right = c.take<int>(f), w.last = c.take<int>(f), w.after = c.take<int>(f), w.arrive = c.take<int>(f);
  w.bytes = c.o;
  return w;
}

int build_checks(const char *what, int b, const long long *vert_first, const long long *face_first, const void *verts, const void *faces,
                 const void *workspace, long long *max_v, long long *max_f) {
  if (check_mesh_batch(what, b, vert_first, face_first, true, max_v, max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_first[b] < INT_MAX && 3 * face_first[b] < INT_MAX, "%s: %lld vertices or %lld faces (three corners each) reach 2^31", what,
              vert_first[b], face_first[b]);
  BDM_REQUIRE(verts && faces, "%s: an input is NULL", what);
  return check_workspace(what, workspace);
}

}  // namespace

extern "C" size_t bdm_mesh_bvh_bytes(int b, long long sum_f) {
  if (!bvh_sizes_ok(b, 0, sum_f, 0)) return 0;
  return bvh_layout(nullptr, b, sum_f).bytes;
}

extern "C" size_t bdm_mesh_bvh_workspace_bytes(int b, long long sum_v, long long sum_f) {
  if (!bvh_sizes_ok(b, sum_v, sum_f, 0)) return 0;
  return build_ws(nullptr, b, sum_f).bytes;
}

extern "C" int bdm_mesh_bvh_keys(int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first,
                                 long long *keys, void *workspace, void *stream) {
  const char *what = "mesh_bvh_keys";
  long long max_v = 0, max_f = 0;
  if (build_checks(what, b, vert_first, face_first, verts, faces, workspace, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(keys, "%s: the keys are NULL", what);
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const BuildWs w = build_ws(workspace, b, sum_f);
  const Range in[2] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[2] = {{keys, 8 * (size_t)sum_f}, {workspace, w.bytes}};
  if (check_overlap(what, in, 2, out, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  fill_ints((int *)w.lo, 3 * (long long)b, -1, st);
  fill_ints((int *)w.hi, 3 * (long long)b, 0, st);
  const dim3 block(BVH_THREADS);
  if (max_v > 0)
    hipLaunchKernelGGL(bvh_bounds_kernel, dim3((unsigned)cdivll(max_v, BVH_THREADS), (unsigned)b), block, 0, st, verts, w.vert_first, w.lo, w.hi);
  if (max_f > 0)
    hipLaunchKernelGGL(bvh_keys_kernel, dim3((unsigned)cdivll(max_f, BVH_THREADS), (unsigned)b), block, 0, st, verts, faces, w.vert_first,
                       w.face_first, w.lo, w.hi, keys);
  return launch_status(what);
}

extern "C" int bdm_mesh_bvh_build(int b, const float *verts, const int *faces, const long long *vert_first, const long long *face_first,
                                  const long long *keys, const long long *order, int *counts, void *bvh, void *workspace, void *stream) {
  const char *what = "mesh_bvh_build";
  long long max_v = 0, max_f = 0;
  if (build_checks(what, b, vert_first, face_first, verts, faces, workspace, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(keys && order && counts, "%s: the keys, the order or the counts are NULL", what);
  BDM_REQUIRE(bvh && ((uintptr_t)bvh & 15) == 0, "%s: the hierarchy buffer is NULL or not 16-byte aligned", what);
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const BuildWs w = build_ws(workspace, b, sum_f);
  const BvhLayout l = bvh_layout(bvh, b, sum_f);
  const Range in[4] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {keys, 8 * (size_t)sum_f}, {order, 8 * (size_t)sum_f}};
  const Range out[3] = {{counts, 8 * (size_t)b}, {bvh, l.bytes}, {workspace, w.bytes}};
  if (check_overlap(what, in, 4, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  fill_ints(l.head, (long long)BVH_HEAD_INTS * b, 0, st);
  fill_ints(counts, 2 * (long long)b, 0, st);
  if (max_f > 0) {
    fill_ints(w.parent, 2 * sum_f, -1, st);
    fill_ints(w.arrive, sum_f, 0, st);
    const dim3 grid((unsigned)cdivll(max_f, BVH_THREADS), (unsigned)b), block(BVH_THREADS);
    hipLaunchKernelGGL(bvh_head_kernel, grid, block, 0, st, keys, w.face_first, l.head, counts);
    hipLaunchKernelGGL(bvh_tree_kernel, grid, block, 0, st, keys, w.face_first, l.head, l.nodes, w.parent, w.right, w.last, w.after);
    hipLaunchKernelGGL(bvh_fit_kernel, grid, block, 0, st, verts, faces, w.vert_first, w.face_first, order, l.head, l.nodes, w.parent, w.right,
                       w.last, w.after, w.arrive);
  }
  return launch_status(what);
}
