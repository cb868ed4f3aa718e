// mesh_incidence.h -- what the operators on the vertex incidence of packed triangle meshes share (mesh_clean.hip, mesh_fill.hip;
// DESIGN.md section 17.1): the checks every entry point starts with, an int fill, the exclusive int scan, the connected-face rule,
// the two passes that give every packed vertex a segment of two records per face around it, and the per-thread sort of a segment.
// Integer code only.  What a record is (Rec, below) and the limits on the sums stay with the operator.  The other mesh operators
// take MESH_THREADS, the checks, fill_ints and connected_face from here (mesh_render.hip: the first and the last only).
//
// The library is built one translation unit at a time without relocatable device code, so the kernels have internal linkage: every
// .hip that includes this header gets its own instances.
//   fill_ints_kernel        an int array set to one value.
//   scan_kernel<false>      one workgroup per MESH_CHUNK entries: their sum.  scan_top_kernel: one workgroup, the exclusive scan of
//   scan_kernel<true>       those sums in place.  Then every workgroup scans its entries again, plus its offset.
//   incidence_kernel<false, Rec>  one thread per face: a connected face adds 2 to the counter of each of its vertices.
//   incidence_kernel<true, Rec>   the same walk: claims two slots per vertex (atomicAdd on a cursor) and writes the corner's two records.
#pragma once
#include "ragged.h"

#include <stdint.h>

namespace bdm {

constexpr int MESH_THREADS = 256;
constexpr int MESH_CHUNK = 4 * MESH_THREADS;   // entries per workgroup of the scan
constexpr int MESH_MAX_B = 65535;              // gridDim.y
constexpr int MESH_INSERTION_MAX = 32;         // longer segments are heap-sorted

namespace {

// ---- host checks ----------------------------------------------------------------------------------------------------------------------
// The limit on b and, for b >= 1, the host offset arrays -> BDM_OK with the largest per-mesh counts, or BDM_ERR_ARG with the error
// set.  face_first may be NULL when the call uses no faces (max_f = 0 then).  The operator's limits on the sums come next, then
// check_workspace: violations are reported in that order.
int check_mesh_batch(const char *what, int b, const long long *vert_first, const long long *face_first, bool needs_faces, long long *max_v,
                     long long *max_f) {
  BDM_REQUIRE(b >= 0 && b <= MESH_MAX_B, "%s: batch size %d outside 0 .. %d", what, b, MESH_MAX_B);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_first && (face_first || !needs_faces), "%s: an offset array is NULL", what);
  *max_f = 0;
  if (check_first(what, "mesh", b, vert_first, max_v) != BDM_OK) return BDM_ERR_ARG;
  if (face_first && check_first(what, "mesh", b, face_first, max_f) != BDM_OK) return BDM_ERR_ARG;
  return BDM_OK;
}

int check_workspace(const char *what, const void *workspace) {
  BDM_REQUIRE(workspace, "%s: the workspace is NULL", what);
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace is not 16-byte aligned", what);
  return BDM_OK;
}

long long scan_blocks(long long n) { return cdivll(n, MESH_CHUNK); }

#if defined(__HIPCC__)
__global__ __launch_bounds__(MESH_THREADS) void fill_ints_kernel(int *__restrict__ a, long long n, int value) {
  const long long i = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i < n) a[i] = value;
}

void fill_ints(int *a, long long n, int value, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(fill_ints_kernel, dim3((unsigned)cdivll(n, MESH_THREADS)), dim3(MESH_THREADS), 0, s, a, n, value);
}

// ---- exclusive scan of n int32 entries in place; n = n_host, or *n_dev + 1 when n_dev is given (n_host then bounds the grid) --------
template <bool WRITE>
__global__ __launch_bounds__(MESH_THREADS) void scan_kernel(int *__restrict__ a, long long n_host, const int *__restrict__ n_dev,
                                                            int *__restrict__ bsum) {
  __shared__ int buf[MESH_THREADS];
  const long long n = n_dev ? (long long)*n_dev + 1 : n_host;
  const long long base = (long long)blockIdx.x * MESH_CHUNK + 4 * (long long)threadIdx.x;
  if ((long long)blockIdx.x * MESH_CHUNK >= n) return;   // the whole workgroup leaves: no barrier is left waiting (never with a host count)
  int v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = base + e < n ? a[base + e] : 0;
  const int s = (v[0] + v[1]) + (v[2] + v[3]);
  const int incl = block_scan<int, MESH_THREADS>(s, buf);
  if (WRITE) {
    int run = bsum[blockIdx.x] + incl - s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (base + e < n) a[base + e] = run;
      run += v[e];
    }
  } else if (threadIdx.x == MESH_THREADS - 1) {
    bsum[blockIdx.x] = incl;
  }
}

__global__ __launch_bounds__(MESH_THREADS) void scan_top_kernel(int *__restrict__ bsum, long long n_host, const int *__restrict__ n_dev) {
  __shared__ int buf[MESH_THREADS];
  const long long n = n_dev ? (long long)*n_dev + 1 : n_host;
  const int nb = (int)((n + MESH_CHUNK - 1) / MESH_CHUNK);
  int carry = 0;
  for (int c0 = 0; c0 < nb; c0 += MESH_THREADS) {   // uniform trip count
    const int i = c0 + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    const int incl = block_scan<int, MESH_THREADS>(v, buf);
    if (i < nb) bsum[i] = carry + incl - v;
    buf[threadIdx.x] = incl;
    __syncthreads();
    carry += buf[MESH_THREADS - 1];
    __syncthreads();
  }
}

// exclusive scan in place of a[0 .. n), n = n_host (>= 1), or *n_dev + 1 <= n_host; bsum: scan_blocks(n_host) ints
void exclusive_scan_ints(int *a, long long n_host, const int *n_dev, int *bsum, hipStream_t s) {
  const unsigned nb = (unsigned)scan_blocks(n_host);
  hipLaunchKernelGGL(scan_kernel<false>, dim3(nb), dim3(MESH_THREADS), 0, s, a, n_host, n_dev, bsum);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(MESH_THREADS), 0, s, bsum, n_host, n_dev);
  hipLaunchKernelGGL(scan_kernel<true>, dim3(nb), dim3(MESH_THREADS), 0, s, a, n_host, n_dev, bsum);
}

// ---- incidence ------------------------------------------------------------------------------------------------------------------------
// the three indices of face `row` if it is a connected face of a mesh of nv vertices: all in range and pairwise different
__device__ __forceinline__ bool connected_face(const int *__restrict__ faces, long long row, long long nv, int (&idx)[3]) {
  const int *fp = faces + (size_t)row * 3;
  idx[0] = fp[0], idx[1] = fp[1], idx[2] = fp[2];
  if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0 || idx[0] >= nv || idx[1] >= nv || idx[2] >= nv) return false;
  return idx[0] != idx[1] && idx[1] != idx[2] && idx[0] != idx[2];
}

// Rec: `type`, and `corner(idx, i, c, r0, r1)`, the two records of corner c of connected face i (indices idx) of its mesh.
// WRITE = false: first[g] += 2 per connected face around packed vertex g.  WRITE = true: first is the scanned array; two slots of g's
// segment are claimed on cursor[g] and take the corner's records.
template <bool WRITE, class Rec>
__global__ __launch_bounds__(MESH_THREADS) void incidence_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                 const long long *__restrict__ face_first, int *__restrict__ first,
                                                                 int *__restrict__ cursor, typename Rec::type *__restrict__ rec) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  int idx[3];
  if (!connected_face(faces, fbase + i, vert_first[m + 1] - vbase, idx)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long g = vbase + idx[c];
    if (WRITE) {
      const int slot = first[g] + atomicAdd(cursor + g, 2);   // < first[g + 1]: the count pass added 2 for this face
      Rec::corner(idx, (int)i, c, rec[slot], rec[slot + 1]);
    } else {
      atomicAdd(first + g, 2);
    }
  }
}

// first and cursor (sum V + 1 ints each) zeroed, the faces counted, first scanned, the records written: packed vertex g then owns
// rec[first[g] .. first[g + 1]), in no order.  bsum: scan_blocks(sum V + 1) ints.
template <class Rec>
void build_incidence(int b, long long sum_v, long long max_f, const int *faces, const long long *vert_first, const long long *face_first,
                     int *first, int *cursor, int *bsum, typename Rec::type *rec, hipStream_t s) {
  const dim3 grid((unsigned)cdivll(max_f, MESH_THREADS), (unsigned)b), block(MESH_THREADS);
  fill_ints(first, sum_v + 1, 0, s);
  fill_ints(cursor, sum_v + 1, 0, s);
  if (max_f > 0) hipLaunchKernelGGL((incidence_kernel<false, Rec>), grid, block, 0, s, faces, vert_first, face_first, first, cursor, rec);
  exclusive_scan_ints(first, sum_v + 1, nullptr, bsum, s);
  if (max_f > 0) hipLaunchKernelGGL((incidence_kernel<true, Rec>), grid, block, 0, s, faces, vert_first, face_first, first, cursor, rec);
}

// ---- one thread sorts one segment -----------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void sift_down(T *__restrict__ a, int root, int end) {   // max-heap on a[0 .. end)
  const T v = a[root];
  for (;;) {   // at most log2(end) steps: the child index doubles
    int child = 2 * root + 1;
    if (child >= end) break;
    if (child + 1 < end && a[child + 1] > a[child]) ++child;
    if (a[child] <= v) break;
    a[root] = a[child];
    root = child;
  }
  a[root] = v;
}

// a[0 .. len) ascending in place: insertion sort, heap sort above MESH_INSERTION_MAX entries
template <class T>
__device__ __forceinline__ void sort_segment(T *__restrict__ a, int len) {
  if (len <= MESH_INSERTION_MAX) {
    for (int i = 1; i < len; ++i) {
      const T v = a[i];
      int j = i;
      for (; j > 0 && a[j - 1] > v; --j) a[j] = a[j - 1];
      a[j] = v;
    }
  } else {
    for (int root = len / 2 - 1; root >= 0; --root) sift_down(a, root, len);
    for (int end = len - 1; end > 0; --end) {
      const T top = a[0];
      a[0] = a[end];
      a[end] = top;
      sift_down(a, 0, end);
    }
  }
}
#endif

}  // namespace

}  // namespace bdm
