// mesh_emit.h -- the tail that the operators which write new meshes share (mesh_fill.hip, mesh_decimate.hip, mesh_qem.hip; DESIGN.md
// section 17.2): the checks their output entry points open with, the per-mesh largest finite magnitude, the segments that gather the
// old vertices a new vertex stands for, and the order-free fixed-point mean over such a set (bdm_hip.h section 19 rule 5).  A value v
// of a set whose largest finite magnitude has the bits amax_bits is quantised to rint(v 2^e) as a 64-bit integer, the integers are
// summed in any order, and the mean is one float64 division rounded once to float32.  How a set is walked, which vertex represents
// it and the limits on the sums stay with the operator.
//
// Kernels (internal linkage: every .hip that includes this header gets its own instances).
//   amax_clear_kernel     dst[stride m] = 0 for every mesh m.
//   attr_amax_kernel      dst[stride m] = the bits of the largest finite |attribute| of mesh m (one integer atomic max per workgroup).
#pragma once
#include "mesh_incidence.h"
#include "align_solve.h"   // align_pow2

#include <math.h>

namespace bdm {

constexpr int MESH_MAX_C = 16;   // attribute channels (bdm_hip.h sections 19, 20 and 23)

namespace {

// ---- host checks ----------------------------------------------------------------------------------------------------------------------
// nv -> ov vertices and nf -> of faces can be what a decimator leaves of a mesh
inline bool decimated_sizes_ok(long long nv, long long ov, long long nf, long long of) {
  return ov <= nv && (nv == 0 || ov >= 1) && of <= nf && (of == 0 || ov >= 3);
}

// What an output entry point checks before it touches the workspace, violations reported in this order: the channel bound, the
// operator's own checks on the input batch (batch() -> BDM_OK or the error set), the host offsets of the outputs, every mesh's sizes
// under sizes_ok(nv, ov, nf, of) ("... cannot be a <kind> mesh"), and pointers, whether every array argument is non-NULL.
template <class Batch, class Sizes>
int check_emit(const char *what, const char *kind, int b, int c, const long long *vert_first, const long long *face_first,
               const long long *out_vert_first, const long long *out_face_first, bool pointers, Batch batch, Sizes sizes_ok) {
  BDM_REQUIRE(c >= 0 && c <= MESH_MAX_C, "%s: %d attribute channels outside 0 .. %d", what, c, MESH_MAX_C);
  if (batch() != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(out_vert_first && out_face_first, "%s: an output offset array is NULL", what);
  long long largest = 0;
  if (check_first(what, "mesh", b, out_vert_first, &largest) != BDM_OK) return BDM_ERR_ARG;
  if (check_first(what, "mesh", b, out_face_first, &largest) != BDM_OK) return BDM_ERR_ARG;
  for (int m = 0; m < b; ++m) {
    const long long nv = vert_first[m + 1] - vert_first[m], nf = face_first[m + 1] - face_first[m];
    const long long ov = out_vert_first[m + 1] - out_vert_first[m], of = out_face_first[m + 1] - out_face_first[m];
    BDM_REQUIRE(sizes_ok(nv, ov, nf, of), "%s: mesh %d: %lld -> %lld vertices and %lld -> %lld faces cannot be a %s mesh", what, m, nv, ov, nf,
                of, kind);
  }
  BDM_REQUIRE(pointers, "%s: an input or an output is NULL", what);
  return BDM_OK;
}

#if defined(__HIPCC__)
// ---- the largest finite magnitude ---------------------------------------------------------------------------------------------------
// top raised to the bits of the largest finite |value| of a row of n floats (bits of non-negative floats order as integers)
__device__ __forceinline__ unsigned amax_fold(const float *__restrict__ row, int n, unsigned top) {
  for (int d = 0; d < n; ++d) {
    const float a = fabsf(row[d]);
    if (a < INFINITY) top = max(top, __float_as_uint(a));
  }
  return top;
}

// LANES words per thread folded over the workgroup in one LDS tree, lanes below MINS by minimum and the others by maximum, then
// one integer atomic per lane into dst[lane].  Every thread of the workgroup calls it.
template <int LANES, int MINS>
__device__ __forceinline__ void block_fold_atomic(const unsigned (&v)[LANES], unsigned *__restrict__ dst) {
  __shared__ unsigned buf[LANES][MESH_THREADS];
  const int t = threadIdx.x;
#pragma unroll
  for (int l = 0; l < LANES; ++l) buf[l][t] = v[l];
  __syncthreads();
  for (int off = MESH_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int l = 0; l < LANES; ++l) buf[l][t] = l < MINS ? min(buf[l][t], buf[l][t + off]) : max(buf[l][t], buf[l][t + off]);
    }
    __syncthreads();
  }
  if (t < MINS) atomicMin(dst + t, buf[t][0]);
  else if (t < LANES) atomicMax(dst + t, buf[t][0]);
}

__global__ __launch_bounds__(MESH_THREADS) void amax_clear_kernel(int b, int stride, unsigned *__restrict__ dst) {
  const int m = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (m < b) dst[(size_t)stride * m] = 0u;
}

__global__ __launch_bounds__(MESH_THREADS) void attr_amax_kernel(int c, const float *__restrict__ attrs, const long long *__restrict__ vert_first,
                                                                 int stride, unsigned *__restrict__ dst) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * MESH_THREADS >= nv) return;   // the whole workgroup
  const unsigned top[1] = {i < nv ? amax_fold(attrs + (size_t)c * (size_t)(vbase + i), c, 0) : 0};
  block_fold_atomic<1, 0>(top, dst + (size_t)stride * m);
}

// ---- member segments ------------------------------------------------------------------------------------------------------------------
// Vertex i of the mesh at vbase is represented by vertex r of the same mesh (itself when it survives): r noted, the representative
// flagged for the rank scan, its segment's size counted at it (seg zeroed before).
__device__ __forceinline__ void member_flag(long long vbase, long long i, int r, int *__restrict__ rep, int *__restrict__ rank,
                                            int *__restrict__ seg) {
  rep[vbase + i] = r;
  rank[vbase + i] = r == i ? 1 : 0;
  atomicAdd(seg + vbase + r, 1);
}

// rank and seg are scanned: vertex i goes into its representative's segment member[seg[g] .. seg[g + 1]) (claimed on a cursor, so in
// arrival order) and vert_map gets the representative's rank within the mesh -> g, the representative's packed index
__device__ __forceinline__ long long member_place(long long vbase, long long i, const int *__restrict__ rep, const int *__restrict__ rank,
                                                  const int *__restrict__ seg, int *__restrict__ cursor, int *__restrict__ member,
                                                  int *__restrict__ vert_map) {
  const long long g = vbase + rep[vbase + i];
  member[seg[g] + atomicAdd(cursor + g, 1)] = (int)i;
  vert_map[vbase + i] = rank[g] - rank[vbase];
  return g;
}

// The host sequence around them: seg and cursor zeroed, flag() launches the kernel that calls member_flag for every vertex, the two
// scans, place() launches the one that calls member_place.  rank (sum V + 1 entries, the last one 0) is the caller's to prepare.
template <class Flag, class Place>
void build_member_segments(long long sum_v, int *rank, int *seg, int *cursor, int *bsum, hipStream_t s, Flag flag, Place place) {
  fill_ints(seg, sum_v + 1, 0, s);
  fill_ints(cursor, sum_v, 0, s);
  flag();
  exclusive_scan_ints(rank, sum_v + 1, nullptr, bsum, s);
  exclusive_scan_ints(seg, sum_v + 1, nullptr, bsum, s);
  place();
}

// ---- the fixed-point mean -------------------------------------------------------------------------------------------------------------
// the exponent e of the fixed point: every finite |value| <= amax quantises to rint(value 2^e) below 2^40 in magnitude
__device__ __forceinline__ int mean_scale_exp(unsigned amax_bits) {
  const int field = (int)((amax_bits >> 23) & 0xffu);
  return 39 - ((field < 1 ? 1 : field) - 127);   // amax < 2^(E + 1), E = its exponent (zero and denormals: -126)
}

// S 2^-e / n in float64, rounded once to float32
__device__ __forceinline__ float mean_of_sum(long long s, double inv, double n) { return (float)(((double)s * inv) / n); }

// The mean of rows of up to N channels under the fixed point of amax_bits.  CHECKED: a non-finite value is left out of its channel's
// sum and turns the channel's mean into NaN (attributes); unchecked rows hold finite values only (the positions of merged vertices).
template <int N, bool CHECKED>
struct FixedMean {
  long long sum[N];
  bool bad[N];
  double q, inv;   // 2^e, 2^-e

  __device__ __forceinline__ explicit FixedMean(unsigned amax_bits) {
    const int e = mean_scale_exp(amax_bits);
    q = align_pow2(e), inv = align_pow2(-e);
#pragma unroll
    for (int d = 0; d < N; ++d) sum[d] = 0, bad[d] = false;
  }
  // one member's row of n <= N values
  __device__ __forceinline__ void add(const float *__restrict__ row, int n) {
#pragma unroll
    for (int d = 0; d < N; ++d) {
      if (d >= n) break;
      const float v = row[d];
      if (!CHECKED || fabsf(v) < INFINITY) sum[d] += (long long)rint((double)v * q);
      else bad[d] = true;
    }
  }
  // the means over `count` members
  __device__ __forceinline__ void write(float *__restrict__ out, int n, double count) const {
#pragma unroll
    for (int d = 0; d < N; ++d) {
      if (d >= n) break;
      out[d] = CHECKED && bad[d] ? NAN : mean_of_sum(sum[d], inv, count);
    }
  }
};
#endif

}  // namespace

}  // namespace bdm
