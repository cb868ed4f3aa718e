// ragged.h -- what the operators on packed, ragged batches share on the host side (mesh_metrics.hip, knn.hip, face_point.hip,
// align.hip, and through mesh_incidence.h mesh_render.hip, mesh_clean.hip, mesh_fill.hip, mesh_decimate.hip, mesh_voxel.hip and
// mesh_qem.hip): the checks on
// the host "first row" offset arrays, their upload, the overlap checks of the pointer arguments, the workspace paddings and the
// carver that lays a workspace out, and the workgroup scan of mesh_metrics.hip and mesh_incidence.h.  The limits on batch sizes and
// sums differ per operator and stay at the call sites.
#pragma once
#include "common.h"

namespace bdm {

// `first` (b + 1 host entries, b >= 1) starts at 0 and never decreases -> 0 with max_count = the largest per-entry count, or 1 with
// the error set.  noun ("mesh", "entry") names an entry in the message.
int check_first(const char *what, const char *noun, int b, const long long *first, long long *max_count);

// The two host offset arrays (b + 1 entries each) into dev_a and dev_b on stream s.  The values travel inside the launch arguments,
// 32 per launch: no host-to-device copy and no synchronisation, so the caller may free its arrays as soon as this returns, and the
// call is safe under stream capture.  first_b == NULL sends zeros.
void send_offsets(int b, const long long *first_a, const long long *first_b, long long *dev_a, long long *dev_b, hipStream_t s);

struct Range {
  const void *p;
  size_t bytes;
};
// a NULL or empty range overlaps nothing
static inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const char *pa = (const char *)a, *pb = (const char *)b;
  return pa < pb + nb && pb < pa + na;
}
// no output overlaps an input or another output -> 0, or 1 with the error set
int check_overlap(const char *what, const Range *in, int n_in, const Range *out, int n_out);

static inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
// the two offset arrays of a batch of b, side by side, padded to 16 bytes
static inline size_t offsets_bytes(int b) { return align16(2 * sizeof(long long) * (size_t)(b + 1)); }
// Hands out the pieces of a workspace one after the other, each padded to 16 bytes; o is the size so far.  p may be NULL when only
// the size is wanted (the pointers are then not to be used).
struct Carve {
  char *p;
  size_t o;
  template <class T>
  T *take(size_t count) {
    T *piece = (T *)(p + o);
    o += align16(sizeof(T) * count);
    return piece;
  }
  // the two offset arrays of a batch of b (offsets_bytes): the second one starts b + 1 entries after the first
  long long *take_offsets(int b) { return take<long long>(2 * (size_t)(b + 1)); }
};

#if defined(__HIPCC__)
// inclusive scan of one value per thread over a workgroup of THREADS (Hillis-Steele in LDS) -> this thread's prefix; buf: THREADS
// entries.  Every thread of the workgroup calls it.
template <typename T, int THREADS>
__device__ __forceinline__ T block_scan(T v, T *buf) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const T add = t >= off ? buf[t - off] : (T)0;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  const T r = buf[t];
  __syncthreads();   // buf is free again
  return r;
}
#endif

}  // namespace bdm
