// face_point.hip -- the squared distance from every face of a mesh to the nearest point of its cloud, as gfx950 kernels (bdm_hip.h
// section 17; the face-to-point half of pytorch3d's point_mesh_face_distance, restated from its published
// behaviour).  The pair rule and the face record are point_face.h's, shared with mesh_metrics.hip: this file only exchanges the loops.
//
// Kernels.
//   (ragged.h)          send_offsets: the three host offset arrays travel as launch arguments into the workspace.
//   fp_record_kernel    one thread per face: the 64-byte record (point_face.h); for the split form also the preset of the face's key.
//   fp_dist_kernel<false>  resident: one thread per face, one workgroup per FP_THREADS faces of one mesh.  The thread keeps its record
//                       (and the nine edge differences, hoisted by the compiler) in registers; the cloud goes through LDS in tiles
//                       of FP_TILE points, one float4 each, and every lane reads the SAME point (a broadcast ds_read_b128: no bank
//                       conflict).  Points are visited in ascending order, so `d < best` alone implements the tie rule.
//   fp_dist_kernel<true>   split: the tiles of a cloud are divided over gridDim.z chunks; a thread that found a finite d sends
//                       (bits of d) << 32 | index through ONE 64-bit integer atomicMin (a vector atomic on global memory) to its
//                       face's key.  d has its sign bit clear, so the keys order like (d, index): the minimum is order-free.
//   fp_finish_kernel    split: one thread per face decodes its key; the untouched preset decodes to (+inf, -1).
#include "../../include/bdm_hip.h"
#include "common.h"
#include "point_face.h"
#include "ragged.h"

#include <limits.h>

#pragma clang fp contract(off)

using namespace bdm;

#define FP_THREADS 256
#define FP_TILE 1024                      // points per LDS tile: 16 KiB
#define FP_MAX_FACES (1 << 24)            // per mesh, as section 14
#define FP_MAX_B 65535                    // gridDim.y
#define FP_MAX_CHUNKS 65535               // gridDim.z
#define FP_CUS 256                        // the chooser's constant: compute units of the MI355X
#define FP_SPLIT_BELOW (8 * FP_CUS)       // resident workgroups under which the chooser splits (measured: DESIGN.md section 21)
#define FP_SPLIT_TARGET (16 * FP_CUS)     // workgroups the split form aims at
#define FP_KEY_NONE 0x7F800000FFFFFFFFull // bits(+inf) << 32 | 0xFFFFFFFF: decodes to (+inf, -1)

namespace {

__global__ __launch_bounds__(FP_THREADS) void fp_record_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const long long *__restrict__ vert_first,
                                                               const long long *__restrict__ face_first, float4 *__restrict__ rec,
                                                               unsigned long long *__restrict__ keys) {
  const int m = blockIdx.y;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const long long i = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  mm_record_store(verts, faces, base + i, vbase, vert_first[m + 1] - vbase, rec + (size_t)(base + i) * 4);
  if (keys) keys[base + i] = FP_KEY_NONE;
}

template <bool SPLIT>
__global__ __launch_bounds__(FP_THREADS) void fp_dist_kernel(const float *__restrict__ points, const float4 *__restrict__ rec,
                                                             const long long *__restrict__ face_first,
                                                             const long long *__restrict__ point_first, float *__restrict__ sqdist,
                                                             int *__restrict__ point_idx, unsigned long long *__restrict__ keys) {
  __shared__ float4 tile[FP_TILE];
  const int m = blockIdx.y;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const long long first = (long long)blockIdx.x * FP_THREADS;
  if (first >= nf) return;   // the whole workgroup: no barrier is left waiting
  const long long i = first + threadIdx.x;
  const bool live = i < nf;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
  if (live) {
    const float4 *r = rec + (size_t)(base + i) * 4;
    r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3];
  }
  const bool valid = r3.x != 0.f;
  const long long pbase = point_first[m], np = point_first[m + 1] - pbase;   // np < 2^31
  const long long tiles = (np + FP_TILE - 1) / FP_TILE;
  const long long t_lo = SPLIT ? ((long long)blockIdx.z * tiles) / gridDim.z : 0;
  const long long t_hi = SPLIT ? ((long long)(blockIdx.z + 1) * tiles) / gridDim.z : tiles;
  float best = INFINITY;
  int idx = -1;
  for (long long t = t_lo; t < t_hi; ++t) {   // uniform over the workgroup
    const long long p0 = t * FP_TILE;
    const int cnt = np - p0 < FP_TILE ? (int)(np - p0) : FP_TILE;
    __syncthreads();   // the previous tile has been read by everybody
    for (int k = threadIdx.x; k < cnt; k += FP_THREADS) {
      const float *q = points + (size_t)(pbase + p0 + k) * 3;
      tile[k] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float4 q = tile[j];
      const float d = mm_pair_sqdist(q.x, q.y, q.z, r0, r1, r2, r3);
      if (d < best) { best = d; idx = (int)p0 + j; }   // ascending point order: the first of equal distances stays; NaN and +inf never enter
    }
  }
  if (!live) return;
  if (!valid) { best = INFINITY; idx = -1; }   // the zero record of an invalid face ran along
  if (SPLIT) {
    if (idx >= 0) atomicMin(keys + (base + i), ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)idx);
  } else {
    sqdist[base + i] = best;
    point_idx[base + i] = idx;
  }
}

__global__ __launch_bounds__(FP_THREADS) void fp_finish_kernel(long long sum_f, const unsigned long long *__restrict__ keys,
                                                               float *__restrict__ sqdist, int *__restrict__ point_idx) {
  const long long g = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
  if (g >= sum_f) return;
  const unsigned long long key = keys[g];
  sqdist[g] = __uint_as_float((unsigned int)(key >> 32));
  point_idx[g] = (int)(unsigned int)key;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct FpWs {
  float4 *rec;                                       // [sum_f][4]
  unsigned long long *keys;                          // [sum_f]
  long long *vert_first, *face_first, *point_first;  // [b + 1] each
  long long *unused;                                 // [b + 1]: the second array of the second upload
  size_t bytes;
};

FpWs fp_ws(void *ws, int b, long long sum_f) {
  FpWs w;
  char *p = (char *)ws;
  size_t off = 0;
  w.rec = (float4 *)p; off += 64 * (size_t)sum_f;
  w.keys = (unsigned long long *)(p + off); off = align16(off + 8 * (size_t)sum_f);
  w.vert_first = (long long *)(p + off);
  w.face_first = w.vert_first + (b + 1); off += offsets_bytes(b);
  w.point_first = (long long *)(p + off);
  w.unused = w.point_first + (b + 1); off += offsets_bytes(b);
  w.bytes = off;
  return w;
}

bool fp_sizes_ok(int b, long long sum_f) { return b >= 0 && b <= FP_MAX_B && sum_f >= 0 && sum_f <= INT_MAX; }

bool fp_chooser_sizes_ok(int b, long long sum_f, long long sum_p, long long max_p, long long workgroups) {
  return fp_sizes_ok(b, sum_f) && sum_p >= 0 && sum_p <= INT_MAX && max_p >= 0 && max_p <= sum_p && workgroups >= 0 &&
         workgroups <= sum_f;
}

// The chooser: chunks of the split form, 1 = the resident form.  Split iff the resident form would keep fewer than 8 workgroups per
// compute unit busy (about what the chip holds at once: 7 by registers) and the largest cloud has more than one tile; then the
// fewest chunks that reach 16 per compute unit, at most one per tile.
int fp_chunks(long long max_p, long long workgroups) {
  const long long tiles = cdivll(max_p, FP_TILE);
  if (workgroups <= 0 || workgroups >= FP_SPLIT_BELOW || tiles <= 1) return 1;
  long long c = cdivll(FP_SPLIT_TARGET, workgroups);
  if (c > tiles) c = tiles;
  if (c > FP_MAX_CHUNKS) c = FP_MAX_CHUNKS;
  return (int)c;
}

}  // namespace

extern "C" size_t bdm_face_point_distance_workspace_bytes(int b, long long sum_f) {
  if (!fp_sizes_ok(b, sum_f)) return 0;
  return fp_ws(nullptr, b, sum_f).bytes;
}

extern "C" int bdm_face_point_distance_variant(int b, long long sum_f, long long sum_p, long long max_p, long long workgroups) {
  if (!fp_chooser_sizes_ok(b, sum_f, sum_p, max_p, workgroups)) return 0;
  return fp_chunks(max_p, workgroups) > 1 ? 2 : 1;
}

extern "C" int bdm_face_point_distance_chunks(int b, long long sum_f, long long sum_p, long long max_p, long long workgroups) {
  if (!fp_chooser_sizes_ok(b, sum_f, sum_p, max_p, workgroups)) return 0;
  return fp_chunks(max_p, workgroups);
}

extern "C" int bdm_face_point_distance(int b, int form, int chunks, const float *verts, const int *faces, const long long *vert_first,
                                       const long long *face_first, const float *points, const long long *point_first, float *sqdist,
                                       int *point_idx, void *workspace, void *stream) {
  const char *what = "face_point_distance";
  BDM_REQUIRE(b >= 0 && b <= FP_MAX_B, "%s: batch size %d outside 0 .. %d", what, b, FP_MAX_B);
  BDM_REQUIRE(form >= 0 && form <= 2, "%s: form %d is none of 0 (chooser), 1 (resident), 2 (split)", what, form);
  BDM_REQUIRE(chunks >= 0 && chunks <= FP_MAX_CHUNKS, "%s: %d chunks outside 0 .. %d", what, chunks, FP_MAX_CHUNKS);
  BDM_REQUIRE(form == 2 || chunks <= (form == 1 ? 1 : 0), "%s: only the split form (2) takes a chunk count", what);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_first && face_first && point_first, "%s: an offset array is NULL", what);
  long long max_v = 0, max_f = 0, max_p = 0;
  if (check_first(what, "mesh", b, vert_first, &max_v) != BDM_OK || check_first(what, "mesh", b, face_first, &max_f) != BDM_OK ||
      check_first(what, "cloud", b, point_first, &max_p) != BDM_OK)
    return BDM_ERR_ARG;
  BDM_REQUIRE(max_f <= FP_MAX_FACES, "%s: a mesh has %lld faces, more than %d", what, max_f, FP_MAX_FACES);
  const long long sum_v = vert_first[b], sum_f = face_first[b], sum_p = point_first[b];
  BDM_REQUIRE(sum_v <= INT_MAX && sum_f <= INT_MAX && sum_p <= INT_MAX, "%s: %lld vertices, %lld faces or %lld points reach 2^31", what,
              sum_v, sum_f, sum_p);
  if (sum_f == 0) return BDM_OK;
  BDM_REQUIRE(verts && faces && points && sqdist && point_idx && workspace, "%s: an input, an output or the workspace is NULL", what);
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace is not 16-byte aligned", what);
  const FpWs ws = fp_ws(workspace, b, sum_f);
  const Range in[3] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {points, 12 * (size_t)sum_p}};
  const Range out[3] = {{sqdist, 4 * (size_t)sum_f}, {point_idx, 4 * (size_t)sum_f}, {workspace, ws.bytes}};
  if (check_overlap(what, in, 3, out, 3) != BDM_OK) return BDM_ERR_ARG;
  if (form != 2) {
    long long workgroups = 0;
    for (int m = 0; m < b; ++m) workgroups += cdivll(face_first[m + 1] - face_first[m], FP_THREADS);
    chunks = form == 1 ? 1 : fp_chunks(max_p, workgroups);
    form = chunks > 1 ? 2 : 1;
  } else if (chunks == 0) {   // the split form asked for by name: two chunks unless the chooser wants more
    long long workgroups = 0;
    for (int m = 0; m < b; ++m) workgroups += cdivll(face_first[m + 1] - face_first[m], FP_THREADS);
    chunks = fp_chunks(max_p, workgroups);
    if (chunks < 2) chunks = 2;
  }
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, ws.vert_first, ws.face_first, st);
  send_offsets(b, point_first, nullptr, ws.point_first, ws.unused, st);
  const dim3 grid((unsigned)cdivll(max_f, FP_THREADS), (unsigned)b);
  hipLaunchKernelGGL(fp_record_kernel, grid, dim3(FP_THREADS), 0, st, verts, faces, ws.vert_first, ws.face_first, ws.rec,
                     form == 2 ? ws.keys : (unsigned long long *)nullptr);
  if (form == 2) {
    hipLaunchKernelGGL(fp_dist_kernel<true>, dim3(grid.x, grid.y, (unsigned)chunks), dim3(FP_THREADS), 0, st, points, ws.rec,
                       ws.face_first, ws.point_first, sqdist, point_idx, ws.keys);
    hipLaunchKernelGGL(fp_finish_kernel, dim3((unsigned)cdivll(sum_f, FP_THREADS)), dim3(FP_THREADS), 0, st, sum_f, ws.keys, sqdist,
                       point_idx);
  } else {
    hipLaunchKernelGGL(fp_dist_kernel<false>, grid, dim3(FP_THREADS), 0, st, points, ws.rec, ws.face_first, ws.point_first, sqdist,
                       point_idx, (unsigned long long *)nullptr);
  }
  return launch_status(what);
}
