// mesh_metrics.hip -- scoring triangle meshes: area-weighted surface samples and the squared distance from points to the nearest
// face, as gfx950 kernels (bdm_hip.h section 14; restates pytorch3d's sample_points_from_meshes and the
// point-to-face half of point_mesh_face_distance; pytorch3d is not installed, so the rule is this project's own text).
//
// The rule in one paragraph: everything a face contributes (edges, normal n, nn = n . n, squared edge lengths) is float32, rounded
// operation by operation.  The sampler turns the doubled areas sqrt(nn) into integers q_i = rint(a_i / amax * 2^30), scans them in
// int64 and picks the face of a sample by the high half of (64 random bits) x (total); the distance is the minimum over the faces
// of min(three segment distances, plane distance if the point projects inside), the lowest face index winning ties.  Nothing
// depends on execution order: the sums are integers, the only atomic is an integer maximum.
//
// Kernels.
//   (ragged.h)          send_offsets: the two host offset arrays travel as launch arguments into the workspace.
//   mm_area_kernel      one thread per face: a = sqrt(nn) (0 = invalid) into the workspace, atomicMax of its bits per mesh.
//   mm_count_write_kernel<false>  one workgroup per MM_THREADS faces: the sum of their q.
//   mm_scan_kernel      one workgroup per mesh: exclusive scan of the workgroup sums in place, the total.
//   mm_count_write_kernel<true>   one workgroup per MM_THREADS faces: q again, scanned inside the workgroup, plus its offset -> C.
//   mm_sample_kernel    one thread per sample: Philox words, binary search in C, barycentric point and the face's unit normal.
//   mm_record_kernel    one thread per face: the 64-byte record (v0, v1, v2, n, nn, l2_0 .. l2_2), nn = 0 for an invalid face.
//                       The record, the face load and the pair rule itself (mm_pair_sqdist) live in point_face.h, which
//                       face_point.hip shares: one definition for both directions of the distance.
//   mm_dist_kernel      one thread per point, one workgroup per MM_THREADS points: the records of MM_TILE faces at a time go through
//                       LDS, component-major (four float4 planes), and every lane reads the SAME record (a broadcast read: no bank
//                       conflict, one ds_read_b128 per 16 bytes for the whole wave); the running (sqdist, face) stays in registers.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "point_face.h"
#include "ragged.h"

#include <limits.h>

#pragma clang fp contract(off)

using namespace bdm;

#define MM_THREADS 256
#define MM_TILE 256                       // faces per LDS tile of mm_dist_kernel: 16 KiB
#define MM_MAX_FACES (1 << 24)            // per mesh: C_last <= 2^54
#define MM_MAX_B 65535                    // gridDim.y
#define MM_Q_ONE 1073741824.f             // 2^30

namespace {

// ---- sampler ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_THREADS) void mm_area_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                             const long long *__restrict__ vert_first,
                                                             const long long *__restrict__ face_first, float *__restrict__ area,
                                                             unsigned int *__restrict__ amax_bits) {
  const int m = blockIdx.y;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x;
  if (i >= nf) return;
  MmFace f;
  const long long vbase = vert_first[m];
  const float a = mm_face_load(verts, faces, base + i, vbase, vert_first[m + 1] - vbase, f) ? sqrtf(f.nn) : 0.f;
  area[base + i] = a;
  if (a > 0.f) atomicMax(amax_bits + m, __float_as_uint(a));   // non-negative floats order like their bit patterns
}

__device__ __forceinline__ long long mm_weight(float a, float amax) {
  return a > 0.f ? (long long)rintf((a / amax) * MM_Q_ONE) : 0ll;   // a > 0 implies amax >= a > 0
}

template <bool WRITE>
__global__ __launch_bounds__(MM_THREADS) void mm_count_write_kernel(int nb_max, const long long *__restrict__ face_first,
                                                                    const float *__restrict__ area,
                                                                    const unsigned int *__restrict__ amax_bits,
                                                                    long long *__restrict__ bsum, long long *__restrict__ cum) {
  __shared__ long long buf[MM_THREADS];
  const int m = blockIdx.y;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const long long first = (long long)blockIdx.x * MM_THREADS;
  if (first >= nf) return;   // the whole workgroup: no barrier is left waiting
  const long long i = first + threadIdx.x;
  const float amax = __uint_as_float(amax_bits[m]);
  const long long q = i < nf ? mm_weight(area[base + i], amax) : 0ll;
  const long long incl = block_scan<long long, MM_THREADS>(q, buf);
  if (WRITE) {
    if (i < nf) cum[base + i] = bsum[(size_t)m * nb_max + blockIdx.x] + incl;
  } else if (threadIdx.x == MM_THREADS - 1) {
    bsum[(size_t)m * nb_max + blockIdx.x] = incl;
  }
}

// one workgroup per mesh: bsum[m][0 .. nb) -> its exclusive scan, in place; total[m] = the sum (C_last)
__global__ __launch_bounds__(MM_THREADS) void mm_scan_kernel(int nb_max, const long long *__restrict__ face_first,
                                                             long long *__restrict__ bsum, long long *__restrict__ total) {
  __shared__ long long buf[MM_THREADS];
  const int m = blockIdx.x;
  const long long nf = face_first[m + 1] - face_first[m];
  const int nb = (int)((nf + MM_THREADS - 1) / MM_THREADS);   // <= nb_max
  long long *a = bsum + (size_t)m * nb_max;
  long long carry = 0;
  for (int c0 = 0; c0 < nb; c0 += MM_THREADS) {   // uniform trip count
    const int i = c0 + threadIdx.x;
    const long long v = i < nb ? a[i] : 0ll;
    const long long incl = block_scan<long long, MM_THREADS>(v, buf);
    if (i < nb) a[i] = carry + incl - v;
    buf[threadIdx.x] = incl;
    __syncthreads();
    carry += buf[MM_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[m] = carry;
}

struct U4 { uint32_t v[4]; };

// Philox4x32-10 as rng_ops.hip states it (Salmon et al., SC'11)
__device__ __forceinline__ U4 mm_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  U4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

__global__ __launch_bounds__(MM_THREADS) void mm_sample_kernel(int s, const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const long long *__restrict__ vert_first,
                                                               const long long *__restrict__ face_first,
                                                               const long long *__restrict__ cum, const long long *__restrict__ total,
                                                               const unsigned long long *__restrict__ keys, uint32_t draw,
                                                               uint32_t purpose, float *__restrict__ points,
                                                               int *__restrict__ face_idx, float *__restrict__ normals) {
  const int m = blockIdx.y;
  const long long j = (long long)blockIdx.x * MM_THREADS + threadIdx.x;   // 64-bit: the last workgroup may reach past 2^31 - 1
  if (j >= s) return;
  const size_t o = (size_t)m * s + j;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const unsigned long long c_last = (unsigned long long)total[m];
  float px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
  int face = -1;
  if (c_last != 0) {
    const unsigned long long key = keys[m];
    const U4 w = mm_philox((uint32_t)j, 0u, draw, purpose, (uint32_t)key, (uint32_t)(key >> 32));
    const long long t = (long long)__umul64hi(((unsigned long long)w.v[0] << 32) | w.v[1], c_last);   // < c_last <= 2^54
    const long long *c = cum + base;
    long long lo = 0, hi = nf - 1;   // invariant: the answer lies in [lo, hi]; c[nf - 1] = c_last > t
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (c[mid] > t) hi = mid; else lo = mid + 1;
    }
    face = (int)lo;
    MmFace f;
    const long long vbase = vert_first[m];
    mm_face_load(verts, faces, base + lo, vbase, vert_first[m + 1] - vbase, f);   // q > 0: the face is valid
    const float u1 = (float)(w.v[2] >> 8) * 5.9604644775390625e-08f, u2 = (float)(w.v[3] >> 8) * 5.9604644775390625e-08f;
    const float su = sqrtf(u1);
    const float b0 = 1.f - su, b1 = su * (1.f - u2), b2 = su * u2;
    px = (b0 * f.v0x + b1 * f.v1x) + b2 * f.v2x;
    py = (b0 * f.v0y + b1 * f.v1y) + b2 * f.v2y;
    pz = (b0 * f.v0z + b1 * f.v1z) + b2 * f.v2z;
    const float a = sqrtf(f.nn);
    nx = f.nx / a; ny = f.ny / a; nz = f.nz / a;
  }
  points[o * 3] = px; points[o * 3 + 1] = py; points[o * 3 + 2] = pz;
  if (face_idx) face_idx[o] = face;
  if (normals) { normals[o * 3] = nx; normals[o * 3 + 1] = ny; normals[o * 3 + 2] = nz; }
}

// ---- distance ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_THREADS) void mm_record_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const long long *__restrict__ vert_first,
                                                               const long long *__restrict__ face_first, float4 *__restrict__ rec) {
  const int m = blockIdx.y;
  const long long base = face_first[m], nf = face_first[m + 1] - base;
  const long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  mm_record_store(verts, faces, base + i, vbase, vert_first[m + 1] - vbase, rec + (size_t)(base + i) * 4);
}

__global__ __launch_bounds__(MM_THREADS) void mm_dist_kernel(int p, const float *__restrict__ points, const int *__restrict__ order,
                                                             const float4 *__restrict__ rec, const long long *__restrict__ face_first,
                                                             float *__restrict__ sqdist, int *__restrict__ face_idx) {
  __shared__ float4 tile[4][MM_TILE];   // component-major: plane c holds float4 c of every record of the tile
  const int m = blockIdx.y;
  const long long k = (long long)blockIdx.x * MM_THREADS + threadIdx.x;   // 64-bit: the last workgroup may reach past 2^31 - 1
  const long long base = face_first[m];
  const int nf = (int)(face_first[m + 1] - base);   // <= 2^24
  bool live = k < p;
  int pt = 0;
  if (live) {
    pt = order ? order[(size_t)m * p + k] : (int)k;
    live = pt >= 0 && pt < p;
  }
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float *q = points + ((size_t)m * p + pt) * 3;
    x = q[0]; y = q[1]; z = q[2];
  }
  float best = INFINITY;
  int idx = -1;
  for (int t0 = 0; t0 < nf; t0 += MM_TILE) {   // uniform over the workgroup
    __syncthreads();   // the previous tile has been read by everybody
    const int mine = t0 + (int)threadIdx.x;   // MM_TILE == MM_THREADS: one record per thread
    if (mine < nf) {
      const float4 *r = rec + (size_t)(base + mine) * 4;
      tile[0][threadIdx.x] = r[0]; tile[1][threadIdx.x] = r[1]; tile[2][threadIdx.x] = r[2]; tile[3][threadIdx.x] = r[3];
    }
    __syncthreads();
    const int cnt = nf - t0 < MM_TILE ? nf - t0 : MM_TILE;
    for (int j = 0; j < cnt; ++j) {
      const float4 r3 = tile[3][j];
      if (r3.x == 0.f) continue;   // invalid face: the same for every lane
      const float4 r0 = tile[0][j], r1 = tile[1][j], r2 = tile[2][j];
      const float d = mm_pair_sqdist(x, y, z, r0, r1, r2, r3);
      if (d < best) { best = d; idx = t0 + j; }   // ascending face order: the first of equal distances stays
    }
  }
  if (!live) return;
  if (!(finite1(x) && finite1(y) && finite1(z))) { best = INFINITY; idx = -1; }
  const size_t o = (size_t)m * p + pt;
  sqdist[o] = best;
  face_idx[o] = idx;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct MmSampleWs {
  long long *vert_first, *face_first;  // [b + 1] each
  long long *total;                    // [b]
  unsigned int *amax_bits;             // [b]
  long long *bsum;                     // [b][nb_max]
  long long *cum;                      // [sum_f]
  float *area;                         // [sum_f]
  int nb_max;
  size_t bytes;
};

MmSampleWs mm_sample_ws(void *ws, int b, long long sum_f, long long max_faces) {
  MmSampleWs w;
  char *p = (char *)ws;
  size_t off = 0;
  w.nb_max = (int)((max_faces + MM_THREADS - 1) / MM_THREADS);
  w.vert_first = (long long *)(p + off); off += sizeof(long long) * (size_t)(b + 1);
  w.face_first = (long long *)(p + off); off += sizeof(long long) * (size_t)(b + 1);
  w.total = (long long *)(p + off); off += sizeof(long long) * (size_t)b;
  w.bsum = (long long *)(p + off); off += sizeof(long long) * (size_t)b * w.nb_max;
  w.cum = (long long *)(p + off); off += sizeof(long long) * (size_t)sum_f;
  w.amax_bits = (unsigned int *)(p + off); off += sizeof(unsigned int) * (size_t)b;
  w.area = (float *)(p + off); off += sizeof(float) * (size_t)sum_f;
  w.bytes = align16(off);
  return w;
}

struct MmDistWs {
  float4 *rec;                         // [sum_f][4]
  long long *vert_first, *face_first;  // [b + 1] each
  size_t bytes;
};

MmDistWs mm_dist_ws(void *ws, int b, long long sum_f) {
  MmDistWs w;
  char *p = (char *)ws;
  const size_t rec_bytes = 64 * (size_t)sum_f;
  w.rec = (float4 *)p;
  w.vert_first = (long long *)(p + rec_bytes);
  w.face_first = w.vert_first + (b + 1);
  w.bytes = rec_bytes + offsets_bytes(b);   // rec_bytes is a multiple of 64
  return w;
}

// the checks on the offset arrays both entry points share -> 0, or 1 with the error set; max_f = the largest face count
int mm_check_offsets(const char *what, int b, const long long *vert_first, const long long *face_first, long long &max_f) {
  long long max_v = 0;
  if (check_first(what, "mesh", b, vert_first, &max_v) != BDM_OK || check_first(what, "mesh", b, face_first, &max_f) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(max_f <= MM_MAX_FACES, "%s: a mesh has %lld faces, more than %d", what, max_f, MM_MAX_FACES);
  BDM_REQUIRE(vert_first[b] <= INT_MAX && face_first[b] <= INT_MAX, "%s: %lld vertices or %lld faces reach 2^31", what, vert_first[b],
              face_first[b]);
  return BDM_OK;
}

bool mm_sizes_ok(int b, long long sum_f) { return b >= 0 && b <= MM_MAX_B && sum_f >= 0 && sum_f <= INT_MAX; }

}  // namespace

extern "C" size_t bdm_mesh_sample_workspace_bytes(int b, long long sum_f, long long max_faces) {
  if (!mm_sizes_ok(b, sum_f) || max_faces < 0 || max_faces > MM_MAX_FACES || max_faces > sum_f) return 0;
  return mm_sample_ws(nullptr, b, sum_f, max_faces).bytes;
}

extern "C" int bdm_mesh_sample_points(int b, int s, long long max_faces, const float *verts, const int *faces,
                                      const long long *vert_first, const long long *face_first, const unsigned long long *keys,
                                      unsigned int draw, unsigned int purpose, float *points, int *face_idx, float *normals,
                                      void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0 && b <= MM_MAX_B, "mesh_sample_points: batch size %d outside 0 .. %d", b, MM_MAX_B);
  BDM_REQUIRE(s >= 0, "mesh_sample_points: negative sample count");
  BDM_REQUIRE((long long)b * s <= INT_MAX, "mesh_sample_points: %d meshes of %d samples reach 2^31", b, s);
  if (b == 0 || s == 0) return BDM_OK;
  BDM_REQUIRE(verts && faces && vert_first && face_first && keys && points && workspace,
              "mesh_sample_points: an input, the points or the workspace is NULL");
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "mesh_sample_points: the workspace is not 16-byte aligned");
  long long max_f = 0;
  if (mm_check_offsets("mesh_sample_points", b, vert_first, face_first, max_f) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(max_faces == max_f, "mesh_sample_points: max_faces = %lld, the largest mesh has %lld", max_faces, max_f);
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const MmSampleWs ws = mm_sample_ws(workspace, b, sum_f, max_f);
  const size_t n = (size_t)b * s;
  const Range in[3] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {keys, 8 * (size_t)b}};
  const Range out[4] = {{points, 12 * n}, {face_idx, 4 * n}, {normals, 12 * n}, {workspace, ws.bytes}};
  if (check_overlap("mesh_sample_points", in, 3, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, ws.vert_first, ws.face_first, st);
  if (hipMemsetAsync(ws.amax_bits, 0, sizeof(unsigned int) * (size_t)b, st) != hipSuccess) return launch_status("mesh_sample_points (memset)");
  if (ws.nb_max > 0) {
    const dim3 grid((unsigned)ws.nb_max, (unsigned)b);
    hipLaunchKernelGGL(mm_area_kernel, grid, dim3(MM_THREADS), 0, st, verts, faces, ws.vert_first, ws.face_first, ws.area, ws.amax_bits);
    hipLaunchKernelGGL(mm_count_write_kernel<false>, grid, dim3(MM_THREADS), 0, st, ws.nb_max, ws.face_first, ws.area, ws.amax_bits,
                       ws.bsum, ws.cum);
  }
  hipLaunchKernelGGL(mm_scan_kernel, dim3((unsigned)b), dim3(MM_THREADS), 0, st, ws.nb_max, ws.face_first, ws.bsum, ws.total);
  if (ws.nb_max > 0)
    hipLaunchKernelGGL(mm_count_write_kernel<true>, dim3((unsigned)ws.nb_max, (unsigned)b), dim3(MM_THREADS), 0, st, ws.nb_max,
                       ws.face_first, ws.area, ws.amax_bits, ws.bsum, ws.cum);
  hipLaunchKernelGGL(mm_sample_kernel, dim3((unsigned)cdivll(s, MM_THREADS), (unsigned)b), dim3(MM_THREADS), 0, st, s, verts, faces,
                     ws.vert_first, ws.face_first, ws.cum, ws.total, keys, draw, purpose, points, face_idx, normals);
  return launch_status("mesh_sample_points");
}

extern "C" size_t bdm_point_mesh_distance_workspace_bytes(int b, long long sum_f) {
  if (!mm_sizes_ok(b, sum_f)) return 0;
  return mm_dist_ws(nullptr, b, sum_f).bytes;
}

extern "C" int bdm_point_mesh_distance_variant(int b, int p, long long sum_f, int has_order) {
  (void)has_order;
  if (!mm_sizes_ok(b, sum_f) || p < 0 || (long long)b * p > INT_MAX) return 0;
  return 1;   // the exhaustive form: the only one built (bdm_hip.h section 14)
}

extern "C" int bdm_point_mesh_distance(int b, int p, int form, const float *verts, const int *faces, const long long *vert_first,
                                       const long long *face_first, const float *points, const int *order, float *sqdist,
                                       int *face_idx, void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0 && b <= MM_MAX_B, "point_mesh_distance: batch size %d outside 0 .. %d", b, MM_MAX_B);
  BDM_REQUIRE(p >= 0, "point_mesh_distance: negative point count");
  BDM_REQUIRE((long long)b * p <= INT_MAX, "point_mesh_distance: %d meshes of %d points reach 2^31", b, p);
  BDM_REQUIRE(form != 2, "point_mesh_distance: the culled form is not built (no margin keeps its bits: bdm_hip.h section 14)");
  BDM_REQUIRE(form == 0 || form == 1, "point_mesh_distance: form %d is none of 0 (chooser), 1 (exhaustive)", form);
  if (b == 0 || p == 0) return BDM_OK;
  BDM_REQUIRE(verts && faces && vert_first && face_first && points && sqdist && face_idx && workspace,
              "point_mesh_distance: an input, an output or the workspace is NULL");
  BDM_REQUIRE(((uintptr_t)workspace & 15) == 0, "point_mesh_distance: the workspace is not 16-byte aligned");
  long long max_f = 0;
  if (mm_check_offsets("point_mesh_distance", b, vert_first, face_first, max_f) != BDM_OK) return BDM_ERR_ARG;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const MmDistWs ws = mm_dist_ws(workspace, b, sum_f);
  const size_t n = (size_t)b * p;
  const Range in[4] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {points, 12 * n}, {order, 4 * n}};
  const Range out[3] = {{sqdist, 4 * n}, {face_idx, 4 * n}, {workspace, ws.bytes}};
  if (check_overlap("point_mesh_distance", in, 4, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, ws.vert_first, ws.face_first, st);
  if (max_f > 0)
    hipLaunchKernelGGL(mm_record_kernel, dim3((unsigned)cdivll(max_f, MM_THREADS), (unsigned)b), dim3(MM_THREADS), 0, st, verts, faces,
                       ws.vert_first, ws.face_first, ws.rec);
  hipLaunchKernelGGL(mm_dist_kernel, dim3((unsigned)cdivll(p, MM_THREADS), (unsigned)b), dim3(MM_THREADS), 0, st, p, points, order, ws.rec,
                     ws.face_first, sqdist, face_idx);
  return launch_status("point_mesh_distance");
}
