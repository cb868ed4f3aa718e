// mesh_decimate.hip -- vertex-clustering simplification of a packed batch of triangle meshes (Open3D's simplify_vertex_clustering by
// name and meaning) as gfx950 kernels (bdm_hip.h section 20; the rule is this project's own text).
//
// The rule in one paragraph: per mesh, lo / hi are the bounds of the finite vertices and h the cell size (given, or the largest extent
// over the resolution, 1 where that is zero or not finite).  A finite vertex lies in cell k_a = min(floorf((c_a - lo_a) / h), 2^21 - 1),
// key kx | ky << 21 | kz << 42; equal keys form a cluster, a non-finite vertex is a cluster of its own.  A cluster's leader is its
// smallest member; the new vertices are the clusters in ascending leader.  A cluster of one is copied; a larger one takes the leader's
// row ("first") or section 19's fixed-point mean over its members ("average").  A connected face is mapped through the clusters,
// dropped when two corners fall together, and dropped as a duplicate when a face of a lower index has the same vertex set.  Nothing
// depends on execution order: leaders and kept faces are minima, counts and coordinate sums are integers.
//
// Kernels.
//   (ragged.h)            send_offsets: the host offset arrays (and the bits of the per-mesh cell sizes) travel as launch arguments.
//   (mesh_incidence.h)    fill_ints_kernel; scan_kernel<false / true>, scan_top_kernel; connected_face.
//   md_table_kernel       the open-addressing table emptied: keys to the marker with bit 63 set, values to INT_MAX.
//   md_bounds_kernel      per mesh lo / hi of the finite vertices and the largest finite |coordinate|: order-preserving bits, reduced in
//                         LDS, one integer atomic minimum / maximum per workgroup (mesh_emit.h's block_fold_atomic).
//   (mesh_emit.h)         amax_clear_kernel, attr_amax_kernel: the largest finite |attribute| into stat[8 m + 7]; member_flag,
//                         member_place and build_member_segments: the clusters' member segments; FixedMean: section 19's mean.
//   md_cell_kernel        one thread per mesh: h.
//   md_insert_kernel      one thread per vertex: its key claims a slot of the mesh's region (64-bit compare-and-swap on the key), then an
//                         atomic minimum of the member index on the slot's leader.  Slot placement depends on arrival order; only
//                         key -> leader leaves the table (md_leader_kernel reads it back per vertex).
//   md_leader_kernel      the leader read back per vertex -> member_flag.
//   md_member_kernel      member_place, and around it the per-mesh vertex counts.
//   md_face_insert_kernel one thread per face: not connected / collapsed, or the sorted new triple (3 x 21 bits) claims a slot of the
//                         same table and takes the minimum of the old face index.
//   md_face_keep_kernel   kept = (minimum == own index); flags for the scan; per-mesh face counts.  md_face_map_kernel: face_map out.
//   md_vertex_out_kernel  one thread per cluster (at its leader): copies a row, or walks the segment into two FixedMean.
//                         md_face_out_kernel: the kept faces.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "mesh_incidence.h"
#include "mesh_emit.h"

#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>

#pragma clang fp contract(off)

using namespace bdm;

#define MD_THREADS MESH_THREADS
#define MD_COUNTS 8                       // per-mesh counters, in the order of bdm_hip.h section 20
#define MD_MAX_V (1 << 21)                // vertices per mesh, exclusive
#define MD_MAX_CELL ((1 << 21) - 1)
#define MD_MAX_R 1024
#define MD_EMPTY 0x8000000000000000ull    // no key has bit 63
#define MD_BAD (-3)
#define MD_DUPLICATE (-2)
#define MD_COLLAPSED (-1)

namespace {

typedef unsigned long long md_key;

// floats as unsigned integers of the same order (-0 below +0: the rule does not look at the sign of a zero)
__device__ __forceinline__ unsigned md_ordered(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// (without a select: the instruction selector of ROCm 7.2 crashes on the selected bits going into md_cell_kernel's subtraction)
__device__ __forceinline__ float md_unordered(unsigned o) { return __uint_as_float(o ^ (~(unsigned)((int)o >> 31) | 0x80000000u)); }

__device__ __forceinline__ bool md_finite3(const float *p) {
  return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;
}

// the first slot of a key in a region of cap slots: the upper half of a 64-bit mix, scaled (cap < 2^23)
__device__ __forceinline__ unsigned md_slot0(md_key key, unsigned cap) {
  md_key x = key;
  x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27, x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return (unsigned)(((x >> 32) * (md_key)cap) >> 32);
}

// key -> its slot in the region (claimed if new), the slot's value lowered to `index`; -1 when `cap` probes found no room (never:
// a region has more slots than its mesh has keys)
__device__ __forceinline__ int md_insert(md_key *__restrict__ tkey, int *__restrict__ tval, unsigned cap, md_key key, int index) {
  unsigned s = md_slot0(key, cap);
  for (unsigned probe = 0; probe < cap; ++probe) {
    const md_key seen = atomicCAS(tkey + s, MD_EMPTY, key);
    if (seen == MD_EMPTY || seen == key) {
      atomicMin(tval + s, index);
      return (int)s;
    }
    s = s + 1 == cap ? 0 : s + 1;
  }
  return -1;
}

__global__ __launch_bounds__(MD_THREADS) void md_table_kernel(long long n, md_key *__restrict__ tkey, int *__restrict__ tval) {
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i < n) tkey[i] = MD_EMPTY, tval[i] = INT_MAX;
}

__global__ __launch_bounds__(MD_THREADS) void md_stat_kernel(int n, unsigned *__restrict__ stat) {
  const int i = blockIdx.x * MD_THREADS + threadIdx.x;
  if (i < n) stat[i] = (i & 7) < 3 ? 0xffffffffu : 0u;   // lo starts above every ordered value, hi and the maxima below
}

// stat[8 m + 0..2] lo, [3..5] hi (ordered bits), [6] the bits of the largest finite |coordinate|
__global__ __launch_bounds__(MD_THREADS) void md_bounds_kernel(const float *__restrict__ verts, const long long *__restrict__ vert_first,
                                                               unsigned *__restrict__ stat) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * MD_THREADS >= nv) return;   // the whole workgroup
  unsigned v[7] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, 0, 0};   // lo, hi, amax
  if (i < nv) {
    const float *p = verts + 3 * (size_t)(vbase + i);
    v[6] = amax_fold(p, 3, 0);
    if (md_finite3(p))
      for (int d = 0; d < 3; ++d) v[d] = v[3 + d] = md_ordered(p[d]);
  }
  block_fold_atomic<7, 3>(v, stat + 8 * m);
}

// cell[m] = h.  given[m] holds the bits of a float: the mesh's cell size, or with by_resolution the resolution, the same for every
// mesh; h is then the largest extent over it, 1 where that is zero or not finite.
__global__ __launch_bounds__(MD_THREADS) void md_cell_kernel(int b, int by_resolution, const long long *__restrict__ given,
                                                             const unsigned *__restrict__ stat, float *__restrict__ cell) {
  const int m = blockIdx.x * MD_THREADS + threadIdx.x;
  if (m >= b) return;
  const float value = __uint_as_float((unsigned)given[m]);
  float h = value;
  if (by_resolution) {
    const unsigned *s = stat + 8 * m;
    h = 0.0f;
    if (s[0] <= s[3]) {   // a finite vertex exists
      float ext = 0.0f;
      for (int d = 0; d < 3; ++d) ext = fmaxf(ext, md_unordered(s[3 + d]) - md_unordered(s[d]));
      h = ext / value;
    }
    if (!(h > 0.0f && h < INFINITY)) h = 1.0f;
  }
  cell[m] = h;
}

// one thread per vertex: slot[g] = the slot of its key within its mesh's region, -1 for a non-finite vertex
__global__ __launch_bounds__(MD_THREADS) void md_insert_kernel(const float *__restrict__ verts, const long long *__restrict__ vert_first,
                                                               const unsigned *__restrict__ stat, const float *__restrict__ cell,
                                                               md_key *__restrict__ tkey, int *__restrict__ tval, int *__restrict__ slot) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= nv) return;
  const float *p = verts + 3 * (size_t)(vbase + i);
  if (!md_finite3(p)) {
    slot[vbase + i] = -1;
    return;
  }
  const float h = cell[m];
  md_key key = 0;
  for (int d = 0; d < 3; ++d) {
    const float q = floorf((p[d] - md_unordered(stat[8 * m + d])) / h);
    const md_key k = q >= 2097152.0f ? MD_MAX_CELL : (q > 0.0f ? (md_key)(int)q : 0);
    key |= k << (21 * d);
  }
  const long long region = 2 * vbase + m;
  slot[vbase + i] = md_insert(tkey + region, tval + region, (unsigned)(2 * nv + 1), key, (int)i);
}

// member_flag at the leader the table holds for the vertex's key (rank's entry sum V: 0)
__global__ __launch_bounds__(MD_THREADS) void md_leader_kernel(const long long *__restrict__ vert_first, long long sum_v,
                                                               const int *__restrict__ tval, const int *__restrict__ slot,
                                                               int *__restrict__ lead, int *__restrict__ rank, int *__restrict__ seg) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (m == 0 && i == 0) rank[sum_v] = 0;
  if (i >= nv) return;
  const int s = slot[vbase + i];
  int l = (int)i;
  if (s >= 0) l = tval[2 * vbase + m + s];
  if (l < 0 || l > i) l = (int)i;   // never: the minimum over the members is at most i
  member_flag(vbase, i, l, lead, rank, seg);
}

// counts of mesh m: 0 new_vertices, 1 new_faces, 2 collapsed_faces, 3 duplicate_faces, 4 bad_faces, 5 nonfinite_vertices,
// 6 largest_cluster, 7 merged_vertices.  rank and seg are scanned: the cluster of leader g holds member[seg[g] .. seg[g + 1]).
__global__ __launch_bounds__(MD_THREADS) void md_member_kernel(const long long *__restrict__ vert_first, const int *__restrict__ slot,
                                                               const int *__restrict__ lead, const int *__restrict__ rank,
                                                               const int *__restrict__ seg, int *__restrict__ cursor,
                                                               int *__restrict__ member, int *__restrict__ vert_map,
                                                               int *__restrict__ counts) {
  __shared__ int part[3];   // non-finite, largest, merged
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * MD_THREADS >= nv) return;
  if (threadIdx.x < 3) part[threadIdx.x] = 0;
  __syncthreads();
  if (i < nv) {
    const long long g = member_place(vbase, i, lead, rank, seg, cursor, member, vert_map);
    const int size = seg[g + 1] - seg[g];
    if (slot[vbase + i] < 0) atomicAdd(part + 0, 1);
    if (g == vbase + i) atomicMax(part + 1, size);
    if (size > 1) atomicAdd(part + 2, 1);
    if (i == 0) counts[MD_COUNTS * m + 0] = rank[vbase + nv] - rank[vbase];
  }
  __syncthreads();
  if (threadIdx.x == 0 && part[0]) atomicAdd(counts + MD_COUNTS * m + 5, part[0]);
  if (threadIdx.x == 1 && part[1]) atomicMax(counts + MD_COUNTS * m + 6, part[1]);
  if (threadIdx.x == 2 && part[2]) atomicAdd(counts + MD_COUNTS * m + 7, part[2]);
}

// the new indices of a connected face that does not collapse -> true; code: MD_BAD or MD_COLLAPSED otherwise
__device__ __forceinline__ bool md_map_face(const int *__restrict__ faces, const int *__restrict__ lead, const int *__restrict__ rank,
                                            long long row, long long vbase, long long nv, int (&nw)[3], int &code) {
  int idx[3];
  if (!connected_face(faces, row, nv, idx)) {
    code = MD_BAD;
    return false;
  }
  for (int k = 0; k < 3; ++k) nw[k] = rank[vbase + lead[vbase + idx[k]]] - rank[vbase];
  if (nw[0] == nw[1] || nw[1] == nw[2] || nw[0] == nw[2]) {
    code = MD_COLLAPSED;
    return false;
  }
  return true;
}

// one thread per face: fcode[f] = MD_BAD, MD_COLLAPSED or the slot of its vertex set within its mesh's region
__global__ __launch_bounds__(MD_THREADS) void md_face_insert_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                    const long long *__restrict__ face_first, const int *__restrict__ lead,
                                                                    const int *__restrict__ rank, md_key *__restrict__ tkey,
                                                                    int *__restrict__ tval, int *__restrict__ fcode) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  int nw[3], code;
  if (md_map_face(faces, lead, rank, fbase + i, vbase, vert_first[m + 1] - vbase, nw, code)) {
    const int lo = min(nw[0], min(nw[1], nw[2])), hi = max(nw[0], max(nw[1], nw[2])), mid = nw[0] + nw[1] + nw[2] - lo - hi;
    const md_key key = (md_key)lo | ((md_key)mid << 21) | ((md_key)hi << 42);
    const long long region = 2 * fbase + m;
    code = md_insert(tkey + region, tval + region, (unsigned)(2 * nf + 1), key, (int)i);
    if (code < 0) code = MD_BAD;   // never
  }
  fcode[fbase + i] = code;
}

// frank[f] = 1 for a kept face (entry sum F: 0); face_map gets the codes of the dropped ones
__global__ __launch_bounds__(MD_THREADS) void md_face_keep_kernel(const long long *__restrict__ face_first, long long sum_f,
                                                                  const int *__restrict__ tval, const int *__restrict__ fcode,
                                                                  int *__restrict__ frank, int *__restrict__ face_map,
                                                                  int *__restrict__ counts) {
  __shared__ int part[3];   // collapsed, duplicate, bad
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (m == 0 && i == 0) frank[sum_f] = 0;
  if ((long long)blockIdx.x * MD_THREADS >= nf) return;
  if (threadIdx.x < 3) part[threadIdx.x] = 0;
  __syncthreads();
  if (i < nf) {
    int code = fcode[fbase + i];
    if (code >= 0) code = tval[2 * fbase + m + code] == i ? 0 : MD_DUPLICATE;
    frank[fbase + i] = code == 0 ? 1 : 0;
    face_map[fbase + i] = code;
    if (code < 0) atomicAdd(part + (-1 - code), 1);
  }
  __syncthreads();
  if (threadIdx.x < 3 && part[threadIdx.x]) atomicAdd(counts + MD_COUNTS * m + 2 + threadIdx.x, part[threadIdx.x]);
}

// frank is scanned
__global__ __launch_bounds__(MD_THREADS) void md_face_map_kernel(const long long *__restrict__ face_first, const int *__restrict__ frank,
                                                                 int *__restrict__ face_map, int *__restrict__ counts) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= nf) return;
  if (frank[fbase + i + 1] - frank[fbase + i] == 1) face_map[fbase + i] = frank[fbase + i] - frank[fbase];
  if (i == 0) counts[MD_COUNTS * m + 1] = frank[fbase + nf] - frank[fbase];
}

// ---- output ---------------------------------------------------------------------------------------------------------------------------
// one thread per vertex; the leader of a cluster writes the cluster's row (never one the caller's sizes do not hold)
__global__ __launch_bounds__(MD_THREADS) void md_vertex_out_kernel(int c, int average, const float *__restrict__ verts,
                                                                   const float *__restrict__ attrs, const long long *__restrict__ vert_first,
                                                                   const long long *__restrict__ out_vert_first, const int *__restrict__ lead,
                                                                   const int *__restrict__ rank, const int *__restrict__ seg,
                                                                   const int *__restrict__ member, const unsigned *__restrict__ stat,
                                                                   float *__restrict__ verts_out, float *__restrict__ attrs_out) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= nv || lead[vbase + i] != i) return;
  const long long g = vbase + i, row = rank[g] - rank[vbase];
  if (row >= out_vert_first[m + 1] - out_vert_first[m]) return;
  const int size = seg[g + 1] - seg[g];
  unsigned *o = (unsigned *)verts_out + 3 * (size_t)(out_vert_first[m] + row);
  unsigned *oa = (unsigned *)attrs_out + (size_t)c * (size_t)(out_vert_first[m] + row);
  if (size <= 1 || !average) {   // the row's bits
    const unsigned *p = (const unsigned *)verts + 3 * (size_t)g, *q = (const unsigned *)attrs + (size_t)c * (size_t)g;
    for (int d = 0; d < 3; ++d) o[d] = p[d];
    for (int d = 0; d < c; ++d) oa[d] = q[d];
    return;
  }
  FixedMean<3, false> mv(stat[8 * m + 6]);   // a non-finite vertex is a cluster of its own
  FixedMean<MESH_MAX_C, true> ma(stat[8 * m + 7]);
  const int *mem = member + seg[g];
  for (int t = 0; t < size; ++t) {   // the segment's order depends on arrival; integer sums do not
    const long long a = vbase + mem[t];
    mv.add(verts + 3 * (size_t)a, 3);
    ma.add(attrs + (size_t)c * (size_t)a, c);
  }
  mv.write((float *)o, 3, (double)size);
  ma.write((float *)oa, c, (double)size);
}

__global__ __launch_bounds__(MD_THREADS) void md_face_out_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                 const long long *__restrict__ face_first,
                                                                 const long long *__restrict__ out_face_first, const int *__restrict__ lead,
                                                                 const int *__restrict__ rank, const int *__restrict__ frank,
                                                                 int *__restrict__ faces_out) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= nf || frank[fbase + i + 1] - frank[fbase + i] != 1) return;
  const long long row = frank[fbase + i] - frank[fbase];
  if (row >= out_face_first[m + 1] - out_face_first[m]) return;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const int *fp = faces + 3 * (size_t)(fbase + i);
  int *o = faces_out + 3 * (size_t)(out_face_first[m] + row);
  for (int k = 0; k < 3; ++k) {
    const int a = fp[k];
    o[k] = a >= 0 && a < nv ? rank[vbase + lead[vbase + a]] - rank[vbase] : 0;   // a kept face is connected
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool md_sizes_ok(int b, long long sum_v, long long sum_f) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_f >= 0 && sum_v < INT_MAX && 3 * sum_f < INT_MAX;
}

// offsets | output offsets | the given cell sizes | stat (8 b) | cell (b) | table keys, values (2 max(sum V, sum F) + b each) |
// slot, lead, cursor, member (sum V each) | rank, seg (sum V + 1 each) | fcode (sum F) | frank (sum F + 1) | partial sums
struct MdWs {
  long long *vert_first, *face_first, *out_vert_first, *out_face_first, *given;
  unsigned *stat;
  float *cell;
  md_key *tkey;
  int *tval, *slot, *lead, *cursor, *member, *rank, *seg, *fcode, *frank, *bsum;
  long long table;
  size_t bytes;
};
MdWs md_ws(void *ws, int b, long long sum_v, long long sum_f) {
  Carve c{(char *)ws, 0};
  MdWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.out_vert_first = c.take_offsets(b), w.out_face_first = w.out_vert_first + (b + 1);
  w.given = c.take_offsets(b);
  w.stat = c.take<unsigned>(8 * (size_t)b);
  w.cell = c.take<float>((size_t)b);
  w.table = 2 * (sum_v > sum_f ? sum_v : sum_f) + b;
  w.tkey = c.take<md_key>((size_t)w.table);
  w.tval = c.take<int>((size_t)w.table);
  int **per_v[4] = {&w.slot, &w.lead, &w.cursor, &w.member};
  for (int i = 0; i < 4; ++i) *per_v[i] = c.take<int>((size_t)sum_v);
  w.rank = c.take<int>((size_t)sum_v + 1);
  w.seg = c.take<int>((size_t)sum_v + 1);
  w.fcode = c.take<int>((size_t)sum_f);
  w.frank = c.take<int>((size_t)sum_f + 1);
  w.bsum = c.take<int>((size_t)scan_blocks((sum_v > sum_f ? sum_v : sum_f) + 1));
  w.bytes = c.o;
  return w;
}

// the checks both entry points share -> BDM_OK with the largest per-mesh counts
int md_check(const char *what, int b, int resolution, const float *voxel_size, int contraction, const long long *vert_first,
             const long long *face_first, const void *workspace, long long &max_v, long long &max_f) {
  if (check_mesh_batch(what, b, vert_first, face_first, true, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(max_v < MD_MAX_V, "%s: a mesh of %lld vertices reaches 2^21", what, max_v);
  BDM_REQUIRE(vert_first[b] < INT_MAX && 3 * face_first[b] < INT_MAX, "%s: %lld vertices or %lld faces (three corners each) reach 2^31", what,
              vert_first[b], face_first[b]);
  BDM_REQUIRE(contraction == 0 || contraction == 1, "%s: contraction=%d is neither 0 (average) nor 1 (first)", what, contraction);
  if (voxel_size) {
    BDM_REQUIRE(resolution == 0, "%s: both a resolution (%d) and voxel sizes are given", what, resolution);
    for (int m = 0; m < b; ++m)
      BDM_REQUIRE(voxel_size[m] > 0.0f && voxel_size[m] < INFINITY, "%s: mesh %d: voxel_size %g is not positive and finite", what, m,
                  (double)voxel_size[m]);
  } else {
    BDM_REQUIRE(resolution >= 1 && resolution <= MD_MAX_R, "%s: resolution=%d outside 1 .. %d (and no voxel sizes)", what, resolution, MD_MAX_R);
  }
  return check_workspace(what, workspace);
}

}  // namespace

extern "C" size_t bdm_mesh_decimate_workspace_bytes(int b, long long sum_v, long long sum_f) {
  if (!md_sizes_ok(b, sum_v, sum_f)) return 0;
  return md_ws(nullptr, b, sum_v, sum_f).bytes;
}

extern "C" int bdm_mesh_cluster(int b, int resolution, const float *voxel_size, int contraction, const float *verts, const int *faces,
                                const long long *vert_first, const long long *face_first, int *vert_map, int *face_map, int *mesh_counts,
                                void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  if (md_check("mesh_cluster", b, resolution, voxel_size, contraction, vert_first, face_first, workspace, max_v, max_f) != BDM_OK)
    return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(verts && faces && vert_map && face_map && mesh_counts, "mesh_cluster: an input or an output is NULL");
  const MdWs w = md_ws(workspace, b, sum_v, sum_f);
  const Range in[2] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[4] = {{vert_map, 4 * (size_t)sum_v}, {face_map, 4 * (size_t)sum_f}, {mesh_counts, 4 * MD_COUNTS * (size_t)b},
                          {workspace, w.bytes}};
  if (check_overlap("mesh_cluster", in, 2, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  std::vector<long long> given((size_t)b + 1, 0);   // the bits of the cell sizes, or of the resolution, ride the same way
  for (int m = 0; m < b; ++m) {
    const float value = voxel_size ? voxel_size[m] : (float)resolution;
    unsigned bits;
    memcpy(&bits, &value, 4);
    given[m] = bits;
  }
  send_offsets(b, given.data(), nullptr, w.given, w.given + (b + 1), st);
  fill_ints(mesh_counts, (long long)MD_COUNTS * b, 0, st);
  hipLaunchKernelGGL(md_stat_kernel, dim3((unsigned)cdivll(8 * (long long)b, MD_THREADS)), dim3(MD_THREADS), 0, st, 8 * b, w.stat);
  fill_ints(w.rank, sum_v + 1, 0, st);    // a batch without vertices or faces still leaves an empty plan behind
  fill_ints(w.frank, sum_f + 1, 0, st);
  const dim3 block(MD_THREADS);
  if (max_v > 0) {   // with no vertex at all every face is bad: the face kernels below find that out
    const dim3 grid_v((unsigned)cdivll(max_v, MD_THREADS), (unsigned)b);
    hipLaunchKernelGGL(md_table_kernel, dim3((unsigned)cdivll(2 * sum_v + b, MD_THREADS)), block, 0, st, 2 * sum_v + b, w.tkey, w.tval);
    hipLaunchKernelGGL(md_bounds_kernel, grid_v, block, 0, st, verts, w.vert_first, w.stat);
    hipLaunchKernelGGL(md_cell_kernel, dim3((unsigned)cdivll(b, MD_THREADS)), block, 0, st, b, voxel_size ? 0 : 1, w.given, w.stat, w.cell);
    hipLaunchKernelGGL(md_insert_kernel, grid_v, block, 0, st, verts, w.vert_first, w.stat, w.cell, w.tkey, w.tval, w.slot);
    build_member_segments(
        sum_v, w.rank, w.seg, w.cursor, w.bsum, st,
        [&] { hipLaunchKernelGGL(md_leader_kernel, grid_v, block, 0, st, w.vert_first, sum_v, w.tval, w.slot, w.lead, w.rank, w.seg); },
        [&] {
          hipLaunchKernelGGL(md_member_kernel, grid_v, block, 0, st, w.vert_first, w.slot, w.lead, w.rank, w.seg, w.cursor, w.member, vert_map,
                             mesh_counts);
        });
  }
  if (max_f == 0) return launch_status("mesh_cluster");
  const dim3 grid_f((unsigned)cdivll(max_f, MD_THREADS), (unsigned)b);
  hipLaunchKernelGGL(md_table_kernel, dim3((unsigned)cdivll(2 * sum_f + b, MD_THREADS)), block, 0, st, 2 * sum_f + b, w.tkey, w.tval);
  hipLaunchKernelGGL(md_face_insert_kernel, grid_f, block, 0, st, faces, w.vert_first, w.face_first, w.lead, w.rank, w.tkey, w.tval, w.fcode);
  hipLaunchKernelGGL(md_face_keep_kernel, grid_f, block, 0, st, w.face_first, sum_f, w.tval, w.fcode, w.frank, face_map, mesh_counts);
  exclusive_scan_ints(w.frank, sum_f + 1, nullptr, w.bsum, st);
  hipLaunchKernelGGL(md_face_map_kernel, grid_f, block, 0, st, w.face_first, w.frank, face_map, mesh_counts);
  return launch_status("mesh_cluster");
}

extern "C" int bdm_mesh_decimate(int b, int resolution, const float *voxel_size, int contraction, int c, const float *verts, const float *attrs,
                                 const int *faces, const long long *vert_first, const long long *face_first, const long long *out_vert_first,
                                 const long long *out_face_first, float *verts_out, float *attrs_out, int *faces_out, void *workspace,
                                 void *stream) {
  long long max_v = 0, max_f = 0;
  const auto batch = [&] { return md_check("mesh_decimate", b, resolution, voxel_size, contraction, vert_first, face_first, workspace, max_v, max_f); };
  if (check_emit("mesh_decimate", "decimated", b, c, vert_first, face_first, out_vert_first, out_face_first,
                 verts && attrs && faces && verts_out && attrs_out && faces_out, batch, decimated_sizes_ok) != BDM_OK)
    return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b], out_v = out_vert_first[b], out_f = out_face_first[b];
  const MdWs w = md_ws(workspace, b, sum_v, sum_f);
  const Range in[3] = {{verts, 12 * (size_t)sum_v}, {attrs, 4 * (size_t)c * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[4] = {{verts_out, 12 * (size_t)out_v}, {attrs_out, 4 * (size_t)c * (size_t)out_v}, {faces_out, 12 * (size_t)out_f},
                          {workspace, w.bytes}};
  if (check_overlap("mesh_decimate", in, 3, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (max_v == 0) return BDM_OK;   // nothing to write
  send_offsets(b, out_vert_first, out_face_first, w.out_vert_first, w.out_face_first, st);
  const dim3 block(MD_THREADS);
  const dim3 grid_v((unsigned)cdivll(max_v, MD_THREADS), (unsigned)b);
  const int average = contraction == 0;
  if (average && c > 0) {
    hipLaunchKernelGGL(amax_clear_kernel, dim3((unsigned)cdivll(b, MD_THREADS)), block, 0, st, b, 8, w.stat + 7);
    hipLaunchKernelGGL(attr_amax_kernel, grid_v, block, 0, st, c, attrs, w.vert_first, 8, w.stat + 7);
  }
  hipLaunchKernelGGL(md_vertex_out_kernel, grid_v, block, 0, st, c, average, verts, attrs, w.vert_first, w.out_vert_first, w.lead, w.rank, w.seg,
                     w.member, w.stat, verts_out, attrs_out);
  if (max_f > 0 && out_f > 0)
    hipLaunchKernelGGL(md_face_out_kernel, dim3((unsigned)cdivll(max_f, MD_THREADS), (unsigned)b), block, 0, st, faces, w.vert_first, w.face_first,
                       w.out_face_first, w.lead, w.rank, w.frank, faces_out);
  return launch_status("mesh_decimate");
}
