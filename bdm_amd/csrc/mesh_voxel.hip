// mesh_voxel.hip -- solid voxelisation of a packed batch of triangle meshes by parity counting along grid-aligned rays, as gfx950
// kernels (bdm_hip.h section 21; the rule is this project's own text, restated by tests/mesh_voxel_ref.py).
//
// The rule in one paragraph: per mesh a grid of R cells per axis, origin o and cell size h.  A vertex snaps to q_a = rintf(((v_a - o_a)
// / h) * 256) in float32, operation by operation (no contraction, division correctly rounded); it is usable when finite with every
// |q_a| <= 2^19.  The centre of cell i sits at 256 i + 128.  A face with an index out of range, a repeated index or an unusable vertex
// is dropped and counted.  Every predicate is evaluated at the centre moved by (eps, eps^2, eps^3), eps positive and infinitesimal, so
// the ties of all three rays describe one point that is never on the surface.  Ray along axis w, (u, v) the two other axes in
// increasing order: the column centre is covered when the three int64 edge functions of the face (corners b and c swapped when its
// projected area is negative; area 0 contributes nothing) are > 0, or == 0 on an owned edge (tri_cover.h).  Cell k of a covered column
// lies below the face when sign~(g(k)) sign(n_w) < 0, n = (b - a) x (c - a), g(k) = n . (p_k - a), sign~(0) = the sign of the first
// non-zero of (n_x, n_y, n_z).  The face flips the parity of the cells below it; a cell is inside along w when its flips are odd.
// Nothing depends on execution order: the only atomics are integer XORs and integer adds.
//
// Integer bounds.  |q| <= 2^19 and R <= 512 put the centres in [128, 2^17): a difference of two vertices is at most 2^20 in magnitude
// and so is a centre minus a vertex (2^17 + 2^19 < 2^20).  An edge function and a normal component are a difference of two products
// of such differences: at most 2 * 2^40 = 2^41.  g is a sum of three products of a normal component and a difference: at most
// 3 * 2^41 * 2^20 = 3 * 2^61 < 2^63.  Everything below is int64 and exact.
//
// Kernels, after send_offsets (ragged.h) has put the offsets and the bits of the frames into the workspace.
//   mv_snap_kernel     one thread per vertex: (qx, qy, qz, usable), 16 bytes.
//   mv_flip_kernel     one thread per (face, axis): set-up (mv_setup), the box of the column centres the projection can cover clamped to
//                      the grid, then every centre of the box (tri_walk_boxes of tri_cover.h: small boxes by their lane, large ones by
//                      the whole wave) through mv_column: coverage, the number c of cells below by a binary search with the exact
//                      predicate (below is monotone in k: g is linear in k with slope 256 n_w), and for c > 0 one atomicXor of bit
//                      c - 1 into the column's flip words (ceil(R / 32) words per column, axis and mesh).  Faces used and dropped are
//                      summed on chip, one atomic add each per workgroup.
//   mv_parity_kernel   one thread per column: the suffix XOR of its flip words in place (shift-doubling inside a word, a carry across
//                      words): bit k becomes the parity of cell k.
//   mv_resolve_kernel  one thread per cell of a workgroup's strip, 256 neighbouring cells at a time: the three parities, occupancy by
//                      mode, the optional axes bits; the five cell counts are summed on chip (ballots, LDS), one atomic add each per
//                      workgroup, at most 2048 workgroups per mesh.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "mesh_incidence.h"
#include "tri_cover.h"

#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>

#pragma clang fp contract(off)

using namespace bdm;

#define MV_THREADS MESH_THREADS
#define MV_GUARD 524288.f                 // 2^19
#define MV_MAX_R 512
#define MV_STRIPS 2048                    // workgroups of the resolve kernel per mesh, at most
#define MV_COUNTS 8                       // per-mesh counters, in the order of bdm_hip.h section 21

namespace {

__device__ __forceinline__ float mv_lo_float(long long bits) { return __uint_as_float((unsigned)((unsigned long long)bits & 0xffffffffull)); }
__device__ __forceinline__ float mv_hi_float(long long bits) { return __uint_as_float((unsigned)((unsigned long long)bits >> 32)); }

// frame_a[m] = bits(o_x) | bits(o_y) << 32, frame_b[m] = bits(o_z) | bits(h) << 32
__global__ __launch_bounds__(MV_THREADS) void mv_snap_kernel(const float *__restrict__ verts, const long long *__restrict__ vert_first,
                                                             const long long *__restrict__ frame_a, const long long *__restrict__ frame_b,
                                                             int4 *__restrict__ vrec) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
  if (i >= nv) return;
  const float ox = mv_lo_float(frame_a[m]), oy = mv_hi_float(frame_a[m]), oz = mv_lo_float(frame_b[m]), h = mv_hi_float(frame_b[m]);
  const float *p = verts + 3 * (size_t)(vbase + i);
  const float qx = rintf(((p[0] - ox) / h) * (float)TRI_SNAP), qy = rintf(((p[1] - oy) / h) * (float)TRI_SNAP),
              qz = rintf(((p[2] - oz) / h) * (float)TRI_SNAP);
  // NaN fails every comparison; fabsf(inf) <= 2^19 is false
  const bool usable = finite3(p[0], p[1], p[2]) && fabsf(qx) <= MV_GUARD && fabsf(qy) <= MV_GUARD && fabsf(qz) <= MV_GUARD;
  vrec[vbase + i] = usable ? make_int4((int)qx, (int)qy, (int)qz, 1) : make_int4(0, 0, 0, 0);
}

// One face seen along one axis: its corners in the projection plane, wound positive, and G(k) = sign(n_w) g(k) as
// nu (pu - au) + nv (pv - av) + base + slope k.
struct MvItem {
  Tri2 t;                          // (u, v) of the corners
  long long nu, nv, base, slope;   // slope = 256 |n_w| > 0
  bool tie_below;                  // G(k) == 0: the perturbed centre lies below
  unsigned *col;                   // the flip words of the item's mesh and axis
};

__device__ __forceinline__ int mv_pick(const int4 &q, int axis) { return axis == 0 ? q.x : (axis == 1 ? q.y : q.z); }

// 0: the face is dropped; 1: it is used and contributes nothing along w (projected area 0); 2: it is used, f is set (but for col)
__device__ __forceinline__ int mv_setup(const int *__restrict__ faces, const int4 *__restrict__ vrec, long long row, long long vbase, long long nv,
                                        int w, MvItem &f) {
  int idx[3];
  if (!connected_face(faces, row, nv, idx)) return 0;
  const int4 a = vrec[vbase + idx[0]], b = vrec[vbase + idx[1]], c = vrec[vbase + idx[2]];
  if (!(a.w && b.w && c.w)) return 0;
  const int u = w == 0 ? 1 : 0, v = w == 2 ? 1 : 2;   // the two other axes in increasing order
  const int au = mv_pick(a, u), av = mv_pick(a, v), aw = mv_pick(a, w);
  const int bu = mv_pick(b, u), bv = mv_pick(b, v), cu = mv_pick(c, u), cv = mv_pick(c, v);
  int2 pb = make_int2(bu, bv), pc = make_int2(cu, cv);
  if (tri_wind(f.t, make_int2(au, av), pb, pc) == 0) return 1;
  const long long e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z, e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
  const long long nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const long long n_u = u == 0 ? nx : ny, n_v = v == 1 ? ny : nz, n_w = w == 0 ? nx : (w == 1 ? ny : nz);   // n_w = +-area, not 0
  const long long first = nx != 0 ? nx : (ny != 0 ? ny : nz);
  const bool neg = n_w < 0;
  f.nu = neg ? -n_u : n_u, f.nv = neg ? -n_v : n_v;
  const long long mag = neg ? -n_w : n_w;
  f.base = mag * (long long)(TRI_SNAP / 2 - aw);
  f.slope = mag * TRI_SNAP;
  f.tie_below = (first < 0) != neg;   // sign(first) sign(n_w) < 0
  return 2;
}

// the column (iu, iv) of item f: nothing when its centre is not covered, else one XOR of bit c - 1 when c > 0 cells lie below the face.
// f.col is [word][iu][iv]: word k of all columns lies together, so that the lanes of the resolve kernel, which run along iv, read
// neighbouring words.  0 <= iu, iv < r: the box is clamped to the grid.
__device__ __forceinline__ void mv_column(const MvItem &f, int iu, int iv, int r) {
  long long e0, e1, e2;
  if (!tri_covers<false>(f.t, iu, iv, e0, e1, e2)) return;   // both axes of the plane run upwards
  const long long g0 = f.nu * (tri_centre(iu) - f.t.ax) + f.nv * (tri_centre(iv) - f.t.ay) + f.base;
  int lo = 0, hi = r;   // below(k) for k < lo, not below(k) for k >= hi; at most 10 halvings for r <= 512
  for (int step = 0; step < 10 && lo < hi; ++step) {
    const int mid = (lo + hi) >> 1;
    const long long g = g0 + f.slope * mid;
    if (g < 0 || (g == 0 && f.tie_below)) lo = mid + 1; else hi = mid;
  }
  if (lo > 0) atomicXor(f.col + ((size_t)((lo - 1) >> 5) * r + iu) * r + iv, 1u << ((lo - 1) & 31));   // lo - 1 < r: a word of the column
}

// flips: [b][3][words][r][r], zeroed.  counts[8 m + 0] += faces used, [8 m + 1] += faces dropped.
__global__ __launch_bounds__(MV_THREADS) void mv_flip_kernel(int r, int words, const int *__restrict__ faces, const int4 *__restrict__ vrec,
                                                             const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                             unsigned *__restrict__ flips, int *__restrict__ counts) {
  __shared__ int part[2];
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  if ((long long)blockIdx.x * MV_THREADS >= 3 * nf) return;   // the whole workgroup: no lane may leave alone before the walk below
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  if (threadIdx.x < 2) part[threadIdx.x] = 0;
  __syncthreads();
  const long long t = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
  const int i = (int)(t / 3), w = (int)(t - 3 * (long long)i);   // 3 nf < 2^31
  const auto setup = [&](int bi, int bw, MvItem &g) {   // the lane's own face and axis, or broadcast ones
    g.col = flips + ((size_t)3 * m + bw) * r * r * words;
    return mv_setup(faces, vrec, fbase + bi, vbase, nv, bw, g);
  };
  MvItem f;
  int ua = 0, ub = -1, va = 0, vb = -1;
  bool live = i < nf;
  if (live) {
    const int state = setup(i, w, f);
    if (w == 0) atomicAdd(part + (state == 0 ? 1 : 0), 1);
    live = state == 2 && tri_box(f.t, r, r, ua, ub, va, vb);
  }
  // a large item is set up again from its broadcast face and axis
  tri_walk_boxes(live, ua, ub, va, vb, f, [&](int src, MvItem &g) { return setup(__shfl(i, src), __shfl(w, src), g) == 2; },
                 [&](const MvItem &g, int iu, int iv) { mv_column(g, iu, iv, r); });
  __syncthreads();
  if (threadIdx.x < 2 && part[threadIdx.x]) atomicAdd(counts + MV_COUNTS * m + threadIdx.x, part[threadIdx.x]);
}

// one thread per column: flip words -> parity words in place.  Bit k of the result is the XOR of the flip bits j >= k of the column.
__global__ __launch_bounds__(MV_THREADS) void mv_parity_kernel(long long columns, int rr, int words, unsigned *__restrict__ flips) {
  const long long col = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
  if (col >= columns) return;
  const long long block = col / rr;   // mesh and axis; rr = r r columns each
  unsigned *p = flips + (size_t)block * rr * words + (size_t)(col - block * rr);
  unsigned carry = 0;   // the parity of all bits of the words above
  for (int k = words - 1; k >= 0; --k) {   // words <= 16
    unsigned y = p[(size_t)k * rr];
    y ^= y >> 1, y ^= y >> 2, y ^= y >> 4, y ^= y >> 8, y ^= y >> 16;   // bit j = the XOR of the word's bits >= j
    if (carry) y = ~y;
    carry = y & 1u;
    p[(size_t)k * rr] = y;
  }
}

// counts[8 m + 2 ..]: occupied along x, y, z, occupied by mode, disagree.  mode: 0 vote, 1 x, 2 y, 3 z.  A workgroup takes a strip of
// `strip` cells (a multiple of the workgroup size), 256 neighbouring cells at a time, so that a mesh ends in at most MV_STRIPS x 5
// atomic adds: the five counters of a mesh share a cache line, and with one workgroup per 256 cells the adds on it take longer than
// everything else in the call.
__global__ __launch_bounds__(MV_THREADS) void mv_resolve_kernel(int r, int words, int mode, int strip, const unsigned *__restrict__ parity,
                                                                unsigned char *__restrict__ occupancy, unsigned char *__restrict__ axes,
                                                                int *__restrict__ counts) {
  __shared__ int part[5];
  const int m = blockIdx.y;
  const int cells = r * r * r;   // b r^3 < 2^31
  const long long start = (long long)blockIdx.x * strip;   // the grid covers r^3 once; start + strip < 2^32
  if (threadIdx.x < 5) part[threadIdx.x] = 0;
  __syncthreads();
  const unsigned *pm = parity + (size_t)m * 3 * r * r * words;
  const size_t axis_words = (size_t)r * r * words;
  int sum[5] = {0, 0, 0, 0, 0};   // per wave: the ballots are uniform
  for (int off = 0; off < strip; off += MV_THREADS) {   // uniform trip count
    const long long e = start + off + threadIdx.x;
    const bool live = e < cells;
    unsigned bits = 0;
    if (live) {
      const int ix = (int)e / (r * r), rem = (int)e - ix * (r * r), iy = rem / r, iz = rem - iy * r;
      const unsigned px = pm[((size_t)(ix >> 5) * r + iy) * r + iz] >> (ix & 31);   // lanes run along iz: neighbouring words
      const unsigned py = pm[axis_words + ((size_t)(iy >> 5) * r + ix) * r + iz] >> (iy & 31);
      const unsigned pz = pm[2 * axis_words + ((size_t)(iz >> 5) * r + ix) * r + iy] >> (iz & 31);
      bits = (px & 1u) | ((py & 1u) << 1) | ((pz & 1u) << 2);
    }
    const unsigned votes = __popc(bits);
    const bool occ = mode == 0 ? votes >= 2 : ((bits >> (mode - 1)) & 1u) != 0;
    if (live) {
      const size_t at = (size_t)m * cells + (size_t)e;
      occupancy[at] = occ ? 1 : 0;
      if (axes) axes[at] = (unsigned char)bits;
    }
    const bool flag[5] = {(bits & 1u) != 0, (bits & 2u) != 0, (bits & 4u) != 0, occ, votes == 1 || votes == 2};
#pragma unroll
    for (int k = 0; k < 5; ++k) sum[k] += __popcll(__ballot(flag[k]));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (sum[k]) atomicAdd(part + k, sum[k]);
  }
  __syncthreads();
  if (threadIdx.x < 5 && part[threadIdx.x]) atomicAdd(counts + MV_COUNTS * m + 2 + threadIdx.x, part[threadIdx.x]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool mv_sizes_ok(int b, long long sum_v, long long sum_f, int r) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_f >= 0 && sum_v < INT_MAX && 3 * sum_f < INT_MAX && r >= 1 && r <= MV_MAX_R &&
         (long long)b * r * r * r <= INT_MAX;
}

// offsets | frames | the vertex records (sum V) | the flip / parity words (b 3 ceil(R / 32) R R)
struct MvWs {
  long long *vert_first, *face_first, *frame_a, *frame_b;
  int4 *vrec;
  unsigned *flips;
  int words;
  size_t flip_words, bytes;
};
MvWs mv_ws(void *ws, int b, long long sum_v, int r) {
  Carve c{(char *)ws, 0};
  MvWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.frame_a = c.take_offsets(b), w.frame_b = w.frame_a + (b + 1);
  w.vrec = c.take<int4>((size_t)sum_v);
  w.words = (r + 31) / 32;
  w.flip_words = (size_t)b * 3 * r * r * w.words;
  w.flips = c.take<unsigned>(w.flip_words);
  w.bytes = c.o;
  return w;
}

unsigned long long mv_bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return u;
}

}  // namespace

extern "C" size_t bdm_mesh_voxelize_workspace_bytes(int b, long long sum_v, long long sum_f, int resolution) {
  if (!mv_sizes_ok(b, sum_v, sum_f, resolution)) return 0;
  return mv_ws(nullptr, b, sum_v, resolution).bytes;
}

extern "C" int bdm_mesh_voxelize(int b, int resolution, int mode, const float *origin, const float *cell, const float *verts, const int *faces,
                                 const long long *vert_first, const long long *face_first, unsigned char *occupancy, unsigned char *axes,
                                 int *counts, void *workspace, void *stream) {
  const char *what = "mesh_voxelize";
  const int r = resolution;
  long long max_v = 0, max_f = 0;
  if (check_mesh_batch(what, b, vert_first, face_first, true, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  BDM_REQUIRE(r >= 1 && r <= MV_MAX_R, "%s: resolution=%d outside 1 .. %d", what, r, MV_MAX_R);
  BDM_REQUIRE(mode >= 0 && mode <= 3, "%s: mode=%d is none of 0 (vote), 1 (x), 2 (y), 3 (z)", what, mode);
  BDM_REQUIRE((long long)b * r * r * r <= INT_MAX, "%s: %d grids of %d^3 cells reach 2^31", what, b, r);
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(sum_v < INT_MAX && 3 * sum_f < INT_MAX, "%s: %lld vertices or %lld faces (three corners each) reach 2^31", what, sum_v, sum_f);
  BDM_REQUIRE(origin && cell, "%s: the origins or the cell sizes are NULL", what);
  for (int m = 0; m < b; ++m) {
    BDM_REQUIRE(cell[m] > 0.0f && cell[m] < INFINITY, "%s: mesh %d: cell size %g is not positive and finite", what, m, (double)cell[m]);
    for (int d = 0; d < 3; ++d)
      BDM_REQUIRE(fabsf(origin[3 * m + d]) < INFINITY, "%s: mesh %d: origin[%d] = %g is not finite", what, m, d, (double)origin[3 * m + d]);
  }
  BDM_REQUIRE(verts && faces && occupancy && counts, "%s: an input or an output is NULL", what);
  if (check_workspace(what, workspace) != BDM_OK) return BDM_ERR_ARG;
  const MvWs w = mv_ws(workspace, b, sum_v, r);
  const size_t cells = (size_t)b * r * r * r;
  const Range in[2] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[4] = {{occupancy, cells}, {axes, cells}, {counts, 4 * MV_COUNTS * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap(what, in, 2, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  std::vector<long long> fa((size_t)b + 1, 0), fb((size_t)b + 1, 0);   // the bits of the frames ride the same way
  for (int m = 0; m < b; ++m) {
    fa[m] = (long long)(mv_bits(origin[3 * m]) | (mv_bits(origin[3 * m + 1]) << 32));
    fb[m] = (long long)(mv_bits(origin[3 * m + 2]) | (mv_bits(cell[m]) << 32));
  }
  send_offsets(b, fa.data(), fb.data(), w.frame_a, w.frame_b, st);
  fill_ints(counts, (long long)MV_COUNTS * b, 0, st);
  if (hipMemsetAsync(w.flips, 0, sizeof(unsigned) * w.flip_words, st) != hipSuccess) return launch_status("mesh_voxelize (memset)");
  const dim3 block(MV_THREADS);
  if (max_v > 0)
    hipLaunchKernelGGL(mv_snap_kernel, dim3((unsigned)cdivll(max_v, MV_THREADS), (unsigned)b), block, 0, st, verts, w.vert_first, w.frame_a,
                       w.frame_b, w.vrec);
  if (max_f > 0) {   // without a vertex every face is dropped: the kernel counts that
    hipLaunchKernelGGL(mv_flip_kernel, dim3((unsigned)cdivll(3 * max_f, MV_THREADS), (unsigned)b), block, 0, st, r, w.words, faces, w.vrec,
                       w.vert_first, w.face_first, w.flips, counts);
    const long long columns = (long long)b * 3 * r * r;
    hipLaunchKernelGGL(mv_parity_kernel, dim3((unsigned)cdivll(columns, MV_THREADS)), block, 0, st, columns, r * r, w.words, w.flips);
  }
  const long long grid_cells = (long long)r * r * r;
  const int strip = (int)(cdivll(cdivll(grid_cells, MV_STRIPS), MV_THREADS) * MV_THREADS);   // <= 2^27 / 2^11 + 256
  hipLaunchKernelGGL(mv_resolve_kernel, dim3((unsigned)cdivll(grid_cells, strip), (unsigned)b), block, 0, st, r, w.words, mode, strip, w.flips,
                     occupancy, axes, counts);
  return launch_status(what);
}
