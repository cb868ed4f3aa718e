// mesh_fill.hip -- closing the holes of triangle meshes: the boundary loops of a packed batch and a centroid fan over every small
// simple one, as gfx950 kernels (bdm_hip.h section 19; the rule is this project's own text).
//
// The rule in one paragraph: connected face f (mesh_clean.hip's) has half-edges 3f + k running v_k -> v_{k+1}.  a -> x is a boundary
// half-edge when exactly one half-edge runs a -> x and none x -> a; an edge with one each way is interior, everything else irregular.
// The successor of boundary half-edge p -> a is found by rotating about a through interior edges until a boundary half-edge (the
// successor) or an irregular edge (blocked) turns up.  A loop is a cycle of successors, its label its smallest half-edge; it is filled
// iff it has at most max_hole_edges half-edges, no vertex twice and finite source vertices.  A filled loop gets one vertex, the
// fixed-point mean of its sources, and one face (b, a, c) per half-edge a -> b.  Nothing depends on execution order: segments are
// sorted, labels are minima, counts and coordinate sums are integers.
//
// Kernels.
//   (ragged.h)            send_offsets: the host offset arrays travel as launch arguments into the workspace.
//   (mesh_incidence.h)    fill_ints_kernel; scan_kernel<false / true>, scan_top_kernel: the entry count may live on the device (the
//                         compacted list); incidence_kernel<false / true, MfKeys>: the records of a corner are two 64-bit keys
//                         neighbour << 32 | direction << 31 | half-edge (direction 0: vertex -> neighbour, 1: neighbour -> vertex).
//   mf_sort_kernel        one thread per vertex: sorts its segment of keys (sort_segment).
//   mf_classify_kernel    one thread per half-edge: boundary or not; presets the three per-half-edge outputs.
//   mf_compact_kernel     one thread per half-edge: a boundary half-edge moves to its scanned place (order kept).
//   Everything below runs on the compacted list, grid-stride, its length read from the device:
//   mf_walk_kernel        the rotation about the target vertex -> successor or blocked.
//   mf_double_kernel      one pointer-doubling round, Jacobi: reads one state array, writes the other.
//   mf_label_kernel       labels out, loop sizes (integer atomic adds), pinched and non-finite flags (flag stores by atomic or).
//   mf_decide_kernel      one thread per loop root: the loop's flags, the per-mesh counts.  mf_face_flag_kernel: which half-edges get a face.
//   mf_amax_kernel        per mesh the bits of the largest finite |coordinate| and |attribute| in one launch (mesh_emit.h's amax_fold
//                         and block_fold_atomic: one integer atomic max per lane and workgroup).
//   mf_copy_kernel        old rows to their place in the outputs.
//   mf_mean_kernel        one thread per filled loop: walks the loop and feeds mesh_emit.h's FixedMean (64-bit integer sums, one
//                         float64 divide, one rounding to float32).
//   mf_emit_kernel        one thread per boundary half-edge of a filled loop: its face.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "mesh_incidence.h"
#include "mesh_emit.h"
#include "align_solve.h"   // align_ceil_log2

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

using namespace bdm;

#define MF_THREADS MESH_THREADS
#define MF_MAX_EDGES 65535
#define MF_COUNTS 9                       // per-mesh counters, in the order of bdm_hip.h section 19
#define MF_STRIDE_BLOCKS 1024             // grid of the kernels on the compacted list
#define MF_BLOCKED 0x80000000u
#define MF_FILLED 1
#define MF_TOO_LARGE 2
#define MF_PINCHED 4
#define MF_NONFINITE 8

namespace {

typedef long long mf_key;

__device__ __forceinline__ mf_key mf_make_key(int nbr, int dir, int h) { return ((mf_key)nbr << 32) | ((mf_key)dir << 31) | (mf_key)h; }
__device__ __forceinline__ int mf_key_nbr(mf_key k) { return (int)(k >> 32); }
__device__ __forceinline__ int mf_key_dir(mf_key k) { return (int)((k >> 31) & 1); }
__device__ __forceinline__ int mf_key_half(mf_key k) { return (int)(k & 0x7fffffffll); }

struct MfKeys {   // Rec of incidence_kernel: corner c of face i records its outgoing and its incoming half-edge
  typedef mf_key type;
  static __device__ __forceinline__ void corner(const int (&idx)[3], int i, int c, mf_key &r0, mf_key &r1) {
    r0 = mf_make_key(idx[(c + 1) % 3], 0, 3 * i + c);                 // this vertex -> the next one
    r1 = mf_make_key(idx[(c + 2) % 3], 1, 3 * i + (c + 2) % 3);       // the previous one -> this vertex
  }
};

// one thread per packed vertex: its segment of keys sorted ascending in place (the keys are all different: the half-edge is part of them)
__global__ __launch_bounds__(MF_THREADS) void mf_sort_kernel(long long sum_v, const int *__restrict__ first, mf_key *__restrict__ rec) {
  const long long g = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
  if (g < sum_v) sort_segment(rec + first[g], first[g + 1] - first[g]);
}

// the half-edges between a and x in a's sorted segment: how many run a -> x (out) and x -> a (in), and the last x -> a seen
__device__ __forceinline__ void mf_lookup(const mf_key *__restrict__ seg, int len, int x, int &out, int &in, int &in_half) {
  int lo = 0, hi = len;
  const mf_key want = (mf_key)x << 32;
  while (lo < hi) {   // first key >= (x, 0, 0)
    const int mid = (lo + hi) >> 1;
    if (seg[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  out = in = 0, in_half = -1;
  for (int e = lo; e < len; ++e) {
    const mf_key k = seg[e];
    if (mf_key_nbr(k) != x) break;
    if (mf_key_dir(k)) ++in, in_half = mf_key_half(k);
    else ++out;
  }
}

// one thread per half-edge of mesh m: flag[hg] = 1 for a boundary half-edge; the three per-half-edge outputs get their defaults
__global__ __launch_bounds__(MF_THREADS) void mf_classify_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                 const long long *__restrict__ face_first, long long total,
                                                                 const int *__restrict__ first, const mf_key *__restrict__ rec,
                                                                 int *__restrict__ flag, int *__restrict__ halfedge_loop,
                                                                 int *__restrict__ loop_size, int *__restrict__ loop_flags) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long h = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
  if (m == 0 && h == 0) flag[total] = 0;   // the scan's last entry becomes the length of the compacted list
  if (h >= 3 * nf) return;
  const long long vbase = vert_first[m], hg = 3 * fbase + h;
  const int f = (int)(h / 3), k = (int)(h - 3 * (long long)f);
  int idx[3], boundary = 0;
  if (connected_face(faces, fbase + f, vert_first[m + 1] - vbase, idx)) {
    const int a = idx[k], x = idx[(k + 1) % 3];
    const int s0 = first[vbase + a];
    int out, in, in_half;
    mf_lookup(rec + s0, first[vbase + a + 1] - s0, x, out, in, in_half);
    boundary = out == 1 && in == 0;
  }
  flag[hg] = boundary;
  halfedge_loop[hg] = -1;
  loop_size[hg] = 0;
  loop_flags[hg] = 0;
}

// pos = the exclusive scan of the flags
__global__ __launch_bounds__(MF_THREADS) void mf_compact_kernel(const long long *__restrict__ face_first, const int *__restrict__ pos,
                                                                int *__restrict__ bh, int *__restrict__ bm) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long h = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
  if (h >= 3 * nf) return;
  const long long hg = 3 * fbase + h;
  const int j = pos[hg];
  if (pos[hg + 1] - j == 1) bh[j] = (int)hg, bm[j] = m;
}

// ---- on the compacted list ------------------------------------------------------------------------------------------------------------
// state of entry j: x = the entry 2^r successors on (itself once blocked), y = blocked << 31 | the smallest entry among those passed
__global__ __launch_bounds__(MF_THREADS) void mf_walk_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                             const long long *__restrict__ face_first, const int *__restrict__ first,
                                                             const mf_key *__restrict__ rec, const int *__restrict__ pos,
                                                             const int *__restrict__ nb_dev, const int *__restrict__ bh,
                                                             const int *__restrict__ bm, int *__restrict__ succ, uint2 *__restrict__ state) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j < nb; j += (long long)gridDim.x * MF_THREADS) {
    const int m = bm[j];
    const long long fbase = face_first[m], vbase = vert_first[m];
    const int h = (int)(bh[j] - 3 * fbase);
    int f = h / 3, k = h - 3 * f;
    const int *fp = faces + 3 * (size_t)(fbase + f);
    const int a = fp[(k + 1) % 3];   // the target of h: the walk turns about it
    int x = fp[(k + 2) % 3];
    int cur = 3 * f + (k + 1) % 3;   // a -> x in the same face
    const int s0 = first[vbase + a], len = first[vbase + a + 1] - s0;
    int next = -1;
    for (int step = 0; step < len; ++step) {   // every crossing uses up two records of a's segment
      int out, in, in_half;
      mf_lookup(rec + s0, len, x, out, in, in_half);
      if (out == 1 && in == 0) {
        next = cur;
        break;
      }
      if (!(out == 1 && in == 1)) break;   // irregular: blocked
      f = in_half / 3, k = in_half - 3 * f;   // the face (x, a, y) across the edge
      x = faces[3 * (size_t)(fbase + f) + (k + 2) % 3];
      cur = 3 * f + (k + 1) % 3;   // a -> y
    }
    if (next >= 0) {
      const int t = pos[3 * fbase + next];
      succ[j] = t;
      state[j] = make_uint2((unsigned)t, (unsigned)j);
    } else {
      succ[j] = -1;
      state[j] = make_uint2((unsigned)j, MF_BLOCKED | (unsigned)j);
    }
  }
}

__global__ __launch_bounds__(MF_THREADS) void mf_double_kernel(const int *__restrict__ nb_dev, const uint2 *__restrict__ from,
                                                               uint2 *__restrict__ to) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j < nb; j += (long long)gridDim.x * MF_THREADS) {
    const uint2 s = from[j], t = from[s.x];
    const unsigned ls = s.y & ~MF_BLOCKED, lt = t.y & ~MF_BLOCKED;
    to[j] = make_uint2(t.x, ((s.y | t.y) & MF_BLOCKED) | (ls < lt ? ls : lt));
  }
}

// counts of mesh m: 0 boundary_edges, 1 loops, 2 filled, 3 too large, 4 pinched, 5 non-finite, 6 blocked_edges, 7 new vertices, 8 new faces
__global__ __launch_bounds__(MF_THREADS) void mf_label_kernel(const int *__restrict__ faces, const float *__restrict__ verts,
                                                              const long long *__restrict__ vert_first,
                                                              const long long *__restrict__ face_first, const int *__restrict__ first,
                                                              const mf_key *__restrict__ rec, const int *__restrict__ pos,
                                                              const int *__restrict__ nb_dev, const int *__restrict__ bh,
                                                              const int *__restrict__ bm, const uint2 *__restrict__ state,
                                                              int *__restrict__ lab, int *__restrict__ halfedge_loop,
                                                              int *__restrict__ loop_size, int *__restrict__ loop_flags,
                                                              int *__restrict__ counts) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j < nb; j += (long long)gridDim.x * MF_THREADS) {
    const int m = bm[j], hg = bh[j];
    const unsigned y = state[j].y;
    atomicAdd(counts + MF_COUNTS * m + 0, 1);
    if (y & MF_BLOCKED) {
      lab[j] = -2;
      halfedge_loop[hg] = -2;
      atomicAdd(counts + MF_COUNTS * m + 6, 1);
      continue;
    }
    const int root = (int)y, slot = bh[root];
    const long long fbase = face_first[m], vbase = vert_first[m];
    lab[j] = root;
    halfedge_loop[hg] = (int)(slot - 3 * fbase);
    atomicAdd(loop_size + slot, 1);
    const int h = (int)(hg - 3 * fbase);
    const int a = faces[3 * (size_t)(fbase + h / 3) + h % 3];   // the source
    const float *p = verts + 3 * (size_t)(vbase + a);
    int bits = 0;
    if (!(fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY)) bits |= MF_NONFINITE;
    const int s0 = first[vbase + a], s1 = first[vbase + a + 1];
    for (int e = s0; e < s1; ++e) {   // another half-edge of the same loop out of a: pinched
      const mf_key key = rec[e];
      if (mf_key_dir(key) || mf_key_half(key) == h) continue;
      const long long hg2 = 3 * fbase + mf_key_half(key);
      const int j2 = pos[hg2];
      if (pos[hg2 + 1] - j2 == 1 && state[j2].y == y) bits |= MF_PINCHED;
    }
    if (bits) atomicOr(loop_flags + slot, bits);
  }
}

__global__ __launch_bounds__(MF_THREADS) void mf_decide_kernel(int max_hole_edges, const int *__restrict__ nb_dev, const int *__restrict__ bh,
                                                               const int *__restrict__ bm, const int *__restrict__ lab,
                                                               const int *__restrict__ loop_size, int *__restrict__ loop_flags,
                                                               int *__restrict__ wflag, int *__restrict__ wsize, int *__restrict__ rankv,
                                                               int *__restrict__ counts) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j <= nb; j += (long long)gridDim.x * MF_THREADS) {
    int fl = 0, size = 0;
    if (j < nb && lab[j] == j) {
      const int slot = bh[j], m = bm[j];
      size = loop_size[slot];
      fl = loop_flags[slot] | (size > max_hole_edges ? MF_TOO_LARGE : 0);
      if (fl == 0) fl = MF_FILLED;
      loop_flags[slot] = fl;
      int *c = counts + MF_COUNTS * m;
      atomicAdd(c + 1, 1);
      if (fl & MF_FILLED) atomicAdd(c + 2, 1), atomicAdd(c + 7, 1);
      if (fl & MF_TOO_LARGE) atomicAdd(c + 3, 1);
      if (fl & MF_PINCHED) atomicAdd(c + 4, 1);
      if (fl & MF_NONFINITE) atomicAdd(c + 5, 1);
    }
    if (j < nb) wflag[j] = fl, wsize[j] = size;
    rankv[j] = fl == MF_FILLED ? 1 : 0;   // entry nb: the scan's total
  }
}

__global__ __launch_bounds__(MF_THREADS) void mf_face_flag_kernel(const int *__restrict__ nb_dev, const int *__restrict__ bm,
                                                                  const int *__restrict__ lab, const int *__restrict__ wflag,
                                                                  int *__restrict__ rankf, int *__restrict__ counts) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j <= nb; j += (long long)gridDim.x * MF_THREADS) {
    int v = 0;
    if (j < nb && lab[j] >= 0 && wflag[lab[j]] == MF_FILLED) {
      v = 1;
      atomicAdd(counts + MF_COUNTS * bm[j] + 8, 1);
    }
    rankf[j] = v;
  }
}

// ---- filling --------------------------------------------------------------------------------------------------------------------------
// amax[2 m], amax[2 m + 1]: the bits of the largest finite |coordinate| and |attribute| of mesh m (bits of non-negative floats order as ints)
__global__ __launch_bounds__(MF_THREADS) void mf_amax_kernel(int c, const float *__restrict__ verts, const float *__restrict__ attrs,
                                                             const long long *__restrict__ vert_first, unsigned *__restrict__ amax) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
  unsigned top[2] = {0, 0};
  if (i < nv) {
    top[0] = amax_fold(verts + 3 * (size_t)(vbase + i), 3, 0);
    top[1] = amax_fold(attrs + (size_t)c * (size_t)(vbase + i), c, 0);
  }
  block_fold_atomic<2, 0>(top, amax + 2 * m);
}

// rows of `width` 4-byte words: mesh m's n rows from in_first[m] to out_first[m] (never more than the output holds)
__global__ __launch_bounds__(MF_THREADS) void mf_copy_kernel(int width, const unsigned *__restrict__ from, const long long *__restrict__ in_first,
                                                             const long long *__restrict__ out_first, unsigned *__restrict__ to) {
  const int m = blockIdx.y;
  const long long ibase = in_first[m], n = in_first[m + 1] - ibase, obase = out_first[m], room = out_first[m + 1] - obase;
  const long long i = (long long)blockIdx.x * MF_THREADS + threadIdx.x;
  if (i >= (n < room ? n : room) * width) return;
  to[obase * width + i] = from[ibase * width + i];
}

__global__ __launch_bounds__(MF_THREADS) void mf_mean_kernel(int c, const int *__restrict__ faces, const float *__restrict__ verts,
                                                             const float *__restrict__ attrs, const long long *__restrict__ vert_first,
                                                             const long long *__restrict__ face_first,
                                                             const long long *__restrict__ out_vert_first, const int *__restrict__ pos,
                                                             const int *__restrict__ nb_dev, const int *__restrict__ bh,
                                                             const int *__restrict__ bm, const int *__restrict__ succ,
                                                             const int *__restrict__ lab, const int *__restrict__ wflag,
                                                             const int *__restrict__ wsize, const int *__restrict__ rankv,
                                                             const unsigned *__restrict__ amax, float *__restrict__ verts_out,
                                                             float *__restrict__ attrs_out) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j < nb; j += (long long)gridDim.x * MF_THREADS) {
    if (lab[j] != j || wflag[j] != MF_FILLED) continue;
    const int m = bm[j], size = wsize[j];
    const long long fbase = face_first[m], vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
    const long long row = nv + (rankv[j] - rankv[pos[3 * fbase]]);   // the new vertex's index within its mesh
    if (row >= out_vert_first[m + 1] - out_vert_first[m]) continue;    // the caller's sizes do not hold it: never written
    FixedMean<3, false> mv(amax[2 * m]);   // a filled loop has finite sources
    FixedMean<MESH_MAX_C, true> ma(amax[2 * m + 1]);
    int t = (int)j;
    for (int step = 0; step < size; ++step) {   // the loop's half-edges; integer sums do not depend on where the walk starts
      const long long h = bh[t] - 3 * fbase;
      const int a = faces[3 * (size_t)(fbase + h / 3) + h % 3];
      mv.add(verts + 3 * (size_t)(vbase + a), 3);
      ma.add(attrs + (size_t)c * (size_t)(vbase + a), c);
      t = succ[t];
    }
    mv.write(verts_out + 3 * (size_t)(out_vert_first[m] + row), 3, (double)size);
    ma.write(attrs_out + (size_t)c * (size_t)(out_vert_first[m] + row), c, (double)size);
  }
}

__global__ __launch_bounds__(MF_THREADS) void mf_emit_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                             const long long *__restrict__ face_first,
                                                             const long long *__restrict__ out_face_first, const int *__restrict__ pos,
                                                             const int *__restrict__ nb_dev, const int *__restrict__ bh,
                                                             const int *__restrict__ bm, const int *__restrict__ lab,
                                                             const int *__restrict__ rankv, const int *__restrict__ rankf,
                                                             int *__restrict__ faces_out) {
  const int nb = *nb_dev;
  for (long long j = (long long)blockIdx.x * MF_THREADS + threadIdx.x; j < nb; j += (long long)gridDim.x * MF_THREADS) {
    if (rankf[j + 1] - rankf[j] != 1) continue;
    const int m = bm[j];
    const long long fbase = face_first[m], nf = face_first[m + 1] - fbase, nv = vert_first[m + 1] - vert_first[m];
    const int j0 = pos[3 * fbase];   // the mesh's first entry of the compacted list
    const long long row = nf + (rankf[j] - rankf[j0]);
    if (row >= out_face_first[m + 1] - out_face_first[m]) continue;   // the caller's sizes do not hold it: never written
    const long long h = bh[j] - 3 * fbase;
    const int *fp = faces + 3 * (size_t)(fbase + h / 3);
    const int k = (int)(h % 3);
    int *o = faces_out + 3 * (size_t)(out_face_first[m] + row);
    o[0] = fp[(k + 1) % 3], o[1] = fp[k], o[2] = (int)(nv + (rankv[lab[j]] - rankv[j0]));
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool mf_sizes_ok(int b, long long sum_v, long long sum_f) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_f >= 0 && 6 * sum_f <= INT_MAX && sum_v + sum_f < INT_MAX;
}

// offsets | output offsets | first (sum V + 1) | cursor (sum V + 1) | partial sums | records (6 sum F keys) | pos (H + 1) | bh, bm, succ,
// lab, wflag, wsize (H each) | rankv, rankf (H + 1 each) | two state arrays (H pairs each) | amax (2 b);  H = 3 sum F
struct MfWs {
  long long *vert_first, *face_first, *out_vert_first, *out_face_first;
  int *first, *cursor, *bsum, *pos, *bh, *bm, *succ, *lab, *wflag, *wsize, *rankv, *rankf;
  mf_key *rec;
  uint2 *state_a, *state_b;
  unsigned *amax;
  size_t bytes;
};
MfWs mf_ws(void *ws, int b, long long sum_v, long long sum_f) {
  Carve c{(char *)ws, 0};
  MfWs w;
  const size_t H = 3 * (size_t)sum_f;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.out_vert_first = c.take_offsets(b), w.out_face_first = w.out_vert_first + (b + 1);
  w.first = c.take<int>((size_t)(sum_v + 1));
  w.cursor = c.take<int>((size_t)(sum_v + 1));
  const long long longest = sum_v + 1 > (long long)H + 1 ? sum_v + 1 : (long long)H + 1;
  w.bsum = c.take<int>((size_t)scan_blocks(longest));
  w.rec = c.take<mf_key>(6 * (size_t)sum_f);
  w.pos = c.take<int>(H + 1);
  int **per_h[6] = {&w.bh, &w.bm, &w.succ, &w.lab, &w.wflag, &w.wsize};
  for (int i = 0; i < 6; ++i) *per_h[i] = c.take<int>(H);
  w.rankv = c.take<int>(H + 1);
  w.rankf = c.take<int>(H + 1);
  w.state_a = c.take<uint2>(H);
  w.state_b = c.take<uint2>(H);
  w.amax = c.take<unsigned>(2 * (size_t)b);
  w.bytes = c.o;
  return w;
}

int mf_rounds(long long max_f) { return max_f > 0 ? align_ceil_log2(3 * max_f) + 1 : 0; }

// the checks both entry points share -> BDM_OK with the largest per-mesh counts
int mf_check(const char *what, int b, const long long *vert_first, const long long *face_first, const void *workspace, long long &max_v,
             long long &max_f) {
  if (check_mesh_batch(what, b, vert_first, face_first, true, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(6 * face_first[b] <= INT_MAX, "%s: %lld faces: six records per face reach 2^31", what, face_first[b]);
  BDM_REQUIRE(vert_first[b] + face_first[b] < INT_MAX, "%s: %lld vertices and %lld faces: a new vertex index could reach 2^31", what,
              vert_first[b], face_first[b]);
  return check_workspace(what, workspace);
}

unsigned mf_stride_grid(long long sum_f) {
  const long long blocks = cdivll(3 * sum_f + 1, MF_THREADS);
  return (unsigned)(blocks < MF_STRIDE_BLOCKS ? blocks : MF_STRIDE_BLOCKS);
}

}  // namespace

extern "C" size_t bdm_mesh_fill_workspace_bytes(int b, long long sum_v, long long sum_f) {
  if (!mf_sizes_ok(b, sum_v, sum_f)) return 0;
  return mf_ws(nullptr, b, sum_v, sum_f).bytes;
}

extern "C" int bdm_mesh_fill_variant(int b, const long long *face_first) {
  if (b <= 0 || b > MESH_MAX_B || !face_first) return 0;
  long long max_f = 0;
  for (int m = 0; m < b; ++m) {
    const long long nf = face_first[m + 1] - face_first[m];
    max_f = nf > max_f ? nf : max_f;
  }
  if (max_f <= 0 || 6 * face_first[b] > INT_MAX) return 0;
  return 256 + mf_rounds(max_f);
}

extern "C" int bdm_mesh_boundary_loops(int b, int max_hole_edges, const float *verts, const int *faces, const long long *vert_first,
                                       const long long *face_first, int *halfedge_loop, int *loop_size, int *loop_flags, int *mesh_counts,
                                       void *workspace, void *stream) {
  BDM_REQUIRE(max_hole_edges >= 3 && max_hole_edges <= MF_MAX_EDGES, "mesh_boundary_loops: max_hole_edges=%d outside 3 .. %d", max_hole_edges,
              MF_MAX_EDGES);
  long long max_v = 0, max_f = 0;
  if (mf_check("mesh_boundary_loops", b, vert_first, face_first, workspace, max_v, max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b], H = 3 * sum_f;
  BDM_REQUIRE(verts && faces && halfedge_loop && loop_size && loop_flags && mesh_counts, "mesh_boundary_loops: an input or an output is NULL");
  const MfWs w = mf_ws(workspace, b, sum_v, sum_f);
  const Range in[2] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[5] = {{halfedge_loop, 4 * (size_t)H}, {loop_size, 4 * (size_t)H}, {loop_flags, 4 * (size_t)H},
                          {mesh_counts, 4 * MF_COUNTS * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap("mesh_boundary_loops", in, 2, out, 5) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  fill_ints(mesh_counts, (long long)MF_COUNTS * b, 0, st);
  fill_ints(w.pos, H + 1, 0, st);   // a batch without faces still leaves an empty compacted list behind for bdm_mesh_fill_holes
  if (max_f == 0) return launch_status("mesh_boundary_loops");
  const dim3 grid_h((unsigned)cdivll(3 * max_f, MF_THREADS), (unsigned)b);
  const dim3 block(MF_THREADS);
  build_incidence<MfKeys>(b, sum_v, max_f, faces, w.vert_first, w.face_first, w.first, w.cursor, w.bsum, w.rec, st);
  if (sum_v > 0) hipLaunchKernelGGL(mf_sort_kernel, dim3((unsigned)cdivll(sum_v, MF_THREADS)), block, 0, st, sum_v, w.first, w.rec);
  hipLaunchKernelGGL(mf_classify_kernel, grid_h, block, 0, st, faces, w.vert_first, w.face_first, H, w.first, w.rec, w.pos, halfedge_loop,
                     loop_size, loop_flags);
  exclusive_scan_ints(w.pos, H + 1, nullptr, w.bsum, st);
  hipLaunchKernelGGL(mf_compact_kernel, grid_h, block, 0, st, w.face_first, w.pos, w.bh, w.bm);
  const int *nb = w.pos + H;   // the length of the compacted list, on the device
  const dim3 grid_c(mf_stride_grid(sum_f));
  hipLaunchKernelGGL(mf_walk_kernel, grid_c, block, 0, st, faces, w.vert_first, w.face_first, w.first, w.rec, w.pos, nb, w.bh, w.bm, w.succ,
                     w.state_a);
  uint2 *from = w.state_a, *to = w.state_b;
  for (int r = 0, rounds = mf_rounds(max_f); r < rounds; ++r) {
    hipLaunchKernelGGL(mf_double_kernel, grid_c, block, 0, st, nb, from, to);
    uint2 *t = from;
    from = to, to = t;
  }
  hipLaunchKernelGGL(mf_label_kernel, grid_c, block, 0, st, faces, verts, w.vert_first, w.face_first, w.first, w.rec, w.pos, nb, w.bh, w.bm, from,
                     w.lab, halfedge_loop, loop_size, loop_flags, mesh_counts);
  hipLaunchKernelGGL(mf_decide_kernel, grid_c, block, 0, st, max_hole_edges, nb, w.bh, w.bm, w.lab, loop_size, loop_flags, w.wflag, w.wsize,
                     w.rankv, mesh_counts);
  hipLaunchKernelGGL(mf_face_flag_kernel, grid_c, block, 0, st, nb, w.bm, w.lab, w.wflag, w.rankf, mesh_counts);
  exclusive_scan_ints(w.rankv, H + 1, nb, w.bsum, st);
  exclusive_scan_ints(w.rankf, H + 1, nb, w.bsum, st);
  return launch_status("mesh_boundary_loops");
}

extern "C" int bdm_mesh_fill_holes(int b, int c, const float *verts, const float *attrs, const int *faces, const long long *vert_first,
                                   const long long *face_first, const long long *out_vert_first, const long long *out_face_first,
                                   float *verts_out, float *attrs_out, int *faces_out, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  const auto batch = [&] { return mf_check("mesh_fill_holes", b, vert_first, face_first, workspace, max_v, max_f); };
  const auto filled = [](long long nv, long long ov, long long nf, long long of) {
    return ov >= nv && ov - nv <= nf && of >= nf && of - nf <= 3 * nf && of - nf >= 3 * (ov - nv);
  };
  if (check_emit("mesh_fill_holes", "filled", b, c, vert_first, face_first, out_vert_first, out_face_first,
                 verts && attrs && faces && verts_out && attrs_out && faces_out, batch, filled) != BDM_OK)
    return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b], H = 3 * sum_f, out_v = out_vert_first[b], out_f = out_face_first[b];
  const MfWs w = mf_ws(workspace, b, sum_v, sum_f);
  const Range in[3] = {{verts, 12 * (size_t)sum_v}, {attrs, 4 * (size_t)c * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[4] = {{verts_out, 12 * (size_t)out_v}, {attrs_out, 4 * (size_t)c * (size_t)out_v}, {faces_out, 12 * (size_t)out_f},
                          {workspace, w.bytes}};
  if (check_overlap("mesh_fill_holes", in, 3, out, 4) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, out_vert_first, out_face_first, w.out_vert_first, w.out_face_first, st);
  const dim3 block(MF_THREADS);
  if (max_v > 0) {
    hipLaunchKernelGGL(mf_copy_kernel, dim3((unsigned)cdivll(3 * max_v, MF_THREADS), (unsigned)b), block, 0, st, 3, (const unsigned *)verts,
                       w.vert_first, w.out_vert_first, (unsigned *)verts_out);
    if (c > 0)
      hipLaunchKernelGGL(mf_copy_kernel, dim3((unsigned)cdivll(c * max_v, MF_THREADS), (unsigned)b), block, 0, st, c, (const unsigned *)attrs,
                         w.vert_first, w.out_vert_first, (unsigned *)attrs_out);
  }
  if (max_f == 0) return launch_status("mesh_fill_holes");
  hipLaunchKernelGGL(mf_copy_kernel, dim3((unsigned)cdivll(3 * max_f, MF_THREADS), (unsigned)b), block, 0, st, 3, (const unsigned *)faces,
                     w.face_first, w.out_face_first, (unsigned *)faces_out);
  if (out_v == sum_v || max_v == 0) return launch_status("mesh_fill_holes");   // nothing is filled
  fill_ints((int *)w.amax, 2 * (long long)b, 0, st);
  hipLaunchKernelGGL(mf_amax_kernel, dim3((unsigned)cdivll(max_v, MF_THREADS), (unsigned)b), block, 0, st, c, verts, attrs, w.vert_first, w.amax);
  const int *nb = w.pos + H;
  const dim3 grid_c(mf_stride_grid(sum_f));
  hipLaunchKernelGGL(mf_mean_kernel, grid_c, block, 0, st, c, faces, verts, attrs, w.vert_first, w.face_first, w.out_vert_first, w.pos, nb, w.bh,
                     w.bm, w.succ, w.lab, w.wflag, w.wsize, w.rankv, w.amax, verts_out, attrs_out);
  hipLaunchKernelGGL(mf_emit_kernel, grid_c, block, 0, st, faces, w.vert_first, w.face_first, w.out_face_first, w.pos, nb, w.bh, w.bm, w.lab,
                     w.rankv, w.rankf, faces_out);
  return launch_status("mesh_fill_holes");
}
