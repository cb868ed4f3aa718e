// mesh_qem.hip -- quadric edge-collapse decimation of a packed batch of triangle meshes in rounds (Open3D's simplify_quadric_decimation
// by name and meaning) as gfx950 kernels (bdm_hip.h section 23; the rule is this project's own text, restated by
// tests/mesh_qem_ref.py).
//
// The rule in one paragraph: every vertex carries the area-weighted plane quadrics of its faces and of the planes that stand on its
// boundary edges.  A round rebuilds the vertex incidence of the live faces, gives every regular edge a target (the quadric's optimum
// by Cramer's rule, else the cheapest of the two ends and the midpoint), a cost and a validity, and collapses every valid edge whose
// key (cost bits << 32 | lowest half-edge index) is the minimum over the edges at its two ends and at all their neighbours.  Such
// edges neither share nor neighbour an endpoint, so their collapses touch disjoint vertices and faces and commute.  Everything that
// decides is float64, one operation at a time (this object is built without contraction); nothing depends on execution order:
// per-vertex minima are gathered over the sorted incidence segments, counts are integer sums.
//
// Kernels (one thread per vertex, per half-edge or per mesh; gridDim.y = the mesh; a stopped mesh leaves at the top).
//   (ragged.h)            send_offsets: the host offset arrays and the targets travel as launch arguments.
//   (mesh_incidence.h)    fill_ints, exclusive_scan_ints, build_incidence<QRec>, sort_segment, connected_face.
//   q_state_kernel        the per-mesh counters of section 23 set up.  q_init_vert_kernel / q_init_face_kernel: the working copies.
//   q_sort_kernel         a vertex sorts its segment (records neighbour << 32 | half-edge << 1 | direction) and notes its neighbour
//                         count, whether it is on the boundary and whether an irregular edge ends at it.
//   q_quadric_kernel      the initial quadric of a vertex, its terms in ascending (face, kind).
//   q_edge_kernel         the thread of an edge's lowest half-edge: rules 1 - 3 -> its key, or the all-ones key and a counted reason.
//   q_m1_kernel / q_m2_kernel   the minimum key at a vertex; the minimum of those over the vertex and its neighbours.
//   q_select_kernel       selected = key == m2 at both ends.  q_apply_kernel: rule 5, by the selected edge's thread.
//   q_begin_kernel / q_end_kernel / q_report_kernel   the per-round counters, the stopping rule, the read-back.
//   q_root_kernel ... q_face_out_kernel   finish: chains resolved, survivors ranked, members gathered, rows written, over
//                         mesh_emit.h's member_flag / member_place / build_member_segments, amax_clear_kernel / attr_amax_kernel
//                         and FixedMean.
// A one-workgroup form that keeps a small mesh's rounds in LDS is not offered: it was not measured, so it is left out.
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

#define Q_THREADS MESH_THREADS
#define Q_COUNTS 20   // per-mesh counters, in the order of bdm_hip.h section 23
#define Q_MAX_ROUNDS (1 << 20)
#define Q_INVALID 0xffffffffffffffffull
#define Q_BAD (-3)
#define Q_COLLAPSED (-1)
#define Q_BOUNDARY_BIT (1 << 30)
#define Q_IRREGULAR_BIT (1 << 29)
#define Q_NEIGHBOURS 0xffffff

namespace {

typedef unsigned long long q_key;

enum { S_STOP, S_ROUNDS, S_COLLAPSES, S_FACES_IN, S_FACES, S_VERTS_IN, S_VERTS, S_LOCKED, S_BAD, S_MAXCOST, S_SELECTED, S_CANDIDATES, S_REJECT,
       S_TARGET = S_REJECT + 7 };
enum { R_NONMANIFOLD, R_LOCKED, R_COST, R_LINK, R_BOUNDARY, R_VALENCE, R_FLIP, R_NONE };

struct QRec {
  typedef q_key type;
  // corner c of face i: the half-edge that leaves the vertex and the one that arrives
  __device__ static void corner(const int (&idx)[3], int i, int c, q_key &r0, q_key &r1) {
    const int n = c == 2 ? 0 : c + 1, p = c == 0 ? 2 : c - 1;
    r0 = ((q_key)(unsigned)idx[n] << 32) | ((q_key)(unsigned)(3 * i + c) << 1);
    r1 = ((q_key)(unsigned)idx[p] << 32) | ((q_key)(unsigned)(3 * i + p) << 1) | 1ull;
  }
};

__device__ __forceinline__ int rec_nbr(q_key r) { return (int)(r >> 32); }
__device__ __forceinline__ int rec_he(q_key r) { return (int)((unsigned)r >> 1); }

struct Run {
  int nbr, out, in, minhe, begin, end;
};
// the run that starts at s[at] -> the position behind it
__device__ __forceinline__ int read_run(const q_key *__restrict__ s, int len, int at, Run &r) {
  r.nbr = rec_nbr(s[at]), r.out = r.in = 0, r.minhe = INT_MAX, r.begin = at;
  for (; at < len && rec_nbr(s[at]) == r.nbr; ++at) {
    if (s[at] & 1ull) ++r.in;
    else ++r.out;
    r.minhe = min(r.minhe, rec_he(s[at]));
  }
  r.end = at;
  return at;
}
__device__ __forceinline__ bool find_run(const q_key *__restrict__ s, int len, int nbr, Run &r) {
  for (int at = 0; at < len;) {
    at = read_run(s, len, at, r);
    if (r.nbr == nbr) return true;
  }
  return false;
}
__device__ __forceinline__ bool regular(const Run &r) { return (r.out == 1 && r.in <= 1) || (r.out == 0 && r.in == 1); }

// ---- float64, one operation at a time, in the order of the header -------------------------------------------------------------------------
struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 load3(const float *__restrict__ p) { return D3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ D3 q_normal(const D3 &p0, const D3 &p1, const D3 &p2) {
  const double ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const double bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  return D3{ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
}
__device__ __forceinline__ double q_dot(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool q_positive_finite(double v) { return v > 0.0 && v < (double)INFINITY; }

__device__ __forceinline__ void add_plane(double *__restrict__ q, const D3 &n, double d, double s) {
  q[0] += (n.x * n.x) * s, q[1] += (n.x * n.y) * s, q[2] += (n.x * n.z) * s, q[3] += (n.x * d) * s;
  q[4] += (n.y * n.y) * s, q[5] += (n.y * n.z) * s, q[6] += (n.y * d) * s;
  q[7] += (n.z * n.z) * s, q[8] += (n.z * d) * s, q[9] += (d * d) * s;
}

__device__ __forceinline__ double q_error(const double *__restrict__ q, const D3 &v) {
  const double a = ((q[0] * v.x) * v.x + (q[4] * v.y) * v.y) + (q[7] * v.z) * v.z;
  const double b = ((q[1] * v.x) * v.y + (q[2] * v.x) * v.z) + (q[5] * v.y) * v.z;
  const double c = (q[3] * v.x + q[6] * v.y) + q[8] * v.z;
  return ((a + 2.0 * b) + 2.0 * c) + q[9];
}
__device__ __forceinline__ double q_clamp(double e) { return e > 0.0 ? e : (e == e ? 0.0 : e); }

// rule 2 -> the cost; t the float64 target
__device__ __forceinline__ double q_target(const double *__restrict__ q, const D3 &pa, const D3 &pb, D3 &t) {
  const double c00 = q[4] * q[7] - q[5] * q[5];
  const double c01 = q[1] * q[7] - q[5] * q[2];
  const double c02 = q[1] * q[5] - q[4] * q[2];
  const double det = (q[0] * c00 - q[1] * c01) + q[2] * c02;
  const double tr = (q[0] + q[4]) + q[7];
  const D3 mid{(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
  const double dx = pb.x - pa.x, dy = pb.y - pa.y, dz = pb.z - pa.z;
  const double len2 = (dx * dx + dy * dy) + dz * dz;
  if (fabs(det) > 0x1p-40 * ((tr * tr) * tr)) {
    const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
    const double m0 = r1 * q[7] - q[5] * r2;
    const double m1 = r1 * q[5] - q[4] * r2;
    const double m2 = q[1] * r2 - r1 * q[2];
    const D3 o{((r0 * c00 - q[1] * m0) + q[2] * m1) / det, ((q[0] * m0 - r0 * c01) + q[2] * m2) / det,
               ((r0 * c02 - q[0] * m1) - q[1] * m2) / det};
    const double ox = o.x - mid.x, oy = o.y - mid.y, oz = o.z - mid.z;
    if ((ox * ox + oy * oy) + oz * oz <= len2) {
      t = o;
      return q_clamp(q_error(q, o));
    }
  }
  t = pa;
  double cost = q_clamp(q_error(q, pa));
  const double cb = q_clamp(q_error(q, pb));
  if (cb < cost) t = pb, cost = cb;
  const double cm = q_clamp(q_error(q, mid));
  if (cm < cost) t = mid, cost = cm;
  return cost;
}

// ---- init ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(Q_THREADS) void q_state_kernel(int b, const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                            const long long *__restrict__ target, int *__restrict__ state) {
  const int m = blockIdx.x * Q_THREADS + threadIdx.x;
  if (m >= b) return;
  int *s = state + Q_COUNTS * m;
  for (int k = 0; k < Q_COUNTS; ++k) s[k] = 0;
  s[S_VERTS_IN] = s[S_VERTS] = (int)(vert_first[m + 1] - vert_first[m]);
  s[S_FACES_IN] = (int)(face_first[m + 1] - face_first[m]);
  s[S_TARGET] = (int)target[m];
}

__global__ __launch_bounds__(Q_THREADS) void q_init_vert_kernel(const float *__restrict__ verts, const long long *__restrict__ vert_first,
                                                                float *__restrict__ pos, int *__restrict__ vlive, int *__restrict__ locked,
                                                                int *__restrict__ parent) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv) return;
  const long long g = vbase + i;
  const float *p = verts + 3 * (size_t)g;
  for (int d = 0; d < 3; ++d) pos[3 * (size_t)g + d] = p[d];
  vlive[g] = 1, parent[g] = (int)i;
  locked[g] = fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY ? 0 : 1;
}

__global__ __launch_bounds__(Q_THREADS) void q_init_face_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                const long long *__restrict__ face_first, int *__restrict__ wfaces,
                                                                int *__restrict__ fcode, int *__restrict__ locked, int *__restrict__ state) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * Q_THREADS >= nf) return;   // the whole workgroup
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  int ok = 0, bad = 0;
  if (i < nf) {
    int idx[3];
    ok = connected_face(faces, fbase + i, nv, idx) ? 1 : 0;
    bad = 1 - ok;
    int *o = wfaces + 3 * (size_t)(fbase + i);
    for (int k = 0; k < 3; ++k) {
      o[k] = ok ? idx[k] : -1;
      if (!ok && idx[k] >= 0 && idx[k] < nv) locked[vbase + idx[k]] = 1;
    }
    fcode[fbase + i] = ok ? 0 : Q_BAD;
  }
  const int n_ok = __syncthreads_count(ok), n_bad = __syncthreads_count(bad);
  if (threadIdx.x == 0 && n_ok) atomicAdd(state + Q_COUNTS * m + S_FACES, n_ok);
  if (threadIdx.x == 1 && n_bad) atomicAdd(state + Q_COUNTS * m + S_BAD, n_bad);
}

// a vertex sorts its segment; vinfo = neighbours | boundary | irregular
__global__ __launch_bounds__(Q_THREADS) void q_sort_kernel(const long long *__restrict__ vert_first, const int *__restrict__ state,
                                                           const int *__restrict__ first, q_key *__restrict__ rec, int *__restrict__ vinfo) {
  const int m = blockIdx.y;
  if (state[Q_COUNTS * m + S_STOP]) return;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv) return;
  const long long g = vbase + i;
  q_key *s = rec + first[g];
  const int len = first[g + 1] - first[g];
  sort_segment(s, len);
  int info = 0;
  Run r;
  for (int at = 0; at < len;) {
    at = read_run(s, len, at, r);
    ++info;
    if (r.out + r.in == 1) info |= Q_BOUNDARY_BIT;
    if (!regular(r)) info |= Q_IRREGULAR_BIT;
  }
  vinfo[g] = info;
}

// face `f` of the mesh -> its normal and area; false when the float64 normal is zero or not finite
__device__ __forceinline__ bool q_face(const int *__restrict__ wfaces, const float *__restrict__ pos, long long fbase, long long vbase, int f,
                                       int (&idx)[3], D3 (&p)[3], D3 &n, double &l2, double &area) {
  const int *fp = wfaces + 3 * (size_t)(fbase + f);
  for (int k = 0; k < 3; ++k) idx[k] = fp[k], p[k] = load3(pos + 3 * (size_t)(vbase + idx[k]));
  n = q_normal(p[0], p[1], p[2]);
  l2 = q_dot(n, n);
  if (!q_positive_finite(l2)) return false;
  area = 0.5 * sqrt(l2);
  return true;
}

__global__ __launch_bounds__(Q_THREADS) void q_quadric_kernel(double weight, const long long *__restrict__ vert_first,
                                                              const long long *__restrict__ face_first, const int *__restrict__ wfaces,
                                                              const float *__restrict__ pos, const int *__restrict__ first,
                                                              const q_key *__restrict__ rec, const int *__restrict__ locked,
                                                              double *__restrict__ quad, int *__restrict__ state) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * Q_THREADS >= nv) return;
  int is_locked = 0;
  if (i < nv) {
    const long long g = vbase + i, fbase = face_first[m];
    is_locked = locked[g];
    const q_key *s = rec + first[g];
    const int len = first[g + 1] - first[g];
    double q[10];
    for (int k = 0; k < 10; ++k) q[k] = 0.0;
    for (int last = -1;;) {   // the faces around the vertex in ascending index: one pass over the segment per face
      int f = INT_MAX, c = 0;
      for (int t = 0; t < len; ++t) {
        if (s[t] & 1ull) continue;
        const int he = rec_he(s[t]);
        if (he / 3 > last && he / 3 < f) f = he / 3, c = he % 3;
      }
      if (f == INT_MAX) break;
      last = f;
      int idx[3];
      D3 p[3], n;
      double l2, area;
      if (!q_face(wfaces, pos, fbase, vbase, f, idx, p, n, l2, area)) continue;
      add_plane(q, n, -q_dot(n, p[0]), area / l2);
      for (int side = 0; side < 2; ++side) {   // the half-edge that leaves the vertex, then the one that arrives
        const int e = side == 0 ? c : (c + 2) % 3, e1 = (e + 1) % 3;
        Run r;
        if (!find_run(s, len, side == 0 ? idx[e1] : idx[e], r) || r.out + r.in != 1) continue;
        const double ex = p[e1].x - p[e].x, ey = p[e1].y - p[e].y, ez = p[e1].z - p[e].z;
        const D3 mn{ey * n.z - ez * n.y, ez * n.x - ex * n.z, ex * n.y - ey * n.x};
        const double ml2 = q_dot(mn, mn);
        if (!q_positive_finite(ml2)) continue;
        add_plane(q, mn, -q_dot(mn, p[e]), (weight * area) / ml2);
      }
    }
    for (int k = 0; k < 10; ++k) quad[10 * (size_t)g + k] = q[k];
  }
  const int n_locked = __syncthreads_count(is_locked);
  if (threadIdx.x == 0 && n_locked) atomicAdd(state + Q_COUNTS * m + S_LOCKED, n_locked);
}

__global__ __launch_bounds__(Q_THREADS) void q_stop0_kernel(int b, int *__restrict__ state) {
  const int m = blockIdx.x * Q_THREADS + threadIdx.x;
  if (m >= b) return;
  int *s = state + Q_COUNTS * m;
  if (s[S_FACES] <= s[S_TARGET]) s[S_STOP] = 1;
}

// ---- a round --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(Q_THREADS) void q_begin_kernel(int b, int *__restrict__ state) {
  const int m = blockIdx.x * Q_THREADS + threadIdx.x;
  if (m >= b) return;
  int *s = state + Q_COUNTS * m;
  if (s[S_STOP]) return;
  s[S_SELECTED] = s[S_CANDIDATES] = 0;
  for (int k = 0; k < 7; ++k) s[S_REJECT + k] = 0;
}

// rules 1 - 3 for the edge whose lowest half-edge is h = a -> b of face f -> the reason, or R_NONE with the key
__device__ __forceinline__ int q_evaluate(double maximum_error, long long vbase, long long fbase, const int *__restrict__ wfaces,
                                          const float *__restrict__ pos, const double *__restrict__ quad, const int *__restrict__ first,
                                          const q_key *__restrict__ rec, const int *__restrict__ vinfo, const int *__restrict__ locked,
                                          int h, int a, int b, const Run &run, q_key &key, float (&t32)[3]) {
  const int lo = min(a, b), hi = max(a, b);
  const long long gl = vbase + lo, gh = vbase + hi;
  if (!regular(run) || ((vinfo[gl] | vinfo[gh]) & Q_IRREGULAR_BIT)) return R_NONMANIFOLD;
  if (locked[gl] | locked[gh]) return R_LOCKED;
  double q[10];
  for (int k = 0; k < 10; ++k) q[k] = quad[10 * (size_t)gl + k] + quad[10 * (size_t)gh + k];
  const D3 pl = load3(pos + 3 * (size_t)gl), ph = load3(pos + 3 * (size_t)gh);
  D3 t;
  const double cost = q_target(q, pl, ph, t);
  const float fc = (float)cost;
  if (!(cost <= maximum_error && fc < INFINITY)) return R_COST;
  t32[0] = (float)t.x, t32[1] = (float)t.y, t32[2] = (float)t.z;
  const D3 tt{(double)t32[0], (double)t32[1], (double)t32[2]};
  const bool interior = run.out + run.in == 2;
  const q_key *sl = rec + first[gl], *sh = rec + first[gh], *sa = rec + first[vbase + a];
  const int ll = first[gl + 1] - first[gl], lh = first[gh + 1] - first[gh];
  int common = 0;
  for (int i = 0, j = 0; i < ll && j < lh;) {
    const int x = rec_nbr(sl[i]), y = rec_nbr(sh[j]);
    if (x < y) ++i;
    else if (y < x) ++j;
    else {
      ++common;
      while (i < ll && rec_nbr(sl[i]) == x) ++i;
      while (j < lh && rec_nbr(sh[j]) == x) ++j;
    }
  }
  if (common != (interior ? 2 : 1)) return R_LINK;
  if (interior && (vinfo[gl] & vinfo[gh] & Q_BOUNDARY_BIT)) return R_BOUNDARY;
  for (int at = run.begin; at < run.end; ++at) {   // the run of b in a's segment: the one or two faces at the edge
    const int *fp = wfaces + 3 * (size_t)(fbase + rec_he(sa[at]) / 3);
    const int c = fp[0] != a && fp[0] != b ? fp[0] : (fp[1] != a && fp[1] != b ? fp[1] : fp[2]);
    const int info = vinfo[vbase + c];
    if ((info & Q_NEIGHBOURS) < ((info & Q_BOUNDARY_BIT) ? 3 : 4)) return R_VALENCE;
  }
  for (int side = 0; side < 2; ++side) {
    const int other = side == 0 ? hi : lo;
    const q_key *s = side == 0 ? sl : sh;
    const int len = side == 0 ? ll : lh;
    for (int at = 0; at < len; ++at) {
      if (s[at] & 1ull) continue;
      const int he = rec_he(s[at]), c = he % 3;
      const int *fp = wfaces + 3 * (size_t)(fbase + he / 3);
      if (fp[0] == other || fp[1] == other || fp[2] == other) continue;
      D3 p[3];
      for (int k = 0; k < 3; ++k) p[k] = load3(pos + 3 * (size_t)(vbase + fp[k]));
      const D3 old = q_normal(p[0], p[1], p[2]);
      p[c] = tt;
      if (!(q_dot(q_normal(p[0], p[1], p[2]), old) > 0.0)) return R_FLIP;
    }
  }
  key = ((q_key)__float_as_uint(fc) << 32) | (q_key)(unsigned)h;
  return R_NONE;
}

// the half-edge i of the mesh -> (a, b) and the run of b in a's segment; false for a dead face or a half-edge that is not its edge's lowest
__device__ __forceinline__ bool q_owner(long long vbase, long long fbase, const int *__restrict__ wfaces, const int *__restrict__ first,
                                        const q_key *__restrict__ rec, long long i, int &a, int &b, Run &run) {
  const int *fp = wfaces + 3 * (size_t)(fbase + i / 3);
  const int c = (int)(i % 3);
  a = fp[c], b = fp[c == 2 ? 0 : c + 1];
  if (a < 0) return false;
  const long long g = vbase + a;
  return find_run(rec + first[g], first[g + 1] - first[g], b, run) && run.minhe == i;
}

__global__ __launch_bounds__(Q_THREADS) void q_edge_kernel(double maximum_error, const long long *__restrict__ vert_first,
                                                           const long long *__restrict__ face_first, const int *__restrict__ wfaces,
                                                           const float *__restrict__ pos, const double *__restrict__ quad,
                                                           const int *__restrict__ first, const q_key *__restrict__ rec,
                                                           const int *__restrict__ vinfo, const int *__restrict__ locked,
                                                           q_key *__restrict__ key, int *__restrict__ state) {
  __shared__ int part[8];   // seven reasons, the candidates
  const int m = blockIdx.y;
  if (state[Q_COUNTS * m + S_STOP]) return;
  const long long fbase = face_first[m], nh = 3 * (face_first[m + 1] - fbase);
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * Q_THREADS >= nh) return;
  if (threadIdx.x < 8) part[threadIdx.x] = 0;
  __syncthreads();
  if (i < nh) {
    const long long vbase = vert_first[m];
    int a, b;
    Run run;
    q_key k = Q_INVALID;
    if (q_owner(vbase, fbase, wfaces, first, rec, i, a, b, run)) {
      float t32[3];
      const int why = q_evaluate(maximum_error, vbase, fbase, wfaces, pos, quad, first, rec, vinfo, locked, (int)i, a, b, run, k, t32);
      atomicAdd(part + 7, 1);
      if (why != R_NONE) atomicAdd(part + why, 1);
    }
    key[3 * fbase + i] = k;
  }
  __syncthreads();
  if (threadIdx.x < 7 && part[threadIdx.x]) atomicAdd(state + Q_COUNTS * m + S_REJECT + threadIdx.x, part[threadIdx.x]);
  if (threadIdx.x == 7 && part[7]) atomicAdd(state + Q_COUNTS * m + S_CANDIDATES, part[7]);
}

// HOP = false: m1[v] = the minimum key over the edges at v.  HOP = true: out[v] = the minimum of in over v and its neighbours.
template <bool HOP>
__global__ __launch_bounds__(Q_THREADS) void q_min_kernel(const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                          const int *__restrict__ state, const int *__restrict__ first,
                                                          const q_key *__restrict__ rec, const q_key *__restrict__ in, q_key *__restrict__ out) {
  const int m = blockIdx.y;
  if (state[Q_COUNTS * m + S_STOP]) return;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv) return;
  const long long g = vbase + i, hbase = 3 * face_first[m];
  const q_key *s = rec + first[g];
  const int len = first[g + 1] - first[g];
  q_key best = HOP ? in[g] : Q_INVALID;
  Run r;
  for (int at = 0; at < len;) {
    at = read_run(s, len, at, r);
    const q_key k = HOP ? in[vbase + r.nbr] : in[hbase + r.minhe];
    best = k < best ? k : best;
  }
  out[g] = best;
}

__global__ __launch_bounds__(Q_THREADS) void q_select_kernel(const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                             const int *__restrict__ wfaces, const q_key *__restrict__ key,
                                                             const q_key *__restrict__ m2, int *__restrict__ sel, int *__restrict__ state) {
  __shared__ int top;
  const int m = blockIdx.y;
  if (state[Q_COUNTS * m + S_STOP]) return;
  const long long fbase = face_first[m], nh = 3 * (face_first[m + 1] - fbase);
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if ((long long)blockIdx.x * Q_THREADS >= nh) return;
  if (threadIdx.x == 0) top = 0;
  __syncthreads();
  int chosen = 0;
  if (i < nh) {
    const q_key k = key[3 * fbase + i];
    if (k != Q_INVALID) {   // the face of a key is live
      const int *fp = wfaces + 3 * (size_t)(fbase + i / 3);
      const int c = (int)(i % 3);
      const long long vbase = vert_first[m];
      chosen = k == m2[vbase + fp[c]] && k == m2[vbase + fp[c == 2 ? 0 : c + 1]] ? 1 : 0;
      if (chosen) atomicMax(&top, (int)(k >> 32));   // the bits of a non-negative float order as integers
    }
    sel[3 * fbase + i] = chosen;
  }
  const int n = __syncthreads_count(chosen);
  if (threadIdx.x == 0 && n) {
    atomicAdd(state + Q_COUNTS * m + S_SELECTED, n);
    atomicMax(state + Q_COUNTS * m + S_MAXCOST, top);
  }
}

__global__ __launch_bounds__(Q_THREADS) void q_apply_kernel(const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                            const int *__restrict__ sel, const int *__restrict__ first,
                                                            const q_key *__restrict__ rec, int *__restrict__ wfaces, float *__restrict__ pos,
                                                            double *__restrict__ quad, int *__restrict__ vlive, int *__restrict__ parent,
                                                            int *__restrict__ state) {
  const int m = blockIdx.y;
  if (state[Q_COUNTS * m + S_STOP]) return;
  const long long fbase = face_first[m], nh = 3 * (face_first[m + 1] - fbase);
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nh || !sel[3 * fbase + i]) return;
  const long long vbase = vert_first[m];
  const int *fp = wfaces + 3 * (size_t)(fbase + i / 3);   // no other selected edge touches this face
  const int c = (int)(i % 3), a = fp[c], b = fp[c == 2 ? 0 : c + 1];
  const int lo = min(a, b), hi = max(a, b);
  const long long gl = vbase + lo, gh = vbase + hi;
  double q[10];
  for (int k = 0; k < 10; ++k) q[k] = quad[10 * (size_t)gl + k] + quad[10 * (size_t)gh + k];
  D3 t;
  q_target(q, load3(pos + 3 * (size_t)gl), load3(pos + 3 * (size_t)gh), t);
  pos[3 * (size_t)gl + 0] = (float)t.x, pos[3 * (size_t)gl + 1] = (float)t.y, pos[3 * (size_t)gl + 2] = (float)t.z;
  for (int k = 0; k < 10; ++k) quad[10 * (size_t)gl + k] = q[k];
  vlive[gh] = 0, parent[gh] = lo;
  const q_key *s = rec + first[gh];
  const int len = first[gh + 1] - first[gh];
  int died = 0;
  for (int at = 0; at < len; ++at) {
    if (s[at] & 1ull) continue;
    const int he = rec_he(s[at]);
    int *o = wfaces + 3 * (size_t)(fbase + he / 3);
    if (o[0] == lo || o[1] == lo || o[2] == lo) o[0] = o[1] = o[2] = -1, ++died;
    else o[he % 3] = lo;
  }
  int *st = state + Q_COUNTS * m;
  atomicAdd(st + S_FACES, -died), atomicAdd(st + S_VERTS, -1), atomicAdd(st + S_COLLAPSES, 1);
}

__global__ __launch_bounds__(Q_THREADS) void q_end_kernel(int b, int max_rounds, int *__restrict__ state) {
  const int m = blockIdx.x * Q_THREADS + threadIdx.x;
  if (m >= b) return;
  int *s = state + Q_COUNTS * m;
  if (s[S_STOP]) return;
  s[S_ROUNDS] += 1;
  if (s[S_FACES] <= s[S_TARGET]) s[S_STOP] = 1;
  else if (s[S_SELECTED] == 0) s[S_STOP] = 2;
  else if (s[S_ROUNDS] >= max_rounds) s[S_STOP] = 3;
}

// mesh_counts = the state; *active (zeroed before) = the meshes still running
__global__ __launch_bounds__(Q_THREADS) void q_report_kernel(int b, const int *__restrict__ state, int *__restrict__ mesh_counts,
                                                             int *__restrict__ active) {
  const int m = blockIdx.x * Q_THREADS + threadIdx.x;
  int running = 0;
  if (m < b) {
    for (int k = 0; k < Q_COUNTS; ++k) mesh_counts[Q_COUNTS * m + k] = state[Q_COUNTS * m + k];
    running = state[Q_COUNTS * m + S_STOP] == 0 ? 1 : 0;
  }
  const int n = __syncthreads_count(running);
  if (threadIdx.x == 0 && n && active) atomicAdd(active, n);
}

// ---- finish -------------------------------------------------------------------------------------------------------------------------------
// member_flag at the survivor the vertex's chain ends in (a survivor, and no other vertex, is its own parent)
__global__ __launch_bounds__(Q_THREADS) void q_root_kernel(const long long *__restrict__ vert_first, const int *__restrict__ parent,
                                                           int *__restrict__ root, int *__restrict__ rank, int *__restrict__ seg) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv) return;
  int r = (int)i;
  for (long long step = 0; step < nv && parent[vbase + r] != r; ++step) r = parent[vbase + r];   // a chain descends: it ends
  member_flag(vbase, i, r, root, rank, seg);
}

__global__ __launch_bounds__(Q_THREADS) void q_face_flag_kernel(const long long *__restrict__ face_first, const int *__restrict__ wfaces,
                                                                int *__restrict__ frank) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i < nf) frank[fbase + i] = wfaces[3 * (size_t)(fbase + i)] >= 0 ? 1 : 0;
}

// member_place for every vertex
__global__ __launch_bounds__(Q_THREADS) void q_member_kernel(const long long *__restrict__ vert_first, const int *__restrict__ root,
                                                             const int *__restrict__ rank, const int *__restrict__ seg,
                                                             int *__restrict__ cursor, int *__restrict__ member, int *__restrict__ vert_map) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv) return;
  member_place(vbase, i, root, rank, seg, cursor, member, vert_map);
}

// one thread per survivor: its position's bits, and its attribute row: a copy, or the fixed-point mean over its members
__global__ __launch_bounds__(Q_THREADS) void q_vertex_out_kernel(int c, const float *__restrict__ attrs, const long long *__restrict__ vert_first,
                                                                 const long long *__restrict__ out_vert_first, const float *__restrict__ pos,
                                                                 const int *__restrict__ vlive, const int *__restrict__ rank,
                                                                 const int *__restrict__ seg, const int *__restrict__ member,
                                                                 const unsigned *__restrict__ amax, float *__restrict__ verts_out,
                                                                 float *__restrict__ attrs_out) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nv || !vlive[vbase + i]) return;
  const long long g = vbase + i, row = rank[g] - rank[vbase];
  if (row >= out_vert_first[m + 1] - out_vert_first[m]) return;
  unsigned *o = (unsigned *)verts_out + 3 * (size_t)(out_vert_first[m] + row);
  unsigned *oa = (unsigned *)attrs_out + (size_t)c * (size_t)(out_vert_first[m] + row);
  const unsigned *p = (const unsigned *)pos + 3 * (size_t)g;
  for (int d = 0; d < 3; ++d) o[d] = p[d];
  const int size = seg[g + 1] - seg[g];
  if (size <= 1) {
    const unsigned *q = (const unsigned *)attrs + (size_t)c * (size_t)g;
    for (int d = 0; d < c; ++d) oa[d] = q[d];
    return;
  }
  const int *mem = member + seg[g];
  for (int d = 0; d < c; ++d) {   // channel by channel: one sum in registers; the segment's order depends on arrival, integer sums do not
    FixedMean<1, true> mean(amax[m]);
    for (int t = 0; t < size; ++t) mean.add(attrs + (size_t)c * (size_t)(vbase + mem[t]) + d, 1);
    mean.write((float *)oa + d, 1, (double)size);
  }
}

// frank is scanned: face_map, and the rows of the surviving faces through the ranks of their (live) vertices
__global__ __launch_bounds__(Q_THREADS) void q_face_out_kernel(const long long *__restrict__ vert_first, const long long *__restrict__ face_first,
                                                               const long long *__restrict__ out_face_first, const int *__restrict__ wfaces,
                                                               const int *__restrict__ fcode, const int *__restrict__ rank,
                                                               const int *__restrict__ frank, int *__restrict__ face_map,
                                                               int *__restrict__ faces_out) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * Q_THREADS + threadIdx.x;
  if (i >= nf) return;
  const int *fp = wfaces + 3 * (size_t)(fbase + i);
  if (fp[0] < 0) {
    face_map[fbase + i] = fcode[fbase + i] == Q_BAD ? Q_BAD : Q_COLLAPSED;
    return;
  }
  const long long row = frank[fbase + i] - frank[fbase], vbase = vert_first[m];
  face_map[fbase + i] = (int)row;
  if (row >= out_face_first[m + 1] - out_face_first[m]) return;
  int *o = faces_out + 3 * (size_t)(out_face_first[m] + row);
  for (int k = 0; k < 3; ++k) o[k] = rank[vbase + fp[k]] - rank[vbase];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool q_sizes_ok(int b, long long sum_v, long long sum_f) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_f >= 0 && sum_v < INT_MAX && 6 * sum_f < INT_MAX;
}

// offsets | output offsets | targets | state (20 b) | amax (b) | pos (3 sum V floats) | quadrics (10 sum V doubles) | m1, m2 (sum V keys) |
// vlive, locked, parent, vinfo, root, member (sum V each) | first, cursor, rank, seg (sum V + 1 each) | working faces (3 sum F) |
// fcode (sum F) | frank (sum F + 1) | records (6 sum F keys) | keys (3 sum F) | selected (3 sum F) | partial sums
struct QWs {
  long long *vert_first, *face_first, *out_vert_first, *out_face_first, *target;
  int *state;
  unsigned *amax;
  float *pos;
  double *quad;
  q_key *m1, *m2, *rec, *key;
  int *vlive, *locked, *parent, *vinfo, *root, *member, *first, *cursor, *rank, *seg, *wfaces, *fcode, *frank, *sel, *bsum;
  size_t bytes;
};
QWs q_ws(void *ws, int b, long long sum_v, long long sum_f) {
  Carve c{(char *)ws, 0};
  QWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.out_vert_first = c.take_offsets(b), w.out_face_first = w.out_vert_first + (b + 1);
  w.target = c.take_offsets(b);
  w.state = c.take<int>(Q_COUNTS * (size_t)b);
  w.amax = c.take<unsigned>((size_t)b);
  w.pos = c.take<float>(3 * (size_t)sum_v);
  w.quad = c.take<double>(10 * (size_t)sum_v);
  w.m1 = c.take<q_key>((size_t)sum_v), w.m2 = c.take<q_key>((size_t)sum_v);
  int **per_v[6] = {&w.vlive, &w.locked, &w.parent, &w.vinfo, &w.root, &w.member};
  for (int i = 0; i < 6; ++i) *per_v[i] = c.take<int>((size_t)sum_v);
  int **per_v1[4] = {&w.first, &w.cursor, &w.rank, &w.seg};
  for (int i = 0; i < 4; ++i) *per_v1[i] = c.take<int>((size_t)sum_v + 1);
  w.wfaces = c.take<int>(3 * (size_t)sum_f);
  w.fcode = c.take<int>((size_t)sum_f);
  w.frank = c.take<int>((size_t)sum_f + 1);
  w.rec = c.take<q_key>(6 * (size_t)sum_f);
  w.key = c.take<q_key>(3 * (size_t)sum_f);
  w.sel = c.take<int>(3 * (size_t)sum_f);
  w.bsum = c.take<int>((size_t)scan_blocks((sum_v > sum_f ? sum_v : sum_f) + 1));
  w.bytes = c.o;
  return w;
}

// the checks the three entry points share -> BDM_OK with the largest per-mesh counts
int q_check(const char *what, int b, const long long *vert_first, const long long *face_first, const void *workspace, long long &max_v,
            long long &max_f) {
  if (check_mesh_batch(what, b, vert_first, face_first, true, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_first[b] < INT_MAX && 6 * face_first[b] < INT_MAX, "%s: %lld vertices or %lld faces (six records each) reach 2^31", what,
              vert_first[b], face_first[b]);
  return check_workspace(what, workspace);
}

}  // namespace

extern "C" size_t bdm_mesh_qem_workspace_bytes(int b, long long sum_v, long long sum_f) {
  if (!q_sizes_ok(b, sum_v, sum_f)) return 0;
  return q_ws(nullptr, b, sum_v, sum_f).bytes;
}

extern "C" int bdm_mesh_qem_layout(int b, long long sum_v, long long sum_f, long long *offsets) {
  BDM_REQUIRE(q_sizes_ok(b, sum_v, sum_f) && offsets, "mesh_qem_layout: sizes outside the limits, or offsets is NULL");
  const QWs w = q_ws(nullptr, b, sum_v, sum_f);
  const void *piece[6] = {w.pos, w.quad, w.vlive, w.wfaces, w.key, w.sel};
  for (int k = 0; k < 6; ++k) offsets[k] = (long long)((const char *)piece[k] - (const char *)nullptr);
  return BDM_OK;
}

extern "C" int bdm_mesh_qem_init(int b, double boundary_weight, const long long *target_faces, const float *verts, const int *faces,
                                 const long long *vert_first, const long long *face_first, int *mesh_counts, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  if (q_check("mesh_qem_init", b, vert_first, face_first, workspace, max_v, max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(boundary_weight >= 0.0 && boundary_weight < (double)INFINITY, "mesh_qem_init: boundary_weight %g is not finite and >= 0", boundary_weight);
  BDM_REQUIRE(target_faces, "mesh_qem_init: the targets are NULL");
  for (int m = 0; m < b; ++m)
    BDM_REQUIRE(target_faces[m] >= 0 && target_faces[m] < INT_MAX, "mesh_qem_init: mesh %d: a target of %lld faces is outside 0 .. 2^31 - 2", m,
                target_faces[m]);
  BDM_REQUIRE(verts && faces && mesh_counts, "mesh_qem_init: an input or an output is NULL");
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const QWs w = q_ws(workspace, b, sum_v, sum_f);
  const Range in[2] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}};
  const Range out[2] = {{mesh_counts, 4 * Q_COUNTS * (size_t)b}, {workspace, w.bytes}};
  if (check_overlap("mesh_qem_init", in, 2, out, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  std::vector<long long> target((size_t)b + 1, 0);
  for (int m = 0; m < b; ++m) target[m] = target_faces[m];
  send_offsets(b, target.data(), nullptr, w.target, w.target + (b + 1), st);
  const dim3 block(Q_THREADS), grid_b((unsigned)cdivll(b, Q_THREADS));
  hipLaunchKernelGGL(q_state_kernel, grid_b, block, 0, st, b, w.vert_first, w.face_first, w.target, w.state);
  if (max_v > 0) {
    const dim3 grid_v((unsigned)cdivll(max_v, Q_THREADS), (unsigned)b);
    hipLaunchKernelGGL(q_init_vert_kernel, grid_v, block, 0, st, verts, w.vert_first, w.pos, w.vlive, w.locked, w.parent);
    if (max_f > 0) {
      const dim3 grid_f((unsigned)cdivll(max_f, Q_THREADS), (unsigned)b);
      hipLaunchKernelGGL(q_init_face_kernel, grid_f, block, 0, st, faces, w.vert_first, w.face_first, w.wfaces, w.fcode, w.locked, w.state);
      hipLaunchKernelGGL(fill_ints_kernel, dim3((unsigned)cdivll(6 * sum_f, Q_THREADS)), block, 0, st, (int *)w.key, 6 * sum_f, -1);
    }
    build_incidence<QRec>(b, sum_v, max_f, w.wfaces, w.vert_first, w.face_first, w.first, w.cursor, w.bsum, w.rec, st);
    hipLaunchKernelGGL(q_sort_kernel, grid_v, block, 0, st, w.vert_first, w.state, w.first, w.rec, w.vinfo);
    hipLaunchKernelGGL(q_quadric_kernel, grid_v, block, 0, st, boundary_weight, w.vert_first, w.face_first, w.wfaces, w.pos, w.first, w.rec,
                       w.locked, w.quad, w.state);
  } else if (max_f > 0) {   // faces without a vertex: every one is bad
    hipLaunchKernelGGL(q_init_face_kernel, dim3((unsigned)cdivll(max_f, Q_THREADS), (unsigned)b), block, 0, st, faces, w.vert_first, w.face_first,
                       w.wfaces, w.fcode, w.locked, w.state);
  }
  hipLaunchKernelGGL(q_stop0_kernel, grid_b, block, 0, st, b, w.state);
  hipLaunchKernelGGL(q_report_kernel, grid_b, block, 0, st, b, w.state, mesh_counts, (int *)nullptr);
  return launch_status("mesh_qem_init");
}

extern "C" int bdm_mesh_qem_rounds(int b, int rounds, int max_rounds, double maximum_error, const long long *vert_first,
                                   const long long *face_first, int *mesh_counts, int *active, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  if (q_check("mesh_qem_rounds", b, vert_first, face_first, workspace, max_v, max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(rounds >= 1 && rounds <= Q_MAX_ROUNDS, "mesh_qem_rounds: rounds=%d outside 1 .. %d", rounds, Q_MAX_ROUNDS);
  BDM_REQUIRE(max_rounds >= 1 && max_rounds <= Q_MAX_ROUNDS, "mesh_qem_rounds: max_rounds=%d outside 1 .. %d", max_rounds, Q_MAX_ROUNDS);
  BDM_REQUIRE(maximum_error >= 0.0, "mesh_qem_rounds: maximum_error %g is negative or NaN", maximum_error);
  BDM_REQUIRE(mesh_counts && active, "mesh_qem_rounds: an output is NULL");
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  const QWs w = q_ws(workspace, b, sum_v, sum_f);
  const Range out[3] = {{mesh_counts, 4 * Q_COUNTS * (size_t)b}, {active, 4}, {workspace, w.bytes}};
  if (check_overlap("mesh_qem_rounds", nullptr, 0, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(Q_THREADS), grid_b((unsigned)cdivll(b, Q_THREADS));
  if (max_v > 0 && max_f > 0) {
    const dim3 grid_v((unsigned)cdivll(max_v, Q_THREADS), (unsigned)b), grid_h((unsigned)cdivll(3 * max_f, Q_THREADS), (unsigned)b);
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(q_begin_kernel, grid_b, block, 0, st, b, w.state);
      build_incidence<QRec>(b, sum_v, max_f, w.wfaces, w.vert_first, w.face_first, w.first, w.cursor, w.bsum, w.rec, st);
      hipLaunchKernelGGL(q_sort_kernel, grid_v, block, 0, st, w.vert_first, w.state, w.first, w.rec, w.vinfo);
      hipLaunchKernelGGL(q_edge_kernel, grid_h, block, 0, st, maximum_error, w.vert_first, w.face_first, w.wfaces, w.pos, w.quad, w.first, w.rec,
                         w.vinfo, w.locked, w.key, w.state);
      hipLaunchKernelGGL(q_min_kernel<false>, grid_v, block, 0, st, w.vert_first, w.face_first, w.state, w.first, w.rec, w.key, w.m1);
      hipLaunchKernelGGL(q_min_kernel<true>, grid_v, block, 0, st, w.vert_first, w.face_first, w.state, w.first, w.rec, w.m1, w.m2);
      hipLaunchKernelGGL(q_select_kernel, grid_h, block, 0, st, w.vert_first, w.face_first, w.wfaces, w.key, w.m2, w.sel, w.state);
      hipLaunchKernelGGL(q_apply_kernel, grid_h, block, 0, st, w.vert_first, w.face_first, w.sel, w.first, w.rec, w.wfaces, w.pos, w.quad, w.vlive,
                         w.parent, w.state);
      hipLaunchKernelGGL(q_end_kernel, grid_b, block, 0, st, b, max_rounds, w.state);
    }
  }
  fill_ints(active, 1, 0, st);
  hipLaunchKernelGGL(q_report_kernel, grid_b, block, 0, st, b, w.state, mesh_counts, active);
  return launch_status("mesh_qem_rounds");
}

extern "C" int bdm_mesh_qem_finish(int b, int c, const float *attrs, const long long *vert_first, const long long *face_first,
                                   const long long *out_vert_first, const long long *out_face_first, float *verts_out, float *attrs_out,
                                   int *faces_out, int *vert_map, int *face_map, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  const auto batch = [&] { return q_check("mesh_qem_finish", b, vert_first, face_first, workspace, max_v, max_f); };
  if (check_emit("mesh_qem_finish", "decimated", b, c, vert_first, face_first, out_vert_first, out_face_first,
                 attrs && verts_out && attrs_out && faces_out && vert_map && face_map, batch, decimated_sizes_ok) != BDM_OK)
    return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b], out_v = out_vert_first[b], out_f = out_face_first[b];
  const QWs w = q_ws(workspace, b, sum_v, sum_f);
  const Range in[1] = {{attrs, 4 * (size_t)c * (size_t)sum_v}};
  const Range out[6] = {{verts_out, 12 * (size_t)out_v}, {attrs_out, 4 * (size_t)c * (size_t)out_v}, {faces_out, 12 * (size_t)out_f},
                          {vert_map, 4 * (size_t)sum_v}, {face_map, 4 * (size_t)sum_f}, {workspace, w.bytes}};
  if (check_overlap("mesh_qem_finish", in, 1, out, 6) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, out_vert_first, out_face_first, w.out_vert_first, w.out_face_first, st);
  const dim3 block(Q_THREADS);
  if (max_v > 0) {
    const dim3 grid_v((unsigned)cdivll(max_v, Q_THREADS), (unsigned)b);
    fill_ints(w.rank, sum_v + 1, 0, st);
    build_member_segments(
        sum_v, w.rank, w.seg, w.cursor, w.bsum, st,
        [&] { hipLaunchKernelGGL(q_root_kernel, grid_v, block, 0, st, w.vert_first, w.parent, w.root, w.rank, w.seg); },
        [&] { hipLaunchKernelGGL(q_member_kernel, grid_v, block, 0, st, w.vert_first, w.root, w.rank, w.seg, w.cursor, w.member, vert_map); });
    if (c > 0) {
      hipLaunchKernelGGL(amax_clear_kernel, dim3((unsigned)cdivll(b, Q_THREADS)), block, 0, st, b, 1, w.amax);
      hipLaunchKernelGGL(attr_amax_kernel, grid_v, block, 0, st, c, attrs, w.vert_first, 1, w.amax);
    }
    hipLaunchKernelGGL(q_vertex_out_kernel, grid_v, block, 0, st, c, attrs, w.vert_first, w.out_vert_first, w.pos, w.vlive, w.rank, w.seg, w.member,
                       w.amax, verts_out, attrs_out);
  }
  if (max_f > 0) {
    const dim3 grid_f((unsigned)cdivll(max_f, Q_THREADS), (unsigned)b);
    fill_ints(w.frank, sum_f + 1, 0, st);
    hipLaunchKernelGGL(q_face_flag_kernel, grid_f, block, 0, st, w.face_first, w.wfaces, w.frank);
    exclusive_scan_ints(w.frank, sum_f + 1, nullptr, w.bsum, st);
    hipLaunchKernelGGL(q_face_out_kernel, grid_f, block, 0, st, w.vert_first, w.face_first, w.out_face_first, w.wfaces, w.fcode, w.rank, w.frank,
                       face_map, faces_out);
  }
  return launch_status("mesh_qem_finish");
}
