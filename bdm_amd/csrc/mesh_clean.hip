// mesh_clean.hip -- cleaning triangle meshes: the vertex adjacency of a packed batch, its connected components and Taubin smoothing
// over it, as gfx950 kernels (bdm_hip.h section 16; the smoothing restates pytorch3d's taubin_smoothing;
// pytorch3d is not installed, so the rule is this project's own text).
//
// The rule in one paragraph: a face takes part when its three indices are in range and pairwise different ("connected face").  The
// neighbour list of a vertex is the sorted set of the vertices it shares a side of such a face with; a component's label is its
// smallest vertex index, the fixed point of "take the smallest label around you, then jump once"; a smoothing half-step is a
// weighted mean of the neighbours in ascending order, float32, every operation rounded on its own.  Nothing depends on execution
// order: lists are sorted sets, labels a unique fixed point, counts integer sums, float sums sequential per thread.
//
// Kernels.
//   (ragged.h)             send_offsets: the two host offset arrays travel as launch arguments into the workspace.
//   (mesh_incidence.h)     fill_ints_kernel, scan_kernel<false / true>, scan_top_kernel, and incidence_kernel<false / true, McNeighbours>:
//                          the records of a corner are the face's two other vertices.
//   mc_sort_kernel         one thread per vertex: sorts its segment in place (sort_segment), drops the repeats, counts what is left.
//   mc_compact_kernel      one thread per vertex: its list moves to its place in nbr.
//   mc_label_init_kernel, mc_label_round_kernel (Jacobi: reads one label array, writes the other), mc_label_copy_kernel, mc_flag_kernel.
//   mc_root_kernel         1 where label == index; scanned, it ranks the components.  mc_vert_comp_kernel, mc_face_comp_kernel.
//   mc_stage_kernel        12-byte rows -> 16-byte rows.  mc_taubin_kernel<MODE, LAST>: one thread per vertex, neighbouring lanes hold
//                          neighbouring vertices, one 16-byte load per neighbour; LAST writes 12-byte rows to the output.
#include "../../include/bdm_hip.h"
#include "common.h"
#include "mesh_incidence.h"

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

using namespace bdm;

#define MC_THREADS MESH_THREADS
#define MC_MAX_ITER 10000

namespace {

// ---- adjacency ------------------------------------------------------------------------------------------------------------------------
struct McNeighbours {   // Rec of incidence_kernel: a vertex records the two other vertices of every connected face around it
  typedef int type;
  static __device__ __forceinline__ void corner(const int (&idx)[3], int, int c, int &r0, int &r1) { r0 = idx[(c + 1) % 3], r1 = idx[(c + 2) % 3]; }
};

// one thread per packed vertex: its segment raw[first[g] .. first[g + 1]) sorted ascending in place, repeats dropped; degree[g] = what is left
__global__ __launch_bounds__(MC_THREADS) void mc_sort_kernel(long long sum_v, const int *__restrict__ first, int *__restrict__ raw,
                                                             int *__restrict__ degree) {
  const long long g = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (g > sum_v) return;
  if (g == sum_v) {
    degree[g] = 0;   // the scan's last entry becomes the total
    return;
  }
  int *a = raw + first[g];
  const int len = first[g + 1] - first[g];
  sort_segment(a, len);
  int kept = 0;
  for (int i = 0; i < len; ++i) {
    const int v = a[i];
    if (kept == 0 || a[kept - 1] != v) a[kept++] = v;
  }
  degree[g] = kept;
}

__global__ __launch_bounds__(MC_THREADS) void mc_compact_kernel(long long sum_v, const int *__restrict__ first, const int *__restrict__ raw,
                                                                const int *__restrict__ nbr_first, int *__restrict__ nbr) {
  const long long g = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (g >= sum_v) return;
  const int *a = raw + first[g];
  const int o = nbr_first[g], d = nbr_first[g + 1] - o;   // d <= the segment's length
  for (int e = 0; e < d; ++e) nbr[o + e] = a[e];
}

// ---- components -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mc_label_init_kernel(const long long *__restrict__ vert_first, int *__restrict__ label) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i < nv) label[vbase + i] = (int)i;
}

// one Jacobi round: reads `from` only, writes `to`; sets *changed when `mark` and a label moved
__global__ __launch_bounds__(MC_THREADS) void mc_label_round_kernel(const long long *__restrict__ vert_first, const int *__restrict__ nbr_first,
                                                                    const int *__restrict__ nbr, const int *__restrict__ from,
                                                                    int *__restrict__ to, int mark, int *__restrict__ changed) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i >= nv) return;
  const int *lab = from + vbase;   // labels are indices within the mesh, always in [0, nv)
  const int old = lab[i];
  int best = old;
  const int e1 = nbr_first[vbase + i + 1];
  for (int e = nbr_first[vbase + i]; e < e1; ++e) {
    const int j = nbr[e];
    if (j < 0 || j >= nv) continue;   // no list of this mesh holds it
    const int l = lab[j];
    best = l < best ? l : best;
  }
  best = lab[best];   // one pointer jump
  to[vbase + i] = best;
  if (mark && best != old) *changed = 1;   // every writer stores the same value
}

__global__ __launch_bounds__(MC_THREADS) void mc_label_copy_kernel(long long n, const int *__restrict__ from, int *__restrict__ to) {
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i < n) to[i] = from[i];
}

__global__ void mc_flag_kernel(int *__restrict__ changed) {
  if (threadIdx.x == 0) *changed = 0;
}

__global__ __launch_bounds__(MC_THREADS) void mc_root_kernel(const long long *__restrict__ vert_first, long long sum_v,
                                                             const int *__restrict__ label, int *__restrict__ rank) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i < nv) rank[vbase + i] = label[vbase + i] == i ? 1 : 0;
  if (m == 0 && i == 0) rank[sum_v] = 0;   // the scan's last entry becomes the total
}

// rank = the exclusive scan of the roots over the packed vertices: a component's rank within its mesh is rank[root] - rank[first vertex]
__global__ __launch_bounds__(MC_THREADS) void mc_vert_comp_kernel(const long long *__restrict__ vert_first, const int *__restrict__ label,
                                                                  const int *__restrict__ rank, int *__restrict__ vert_comp,
                                                                  int *__restrict__ comp_count, int *__restrict__ comp_verts) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i == 0) comp_count[m] = rank[vbase + nv] - rank[vbase];   // also for a mesh without vertices
  if (i >= nv) return;
  const int c = rank[vbase + label[vbase + i]] - rank[vbase];   // < nv even for labels that are no fixed point
  vert_comp[vbase + i] = c;
  atomicAdd(comp_verts + vbase + c, 1);
}

__global__ __launch_bounds__(MC_THREADS) void mc_face_comp_kernel(const int *__restrict__ faces, const long long *__restrict__ vert_first,
                                                                  const long long *__restrict__ face_first, const int *__restrict__ vert_comp,
                                                                  int *__restrict__ face_comp, int *__restrict__ comp_faces) {
  const int m = blockIdx.y;
  const long long fbase = face_first[m], nf = face_first[m + 1] - fbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i >= nf) return;
  const long long vbase = vert_first[m];
  int idx[3], c = -1;
  if (connected_face(faces, fbase + i, vert_first[m + 1] - vbase, idx)) {
    c = vert_comp[vbase + idx[0]];
    atomicAdd(comp_faces + vbase + c, 1);
  }
  face_comp[fbase + i] = c;
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mc_stage_kernel(long long sum_v, const float *__restrict__ verts, float4 *__restrict__ rows) {
  const long long g = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (g >= sum_v) return;
  const float *p = verts + 3 * (size_t)g;
  rows[g] = make_float4(p[0], p[1], p[2], 0.f);
}

__global__ __launch_bounds__(MC_THREADS) void mc_copy_rows_kernel(long long n, const float *__restrict__ from, float *__restrict__ to) {
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i < n) to[i] = from[i];
}

// one half-step with factor f (omf = fl(1 - f)): MODE 0 inverse length, 1 uniform; LAST writes 12-byte rows to out instead of dst
template <int MODE, bool LAST>
__global__ __launch_bounds__(MC_THREADS) void mc_taubin_kernel(float f, float omf, const long long *__restrict__ vert_first,
                                                               const int *__restrict__ nbr_first, const int *__restrict__ nbr,
                                                               const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                               float *__restrict__ out) {
  const int m = blockIdx.y;
  const long long vbase = vert_first[m], nv = vert_first[m + 1] - vbase;
  const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
  if (i >= nv) return;
  const float4 *rows = src + vbase;
  const float4 p = rows[i];
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
  int d = 0;
  const int e1 = nbr_first[vbase + i + 1];
  for (int e = nbr_first[vbase + i]; e < e1; ++e) {   // ascending: the sums are sequential
    const int j = nbr[e];
    if (j < 0 || j >= nv) continue;   // no list of this mesh holds it
    const float4 q = rows[j];
    float w = 1.f;
    if (MODE == 0) {
      const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      // sqrtf, not __fsqrt_rn: this toolchain's __fsqrt_rn is the native v_sqrt_f32 (1 ulp); sqrtf under
      // -fhip-fp32-correctly-rounded-divide-sqrt is the correctly rounded one, as in mesh_metrics.hip
      w = __fdiv_rn(1.f, __fadd_rn(sqrtf(d2), 1e-12f));
    }
    const float wx = __fmul_rn(w, q.x), wy = __fmul_rn(w, q.y), wz = __fmul_rn(w, q.z);
    sx = d ? __fadd_rn(sx, wx) : wx;
    sy = d ? __fadd_rn(sy, wy) : wy;
    sz = d ? __fadd_rn(sz, wz) : wz;
    sw = d ? __fadd_rn(sw, w) : w;
    ++d;
  }
  float4 r = p;   // d == 0: the bits stay
  if (d) {
    r.x = __fadd_rn(__fmul_rn(omf, p.x), __fmul_rn(f, __fdiv_rn(sx, sw)));
    r.y = __fadd_rn(__fmul_rn(omf, p.y), __fmul_rn(f, __fdiv_rn(sy, sw)));
    r.z = __fadd_rn(__fmul_rn(omf, p.z), __fmul_rn(f, __fdiv_rn(sz, sw)));
  }
  if (LAST) {
    float *o = out + 3 * (size_t)(vbase + i);
    o[0] = r.x, o[1] = r.y, o[2] = r.z;
  } else {
    dst[vbase + i] = r;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool mc_sizes_ok(int b, long long sum_v, long long sum_f) {
  return b >= 0 && b <= MESH_MAX_B && sum_v >= 0 && sum_v < INT_MAX && sum_f >= 0 && 6 * sum_f <= INT_MAX;
}

// workspace of bdm_mesh_adjacency: offsets | first (sum V + 1) | cursor (sum V + 1) | partial sums | raw (6 sum F)
struct McAdjWs {
  long long *vert_first, *face_first;
  int *first, *cursor, *bsum, *raw;
  size_t bytes;
};
McAdjWs mc_adj_ws(void *ws, int b, long long sum_v, long long sum_f) {
  Carve c{(char *)ws, 0};
  McAdjWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.first = c.take<int>((size_t)(sum_v + 1));
  w.cursor = c.take<int>((size_t)(sum_v + 1));
  w.bsum = c.take<int>((size_t)scan_blocks(sum_v + 1));
  w.raw = c.take<int>(6 * (size_t)sum_f);
  w.bytes = c.o;
  return w;
}

// workspace of the components calls: offsets | label (sum V) | label2 (sum V) | rank (sum V + 1) | partial sums
struct McCompWs {
  long long *vert_first, *face_first;
  int *label, *label2, *rank, *bsum;
  size_t bytes;
};
McCompWs mc_comp_ws(void *ws, int b, long long sum_v) {
  Carve c{(char *)ws, 0};
  McCompWs w;
  w.vert_first = c.take_offsets(b), w.face_first = w.vert_first + (b + 1);
  w.label = c.take<int>((size_t)sum_v);
  w.label2 = c.take<int>((size_t)sum_v);
  w.rank = c.take<int>((size_t)(sum_v + 1));
  w.bsum = c.take<int>((size_t)scan_blocks(sum_v + 1));
  w.bytes = c.o;
  return w;
}

size_t mc_taubin_bytes(int b, long long sum_v) { return offsets_bytes(b) + 2 * 16 * (size_t)sum_v; }

// the prologue every entry point shares: the batch checks, the limits on the sums, the workspace pointer; face_first may be NULL when
// the call uses no faces.  -> BDM_OK with nothing_to_do set when the call returns 0 at once
int mc_prologue(const char *what, int b, const long long *vert_first, const long long *face_first, bool needs_faces, const void *workspace,
                long long &max_v, long long &max_f, bool &nothing_to_do) {
  nothing_to_do = true;
  if (check_mesh_batch(what, b, vert_first, face_first, needs_faces, &max_v, &max_f) != BDM_OK) return BDM_ERR_ARG;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_first[b] < INT_MAX, "%s: %lld vertices reach 2^31", what, vert_first[b]);
  BDM_REQUIRE(!face_first || 6 * face_first[b] <= INT_MAX, "%s: %lld faces: six entries per face reach 2^31", what, face_first[b]);
  if (vert_first[b] == 0) return BDM_OK;   // before the workspace is looked at
  if (check_workspace(what, workspace) != BDM_OK) return BDM_ERR_ARG;
  nothing_to_do = false;
  return BDM_OK;
}

}  // namespace

extern "C" size_t bdm_mesh_adjacency_workspace_bytes(int b, long long sum_v, long long sum_f) {
  if (!mc_sizes_ok(b, sum_v, sum_f)) return 0;
  return mc_adj_ws(nullptr, b, sum_v, sum_f).bytes;
}

extern "C" int bdm_mesh_adjacency(int b, const int *faces, const long long *vert_first, const long long *face_first, int *nbr_first,
                                  int *nbr, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  bool nothing = false;
  if (mc_prologue("mesh_adjacency", b, vert_first, face_first, true, workspace, max_v, max_f, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(faces && nbr_first && nbr, "mesh_adjacency: the faces or an output is NULL");
  const McAdjWs w = mc_adj_ws(workspace, b, sum_v, sum_f);
  const Range in[1] = {{faces, 12 * (size_t)sum_f}};
  const Range out[3] = {{nbr_first, 4 * (size_t)(sum_v + 1)}, {nbr, 24 * (size_t)sum_f}, {workspace, w.bytes}};
  if (check_overlap("mesh_adjacency", in, 1, out, 3) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  build_incidence<McNeighbours>(b, sum_v, max_f, faces, w.vert_first, w.face_first, w.first, w.cursor, w.bsum, w.raw, st);
  const unsigned flat_v = (unsigned)cdivll(sum_v + 1, MC_THREADS);
  hipLaunchKernelGGL(mc_sort_kernel, dim3(flat_v), dim3(MC_THREADS), 0, st, sum_v, w.first, w.raw, nbr_first);
  exclusive_scan_ints(nbr_first, sum_v + 1, nullptr, w.bsum, st);
  hipLaunchKernelGGL(mc_compact_kernel, dim3(flat_v), dim3(MC_THREADS), 0, st, sum_v, w.first, w.raw, nbr_first, nbr);
  return launch_status("mesh_adjacency");
}

extern "C" size_t bdm_mesh_components_workspace_bytes(int b, long long sum_v) {
  if (!mc_sizes_ok(b, sum_v, 0)) return 0;
  return mc_comp_ws(nullptr, b, sum_v).bytes;
}

extern "C" int bdm_mesh_components_init(int b, const long long *vert_first, const long long *face_first, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  bool nothing = false;
  if (mc_prologue("mesh_components_init", b, vert_first, face_first, true, workspace, max_v, max_f, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  const McCompWs w = mc_comp_ws(workspace, b, vert_first[b]);
  hipStream_t st = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, w.vert_first, w.face_first, st);
  hipLaunchKernelGGL(mc_label_init_kernel, dim3((unsigned)cdivll(max_v, MC_THREADS), (unsigned)b), dim3(MC_THREADS), 0, st, w.vert_first, w.label);
  return launch_status("mesh_components_init");
}

extern "C" int bdm_mesh_components_rounds(int b, int rounds, const long long *vert_first, const long long *face_first, const int *nbr_first,
                                          const int *nbr, int *changed, void *workspace, void *stream) {
  BDM_REQUIRE(rounds >= 1, "mesh_components_rounds: rounds=%d is not positive", rounds);
  long long max_v = 0, max_f = 0;
  bool nothing = false;
  if (mc_prologue("mesh_components_rounds", b, vert_first, face_first, true, workspace, max_v, max_f, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(nbr_first && nbr && changed, "mesh_components_rounds: the adjacency or the flag is NULL");
  const McCompWs w = mc_comp_ws(workspace, b, sum_v);
  const Range in[2] = {{nbr_first, 4 * (size_t)(sum_v + 1)}, {nbr, 24 * (size_t)sum_f}};
  const Range out[2] = {{changed, 4}, {workspace, w.bytes}};
  if (check_overlap("mesh_components_rounds", in, 2, out, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_flag_kernel, dim3(1), dim3(64), 0, st, changed);
  const dim3 grid((unsigned)cdivll(max_v, MC_THREADS), (unsigned)b);
  int *from = w.label, *to = w.label2;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(mc_label_round_kernel, grid, dim3(MC_THREADS), 0, st, w.vert_first, nbr_first, nbr, from, to, r == rounds - 1 ? 1 : 0,
                       changed);
    int *t = from;
    from = to, to = t;
  }
  if (from != w.label)   // an odd number of rounds left the labels in the second array
    hipLaunchKernelGGL(mc_label_copy_kernel, dim3((unsigned)cdivll(sum_v, MC_THREADS)), dim3(MC_THREADS), 0, st, sum_v, w.label2, w.label);
  return launch_status("mesh_components_rounds");
}

extern "C" int bdm_mesh_components_finish(int b, const int *faces, const long long *vert_first, const long long *face_first, int *vert_comp,
                                          int *face_comp, int *comp_count, int *comp_verts, int *comp_faces, void *workspace, void *stream) {
  long long max_v = 0, max_f = 0;
  bool nothing = false;
  if (mc_prologue("mesh_components_finish", b, vert_first, face_first, true, workspace, max_v, max_f, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(faces && vert_comp && face_comp && comp_count && comp_verts && comp_faces, "mesh_components_finish: the faces or an output is NULL");
  const McCompWs w = mc_comp_ws(workspace, b, sum_v);
  const Range in[1] = {{faces, 12 * (size_t)sum_f}};
  const Range out[6] = {{vert_comp, 4 * (size_t)sum_v}, {face_comp, 4 * (size_t)sum_f}, {comp_count, 4 * (size_t)b},
                          {comp_verts, 4 * (size_t)sum_v}, {comp_faces, 4 * (size_t)sum_v}, {workspace, w.bytes}};
  if (check_overlap("mesh_components_finish", in, 1, out, 6) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid_v((unsigned)cdivll(max_v, MC_THREADS), (unsigned)b);
  hipLaunchKernelGGL(mc_root_kernel, grid_v, dim3(MC_THREADS), 0, st, w.vert_first, sum_v, w.label, w.rank);
  exclusive_scan_ints(w.rank, sum_v + 1, nullptr, w.bsum, st);
  fill_ints(comp_verts, sum_v, 0, st);
  fill_ints(comp_faces, sum_v, 0, st);
  hipLaunchKernelGGL(mc_vert_comp_kernel, grid_v, dim3(MC_THREADS), 0, st, w.vert_first, w.label, w.rank, vert_comp, comp_count, comp_verts);
  if (max_f > 0)
    hipLaunchKernelGGL(mc_face_comp_kernel, dim3((unsigned)cdivll(max_f, MC_THREADS), (unsigned)b), dim3(MC_THREADS), 0, st, faces, w.vert_first,
                       w.face_first, vert_comp, face_comp, comp_faces);
  return launch_status("mesh_components_finish");
}

extern "C" size_t bdm_mesh_taubin_workspace_bytes(int b, long long sum_v) {
  if (!mc_sizes_ok(b, sum_v, 0)) return 0;
  return mc_taubin_bytes(b, sum_v);
}

extern "C" int bdm_mesh_taubin(int b, int num_iter, int mode, float lambd, float mu, const float *verts, const long long *vert_first,
                               const int *nbr_first, const int *nbr, float *verts_out, void *workspace, void *stream) {
  BDM_REQUIRE(num_iter >= 0 && num_iter <= MC_MAX_ITER, "mesh_taubin: num_iter=%d outside 0 .. %d", num_iter, MC_MAX_ITER);
  BDM_REQUIRE(mode == 0 || mode == 1, "mesh_taubin: mode %d is neither 0 (inverse length) nor 1 (uniform)", mode);
  BDM_REQUIRE(fabsf(lambd) < INFINITY && fabsf(mu) < INFINITY, "mesh_taubin: lambd and mu must be finite");
  long long max_v = 0, max_f = 0;
  bool nothing = false;
  if (mc_prologue("mesh_taubin", b, vert_first, nullptr, false, workspace, max_v, max_f, nothing) != BDM_OK) return BDM_ERR_ARG;
  if (nothing) return BDM_OK;
  const long long sum_v = vert_first[b];
  BDM_REQUIRE(verts && nbr_first && nbr && verts_out, "mesh_taubin: an input or the output is NULL");
  // the length of nbr is on the device (nbr_first[sum V]); its first entry stands for it in the overlap test
  const Range in[3] = {{verts, 12 * (size_t)sum_v}, {nbr_first, 4 * (size_t)(sum_v + 1)}, {nbr, 4}};
  const Range out[2] = {{verts_out, 12 * (size_t)sum_v}, {workspace, mc_taubin_bytes(b, sum_v)}};
  if (check_overlap("mesh_taubin", in, 3, out, 2) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned flat_v = (unsigned)cdivll(sum_v, MC_THREADS);
  if (num_iter == 0) {
    hipLaunchKernelGGL(mc_copy_rows_kernel, dim3((unsigned)cdivll(3 * sum_v, MC_THREADS)), dim3(MC_THREADS), 0, st, 3 * sum_v, verts, verts_out);
    return launch_status("mesh_taubin");
  }
  long long *dev_v = (long long *)workspace;
  send_offsets(b, vert_first, nullptr, dev_v, dev_v + (b + 1), st);
  float4 *rows_a = (float4 *)((char *)workspace + offsets_bytes(b)), *rows_b = rows_a + sum_v;
  hipLaunchKernelGGL(mc_stage_kernel, dim3(flat_v), dim3(MC_THREADS), 0, st, sum_v, verts, rows_a);
  const dim3 grid((unsigned)cdivll(max_v, MC_THREADS), (unsigned)b);
  const float one_minus[2] = {1.0f - lambd, 1.0f - mu};   // rounded once, in float32
  const float factor[2] = {lambd, mu};
  float4 *src = rows_a, *dst = rows_b;
  for (int h = 0; h < 2 * num_iter; ++h) {
    const float f = factor[h & 1], omf = one_minus[h & 1];
    const bool last = h == 2 * num_iter - 1;
    if (mode == 0) {
      if (last) hipLaunchKernelGGL((mc_taubin_kernel<0, true>), grid, dim3(MC_THREADS), 0, st, f, omf, dev_v, nbr_first, nbr, src, dst, verts_out);
      else hipLaunchKernelGGL((mc_taubin_kernel<0, false>), grid, dim3(MC_THREADS), 0, st, f, omf, dev_v, nbr_first, nbr, src, dst, verts_out);
    } else {
      if (last) hipLaunchKernelGGL((mc_taubin_kernel<1, true>), grid, dim3(MC_THREADS), 0, st, f, omf, dev_v, nbr_first, nbr, src, dst, verts_out);
      else hipLaunchKernelGGL((mc_taubin_kernel<1, false>), grid, dim3(MC_THREADS), 0, st, f, omf, dev_v, nbr_first, nbr, src, dst, verts_out);
    }
    float4 *t = src;
    src = dst, dst = t;
  }
  return launch_status("mesh_taubin");
}
