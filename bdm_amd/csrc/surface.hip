// Triangle meshes from oriented clouds: fixed-point IMLS grid and surface nets (section 12 of bdm_hip.h).
//
// bdm_surface_grid:
//   surf_box_kernel      one workgroup per cloud: exact bounding box of the valid points -> c, inv, the cloud's "live" flag, counts
//   (memset)             SW, SU = 0
//   surf_scatter_kernel  one thread per (point, x offset, z offset), a loop over the y offsets: integer atomicAdd into SW, SU
//   surf_cell_kernel     one thread per node: is the cell whose lowest corner it is active?  flag + count per workgroup
//   surf_edge_kernel     one thread per (axis, node): code of the edge (0 nothing, 1 quad, 2 reversed quad, 3 skipped) + counts
//   surf_scan_kernel     one workgroup per cloud: exclusive scan of the per-workgroup counts in place -> V, F
//   surf_rank_kernel     the flags of the cells become vertex ids (-1: not active)
// bdm_surface_extract:
//   surf_vertex_kernel   one thread per node: the vertex of its cell
//   surf_face_kernel     one thread per (axis, node): the two triangles of its edge at the scanned offset
// Count, scan and write are separate launches; nothing waits on another workgroup, every loop is bounded by a launch argument.
// Sums are integers, so the order of the atomics cannot change a bit.
//
// The workspace layout, the frame (surf_launch_frame) and the mark stage (surf_launch_mark: surf_cell_kernel ... surf_rank_kernel) are
// shared with bdm_surface_poisson_grid (surface_poisson.hip) through surface_stage.h.
//
// The file is compiled with -ffp-contract=off and correctly rounded division (Makefile): the arithmetic defines integers.
#include "common.h"
#include "bdm_hip.h"
#include "surface_stage.h"

namespace bdm {

// rank of a set flag among the set flags of the workgroup (ascending thread index) and their number; all threads call it
__device__ __forceinline__ int surf_block_rank(bool flag, int &total, int *waves) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) waves[wave] = __popcll(m);
  __syncthreads();
  int before = __popcll(m & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int w = 0; w < SRF_WAVES; ++w) {
    before += w < wave ? waves[w] : 0;
    total += waves[w];
  }
  __syncthreads();   // waves[] may be written again
  return before;
}

__global__ __launch_bounds__(SRF_WIDE) void surf_box_kernel(int n, int r, int s, const float *__restrict__ points,
                                                            const float *__restrict__ normals, float *__restrict__ par,
                                                            int *__restrict__ counts) {
  __shared__ float red[SRF_WIDE / 64][6];
  __shared__ int cnt[SRF_WIDE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cloud = blockIdx.x;
  const float *pts = points + (size_t)cloud * n * 3, *nrm = normals + (size_t)cloud * n * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int valid = 0;
  for (int i = tid; i < n; i += SRF_WIDE) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (finite1(x) && finite1(y) && finite1(z) && finite1(nrm[3 * (size_t)i]) && finite1(nrm[3 * (size_t)i + 1]) &&
        finite1(nrm[3 * (size_t)i + 2])) {
      lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
      ++valid;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], __shfl_xor(lo[a], m)), hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m));
    valid += __shfl_xor(valid, m);
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) red[wave][a] = lo[a], red[wave][3 + a] = hi[a];
    cnt[wave] = valid;
  }
  __syncthreads();
  if (tid != 0) return;
  valid = 0;
  for (int w = 0; w < SRF_WIDE / 64; ++w) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], red[w][a]), hi[a] = fmaxf(hi[a], red[w][3 + a]);
    valid += cnt[w];
  }
  const bool live = valid > 0 && !(lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]);
  float half = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    par[(size_t)cloud * SRF_PAR + a] = __fmul_rn(0.5f, __fadd_rn(lo[a], hi[a]));
    half = fmaxf(half, __fmul_rn(0.5f, __fsub_rn(hi[a], lo[a])));
  }
  par[(size_t)cloud * SRF_PAR + 3] = __fdiv_rn((float)(r - 1 - 2 * (s + 1)), __fmul_rn(2.0f, half));
  reinterpret_cast<int *>(par)[(size_t)cloud * SRF_PAR + 4] = live ? 1 : 0;
  counts[4 * (size_t)cloud] = 0, counts[4 * (size_t)cloud + 1] = 0, counts[4 * (size_t)cloud + 2] = 0, counts[4 * (size_t)cloud + 3] = valid;
}

__global__ __launch_bounds__(SRF_THREADS) void surf_scatter_kernel(int b, int n, int r, int s, const float *__restrict__ points,
                                                                   const float *__restrict__ normals, const float *__restrict__ par,
                                                                   int *__restrict__ sw, int *__restrict__ su) {
  const int side = 2 * s, per = side * side;
  const int item = blockIdx.x * SRF_THREADS + threadIdx.x;   // n * per <= 65536 * 64
  if (item >= n * per) return;
  const int i = item / per, ox = (item % per) / side - s + 1, oz = item % side - s + 1;
  const float s2 = (float)(s * s), lim = 4096.0f * (float)s, rm1 = (float)(r - 1), mid = __fmul_rn(0.5f, rm1);
  const size_t r3 = (size_t)r * r * r;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const float *cp = par + (size_t)cloud * SRF_PAR;
    if (reinterpret_cast<const int *>(cp)[4] == 0) continue;
    const size_t row = ((size_t)cloud * n + i) * 3;
    const float px = points[row], py = points[row + 1], pz = points[row + 2];
    const float nx = normals[row], ny = normals[row + 1], nz = normals[row + 2];
    if (!(finite1(px) && finite1(py) && finite1(pz) && finite1(nx) && finite1(ny) && finite1(nz))) continue;
    const float inv = cp[3];
    const float qx = __fadd_rn(__fmul_rn(__fsub_rn(px, cp[0]), inv), mid), qy = __fadd_rn(__fmul_rn(__fsub_rn(py, cp[1]), inv), mid),
                qz = __fadd_rn(__fmul_rn(__fsub_rn(pz, cp[2]), inv), mid);
    if (!(qx >= 0.0f && qx <= rm1 && qy >= 0.0f && qy <= rm1 && qz >= 0.0f && qz <= rm1)) continue;   // NaN fails too
    const int gx = (int)floorf(qx) + ox, gz = (int)floorf(qz) + oz, by = (int)floorf(qy);
    if (gx < 0 || gx >= r || gz < 0 || gz >= r) continue;
    const float dx = __fsub_rn((float)gx, qx), dz = __fsub_rn((float)gz, qz);
    for (int oy = -s + 1; oy <= s; ++oy) {
      const int gy = by + oy;
      if (gy < 0 || gy >= r) continue;
      const float dy = __fsub_rn((float)gy, qy);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      const float t = __fsub_rn(s2, d2);
      if (!(t > 0.0f)) continue;
      const float w = __fdiv_rn(t, s2);
      const float w3 = __fmul_rn(__fmul_rn(w, w), w);
      const float a = __fadd_rn(__fadd_rn(__fmul_rn(nx, dx), __fmul_rn(ny, dy)), __fmul_rn(nz, dz));
      const float uf = rintf(__fmul_rn(__fmul_rn(w3, a), 4096.0f));
      const int W = (int)rintf(__fmul_rn(w3, 4096.0f));
      const int U = uf != uf ? 0 : (int)fminf(fmaxf(uf, -lim), lim);
      const size_t node = (size_t)cloud * r3 + ((size_t)gx * r + gy) * r + gz;   // all three coordinates checked against [0, r)
      if (W) atomicAdd(&sw[node], W);
      if (U) atomicAdd(&su[node], U);
    }
  }
}

// cell flags: the node is the lowest corner of its cell
__global__ __launch_bounds__(SRF_THREADS) void surf_cell_kernel(int b, int r, int thr, int nb, const int *__restrict__ sw,
                                                                const int *__restrict__ su, int *__restrict__ cell,
                                                                int *__restrict__ cell_bc) {
  __shared__ int waves[SRF_WAVES];
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  const int k = g % r, j = (g / r) % r, i = g / (r * r);
  const bool inside = g < r3 && i < r - 1 && j < r - 1 && k < r - 1;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t base = (size_t)cloud * r3;
    bool active = false;
    if (inside) {
      bool defined = true;
      int neg = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const size_t node = base + g + (c >> 2) * r * r + ((c >> 1) & 1) * r + (c & 1);   // i, j, k < r - 1: inside the grid
        defined = defined && sw[node] >= thr;
        neg += su[node] < 0;
      }
      active = defined && neg >= 1 && neg <= 7;
    }
    if (g < r3) cell[base + g] = active ? 1 : 0;
    int total;
    surf_block_rank(active, total, waves);
    if (threadIdx.x == 0) cell_bc[(size_t)cloud * nb + blockIdx.x] = total;
  }
}

__global__ __launch_bounds__(SRF_THREADS) void surf_edge_kernel(int b, int r, int thr, int nb, const int *__restrict__ sw,
                                                                const int *__restrict__ su, const int *__restrict__ cell,
                                                                unsigned char *__restrict__ eflag, int *__restrict__ edge_bc,
                                                                int *__restrict__ counts) {
  __shared__ int waves[SRF_WAVES];
  const int r3 = r * r * r, axis = blockIdx.x / nb, blk = blockIdx.x % nb, g = blk * SRF_THREADS + threadIdx.x;
  const int co[3] = {g / (r * r), (g / r) % r, g % r}, st[3] = {r * r, r, 1};
  const int u = (axis + 1) % 3, v = (axis + 2) % 3;
  const bool place = g < r3 && co[axis] <= r - 2 && co[u] >= 1 && co[u] <= r - 2 && co[v] >= 1 && co[v] <= r - 2;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t base = (size_t)cloud * r3;
    int code = 0;
    if (place) {
      const size_t lower = base + g, upper = lower + st[axis];   // co[axis] <= r - 2: inside the grid
      if (sw[lower] >= thr && sw[upper] >= thr) {
        const bool nl = su[lower] < 0, nu = su[upper] < 0;
        if (nl != nu) {
          // co[u], co[v] >= 1: the four cells exist
          const bool all4 = cell[lower - st[u] - st[v]] && cell[lower - st[v]] && cell[lower] && cell[lower - st[u]];
          code = all4 ? (nl ? 1 : 2) : 3;
        }
      }
    }
    if (g < r3) eflag[((size_t)cloud * 3 + axis) * r3 + g] = (unsigned char)code;
    int quads, skipped;
    surf_block_rank(code == 1 || code == 2, quads, waves);
    surf_block_rank(code == 3, skipped, waves);
    if (threadIdx.x == 0) {
      edge_bc[((size_t)cloud * 3 + axis) * nb + blk] = quads;
      if (skipped) atomicAdd(&counts[4 * (size_t)cloud + 2], skipped);
    }
  }
}

// exclusive scan of a[0 .. len) in place by one workgroup of SRF_WIDE threads -> the total
__device__ int surf_scan_in_place(int *a, int len, int *buf /* 2 * SRF_WIDE */) {
  const int tid = threadIdx.x, chunk = (len + SRF_WIDE - 1) / SRF_WIDE;
  const int lo = min(tid * chunk, len), hi = min(lo + chunk, len);
  int mine = 0;
  for (int e = lo; e < hi; ++e) mine += a[e];
  int *cur = buf, *nxt = buf + SRF_WIDE;
  cur[tid] = mine;
  __syncthreads();
  for (int step = 1; step < SRF_WIDE; step <<= 1) {
    nxt[tid] = cur[tid] + (tid >= step ? cur[tid - step] : 0);
    __syncthreads();
    int *tmp = cur;
    cur = nxt, nxt = tmp;
  }
  int run = cur[tid] - mine;
  const int total = cur[SRF_WIDE - 1];
  for (int e = lo; e < hi; ++e) {
    const int c = a[e];
    a[e] = run;
    run += c;
  }
  __syncthreads();   // buf may be written again
  return total;
}

__global__ __launch_bounds__(SRF_WIDE) void surf_scan_kernel(int nb, int *__restrict__ cell_bc, int *__restrict__ edge_bc,
                                                             int *__restrict__ counts) {
  __shared__ int buf[2 * SRF_WIDE];
  const int cloud = blockIdx.x;
  const int v = surf_scan_in_place(cell_bc + (size_t)cloud * nb, nb, buf);
  const int q = surf_scan_in_place(edge_bc + (size_t)cloud * 3 * nb, 3 * nb, buf);   // axis-major: the order of the faces
  if (threadIdx.x == 0) counts[4 * (size_t)cloud] = v, counts[4 * (size_t)cloud + 1] = 2 * q;
}

__global__ __launch_bounds__(SRF_THREADS) void surf_rank_kernel(int b, int r, int nb, const int *__restrict__ cell_bc,
                                                                int *__restrict__ cell) {
  __shared__ int waves[SRF_WAVES];
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t at = (size_t)cloud * r3 + g;
    const bool active = g < r3 && cell[at] != 0;
    int total;
    const int rank = surf_block_rank(active, total, waves);
    if (g < r3) cell[at] = active ? cell_bc[(size_t)cloud * nb + blockIdx.x] + rank : -1;
  }
}

__global__ __launch_bounds__(SRF_THREADS) void surf_vertex_kernel(int b, int r, const int *__restrict__ sw, const int *__restrict__ su,
                                                                  const int *__restrict__ cell, const float *__restrict__ par,
                                                                  const long long *__restrict__ vert_offsets, float *__restrict__ verts) {
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= r3) return;
  const int co[3] = {g / (r * r), (g / r) % r, g % r};
  const float mid = __fmul_rn(0.5f, (float)(r - 1));
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t base = (size_t)cloud * r3;
    const int id = cell[base + g];
    if (id < 0) continue;   // an active cell has co[] < r - 1: its corners are inside the grid
    float f[8];
    bool neg[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const size_t node = base + g + (c >> 2) * r * r + ((c >> 1) & 1) * r + (c & 1);
      const int U = su[node];
      f[c] = __fdiv_rn(__int2float_rn(U), __int2float_rn(sw[node]));
      neg[c] = U < 0;
    }
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int crossings = 0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
      for (int axis = 0; axis < 3; ++axis) {
        const int bit = 4 >> axis;
        if (a & bit) continue;
        const int e = a | bit;
        if (neg[a] == neg[e]) continue;
        const float tt = __fdiv_rn(f[a], __fsub_rn(f[a], f[e]));
#pragma unroll
        for (int x = 0; x < 3; ++x) sum[x] = __fadd_rn(sum[x], x == axis ? tt : (float)((a >> (2 - x)) & 1));
        ++crossings;
      }
    }
    const float *cp = par + (size_t)cloud * SRF_PAR;
    float *out = verts + 3 * ((size_t)vert_offsets[cloud] + (size_t)id);
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const float grid = __fadd_rn((float)co[x], __fdiv_rn(sum[x], (float)crossings));
      out[x] = __fadd_rn(__fdiv_rn(__fsub_rn(grid, mid), cp[3]), cp[x]);
    }
  }
}

__global__ __launch_bounds__(SRF_THREADS) void surf_face_kernel(int b, int r, int nb, const int *__restrict__ cell,
                                                                const unsigned char *__restrict__ eflag, const int *__restrict__ edge_bc,
                                                                const long long *__restrict__ face_offsets, int *__restrict__ faces) {
  __shared__ int waves[SRF_WAVES];
  const int r3 = r * r * r, axis = blockIdx.x / nb, blk = blockIdx.x % nb, g = blk * SRF_THREADS + threadIdx.x;
  const int st[3] = {r * r, r, 1};
  const int su_ = st[(axis + 1) % 3], sv_ = st[(axis + 2) % 3];
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const int code = g < r3 ? eflag[((size_t)cloud * 3 + axis) * r3 + g] : 0;
    int total;
    const int rank = surf_block_rank(code == 1 || code == 2, total, waves);
    if (code != 1 && code != 2) continue;   // uniform barriers: surf_block_rank has been left by every thread
    const size_t at = (size_t)cloud * r3 + g;   // a code of 1 or 2 was given only where the four cells exist
    const int c00 = cell[at - su_ - sv_], c10 = cell[at - sv_], c11 = cell[at], c01 = cell[at - su_];
    const int q0 = code == 1 ? c00 : c01, q1 = code == 1 ? c10 : c11, q2 = code == 1 ? c11 : c10, q3 = code == 1 ? c01 : c00;
    const size_t quad = (size_t)edge_bc[((size_t)cloud * 3 + axis) * nb + blk] + (size_t)rank;
    int *out = faces + 3 * ((size_t)face_offsets[cloud] + 2 * quad);
    out[0] = q0, out[1] = q1, out[2] = q2, out[3] = q0, out[4] = q2, out[5] = q3;
  }
}

bool surf_sizes_ok(int b, int n, int r, int s) {
  return b >= 0 && n >= 1 && n <= SRF_N_MAX && r >= SRF_R_MIN && r <= SRF_R_MAX && s >= SRF_S_MIN && s <= SRF_S_MAX &&
         (long long)b * r * r * r < (1ll << 31);
}

int surf_check_sizes(const char *what, int b, int n, int r, int s) {
  BDM_REQUIRE(b >= 0 && n >= 1 && n <= SRF_N_MAX, "%s: bad sizes b=%d n=%d (n in 1..%d)", what, b, n, SRF_N_MAX);
  BDM_REQUIRE(r >= SRF_R_MIN && r <= SRF_R_MAX, "%s: r=%d outside %d..%d", what, r, SRF_R_MIN, SRF_R_MAX);
  BDM_REQUIRE(s >= SRF_S_MIN && s <= SRF_S_MAX, "%s: s=%d outside %d..%d", what, s, SRF_S_MIN, SRF_S_MAX);
  BDM_REQUIRE((long long)b * r * r * r < (1ll << 31), "%s: b r^3 = %lld exceeds int", what, (long long)b * r * r * r);
  return BDM_OK;
}

void surf_launch_frame(int b, int n, int r, int margin, const float *points, const float *normals, const SurfWs &w, int *counts,
                       hipStream_t st) {
  // the kernel's frame leaves s + 1 voxels free on every side: margin = s + 1 is section 12's, a wider one is asked for as a larger s
  hipLaunchKernelGGL(surf_box_kernel, dim3((unsigned)b), dim3(SRF_WIDE), 0, st, n, r, margin - 1, points, normals, w.par, counts);
}

void surf_launch_mark(int b, int r, int thr, const SurfWs &w, int *counts, hipStream_t st) {
  const unsigned gy = (unsigned)b < SRF_GRID_Y ? (unsigned)b : SRF_GRID_Y;
  hipLaunchKernelGGL(surf_cell_kernel, dim3((unsigned)w.nb, gy), dim3(SRF_THREADS), 0, st, b, r, thr, w.nb, w.sw, w.su, w.cell, w.cell_bc);
  hipLaunchKernelGGL(surf_edge_kernel, dim3((unsigned)(3 * w.nb), gy), dim3(SRF_THREADS), 0, st, b, r, thr, w.nb, w.sw, w.su, w.cell,
                     w.eflag, w.edge_bc, counts);
  hipLaunchKernelGGL(surf_scan_kernel, dim3((unsigned)b), dim3(SRF_WIDE), 0, st, w.nb, w.cell_bc, w.edge_bc, counts);
  hipLaunchKernelGGL(surf_rank_kernel, dim3((unsigned)w.nb, gy), dim3(SRF_THREADS), 0, st, b, r, w.nb, w.cell_bc, w.cell);
}

}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_surface_workspace_bytes(int b, int n, int r, int s) {
  if (!surf_sizes_ok(b, n, r, s)) return 0;
  return surf_ws_bytes(b, r);
}

extern "C" int bdm_surface_grid(int b, int n, int r, int s, float min_weight, const float *points, const float *normals, int *counts,
                                void *workspace, void *stream) {
  if (int rc = surf_check_sizes("surface_grid", b, n, r, s)) return rc;
  BDM_REQUIRE(min_weight >= 0.0f && min_weight <= 1.0f, "surface_grid: min_weight=%g outside 0..1", (double)min_weight);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(points && normals && counts && workspace, "surface_grid: null pointer");
  BDM_REQUIRE((const void *)counts != (const void *)points && (const void *)counts != (const void *)normals &&
                  workspace != (const void *)points && workspace != (const void *)normals && workspace != (void *)counts,
              "surface_grid: counts and the workspace must not alias the inputs or each other");
  const SurfWs w = surf_ws(workspace, b, r);
  const int weight = (int)rintf(min_weight * 4096.0f), thr = weight > 1 ? weight : 1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)b < SRF_GRID_Y ? (unsigned)b : SRF_GRID_Y;
  surf_launch_frame(b, n, r, s + 1, points, normals, w, counts, st);
  if (hipMemsetAsync(w.sw, 0, 2 * (size_t)b * w.r3 * sizeof(int), st) != hipSuccess) return launch_status("surface_grid (memset)");
  hipLaunchKernelGGL(surf_scatter_kernel, dim3((unsigned)cdiv(n * 4 * s * s, SRF_THREADS), gy), dim3(SRF_THREADS), 0, st, b, n, r, s,
                     points, normals, w.par, w.sw, w.su);
  surf_launch_mark(b, r, thr, w, counts, st);
  return launch_status("surface_grid");
}

extern "C" int bdm_surface_extract(int b, int n, int r, int s, const long long *vert_offsets, const long long *face_offsets, float *verts,
                                   int *faces, void *workspace, void *stream) {
  if (int rc = surf_check_sizes("surface_extract", b, n, r, s)) return rc;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_offsets && face_offsets && verts && faces && workspace, "surface_extract: null pointer");
  BDM_REQUIRE((void *)verts != (void *)faces && (void *)verts != workspace && (void *)faces != workspace &&
                  (const void *)verts != (const void *)vert_offsets && (const void *)verts != (const void *)face_offsets &&
                  (const void *)faces != (const void *)vert_offsets && (const void *)faces != (const void *)face_offsets,
              "surface_extract: verts and faces must not alias the offsets, the workspace or each other");
  const SurfWs w = surf_ws(workspace, b, r);
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)b < SRF_GRID_Y ? (unsigned)b : SRF_GRID_Y;
  hipLaunchKernelGGL(surf_vertex_kernel, dim3((unsigned)w.nb, gy), dim3(SRF_THREADS), 0, st, b, r, w.sw, w.su, w.cell, w.par, vert_offsets,
                     verts);
  hipLaunchKernelGGL(surf_face_kernel, dim3((unsigned)(3 * w.nb), gy), dim3(SRF_THREADS), 0, st, b, r, w.nb, w.cell, w.eflag, w.edge_bc,
                     face_offsets, faces);
  return launch_status("surface_extract");
}
