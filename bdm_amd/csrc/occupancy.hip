// Occupancy-grid histograms of a set of clouds (section 9 of bdm_hip.h): the GPU half of the JSD measure and of the occupancy
// entropy (bdm_amd/metrics.py).  One kernel.  A workgroup owns whole clouds: a cloud's hits are counted in an r^3 histogram in LDS,
// `active` is "this cloud's count is non-zero", and the histogram is folded into the global ones with integer atomics -- sums of
// integers, so the result carries the same bits for any workgroup order and any split of the clouds over calls.
//
// A point's cell is the kept cell nearest to it: argmin of (x - gx)^2 + (y - gy)^2 + (z - gz)^2 in fp32, unfused, in that order.
// Equal values: the slow path takes the lowest flat index; the fast path takes the lowest index PER AXIS, which can be another
// cell only when a per-axis difference is absorbed by the rounding of the sum (two cells then carry the same fp32 distance).
//   fast path  round every coordinate to its axis index (then compare with both neighbours in fp32); when that cell is kept it is
//              the nearest cell of the whole grid, so of the kept ones too
//   slow path  the rounded cell is masked out (the point is near the sphere's surface, outside it or outside the cube): the points
//              of a chunk that need it are compacted into an LDS list and every (point, grid slab i) item is searched by one thread
//              over the slab's r^2 cells; the items of a point meet in an LDS 64-bit minimum over (distance bits, flat index)
// The kept cells are held as one 32-bit word per (i, j) column (bit k = cell kept), hence r <= 32.  DESIGN.md section 13.
#include "common.h"
#include "bdm_hip.h"

namespace bdm {

constexpr int OCC_THREADS = 1024;  // = points per chunk = capacity of the slow list
constexpr int OCC_MAX_R = 32;      // one mask word per column; 32^3 ints = 128 KiB of the CU's 160
constexpr int OCC_MAX_GRID = 2048;

// bytes of dynamic LDS: best[1024] u64 | sx, sy, sz [1024] | colmask[r^2] | axis[r] | hist[r^3]
static size_t occ_lds_bytes(int r) {
  return (size_t)OCC_THREADS * (8 + 12) + (size_t)r * r * 4 + (size_t)r * 4 + (size_t)r * r * r * 4;
}

// index of the axis coordinate nearest to x: the rounded index, then the fp32 squared differences of it and its two neighbours,
// lowest index on ties (what the argmin over the whole axis gives for an ascending, evenly spaced axis)
__device__ __forceinline__ int occ_axis_index(float x, const float *axis, float a0, float scale, int r) {
  const float t = fminf(fmaxf(rintf((x - a0) * scale), 0.0f), (float)(r - 1));
  const int c = (int)t, lo = max(c - 1, 0), hi = min(c + 1, r - 1);
  int best = lo;
  float e = x - axis[lo];
  e = __fmul_rn(e, e);
  for (int q = lo + 1; q <= hi; ++q) {
    float f = x - axis[q];
    f = __fmul_rn(f, f);
    if (f < e) e = f, best = q;
  }
  return best;
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_grid_kernel(int s, int n, int r, const float *__restrict__ clouds,
                                                                     const float *__restrict__ g_axis,
                                                                     const unsigned char *__restrict__ cell_mask,
                                                                     int *__restrict__ hits, int *__restrict__ active) {
  extern __shared__ unsigned long long occ_lds[];
  __shared__ int nslow;
  const int tid = threadIdx.x, r2 = r * r, r3 = r2 * r;
  unsigned long long *best = occ_lds;
  float *sx = (float *)(best + OCC_THREADS), *sy = sx + OCC_THREADS, *sz = sy + OCC_THREADS;
  unsigned int *colmask = (unsigned int *)(sz + OCC_THREADS);
  float *axis = (float *)(colmask + r2);
  int *hist = (int *)(axis + r);

  for (int c = tid; c < r2; c += OCC_THREADS) {
    unsigned int m = 0;
    for (int k = 0; k < r; ++k) m |= (cell_mask[(size_t)c * r + k] ? 1u : 0u) << k;
    colmask[c] = m;
  }
  if (tid < r) axis[tid] = g_axis[tid];
  for (int c = tid; c < r3; c += OCC_THREADS) hist[c] = 0;
  __syncthreads();
  const float a0 = axis[0], scale = (float)(r - 1) / (axis[r - 1] - a0);

  for (int cloud = blockIdx.x; cloud < s; cloud += gridDim.x) {
    const float *pts = clouds + (size_t)cloud * n * 3;
    for (int base = 0; base < n; base += OCC_THREADS) {
      if (tid == 0) nslow = 0;
      __syncthreads();
      const int idx = base + tid;
      if (idx < n) {
        const float x = pts[3 * (size_t)idx], y = pts[3 * (size_t)idx + 1], z = pts[3 * (size_t)idx + 2];
        if (fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY) {  // a NaN or infinite point is counted nowhere
          const int i = occ_axis_index(x, axis, a0, scale, r), j = occ_axis_index(y, axis, a0, scale, r),
                    k = occ_axis_index(z, axis, a0, scale, r);
          if ((colmask[i * r + j] >> k) & 1u) {
            atomicAdd(&hist[(i * r + j) * r + k], 1);
          } else {
            const int slot = atomicAdd(&nslow, 1);  // < OCC_THREADS: one point per thread and chunk
            sx[slot] = x, sy[slot] = y, sz[slot] = z;
            best[slot] = ~0ull;
          }
        }
      }
      __syncthreads();
      const int L = nslow;
      if (L > 0) {  // uniform over the workgroup
        for (int t = tid; t < L * r; t += OCC_THREADS) {  // L r <= 1024 * 32
          const int p = t % L, i = t / L;  // neighbouring lanes: neighbouring points, (mostly) the same slab
          const float x = sx[p], y = sy[p], z = sz[p];
          float dx = x - axis[i];
          dx = __fmul_rn(dx, dx);
          float bd = INFINITY;
          int bc = -1;
          for (int j = 0; j < r; ++j) {
            const unsigned int m = colmask[i * r + j];
            if (m == 0u) continue;  // a column outside the sphere (neighbouring lanes mostly share the slab, so the column)
            float dy = y - axis[j];
            const float dxy = __fadd_rn(dx, __fmul_rn(dy, dy));
            for (int k = 0; k < r; ++k) {
              float dz = z - axis[k];
              const float d = __fadd_rn(dxy, __fmul_rn(dz, dz));
              // ascending flat index with a strict `<` keeps the lowest index among equals; the first kept cell is taken as it
              // is (a squared distance that overflowed to +inf is still a candidate)
              if (((m >> k) & 1u) && (d < bd || bc < 0)) bd = d, bc = (i * r + j) * r + k;
            }
          }
          // d >= 0 and not NaN: its bit pattern orders like its value
          if (bc >= 0) atomicMin(&best[p], ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned int)bc);
        }
        __syncthreads();
        if (tid < L) {
          const unsigned long long key = best[tid];
          if (key != ~0ull) atomicAdd(&hist[(int)(key & 0xffffffffull)], 1);  // ~0: no cell is kept at all
        }
      }
      __syncthreads();  // nslow is reset, and the list rewritten, only behind this
    }
    // fold this cloud into the global histograms and leave the LDS one zeroed for the next cloud
    for (int c = tid; c < r3; c += OCC_THREADS) {
      const int v = hist[c];
      if (v != 0) {
        hist[c] = 0;
        if (hits) atomicAdd(hits + c, v);
        if (active) atomicAdd(active + c, 1);
      }
    }
    __syncthreads();
  }
}

}  // namespace bdm

using namespace bdm;

extern "C" int bdm_occupancy_grid(int s, int n, int r, const float *clouds, const float *axis, const unsigned char *cell_mask,
                                  int *hits, int *active, void *stream) {
  BDM_REQUIRE(s >= 0 && n >= 1 && r >= 2, "occupancy_grid: bad sizes s=%d n=%d r=%d", s, n, r);
  BDM_REQUIRE(r <= OCC_MAX_R, "occupancy_grid: r=%d exceeds the %d^3 histogram one workgroup holds in LDS", r, OCC_MAX_R);
  BDM_REQUIRE((long long)s * n < (1ll << 31), "occupancy_grid: %d clouds of %d points exceed int", s, n);
  const size_t r3 = (size_t)r * r * r;
  for (int *out : {hits, active})
    if (out && hipMemsetAsync(out, 0, r3 * sizeof(int), (hipStream_t)stream) != hipSuccess) {
      set_error("occupancy_grid: hipMemsetAsync failed");
      return BDM_ERR_LAUNCH;
    }
  if (s == 0 || (!hits && !active)) return BDM_OK;
  BDM_REQUIRE(clouds && axis && cell_mask, "occupancy_grid: null input pointer");
  const size_t lds = occ_lds_bytes(r);
  BDM_ALLOW_LDS(occupancy_grid_kernel, lds);
  hipLaunchKernelGGL(occupancy_grid_kernel, dim3(min(s, OCC_MAX_GRID)), dim3(OCC_THREADS), lds, (hipStream_t)stream, s, n, r, clouds,
                     axis, cell_mask, hits, active);
  return launch_status("occupancy_grid");
}
