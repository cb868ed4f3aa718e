// Closed triangle meshes from oriented clouds: grid Poisson reconstruction (section 22 of bdm_hip.h).
//
// bdm_surface_poisson_grid:
//   surf_box_kernel        (surface.hip) the section-12 frame with a margin of s + 3 voxels
//   (memset)               W, Vx, Vy, Vz, D, phi, the per-cloud accumulators = 0
//   psn_splat_kernel       one thread per (point, x offset, z offset), a loop over the y offsets: integer atomicAdd into W, Vx, Vy, Vz
//   psn_div_kernel         one thread per node: the integer central difference D, stored once as float32
//   per V-cycle, per GLOBAL level (side > PSN_TAIL_SIDE), one thread per node, lanes along z:
//     psn_sweep_kernel x2  damped Jacobi, ping-pong between phi and tmp
//     psn_restrict_kernel  one thread per coarse node: the residual of its 8 children and their mean -> the coarse right-hand side
//     (coarser levels)
//     psn_prolong_kernel   phi += trilinear(coarse phi)
//     psn_sweep_kernel x2
//   per V-cycle psn_tail_kernel: every level from the first of side <= PSN_TAIL_SIDE down to the coarsest in ONE launch, one workgroup
//                          per cloud, all arrays in LDS, workgroup barriers between sweeps.  When level 0 is in the tail (r = 16) the
//                          launch loops over the cycles itself: the whole solve is one launch.
//   psn_max_kernel         max |phi| as an integer atomicMax on the bits
//   psn_sample_kernel      one thread per point: trilinear phi at the sample -> integer, 64-bit wave sum, one atomicAdd per wave
//   psn_level_kernel       one thread per cloud: iso, scale -> info and the frame's spare words
//   psn_handover_kernel    SW = 4096, SU = clamp(rint((phi - iso) * scale)), the border layer raised to 1 and counted
//   psn_separate_kernel x2 the negative diagonal of a checkerboard grid face raised to 1 (no mesh edge with four faces)
//   surf_cell_kernel ... surf_rank_kernel (surface.hip): the mark stage, unchanged
// bdm_surface_poisson_density:
//   psn_density_kernel     one thread per node: the W of the 8 corners of its cell, if active, in vertex order
// The schedule depends on (r, cycles) alone; nothing is read back, nothing waits on another workgroup, every loop is bounded by a
// launch argument.  Sums are integers; every float32 operation is rounded on its own in the order of the header.
//
// The file is compiled with -ffp-contract=off and correctly rounded division (Makefile), as surface.hip.
#include "common.h"
#include "bdm_hip.h"
#include "surface_stage.h"

namespace bdm {

constexpr int PSN_TAIL_SIDE = 20;            // levels of at most this side live in LDS
constexpr int PSN_TAIL_LEVELS = 4;           // 20 -> 10 -> 5, 16 -> 8 -> 4, 14 -> 7, 12 -> 6 -> 3: at most three are used
constexpr int PSN_LDS_FLOATS = 3 * (20 * 20 * 20 + 10 * 10 * 10 + 5 * 5 * 5);   // f, phi, tmp of the largest tail: 109 500 bytes
constexpr int PSN_MAX_LEVELS = 8;            // 256 -> 4: seven
constexpr int PSN_PRE = 2, PSN_POST = 2, PSN_COARSEST = 32;
constexpr int PSN_CYCLES_MAX = 32;
constexpr int PSN_FIX = 4096;
constexpr float PSN_C7 = 0.142857149243354797f;   // float32 nearest 1 / 7: omega / 6 with omega = 6 / 7
constexpr float PSN_SU_LIMIT = 8388608.0f;        // 2^23: every SU is exact as a float32
constexpr int PSN_SEPARATE = 2;                   // passes over the checkerboard faces; even: the last one writes SU

struct PsnLevels {
  int sides[PSN_MAX_LEVELS], count, global;   // global: the number of levels of side > PSN_TAIL_SIDE; the tail's top is level `global`
};

static PsnLevels psn_levels(int r) {
  PsnLevels L;
  L.count = 0, L.global = 0;
  for (int m = r;; m /= 2) {
    L.sides[L.count++] = m;
    if (m > PSN_TAIL_SIDE) ++L.global;
    if (m % 2 != 0 || m <= 4 || L.count == PSN_MAX_LEVELS) break;
  }
  return L;
}

static bool psn_r_ok(int r) {
  if (r < SRF_R_MIN || r > SRF_R_MAX || r % 8 != 0) return false;
  const PsnLevels L = psn_levels(r);
  return L.sides[L.count - 1] <= 8 && L.global < L.count;
}

struct PsnWs {
  int *w, *vx, *vy, *vz;                                  // [b][r3] each
  float *f[PSN_MAX_LEVELS], *phi[PSN_MAX_LEVELS], *tmp[PSN_MAX_LEVELS];   // per level; f[0] = D.  The tail's levels below its top are
                                                                          // used by the one-launch-per-operator form only
  long long *isum;                                        // [b]
  int *maxbits, *used;                                    // [b] each
  size_t bytes;
};

static PsnWs psn_ws(void *ws, int b, int r, const PsnLevels &L) {
  PsnWs p;
  const size_t r3 = (size_t)r * r * r;
  char *at = (char *)ws + surf_ws_bytes(b, r);            // a multiple of 32 bytes for r % 8 == 0
  p.w = (int *)at, p.vx = p.w + b * r3, p.vy = p.vx + b * r3, p.vz = p.vy + b * r3;
  p.f[0] = (float *)(p.vz + b * r3), p.phi[0] = p.f[0] + b * r3;
  p.isum = (long long *)(p.phi[0] + b * r3);
  p.maxbits = (int *)(p.isum + b), p.used = p.maxbits + b;
  float *next = (float *)(p.used + b);
  for (int l = 0; l < L.count; ++l) {
    const size_t m3 = (size_t)b * L.sides[l] * L.sides[l] * L.sides[l];
    if (l > 0) p.f[l] = next, p.phi[l] = next + m3, next += 2 * m3;
    p.tmp[l] = next, next += m3;
  }
  p.bytes = (size_t)((char *)next - (char *)ws);
  return p;
}

// ---- the arithmetic of the solve, shared by the global kernels and the LDS tail -------------------------------------------------------
__device__ __forceinline__ float psn_lap(float c, float xm, float xp, float ym, float yp, float zm, float zp) {
  const float sum = __fadd_rn(__fadd_rn(__fadd_rn(xm, xp), __fadd_rn(ym, yp)), __fadd_rn(zm, zp));
  return __fsub_rn(sum, __fmul_rn(6.0f, c));
}

// (S - 6 phi) at node (i, j, k) = g of a level of side m; the ghost beyond a face is minus the edge value
__device__ __forceinline__ float psn_lap_at(const float *p, int m, int i, int j, int k, int g) {
  const float c = p[g];
  const float xm = i > 0 ? p[g - m * m] : -c, xp = i < m - 1 ? p[g + m * m] : -c;
  const float ym = j > 0 ? p[g - m] : -c, yp = j < m - 1 ? p[g + m] : -c;
  const float zm = k > 0 ? p[g - 1] : -c, zp = k < m - 1 ? p[g + 1] : -c;
  return psn_lap(c, xm, xp, ym, yp, zm, zp);
}

__device__ __forceinline__ float psn_relax(float c, float lap, float f, float h2) {
  return __fadd_rn(c, __fmul_rn(__fsub_rn(lap, __fmul_rn(h2, f)), PSN_C7));
}

__device__ __forceinline__ float psn_mix(float near, float far) { return __fadd_rn(__fmul_rn(0.75f, near), __fmul_rn(0.25f, far)); }

// the coarse value at (x, y, z), each possibly one step outside 0 .. mc - 1: minus the clamped value per axis that is outside
__device__ __forceinline__ float psn_coarse(const float *e, int mc, int x, int y, int z) {
  bool flip = false;
  if (x < 0) x = 0, flip = !flip;
  if (x > mc - 1) x = mc - 1, flip = !flip;
  if (y < 0) y = 0, flip = !flip;
  if (y > mc - 1) y = mc - 1, flip = !flip;
  if (z < 0) z = 0, flip = !flip;
  if (z > mc - 1) z = mc - 1, flip = !flip;
  const float v = e[(x * mc + y) * mc + z];   // all three clamped into the level
  return flip ? -v : v;
}

// trilinear prolongation to the fine node (i, j, k): along z, then y, then x; child 2 K + a takes 0.75 e[K] + 0.25 e[K - 1 + 2 a]
__device__ __forceinline__ float psn_prolong_at(const float *e, int mc, int i, int j, int k) {
  const int I = i >> 1, J = j >> 1, K = k >> 1, I2 = I - 1 + 2 * (i & 1), J2 = J - 1 + 2 * (j & 1), K2 = K - 1 + 2 * (k & 1);
  const float z00 = psn_mix(psn_coarse(e, mc, I, J, K), psn_coarse(e, mc, I, J, K2));
  const float z01 = psn_mix(psn_coarse(e, mc, I, J2, K), psn_coarse(e, mc, I, J2, K2));
  const float z10 = psn_mix(psn_coarse(e, mc, I2, J, K), psn_coarse(e, mc, I2, J, K2));
  const float z11 = psn_mix(psn_coarse(e, mc, I2, J2, K), psn_coarse(e, mc, I2, J2, K2));
  return psn_mix(psn_mix(z00, z01), psn_mix(z10, z11));
}

// the mean of the residuals f - (S - 6 phi) / h2 of the 8 children of coarse node (I, J, K), summed in lexicographic (a, b, c)
__device__ __forceinline__ float psn_restrict_at(const float *phi, const float *f, int m, float ih2, int I, int J, int K) {
  float sum = 0.0f;
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) {
    const int i = 2 * I + (ch >> 2), j = 2 * J + ((ch >> 1) & 1), k = 2 * K + (ch & 1), g = (i * m + j) * m + k;
    const float res = __fsub_rn(f[g], __fmul_rn(psn_lap_at(phi, m, i, j, k, g), ih2));
    sum = ch == 0 ? res : __fadd_rn(sum, res);
  }
  return __fmul_rn(sum, 0.125f);
}

// ---- splat and divergence ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool psn_sample_q(const float *__restrict__ points, const float *__restrict__ normals, const float *cp, size_t row,
                                             int r, float q[3], float nr[3]) {
  const float rm1 = (float)(r - 1), mid = __fmul_rn(0.5f, rm1);
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = points[row + a];
    nr[a] = normals[row + a];
    ok = ok && finite1(p) && finite1(nr[a]);
    q[a] = __fadd_rn(__fmul_rn(__fsub_rn(p, cp[a]), cp[3]), mid);
  }
  return ok && q[0] >= 0.0f && q[0] <= rm1 && q[1] >= 0.0f && q[1] <= rm1 && q[2] >= 0.0f && q[2] <= rm1;   // NaN fails too
}

__device__ __forceinline__ int psn_term(float w3, float na) {
  const float v = rintf(__fmul_rn(__fmul_rn(w3, na), (float)PSN_FIX));
  return v != v ? 0 : (int)fminf(fmaxf(v, -(float)PSN_FIX), (float)PSN_FIX);
}

__global__ __launch_bounds__(SRF_THREADS) void psn_splat_kernel(int b, int n, int r, int s, const float *__restrict__ points,
                                                                const float *__restrict__ normals, const float *__restrict__ par,
                                                                int *__restrict__ gw, int *__restrict__ gx, int *__restrict__ gy_,
                                                                int *__restrict__ gz_) {
  const int side = 2 * s, per = side * side;
  const int item = blockIdx.x * SRF_THREADS + threadIdx.x;   // n * per <= 65536 * 64
  if (item >= n * per) return;
  const int i = item / per, ox = (item % per) / side - s + 1, oz = item % side - s + 1;
  const float s2 = (float)(s * s);
  const size_t r3 = (size_t)r * r * r;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const float *cp = par + (size_t)cloud * SRF_PAR;
    if (reinterpret_cast<const int *>(cp)[4] == 0) continue;
    float q[3], nr[3];
    if (!psn_sample_q(points, normals, cp, ((size_t)cloud * n + i) * 3, r, q, nr)) continue;
    const int gx0 = (int)floorf(q[0]) + ox, gz0 = (int)floorf(q[2]) + oz, by = (int)floorf(q[1]);
    if (gx0 < 0 || gx0 >= r || gz0 < 0 || gz0 >= r) continue;
    const float dx = __fsub_rn((float)gx0, q[0]), dz = __fsub_rn((float)gz0, q[2]);
    for (int oy = -s + 1; oy <= s; ++oy) {
      const int gy0 = by + oy;
      if (gy0 < 0 || gy0 >= r) continue;
      const float dy = __fsub_rn((float)gy0, q[1]);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      const float t = __fsub_rn(s2, d2);
      if (!(t > 0.0f)) continue;
      const float w = __fdiv_rn(t, s2);
      const float w3 = __fmul_rn(__fmul_rn(w, w), w);
      const int W = (int)rintf(__fmul_rn(w3, (float)PSN_FIX));
      const int X = psn_term(w3, nr[0]), Y = psn_term(w3, nr[1]), Z = psn_term(w3, nr[2]);
      const size_t node = (size_t)cloud * r3 + ((size_t)gx0 * r + gy0) * r + gz0;   // all three coordinates checked against [0, r)
      if (W) atomicAdd(&gw[node], W);
      if (X) atomicAdd(&gx[node], X);
      if (Y) atomicAdd(&gy_[node], Y);
      if (Z) atomicAdd(&gz_[node], Z);
    }
  }
}

__global__ __launch_bounds__(SRF_THREADS) void psn_div_kernel(int b, int r, const int *__restrict__ vx, const int *__restrict__ vy,
                                                              const int *__restrict__ vz, float *__restrict__ d) {
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= r3) return;
  const int k = g % r, j = (g / r) % r, i = g / (r * r);
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t at = (size_t)cloud * r3 + g;
    int sum = (i < r - 1 ? vx[at + r * r] : 0) - (i > 0 ? vx[at - r * r] : 0);   // |sum| <= 6 * 65536 * 4096 < 2^31
    sum += (j < r - 1 ? vy[at + r] : 0) - (j > 0 ? vy[at - r] : 0);
    sum += (k < r - 1 ? vz[at + 1] : 0) - (k > 0 ? vz[at - 1] : 0);
    d[at] = __int2float_rn(sum);
  }
}

// ---- the global levels -------------------------------------------------------------------------------------------------------------
// out = one damped-Jacobi sweep of in; zero_in: in is taken as zero everywhere and not read
__global__ __launch_bounds__(SRF_THREADS) void psn_sweep_kernel(int b, int m, float h2, int zero_in, const float *__restrict__ in,
                                                                const float *__restrict__ f, float *__restrict__ out) {
  const int m3 = m * m * m, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= m3) return;
  const int k = g % m, j = (g / m) % m, i = g / (m * m);
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t base = (size_t)cloud * m3;
    const float c = zero_in ? 0.0f : in[base + g];
    const float lap = zero_in ? psn_lap(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f) : psn_lap_at(in + base, m, i, j, k, g);
    out[base + g] = psn_relax(c, lap, f[base + g], h2);
  }
}

__global__ __launch_bounds__(SRF_THREADS) void psn_restrict_kernel(int b, int m, float ih2, const float *__restrict__ phi,
                                                                   const float *__restrict__ f, float *__restrict__ fc) {
  const int mc = m / 2, mc3 = mc * mc * mc, m3 = m * m * m, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= mc3) return;
  const int K = g % mc, J = (g / mc) % mc, I = g / (mc * mc);   // the children 2 I + a < m
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y)
    fc[(size_t)cloud * mc3 + g] = psn_restrict_at(phi + (size_t)cloud * m3, f + (size_t)cloud * m3, m, ih2, I, J, K);
}

__global__ __launch_bounds__(SRF_THREADS) void psn_prolong_kernel(int b, int m, const float *__restrict__ e, float *__restrict__ phi) {
  const int mc = m / 2, mc3 = mc * mc * mc, m3 = m * m * m, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= m3) return;
  const int k = g % m, j = (g / m) % m, i = g / (m * m);
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t at = (size_t)cloud * m3 + g;
    phi[at] = __fadd_rn(phi[at], psn_prolong_at(e + (size_t)cloud * mc3, mc, i, j, k));
  }
}

// ---- the LDS tail ------------------------------------------------------------------------------------------------------------------
// `count` sweeps between cur and nxt (both in LDS); returns with the result in cur (the pointers are swapped)
__device__ void psn_lds_sweeps(float *&cur, float *&nxt, const float *f, int m, float h2, int count) {
  const int m3 = m * m * m;
  for (int it = 0; it < count; ++it) {
    for (int g = threadIdx.x; g < m3; g += SRF_WIDE) {
      const int k = g % m, j = (g / m) % m, i = g / (m * m);
      nxt[g] = psn_relax(cur[g], psn_lap_at(cur, m, i, j, k, g), f[g], h2);
    }
    __syncthreads();
    float *t = cur;
    cur = nxt, nxt = t;
  }
}

__device__ void psn_lds_zero(float *p, int m3) {
  for (int g = threadIdx.x; g < m3; g += SRF_WIDE) p[g] = 0.0f;
  __syncthreads();
}

// levels top .. top + nlev - 1 of sides m0, m0 / 2, ...; h2 of the top level is h2_top; `cycles` V-cycles on the top level from zero
__global__ __launch_bounds__(SRF_WIDE) void psn_tail_kernel(int m0, int nlev, float h2_top, int cycles, int coarsest,
                                                            const float *__restrict__ f_in, float *__restrict__ phi_out) {
  __shared__ float lds[PSN_LDS_FLOATS];
  float *f[PSN_TAIL_LEVELS], *phi[PSN_TAIL_LEVELS], *tmp[PSN_TAIL_LEVELS];
  int side[PSN_TAIL_LEVELS];
  float h2[PSN_TAIL_LEVELS];
  {
    float *at = lds;   // the host checked 3 * sum m_t^3 <= PSN_LDS_FLOATS and nlev <= PSN_TAIL_LEVELS
    int m = m0;
    float h = h2_top;
    for (int t = 0; t < nlev; ++t) {
      const int m3 = m * m * m;
      side[t] = m, h2[t] = h, f[t] = at, phi[t] = at + m3, tmp[t] = at + 2 * m3;
      at += 3 * m3, m /= 2, h *= 4.0f;
    }
  }
  const int top3 = m0 * m0 * m0;
  const size_t base = (size_t)blockIdx.x * top3;
  for (int g = threadIdx.x; g < top3; g += SRF_WIDE) f[0][g] = f_in[base + g], phi[0][g] = 0.0f;
  __syncthreads();
  const int last = nlev - 1;
  for (int cyc = 0; cyc < cycles; ++cyc) {
    for (int t = 0; t < last; ++t) {
      const int m = side[t], mc = side[t + 1], mc3 = mc * mc * mc;
      if (t > 0) psn_lds_zero(phi[t], m * m * m);
      psn_lds_sweeps(phi[t], tmp[t], f[t], m, h2[t], PSN_PRE);
      const float ih2 = 1.0f / h2[t];   // a power of two: exact
      for (int g = threadIdx.x; g < mc3; g += SRF_WIDE) f[t + 1][g] = psn_restrict_at(phi[t], f[t], m, ih2, g / (mc * mc), (g / mc) % mc, g % mc);
      __syncthreads();
    }
    psn_lds_zero(phi[last], side[last] * side[last] * side[last]);
    psn_lds_sweeps(phi[last], tmp[last], f[last], side[last], h2[last], coarsest);
    for (int t = last - 1; t >= 0; --t) {
      const int m = side[t], m3 = m * m * m;
      for (int g = threadIdx.x; g < m3; g += SRF_WIDE)
        phi[t][g] = __fadd_rn(phi[t][g], psn_prolong_at(phi[t + 1], side[t + 1], g / (m * m), (g / m) % m, g % m));
      __syncthreads();
      psn_lds_sweeps(phi[t], tmp[t], f[t], m, h2[t], PSN_POST);
    }
  }
  for (int g = threadIdx.x; g < top3; g += SRF_WIDE) phi_out[base + g] = phi[0][g];
}

// ---- level, hand-over, density ---------------------------------------------------------------------------------------------------
// A workgroup covers PSN_MAX_SPAN nodes.  A wave whose maximum does not exceed what the cloud's word already holds leaves the atomic
// out (the word only grows, so a stale read costs an atomic, never the result): one atomic per wave on one word per cloud serialised
// and made this kernel the longest of the hand-over at r = 128.
constexpr int PSN_MAX_SPAN = 16 * SRF_THREADS;

__global__ __launch_bounds__(SRF_THREADS) void psn_max_kernel(int b, int r, const float *__restrict__ phi, int *__restrict__ maxbits) {
  const int r3 = r * r * r, first = blockIdx.x * PSN_MAX_SPAN + threadIdx.x;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    int bits = 0;
    for (int g = first; g < min(r3, (int)(blockIdx.x + 1) * PSN_MAX_SPAN); g += SRF_THREADS)
      bits = max(bits, __float_as_int(phi[(size_t)cloud * r3 + g]) & 0x7fffffff);   // |phi| >= 0: its bits order as integers
    for (int m = 32; m >= 1; m >>= 1) bits = max(bits, __shfl_xor(bits, m));
    if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(&maxbits[cloud], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&maxbits[cloud], bits);
  }
}

__device__ __forceinline__ float psn_lerp(float a, float c, float t) { return __fadd_rn(a, __fmul_rn(t, __fsub_rn(c, a))); }

__global__ __launch_bounds__(SRF_THREADS) void psn_sample_kernel(int b, int n, int r, const float *__restrict__ points,
                                                                 const float *__restrict__ normals, const float *__restrict__ par,
                                                                 const float *__restrict__ phi, const int *__restrict__ maxbits,
                                                                 long long *__restrict__ isum, int *__restrict__ used) {
  const int i = blockIdx.x * SRF_THREADS + threadIdx.x, r3 = r * r * r;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const float *cp = par + (size_t)cloud * SRF_PAR;
    const float big = __int_as_float(maxbits[cloud]);
    long long term = 0;
    int one = 0;
    float q[3], nr[3];
    if (i < n && reinterpret_cast<const int *>(cp)[4] != 0 && big != 0.0f &&
        psn_sample_q(points, normals, cp, ((size_t)cloud * n + i) * 3, r, q, nr)) {
      const float qs = __fmul_rn(__fdiv_rn(4194304.0f, big), 256.0f);
      int g0[3];
      float t[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) g0[a] = min((int)floorf(q[a]), r - 2), t[a] = __fsub_rn(q[a], (float)g0[a]);   // 0 <= g0 <= r - 2
      const float *p = phi + (size_t)cloud * r3 + ((size_t)g0[0] * r + g0[1]) * r + g0[2];
      const float y00 = psn_lerp(p[0], p[1], t[2]), y01 = psn_lerp(p[r], p[r + 1], t[2]);
      const float y10 = psn_lerp(p[r * r], p[r * r + 1], t[2]), y11 = psn_lerp(p[r * r + r], p[r * r + r + 1], t[2]);
      const float v = psn_lerp(psn_lerp(y00, y01, t[1]), psn_lerp(y10, y11, t[1]), t[0]);
      term = (long long)rintf(__fmul_rn(v, qs)), one = 1;   // |v| <= max |phi| up to rounding: |term| <= 2^30 + 1
    }
    for (int m = 32; m >= 1; m >>= 1) term += __shfl_xor(term, m), one += __shfl_xor(one, m);
    if ((threadIdx.x & 63) == 0 && one) {
      atomicAdd(reinterpret_cast<unsigned long long *>(&isum[cloud]), (unsigned long long)term);
      atomicAdd(&used[cloud], one);
    }
  }
}

__global__ __launch_bounds__(64) void psn_level_kernel(int b, const int *__restrict__ maxbits, const long long *__restrict__ isum,
                                                       const int *__restrict__ used, float *__restrict__ par, int *__restrict__ info) {
  const int cloud = blockIdx.x * 64 + threadIdx.x;
  if (cloud >= b) return;
  const float big = __int_as_float(maxbits[cloud]);
  float iso = 0.0f, scale = 0.0f;
  if (big != 0.0f && used[cloud] > 0) {
    scale = __fdiv_rn(4194304.0f, big);
    iso = __fdiv_rn(__fdiv_rn(__ll2float_rn(isum[cloud]), __int2float_rn(used[cloud])), __fmul_rn(scale, 256.0f));
  }
  par[(size_t)cloud * SRF_PAR + 5] = iso, par[(size_t)cloud * SRF_PAR + 6] = scale;
  info[3 * (size_t)cloud] = 0, info[3 * (size_t)cloud + 1] = __float_as_int(iso), info[3 * (size_t)cloud + 2] = __float_as_int(scale);
}

__global__ __launch_bounds__(SRF_THREADS) void psn_handover_kernel(int b, int r, const float *__restrict__ phi, const float *__restrict__ par,
                                                                   int *__restrict__ sw, int *__restrict__ su, int *__restrict__ info) {
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  const int k = g % r, j = (g / r) % r, i = g / (r * r);
  const bool border = i == 0 || i == r - 1 || j == 0 || j == r - 1 || k == 0 || k == r - 1;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const float iso = par[(size_t)cloud * SRF_PAR + 5], scale = par[(size_t)cloud * SRF_PAR + 6];
    bool raised = false;
    if (g < r3) {
      const size_t at = (size_t)cloud * r3 + g;
      int W = 0, U = 0;
      if (scale != 0.0f) {
        const float u = rintf(__fmul_rn(__fsub_rn(phi[at], iso), scale));
        W = PSN_FIX, U = (int)fminf(fmaxf(u, -PSN_SU_LIMIT), PSN_SU_LIMIT);
        if (border && U < 1) U = 1, raised = true;
      }
      sw[at] = W, su[at] = U;
    }
    const unsigned long long mask = __ballot(raised);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&info[3 * (size_t)cloud], __popcll(mask));
  }
}

// One pass of step 6's separation: a negative node that lies on a grid face whose other diagonal is non-negative while the node across
// the face is negative too becomes 1; every node is judged on `in` and written to `out`.  Surface nets put four faces on the edge
// between the two cells on either side of such a face.
__global__ __launch_bounds__(SRF_THREADS) void psn_separate_kernel(int b, int r, const int *__restrict__ in, int *__restrict__ out) {
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= r3) return;
  const int co[3] = {g / (r * r), (g / r) % r, g % r}, st[3] = {r * r, r, 1};
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const int *p = in + (size_t)cloud * r3;
    int value = p[g];
    if (value < 0) {
      bool hit = false;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const int u = pl == 2 ? 1 : 0, v = pl == 0 ? 1 : 2;   // the planes (x, y), (x, z), (y, z)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const int su = (f & 1) ? 1 : -1, sv = (f & 2) ? 1 : -1;
          const int cu = co[u] + su, cv = co[v] + sv;
          if (cu < 0 || cu >= r || cv < 0 || cv >= r) continue;   // the face's three other nodes are inside the grid
          hit = hit || (p[g + su * st[u] + sv * st[v]] < 0 && p[g + su * st[u]] >= 0 && p[g + sv * st[v]] >= 0);
        }
      }
      if (hit) value = 1;
    }
    out[(size_t)cloud * r3 + g] = value;
  }
}

__global__ __launch_bounds__(SRF_THREADS) void psn_density_kernel(int b, int r, const int *__restrict__ gw, const int *__restrict__ cell,
                                                                  const long long *__restrict__ vert_offsets, float *__restrict__ density) {
  const int r3 = r * r * r, g = blockIdx.x * SRF_THREADS + threadIdx.x;
  if (g >= r3) return;
  for (int cloud = blockIdx.y; cloud < b; cloud += gridDim.y) {
    const size_t base = (size_t)cloud * r3;
    const int id = cell[base + g];
    if (id < 0) continue;   // an active cell has i, j, k < r - 1: its corners are inside the grid
    int sum = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) sum += gw[base + g + (c >> 2) * r * r + ((c >> 1) & 1) * r + (c & 1)];   // <= 8 * 2^28: a 64-bit sum is not needed
    density[(size_t)vert_offsets[cloud] + (size_t)id] = __fmul_rn(__int2float_rn(sum), 1.0f / (8.0f * (float)PSN_FIX));
  }
}

static int psn_check_r(const char *what, int r) {
  BDM_REQUIRE(psn_r_ok(r), "%s: r=%d is not accepted (a multiple of 8 in 16..256 that halves to a side of at most 8)", what, r);
  return BDM_OK;
}

// one V-cycle: the levels l < G run in global memory, one launch per operator; the others in the LDS tail, or, with per_level (the
// form the tail is measured against, tools/surface_poisson_bench.py), in global memory as well, the coarsest level sweep by sweep
static void psn_cycle(int b, const PsnLevels &L, const PsnWs &p, bool per_level, unsigned gy, hipStream_t st) {
  const int G = per_level ? L.count - 1 : L.global;
  for (int l = 0; l < G; ++l) {
    const int m = L.sides[l], m3 = m * m * m, mc3 = m3 / 8;
    const float h2 = (float)(1 << (2 * l));
    const dim3 grid((unsigned)cdiv(m3, SRF_THREADS), gy), block(SRF_THREADS);
    // level 0 continues from the last cycle; a coarser level starts from zero
    hipLaunchKernelGGL(psn_sweep_kernel, grid, block, 0, st, b, m, h2, l > 0 ? 1 : 0, p.phi[l], p.f[l], p.tmp[l]);
    hipLaunchKernelGGL(psn_sweep_kernel, grid, block, 0, st, b, m, h2, 0, p.tmp[l], p.f[l], p.phi[l]);
    hipLaunchKernelGGL(psn_restrict_kernel, dim3((unsigned)cdiv(mc3, SRF_THREADS), gy), block, 0, st, b, m, 1.0f / h2, p.phi[l], p.f[l],
                       p.f[l + 1]);
  }
  if (per_level) {
    const int m = L.sides[G], m3 = m * m * m;
    const dim3 grid((unsigned)cdiv(m3, SRF_THREADS), gy), block(SRF_THREADS);
    for (int it = 0; it < PSN_COARSEST; ++it)   // an even count: the last sweep writes phi
      hipLaunchKernelGGL(psn_sweep_kernel, grid, block, 0, st, b, m, (float)(1 << (2 * G)), it == 0 && G > 0 ? 1 : 0, it % 2 ? p.tmp[G] : p.phi[G],
                         p.f[G], it % 2 ? p.phi[G] : p.tmp[G]);
  } else {
    hipLaunchKernelGGL(psn_tail_kernel, dim3((unsigned)b), dim3(SRF_WIDE), 0, st, L.sides[G], L.count - G, (float)(1 << (2 * G)), 1,
                       PSN_COARSEST, p.f[G], p.phi[G]);
  }
  for (int l = G - 1; l >= 0; --l) {
    const int m = L.sides[l], m3 = m * m * m;
    const float h2 = (float)(1 << (2 * l));
    const dim3 grid((unsigned)cdiv(m3, SRF_THREADS), gy), block(SRF_THREADS);
    hipLaunchKernelGGL(psn_prolong_kernel, grid, block, 0, st, b, m, p.phi[l + 1], p.phi[l]);
    hipLaunchKernelGGL(psn_sweep_kernel, grid, block, 0, st, b, m, h2, 0, p.phi[l], p.f[l], p.tmp[l]);
    hipLaunchKernelGGL(psn_sweep_kernel, grid, block, 0, st, b, m, h2, 0, p.tmp[l], p.f[l], p.phi[l]);
  }
}

}  // namespace bdm

using namespace bdm;

extern "C" size_t bdm_surface_poisson_workspace_bytes(int b, int n, int r, int s) {
  if (!surf_sizes_ok(b, n, r, s) || !psn_r_ok(r)) return 0;
  return psn_ws(nullptr, b, r, psn_levels(r)).bytes;
}

// stages: bit 0 frame, splat and divergence; bit 1 the solve; bit 2 level, hand-over and mark
static int psn_run(int b, int n, int r, int s, int cycles, int stages, bool per_level, const float *points, const float *normals, int *counts,
                   int *info, void *workspace, void *stream) {
  if (int rc = surf_check_sizes("surface_poisson_grid", b, n, r, s)) return rc;
  if (int rc = psn_check_r("surface_poisson_grid", r)) return rc;
  BDM_REQUIRE(cycles >= 1 && cycles <= PSN_CYCLES_MAX, "surface_poisson_grid: cycles=%d outside 1..%d", cycles, PSN_CYCLES_MAX);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(points && normals && counts && info && workspace, "surface_poisson_grid: null pointer");
  const void *ins[2] = {points, normals}, *outs[3] = {counts, info, workspace};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 2; ++i) BDM_REQUIRE(outs[o] != ins[i], "surface_poisson_grid: an output or the workspace aliases an input");
    for (int q = 0; q < o; ++q) BDM_REQUIRE(outs[o] != outs[q], "surface_poisson_grid: counts, info and the workspace alias each other");
  }
  const PsnLevels L = psn_levels(r);
  {
    int floats = 0;
    for (int l = L.global; l < L.count; ++l) floats += 3 * L.sides[l] * L.sides[l] * L.sides[l];
    BDM_REQUIRE(L.count - L.global <= PSN_TAIL_LEVELS && floats <= PSN_LDS_FLOATS, "surface_poisson_grid: the tail of r=%d does not fit LDS", r);
  }
  const SurfWs w = surf_ws(workspace, b, r);
  const PsnWs p = psn_ws(workspace, b, r, L);
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)b < SRF_GRID_Y ? (unsigned)b : SRF_GRID_Y;
  const dim3 nodes((unsigned)w.nb, gy), block(SRF_THREADS);
  if (stages & 1) {
    surf_launch_frame(b, n, r, s + 3, points, normals, w, counts, st);
    // W, Vx, Vy, Vz, D, phi and the accumulators lie together
    if (hipMemsetAsync(p.w, 0, (size_t)((char *)(p.used + b) - (char *)p.w), st) != hipSuccess) return launch_status("surface_poisson_grid (memset)");
    hipLaunchKernelGGL(psn_splat_kernel, dim3((unsigned)cdiv(n * 4 * s * s, SRF_THREADS), gy), block, 0, st, b, n, r, s, points, normals, w.par,
                       p.w, p.vx, p.vy, p.vz);
    hipLaunchKernelGGL(psn_div_kernel, nodes, block, 0, st, b, r, p.vx, p.vy, p.vz, p.f[0]);
  }
  if (stages & 2) {
    if (L.global == 0 && !per_level) {
      hipLaunchKernelGGL(psn_tail_kernel, dim3((unsigned)b), dim3(SRF_WIDE), 0, st, r, L.count, 1.0f, cycles, PSN_COARSEST, p.f[0], p.phi[0]);
    } else {
      for (int c = 0; c < cycles; ++c) psn_cycle(b, L, p, per_level, gy, st);
    }
  }
  if (!(stages & 4)) return launch_status("surface_poisson_grid");
  hipLaunchKernelGGL(psn_max_kernel, dim3((unsigned)cdiv(w.r3, PSN_MAX_SPAN), gy), block, 0, st, b, r, p.phi[0], p.maxbits);
  hipLaunchKernelGGL(psn_sample_kernel, dim3((unsigned)cdiv(n, SRF_THREADS), gy), block, 0, st, b, n, r, points, normals, w.par, p.phi[0],
                     p.maxbits, p.isum, p.used);
  hipLaunchKernelGGL(psn_level_kernel, dim3((unsigned)cdiv(b, 64)), dim3(64), 0, st, b, p.maxbits, p.isum, p.used, w.par, info);
  hipLaunchKernelGGL(psn_handover_kernel, nodes, block, 0, st, b, r, p.phi[0], w.par, w.sw, w.su, info);
  for (int pass = 0; pass < PSN_SEPARATE; ++pass)   // between SU and the cell map's place, which the mark stage writes afterwards
    hipLaunchKernelGGL(psn_separate_kernel, nodes, block, 0, st, b, r, pass % 2 ? w.cell : w.su, pass % 2 ? w.su : w.cell);
  surf_launch_mark(b, r, 1, w, counts, st);
  return launch_status("surface_poisson_grid");
}

extern "C" int bdm_surface_poisson_grid(int b, int n, int r, int s, int cycles, const float *points, const float *normals, int *counts,
                                        int *info, void *workspace, void *stream) {
  return psn_run(b, n, r, s, cycles, 7, false, points, normals, counts, info, workspace, stream);
}

extern "C" int bdm_surface_poisson_grid_staged(int b, int n, int r, int s, int cycles, int stages, int per_level, const float *points,
                                               const float *normals, int *counts, int *info, void *workspace, void *stream) {
  BDM_REQUIRE(stages >= 1 && stages <= 7 && (per_level == 0 || per_level == 1), "surface_poisson_grid_staged: stages=%d per_level=%d", stages,
              per_level);
  return psn_run(b, n, r, s, cycles, stages, per_level != 0, points, normals, counts, info, workspace, stream);
}

extern "C" int bdm_surface_poisson_density(int b, int r, const long long *vert_offsets, float *density, void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0 && (long long)b * r * r * r < (1ll << 31), "surface_poisson_density: bad sizes b=%d r=%d", b, r);
  if (int rc = psn_check_r("surface_poisson_density", r)) return rc;
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(vert_offsets && density && workspace, "surface_poisson_density: null pointer");
  BDM_REQUIRE((const void *)density != (const void *)vert_offsets && (void *)density != workspace && (const void *)vert_offsets != workspace,
              "surface_poisson_density: density, the offsets and the workspace alias each other");
  const SurfWs w = surf_ws(workspace, b, r);
  const PsnWs p = psn_ws(workspace, b, r, psn_levels(r));
  const unsigned gy = (unsigned)b < SRF_GRID_Y ? (unsigned)b : SRF_GRID_Y;
  hipLaunchKernelGGL(psn_density_kernel, dim3((unsigned)w.nb, gy), dim3(SRF_THREADS), 0, (hipStream_t)stream, b, r, p.w, w.cell, vert_offsets,
                     density);
  return launch_status("surface_poisson_density");
}
