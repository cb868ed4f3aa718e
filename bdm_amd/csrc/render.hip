// render.hip -- point-cloud rendering: the K nearest points in depth per pixel and their compositing, as gfx950 kernels
// (the reference renders with pytorch3d: experiments/diffusion_utils.py:185-295, PointsRasterizer + NormWeightedCompositor /
// AlphaCompositor; pytorch3d is a third-party dependency that is not installed here, so its rules are restated: "parity unpinned").
//
// Projection and pixel centres are camera.h's, the one definition sampler_ops.hip and mesh_render.hip use as well (no FMA
// contraction there, none in this file).
// For H != W this is the per-axis convention of this project (each axis spans [-1, 1]); pytorch3d scales the longer axis by the
// aspect ratio instead -- a documented departure.
// Selection: point p is a candidate of a pixel when dx*dx + dy*dy < radius*radius (float32 product) and z >= 0 (NaN and
// behind-camera points never are); the pixel keeps the k candidates with the smallest (z, point index), ascending.  Unused slots
// hold idx = -1, z = -1, d2 = -1 (pytorch3d's fill values).  idx is the index WITHIN the cloud (0 .. n-1), not pytorch3d's index
// into the packed batch -- the second documented departure.
// Compositing over the slots j = 0 .. k-1 in slot order, w_j = 1 - d2_j / radius^2 (float32, one division, one subtraction):
//   compositor 0 (norm_weighted):  sum_j w_j f_j / max(sum_j w_j, 1e-4)
//   compositor 1 (alpha):          sum_j f_j w_j prod_{i<j} (1 - w_i)
// a pixel whose slot 0 is empty takes the background colour unchanged.
//
// Two kernels.  render_project_kernel projects every point once into the workspace, (u, v, z, -) per point.
// render_tile_kernel runs one workgroup per (shape, 16 x 16 pixel tile): it streams ALL projected points of the shape through
// LDS in chunks of 1024, keeps of each chunk only the points whose disc can reach the tile (a conservative test built from the
// same rounded differences the pixels use, compacted with wave ballots in point order), and every thread -- one pixel each --
// inserts the survivors that cover its pixel into a sorted list of K keys held in registers (K is a template parameter: a
// runtime-indexed array would go to scratch).  No atomics, no tile lists in memory: nothing depends on execution order, any number
// of points may fall into one tile, and a tile's cost beyond its own candidates is one 16-byte load and a few compares per point
// of the shape (16384 points = 64 loads per thread), which is why the count / scan / fill binning passes are not worth having at
// these sizes.
#include "../../include/bdm_hip.h"
#include "camera.h"
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)

using namespace bdm;

#define RENDER_TILE 16                        // pixels per tile side: 256 threads = 4 waves, one wave = 4 rows of 16 pixels
#define RENDER_THREADS (RENDER_TILE * RENDER_TILE)
#define RENDER_ITEMS 4                        // points each thread culls per chunk
#define RENDER_CHUNK (RENDER_THREADS * RENDER_ITEMS)
#define RENDER_MAX_K 16
#define RENDER_MAX_C 4
#define RENDER_MAX_RADIUS_PIXELS 8.f

__global__ void render_project_kernel(long long total, int ortho, const float *__restrict__ pts, const float *__restrict__ cams,
                                      int n, float4 *__restrict__ proj) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const Camera c = load_camera(cams, (size_t)(i / n));
    const float *p = pts + (size_t)i * 3;
    float u, v, zv;
    project_point(c, p[0], p[1], p[2], ortho, u, v, zv);
    proj[i] = make_float4(u, v, zv, 0.f);
  }
}

// smallest squared difference any pixel centre between `first` and `last` (the NDC centres of the tile's first and last column
// or row) can have to the coordinate u: fl(a - u) and fl(d * d) are monotone, so the differences of the pixels in between lie
// between the two computed here, and 0 is the bound when they straddle u.  A NaN u makes both differences NaN and the result
// NaN (never < radius^2); an infinite u gives +inf.
__device__ __forceinline__ float min_sq_diff(float first, float last, float u) {
  const float a = first - u, b = last - u;
  if ((a <= 0.f && b >= 0.f) || (a >= 0.f && b <= 0.f)) return 0.f;
  return fminf(a * a, b * b);
}

__device__ __forceinline__ bool key_less(float za, int ia, float zb, int ib) { return za < zb || (za == zb && ia < ib); }

template <int K>
__global__ __launch_bounds__(RENDER_THREADS) void render_tile_kernel(int n, int H, int W, int k, int C, int tiles_x, int ntiles,
                                                                      float radius2, int compositor,
                                                                      const float4 *__restrict__ proj,
                                                                      const float *__restrict__ features,
                                                                      const float *__restrict__ background, int *__restrict__ frag_idx,
                                                                      float *__restrict__ frag_z, float *__restrict__ frag_d2,
                                                                      float *__restrict__ image) {
  __shared__ float4 s_pt[RENDER_CHUNK];
  __shared__ int s_cnt[2][RENDER_ITEMS * (RENDER_THREADS / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bi = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  const int x0 = (tile % tiles_x) * RENDER_TILE, y0 = (tile / tiles_x) * RENDER_TILE;
  const int xi = x0 + (tid & (RENDER_TILE - 1)), yi = y0 + (tid / RENDER_TILE);
  const bool inside = xi < W && yi < H;
  const float xf = pixel_centre(xi, W), yf = pixel_centre(yi, H);
  // NDC centres of the tile's first and last pixel inside the image, per axis
  const int x1 = min(x0 + RENDER_TILE, W) - 1, y1 = min(y0 + RENDER_TILE, H) - 1;
  const float tx0 = pixel_centre(x0, W), tx1 = pixel_centre(x1, W);
  const float ty0 = pixel_centre(y0, H), ty1 = pixel_centre(y1, H);

  float kz[K], kd[K];
  int ki[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { kz[j] = INFINITY; kd[j] = -1.f; ki[j] = INT_MAX; }  // (inf, INT_MAX) sorts behind every candidate

  const float4 *pb = proj + (size_t)bi * n;
  int round = 0;
  for (int base = 0; base < n; base += RENDER_CHUNK, round ^= 1) {
    float4 q[RENDER_ITEMS];
    bool keep[RENDER_ITEMS];
    int off_in_wave[RENDER_ITEMS];
#pragma unroll
    for (int it = 0; it < RENDER_ITEMS; ++it) {
      const int p = base + it * RENDER_THREADS + tid;
      q[it] = p < n ? pb[p] : make_float4(0.f, 0.f, -1.f, 0.f);
      keep[it] = p < n && q[it].z >= 0.f && min_sq_diff(tx0, tx1, q[it].x) + min_sq_diff(ty0, ty1, q[it].y) < radius2;
      q[it].w = __int_as_float(p);
      const unsigned long long m = __ballot(keep[it]);
      off_in_wave[it] = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_cnt[round][it * (RENDER_THREADS / 64) + wave] = __popcll(m);
    }
    __syncthreads();  // counts of this chunk visible; every thread has left the previous chunk's candidate loop
    int total = 0, mine[RENDER_ITEMS];
#pragma unroll
    for (int s = 0; s < RENDER_ITEMS * (RENDER_THREADS / 64); ++s) {  // (item, wave, lane) order = ascending point index
      if ((s & (RENDER_THREADS / 64 - 1)) == wave) mine[s / (RENDER_THREADS / 64)] = total;
      total += s_cnt[round][s];
    }
#pragma unroll
    for (int it = 0; it < RENDER_ITEMS; ++it)
      if (keep[it]) s_pt[mine[it] + off_in_wave[it]] = q[it];  // < RENDER_CHUNK: at most one entry per point of the chunk
    __syncthreads();
    if (inside) {
      for (int s = 0; s < total; ++s) {
        const float4 c = s_pt[s];  // one address per wave: an LDS broadcast
        const float dx = xf - c.x, dy = yf - c.y;
        const float d2 = dx * dx + dy * dy;
        const int id = __float_as_int(c.w);
        if (d2 < radius2 && key_less(c.z, id, kz[K - 1], ki[K - 1])) {
#pragma unroll
          for (int j = K - 1; j >= 1; --j) {  // sorted insert, fully unrolled: the keys stay in registers
            const bool before_prev = key_less(c.z, id, kz[j - 1], ki[j - 1]);
            const bool before_cur = key_less(c.z, id, kz[j], ki[j]);
            kz[j] = before_prev ? kz[j - 1] : (before_cur ? c.z : kz[j]);
            kd[j] = before_prev ? kd[j - 1] : (before_cur ? d2 : kd[j]);
            ki[j] = before_prev ? ki[j - 1] : (before_cur ? id : ki[j]);
          }
          if (key_less(c.z, id, kz[0], ki[0])) { kz[0] = c.z; kd[0] = d2; ki[0] = id; }
        }
      }
    }
    // the next chunk writes s_cnt[round ^ 1] before its first barrier and s_pt only behind it: no barrier needed here
  }
  if (!inside) return;
  const size_t pix = ((size_t)bi * H + yi) * W + xi;
  if (frag_idx || frag_z || frag_d2) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < k) {
        const bool used = ki[j] != INT_MAX;
        if (frag_idx) frag_idx[pix * k + j] = used ? ki[j] : -1;
        if (frag_z) frag_z[pix * k + j] = used ? kz[j] : -1.f;
        if (frag_d2) frag_d2[pix * k + j] = used ? kd[j] : -1.f;
      }
    }
  }
  if (!image) return;
  float acc[RENDER_MAX_C] = {0.f, 0.f, 0.f, 0.f};
  if (ki[0] == INT_MAX) {
#pragma unroll
    for (int ch = 0; ch < RENDER_MAX_C; ++ch)
      if (ch < C) image[pix * C + ch] = background[ch];
    return;
  }
  float wsum = 0.f, trans = 1.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j < k && ki[j] != INT_MAX) {
      const float w = 1.f - kd[j] / radius2;
      const float a = compositor == 0 ? w : w * trans;
      const float *f = features ? features + ((size_t)bi * n + ki[j]) * C : nullptr;
#pragma unroll
      for (int ch = 0; ch < RENDER_MAX_C; ++ch)
        if (ch < C) acc[ch] = acc[ch] + a * (f ? f[ch] : 0.f);
      wsum = wsum + w;
      trans = trans * (1.f - w);
    }
  }
  const float den = compositor == 0 ? fmaxf(wsum, 1e-4f) : 1.f;
#pragma unroll
  for (int ch = 0; ch < RENDER_MAX_C; ++ch)
    if (ch < C) image[pix * C + ch] = compositor == 0 ? acc[ch] / den : acc[ch];
}

extern "C" size_t bdm_render_workspace_bytes(int b, int n, int h, int w, float radius) {
  (void)h; (void)w; (void)radius;
  return sizeof(float4) * (size_t)(b > 0 ? b : 0) * (size_t)(n > 0 ? n : 0);
}

template <int K>
static void launch_tiles(int grid, hipStream_t s, int n, int h, int w, int k, int c, int tiles_x, int ntiles, float r2, int compositor,
                         const float4 *proj, const float *features, const float *background, int *frag_idx, float *frag_z,
                         float *frag_d2, float *image) {
  hipLaunchKernelGGL(render_tile_kernel<K>, dim3(grid), dim3(RENDER_THREADS), 0, s, n, h, w, k, c, tiles_x, ntiles, r2, compositor,
                     proj, features, background, frag_idx, frag_z, frag_d2, image);
}

extern "C" int bdm_render_points(int b, int n, int h, int w, int k, int c, float radius, int ortho, int compositor,
                                 const float *points, const float *cameras, const float *features, const float *background,
                                 int *frag_idx, float *frag_z, float *frag_d2, float *image, void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0 && n >= 1 && h >= 1 && w >= 1, "render_points: bad sizes");
  BDM_REQUIRE(k >= 1 && k <= RENDER_MAX_K, "render_points: points per pixel %d outside 1 .. %d", k, RENDER_MAX_K);
  BDM_REQUIRE(c >= 1 && c <= RENDER_MAX_C, "render_points: %d feature channels outside 1 .. %d", c, RENDER_MAX_C);
  BDM_REQUIRE(radius >= 0.f && radius * (h > w ? h : w) * 0.5f <= RENDER_MAX_RADIUS_PIXELS,
              "render_points: radius %g spans more than %g pixels", radius, RENDER_MAX_RADIUS_PIXELS);
  BDM_REQUIRE((ortho == 0 || ortho == 1) && (compositor == 0 || compositor == 1), "render_points: bad camera or compositor flag");
  BDM_REQUIRE(image == nullptr || background != nullptr, "render_points: an image needs a background colour");
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(points && cameras && workspace, "render_points: points, cameras or workspace is NULL");
  const int tiles_x = cdiv(w, RENDER_TILE), ntiles = tiles_x * cdiv(h, RENDER_TILE);
  BDM_REQUIRE((long long)b * ntiles <= INT_MAX, "render_points: %d shapes x %d tiles exceed the grid", b, ntiles);
  hipStream_t s = (hipStream_t)stream;
  float4 *proj = (float4 *)workspace;
  const long long total = (long long)b * n;
  const int pgrid = (int)(cdivll(total, 256) < 4096 ? cdivll(total, 256) : 4096);
  hipLaunchKernelGGL(render_project_kernel, dim3(pgrid), dim3(256), 0, s, total, ortho, points, cameras, n, proj);
  const int grid = b * ntiles;
  const float r2 = radius * radius;
#define RENDER_LAUNCH(KT) launch_tiles<KT>(grid, s, n, h, w, k, c, tiles_x, ntiles, r2, compositor, proj, features, background, \
                                           frag_idx, frag_z, frag_d2, image)
  // the list length is a compile-time constant; k takes the next instantiated one (its first k slots are the k best)
  if (k <= 1) RENDER_LAUNCH(1);
  else if (k <= 2) RENDER_LAUNCH(2);
  else if (k <= 4) RENDER_LAUNCH(4);
  else if (k <= 8) RENDER_LAUNCH(8);
  else if (k <= 10) RENDER_LAUNCH(10);
  else if (k <= 12) RENDER_LAUNCH(12);
  else RENDER_LAUNCH(16);
#undef RENDER_LAUNCH
  return launch_status("render_points");
}
