// mesh_render.hip -- triangle meshes to pixels: one face per pixel, as gfx950 kernels (bdm_hip.h section 13, DESIGN.md section 17;
// restates pytorch3d's MeshRasterizer at faces_per_pixel = 1, blur_radius = 0 and a Gouraud / flat shader; pytorch3d is not
// installed, so the rule is this project's own text: "parity unpinned").
//
// The rule in one paragraph: vertices are projected in float32, operation by operation (camera.h; no FMA contraction, and in this
// file division correctly rounded), and snapped to 1/256 pixel; coverage is decided by three int64 edge functions at the pixel centre with a
// half-plane rule for centres ON an edge; depth and barycentrics are float32 quotients of those integers; the pixel keeps the
// smallest (bits of z) << 32 | face index.  Nothing depends on execution order: the only atomic is an integer minimum.
//
// Three kernels, after send_offsets (ragged.h) has put the two host offset arrays into the workspace.
//   mesh_vertex_kernel    one thread per vertex: view transform, NDC, screen, snap -> (SX, SY, zv, usable), 16 bytes per vertex.
//   mesh_raster_kernel    one thread per face: set-up (face_setup), the bounding box of the pixel centres it can cover clamped to
//                         the image, then every centre of the box through face_pixel and, for a covered one, atomicMin on the
//                         64-bit key image (preset to all ones).  A box of more than 16 x 16 pixels is not walked by its lane:
//                         after the small faces the wave takes its large faces one at a time (ballot), all 64 lanes spread over
//                         the box, so a full-screen triangle costs a wave and not a thread.  The key is read before the atomic
//                         and a losing fragment skipped: the minimum only ever decreases, so a stale read can only let through
//                         an atomic that then changes nothing.
//   mesh_resolve_kernel   one thread per pixel: the winner's face_setup and face_pixel again -- the same device functions, the
//                         same bits -- then pix_to_face, zbuf, bary (swapped back to the face's own order) and the image.
// The tile-binned form of render.hip (one workgroup per tile streams ALL faces) needs no atomics but reads an 88 000-face mesh
// 196 times at 224 x 224; here every face is read once and costs its own box.
#include "../../include/bdm_hip.h"
#include "camera.h"
#include "common.h"
#include "ragged.h"

#include <limits.h>

#pragma clang fp contract(off)

using namespace bdm;

#define MESH_THREADS 256
#define MESH_SMALL_BOX 16                 // boxes up to 16 x 16 pixel centres are walked by the face's own lane
#define MESH_MAX_C 4
#define MESH_MAX_SIDE 4096
#define MESH_SNAP 256                     // sub-pixel positions per pixel
#define MESH_GUARD 4194304.f              // 2^22: |SX|, |SY| beyond it make the vertex unusable (edge products stay below 2^48)
#define MESH_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

// the mesh that owns packed row `row`: the m in [0, b) with first[m] <= row < first[m + 1] (empty meshes own nothing).
// first[0] == 0 <= row < first[b]; at most 32 halvings for b < 2^31.
__device__ __forceinline__ int mesh_of_row(const long long *__restrict__ first, int b, long long row) {
  int lo = 0, hi = b;  // invariant: first[lo] <= row < first[hi]
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const int mid = lo + ((hi - lo) >> 1);
    if (first[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_vertex_kernel(int b, int sum_v, int ortho, float half_w, float half_h,
                                                                   const float *__restrict__ verts, const float *__restrict__ cams,
                                                                   const long long *__restrict__ vert_first, int4 *__restrict__ vrec) {
  const int i = blockIdx.x * MESH_THREADS + threadIdx.x;  // the grid covers sum_v < 2^31 exactly once
  if (i >= sum_v) return;
  const Camera c = load_camera(cams, (size_t)mesh_of_row(vert_first, b, i));
  const float *p = verts + (size_t)i * 3;
  float u, v, zv;
  project_point(c, p[0], p[1], p[2], ortho, u, v, zv);
  const float px = ((1.f - u) * half_w) * (float)MESH_SNAP, py = ((1.f - v) * half_h) * (float)MESH_SNAP;
  // NaN fails every comparison; fabsf(inf) <= 2^22 is false
  const bool usable = zv > 0.f && zv < INFINITY && fabsf(px) <= MESH_GUARD && fabsf(py) <= MESH_GUARD;
  vrec[i] = usable ? make_int4((int)rintf(px), (int)rintf(py), __float_as_int(zv), 1) : make_int4(0, 0, 0, 0);
}

struct MeshFace {
  int x0, y0, x1, y1, x2, y2;  // snapped screen positions, v1 and v2 swapped when the face was wound with A < 0
  float z0, z1, z2;
  long long area;              // > 0
  bool swapped;
};

__device__ __forceinline__ long long mesh_edge(int ax, int ay, int bx, int by, long long px, long long py) {
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

__device__ __forceinline__ bool mesh_owns(int dx, int dy) { return dy > 0 || (dy == 0 && dx > 0); }

// row: the face's row in the packed array; vbase, nv: first vertex row and vertex count of its mesh.  false = the face is dropped.
__device__ __forceinline__ bool face_setup(const int *__restrict__ faces, const int4 *__restrict__ vrec, long long row, long long vbase,
                                           long long nv, int cull, MeshFace &f) {
  const int *fp = faces + (size_t)row * 3;
  const int i0 = fp[0], i1 = fp[1], i2 = fp[2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return false;
  const int4 a = vrec[vbase + i0], b = vrec[vbase + i1], c = vrec[vbase + i2];
  if (!(a.w && b.w && c.w)) return false;
  long long area = mesh_edge(a.x, a.y, b.x, b.y, c.x, c.y);
  if (area == 0 || (cull && area > 0)) return false;
  f.swapped = area < 0;
  f.x0 = a.x; f.y0 = a.y; f.z0 = __int_as_float(a.z);
  if (f.swapped) {
    f.x1 = c.x; f.y1 = c.y; f.z1 = __int_as_float(c.z);
    f.x2 = b.x; f.y2 = b.y; f.z2 = __int_as_float(b.z);
    area = -area;
  } else {
    f.x1 = b.x; f.y1 = b.y; f.z1 = __int_as_float(b.z);
    f.x2 = c.x; f.y2 = c.y; f.z2 = __int_as_float(c.z);
  }
  f.area = area;
  return true;
}

// the fragment of face f at pixel (xi, yi): false = not covered or dropped; z its depth; WITH_BARY: b0 .. b2 in f's (swapped) order
template <bool WITH_BARY>
__device__ __forceinline__ bool face_pixel(const MeshFace &f, int xi, int yi, int ortho, float &z, float &b0, float &b1, float &b2) {
  const long long px = (long long)MESH_SNAP * xi + MESH_SNAP / 2, py = (long long)MESH_SNAP * yi + MESH_SNAP / 2;
  const long long e0 = mesh_edge(f.x1, f.y1, f.x2, f.y2, px, py);
  const long long e1 = mesh_edge(f.x2, f.y2, f.x0, f.y0, px, py);
  const long long e2 = mesh_edge(f.x0, f.y0, f.x1, f.y1, px, py);
  if (e0 < 0 || e1 < 0 || e2 < 0) return false;
  if (e0 == 0 && !mesh_owns(f.x2 - f.x1, f.y2 - f.y1)) return false;
  if (e1 == 0 && !mesh_owns(f.x0 - f.x2, f.y0 - f.y2)) return false;
  if (e2 == 0 && !mesh_owns(f.x1 - f.x0, f.y1 - f.y0)) return false;
  const float area = (float)f.area;
  const float w0 = (float)e0 / area, w1 = (float)e1 / area, w2 = (float)e2 / area;
  if (ortho) {
    z = w0 * f.z0 + w1 * f.z1 + w2 * f.z2;
    if (WITH_BARY) { b0 = w0; b1 = w1; b2 = w2; }
  } else {
    const float t0 = w0 / f.z0, t1 = w1 / f.z1, t2 = w2 / f.z2;
    const float s = t0 + t1 + t2;
    z = 1.f / s;
    if (WITH_BARY) { b0 = t0 / s; b1 = t1 / s; b2 = t2 / s; }
  }
  return z > 0.f && z < INFINITY;
}

__device__ __forceinline__ void mesh_try_pixel(const MeshFace &f, int xi, int yi, int ortho, unsigned int face_in_mesh,
                                               unsigned long long *__restrict__ keys_of_mesh, int w) {
  float z, u0, u1, u2;
  if (!face_pixel<false>(f, xi, yi, ortho, z, u0, u1, u2)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | face_in_mesh;
  unsigned long long *slot = keys_of_mesh + (size_t)yi * w + xi;  // 0 <= xi < w, 0 <= yi < h: the box is clamped to the image
  if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
}

// pixel centres 256 i + 128 inside [lo, hi] (snapped coordinates), clamped to [0, size): first and last index, first > last = none
__device__ __forceinline__ void mesh_span(int lo, int hi, int size, int &first, int &last) {
  first = max((lo + (MESH_SNAP / 2 - 1)) >> 8, 0);   // ceil((lo - 128) / 256); >> on a negative int is arithmetic
  last = min((hi - MESH_SNAP / 2) >> 8, size - 1);   // floor((hi - 128) / 256)
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_raster_kernel(int b, int sum_f, int h, int w, int ortho, int cull,
                                                                   const int *__restrict__ faces, const int4 *__restrict__ vrec,
                                                                   const long long *__restrict__ vert_first,
                                                                   const long long *__restrict__ face_first,
                                                                   unsigned long long *__restrict__ keys) {
  const int row = blockIdx.x * MESH_THREADS + threadIdx.x;  // the grid covers sum_f < 2^31 exactly once
  MeshFace f;
  int m = 0, xa = 0, xb = -1, ya = 0, yb = -1;
  bool live = row < sum_f;
  if (live) {
    m = mesh_of_row(face_first, b, row);
    live = face_setup(faces, vrec, row, vert_first[m], vert_first[m + 1] - vert_first[m], cull, f);
  }
  if (live) {
    mesh_span(min(f.x0, min(f.x1, f.x2)), max(f.x0, max(f.x1, f.x2)), w, xa, xb);
    mesh_span(min(f.y0, min(f.y1, f.y2)), max(f.y0, max(f.y1, f.y2)), h, ya, yb);
    live = xa <= xb && ya <= yb;
  }
  const bool large = live && (xb - xa >= MESH_SMALL_BOX || yb - ya >= MESH_SMALL_BOX);
  if (live && !large) {
    unsigned long long *km = keys + (size_t)m * h * w;
    const unsigned int id = (unsigned int)(row - face_first[m]);
    for (int yi = ya; yi <= yb; ++yi)        // at most 16 x 16 trips
      for (int xi = xa; xi <= xb; ++xi) mesh_try_pixel(f, xi, yi, ortho, id, km, w);
  }
  // the wave's large faces, one at a time, all lanes on one box; the set-up is redone from the broadcast row (uniform loads)
  unsigned long long todo = __ballot(large);
  const int lane = threadIdx.x & 63;
  for (int trip = 0; trip < 64 && todo; ++trip) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int brow = __shfl(row, src), bm = __shfl(m, src);
    const int bxa = __shfl(xa, src), bxb = __shfl(xb, src), bya = __shfl(ya, src), byb = __shfl(yb, src);
    MeshFace g;
    if (!face_setup(faces, vrec, brow, vert_first[bm], vert_first[bm + 1] - vert_first[bm], cull, g)) continue;  // (it passed once)
    unsigned long long *km = keys + (size_t)bm * h * w;
    const unsigned int id = (unsigned int)(brow - face_first[bm]);
    const int bw = bxb - bxa + 1, count = bw * (byb - bya + 1);  // <= h w <= 2^24
    for (int i = lane; i < count; i += 64) mesh_try_pixel(g, bxa + i % bw, bya + i / bw, ortho, id, km, w);
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_resolve_kernel(int total, int h, int w, int c, int ortho, int cull,
                                                                    const int *__restrict__ faces, const int4 *__restrict__ vrec,
                                                                    const long long *__restrict__ vert_first,
                                                                    const long long *__restrict__ face_first,
                                                                    const unsigned long long *__restrict__ keys,
                                                                    const float *__restrict__ vert_features,
                                                                    const float *__restrict__ face_features,
                                                                    const float *__restrict__ background, int *__restrict__ pix_to_face,
                                                                    float *__restrict__ zbuf, float *__restrict__ bary,
                                                                    float *__restrict__ image) {
  const int pix = blockIdx.x * MESH_THREADS + threadIdx.x;  // total = b h w < 2^31
  if (pix >= total) return;
  const int m = pix / (h * w), rem = pix - m * (h * w), yi = rem / w, xi = rem - yi * w;
  const unsigned long long key = keys[pix];
  MeshFace f;
  float z = -1.f, b0 = -1.f, b1 = -1.f, b2 = -1.f;
  int face = -1;
  long long row = 0;
  const long long vbase = vert_first[m];
  bool hit = key != MESH_EMPTY_KEY;
  if (hit) {
    face = (int)(unsigned int)key;
    row = face_first[m] + face;
    hit = face_setup(faces, vrec, row, vbase, vert_first[m + 1] - vbase, cull, f) && face_pixel<true>(f, xi, yi, ortho, z, b0, b1, b2);
  }
  if (!hit) { face = -1; z = b0 = b1 = b2 = -1.f; }   // (a key always comes from a fragment that passed both: never taken for a hit)
  else if (f.swapped) { const float t = b1; b1 = b2; b2 = t; }
  if (pix_to_face) pix_to_face[pix] = face;
  if (zbuf) zbuf[pix] = z;
  if (bary) {
    float *o = bary + (size_t)pix * 3;
    o[0] = b0; o[1] = b1; o[2] = b2;
  }
  if (!image) return;
  float *o = image + (size_t)pix * c;
  if (!hit) {
#pragma unroll
    for (int ch = 0; ch < MESH_MAX_C; ++ch)
      if (ch < c) o[ch] = background[ch];
    return;
  }
  if (vert_features) {
    const int *fp = faces + (size_t)row * 3;
    const float *f0 = vert_features + (size_t)(vbase + fp[0]) * c, *f1 = vert_features + (size_t)(vbase + fp[1]) * c,
                *f2 = vert_features + (size_t)(vbase + fp[2]) * c;
#pragma unroll
    for (int ch = 0; ch < MESH_MAX_C; ++ch)
      if (ch < c) o[ch] = b0 * f0[ch] + b1 * f1[ch] + b2 * f2[ch];
  } else {
    const float *ff = face_features ? face_features + (size_t)row * c : nullptr;
#pragma unroll
    for (int ch = 0; ch < MESH_MAX_C; ++ch)
      if (ch < c) o[ch] = ff ? ff[ch] : 0.f;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool mesh_sizes_ok(int b, long long sum_v, long long sum_f, int h, int w) {
  return b >= 0 && sum_v >= 0 && sum_v <= INT_MAX && sum_f >= 0 && sum_f <= INT_MAX && h >= 1 && h <= MESH_MAX_SIDE && w >= 1 &&
         w <= MESH_MAX_SIDE && (long long)b * h * w <= INT_MAX;
}

struct MeshWs {
  unsigned long long *keys;  // [b][h][w]
  int4 *vrec;                // [sum_v]
  long long *vert_first, *face_first;  // [b + 1] each
  size_t bytes;
};

static MeshWs mesh_ws(void *ws, int b, long long sum_v, int h, int w) {
  MeshWs m;
  char *p = (char *)ws;
  const size_t key_bytes = sizeof(unsigned long long) * (size_t)b * h * w, rec_bytes = sizeof(int4) * (size_t)sum_v;
  const size_t key_padded = align16(key_bytes);  // the records are loaded 16 bytes at a time
  m.keys = (unsigned long long *)p;
  m.vrec = (int4 *)(p + key_padded);
  m.vert_first = (long long *)(p + key_padded + rec_bytes);
  m.face_first = m.vert_first + (b + 1);
  m.bytes = key_padded + rec_bytes + 2 * sizeof(long long) * (size_t)(b + 1);
  return m;
}

extern "C" size_t bdm_render_meshes_workspace_bytes(int b, long long sum_v, long long sum_f, int h, int w) {
  if (!mesh_sizes_ok(b, sum_v, sum_f, h, w)) return 0;
  return mesh_ws(nullptr, b, sum_v, h, w).bytes;
}

extern "C" int bdm_render_meshes(int b, int h, int w, int c, int ortho, int cull, const float *verts, const int *faces,
                                 const long long *vert_first, const long long *face_first, const float *cameras,
                                 const float *vert_features, const float *face_features, const float *background, int *pix_to_face,
                                 float *zbuf, float *bary, float *image, void *workspace, void *stream) {
  BDM_REQUIRE(b >= 0, "render_meshes: negative batch size");
  BDM_REQUIRE(h >= 1 && h <= MESH_MAX_SIDE && w >= 1 && w <= MESH_MAX_SIDE, "render_meshes: image %d x %d outside 1 .. %d", h, w,
              MESH_MAX_SIDE);
  BDM_REQUIRE(c >= 1 && c <= MESH_MAX_C, "render_meshes: %d feature channels outside 1 .. %d", c, MESH_MAX_C);
  BDM_REQUIRE((ortho == 0 || ortho == 1) && (cull == 0 || cull == 1), "render_meshes: bad camera or cull flag");
  BDM_REQUIRE(!(vert_features && face_features), "render_meshes: vertex features and face features are exclusive");
  BDM_REQUIRE((long long)b * h * w <= INT_MAX, "render_meshes: %d images of %d x %d pixels reach 2^31", b, h, w);
  if (b == 0) return BDM_OK;
  BDM_REQUIRE(verts && faces && vert_first && face_first && cameras && workspace, "render_meshes: an input or the workspace is NULL");
  BDM_REQUIRE(image == nullptr || background != nullptr, "render_meshes: an image needs a background colour");
  long long max_v = 0, max_f = 0;
  if (check_first("render_meshes", "mesh", b, vert_first, &max_v) != BDM_OK || check_first("render_meshes", "mesh", b, face_first, &max_f) != BDM_OK)
    return BDM_ERR_ARG;
  const long long sum_v = vert_first[b], sum_f = face_first[b];
  BDM_REQUIRE(sum_v <= INT_MAX && sum_f <= INT_MAX, "render_meshes: %lld vertices or %lld faces reach 2^31", sum_v, sum_f);
  const MeshWs ws = mesh_ws(workspace, b, sum_v, h, w);
  const size_t pixels = (size_t)b * h * w;
  const Range in[6] = {{verts, 12 * (size_t)sum_v}, {faces, 12 * (size_t)sum_f}, {cameras, 64 * (size_t)b},
                       {vert_features, 4 * (size_t)sum_v * c}, {face_features, 4 * (size_t)sum_f * c}, {background, 4 * (size_t)c}};
  const Range out[5] = {{pix_to_face, 4 * pixels}, {zbuf, 4 * pixels}, {bary, 12 * pixels}, {image, 4 * pixels * c}, {workspace, ws.bytes}};
  if (check_overlap("render_meshes", in, 6, out, 5) != BDM_OK) return BDM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  send_offsets(b, vert_first, face_first, ws.vert_first, ws.face_first, s);
  if (hipMemsetAsync(ws.keys, 0xFF, sizeof(unsigned long long) * pixels, s) != hipSuccess) return launch_status("render_meshes (memset)");
  if (sum_v > 0 && sum_f > 0) {
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)cdivll(sum_v, MESH_THREADS)), dim3(MESH_THREADS), 0, s, b, (int)sum_v, ortho,
                       0.5f * w, 0.5f * h, verts, cameras, ws.vert_first, ws.vrec);
    hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)cdivll(sum_f, MESH_THREADS)), dim3(MESH_THREADS), 0, s, b, (int)sum_f, h, w,
                       ortho, cull, faces, ws.vrec, ws.vert_first, ws.face_first, ws.keys);
  }
  if (pix_to_face || zbuf || bary || image)
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)cdivll((long long)pixels, MESH_THREADS)), dim3(MESH_THREADS), 0, s, (int)pixels,
                       h, w, c, ortho, cull, faces, ws.vrec, ws.vert_first, ws.face_first, ws.keys, vert_features, face_features,
                       background, pix_to_face, zbuf, bary, image);
  return launch_status("render_meshes");
}
