// mesh_render.hip -- triangle meshes to pixels: one face per pixel, as gfx950 kernels (bdm_hip.h section 13, DESIGN.md section 17;
// restates pytorch3d's MeshRasterizer at faces_per_pixel = 1, blur_radius = 0 and a Gouraud / flat shader; pytorch3d is not
// installed, so the rule is this project's own text: "parity unpinned").
//
// The rule in one paragraph: vertices are projected in float32, operation by operation (camera.h; no FMA contraction, and in this
// file division correctly rounded), and snapped to 1/256 pixel; coverage is decided by three int64 edge functions at the pixel centre with a
// half-plane rule for centres ON an edge (tri_cover.h); depth and barycentrics are float32 quotients of those integers; the pixel keeps the
// smallest (bits of z) << 32 | face index.  Nothing depends on execution order: the only atomic is an integer minimum.
//
// Three kernels, after send_offsets (ragged.h) has put the two host offset arrays into the workspace.
//   mesh_vertex_kernel    one thread per vertex: view transform, NDC, screen, snap -> (SX, SY, zv, usable), 16 bytes per vertex.
//   mesh_raster_kernel    one thread per face: set-up (face_setup), the bounding box of the pixel centres it can cover clamped to
//                         the image, then every centre of the box (tri_walk_boxes of tri_cover.h: small boxes by their lane, large
//                         ones by the whole wave) through face_pixel and, for a covered one, atomicMin on the 64-bit key image
//                         (preset to all ones).  The key is read before the atomic and a losing fragment skipped: the minimum
//                         only ever decreases, so a stale read can only let through an atomic that then changes nothing.
//   mesh_resolve_kernel   one thread per pixel: the winner's face_setup and face_pixel again -- the same device functions, the
//                         same bits -- then pix_to_face, zbuf, bary (swapped back to the face's own order) and the image.
// The tile-binned form of render.hip (one workgroup per tile streams ALL faces) needs no atomics but reads an 88 000-face mesh
// 196 times at 224 x 224; here every face is read once and costs its own box.
#include "../../include/bdm_hip.h"
#include "camera.h"
#include "common.h"
#include "mesh_incidence.h"
#include "tri_cover.h"

#include <limits.h>

#pragma clang fp contract(off)

using namespace bdm;

#define MESH_MAX_C 4
#define MESH_MAX_SIDE 4096
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
  const float px = ((1.f - u) * half_w) * (float)TRI_SNAP, py = ((1.f - v) * half_h) * (float)TRI_SNAP;
  // NaN fails every comparison; fabsf(inf) <= 2^22 is false
  const bool usable = zv > 0.f && zv < INFINITY && fabsf(px) <= MESH_GUARD && fabsf(py) <= MESH_GUARD;
  vrec[i] = usable ? make_int4((int)rintf(px), (int)rintf(py), __float_as_int(zv), 1) : make_int4(0, 0, 0, 0);
}

struct MeshFace {
  Tri2 t;                      // snapped screen positions, v1 and v2 swapped when the face was wound with A < 0
  float z0, z1, z2;            // in t's order
  long long area;              // > 0
  bool swapped;
};

// row: the face's row in the packed array; vbase, nv: first vertex row and vertex count of its mesh.  false = the face is dropped.
// connected_face also refuses a repeated index, which changes nothing: such a face has area 0, and no count tells the reasons apart.
__device__ __forceinline__ bool face_setup(const int *__restrict__ faces, const int4 *__restrict__ vrec, long long row, long long vbase,
                                           long long nv, int cull, MeshFace &f) {
  int idx[3];
  if (!connected_face(faces, row, nv, idx)) return false;
  const int4 a = vrec[vbase + idx[0]];
  int4 b = vrec[vbase + idx[1]], c = vrec[vbase + idx[2]];
  if (!(a.w && b.w && c.w)) return false;
  const long long area = tri_wind(f.t, a, b, c);   // b and c change places with their depths
  if (area == 0 || (cull && area > 0)) return false;
  f.swapped = area < 0;
  f.z0 = __int_as_float(a.z), f.z1 = __int_as_float(b.z), f.z2 = __int_as_float(c.z);
  f.area = f.swapped ? -area : area;
  return true;
}

// the fragment of face f at pixel (xi, yi): false = not covered or dropped; z its depth; WITH_BARY: b0 .. b2 in f's (swapped) order
template <bool WITH_BARY>
__device__ __forceinline__ bool face_pixel(const MeshFace &f, int xi, int yi, int ortho, float &z, float &b0, float &b1, float &b2) {
  long long e0, e1, e2;
  if (!tri_covers<true>(f.t, xi, yi, e0, e1, e2)) return false;   // the image's y runs downwards
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

// a face on its way to the key image: what a lane needs per pixel, for its own face or for a broadcast one
struct MeshItem {
  MeshFace f;
  unsigned long long *keys;  // of the face's mesh
  unsigned int id;           // the face's index within its mesh
};

__device__ __forceinline__ void mesh_try_pixel(const MeshItem &it, int xi, int yi, int ortho, int w) {
  float z, u0, u1, u2;
  if (!face_pixel<false>(it.f, xi, yi, ortho, z, u0, u1, u2)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | it.id;
  unsigned long long *slot = it.keys + (size_t)yi * w + xi;  // 0 <= xi < w, 0 <= yi < h: the box is clamped to the image
  if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_raster_kernel(int b, int sum_f, int h, int w, int ortho, int cull,
                                                                   const int *__restrict__ faces, const int4 *__restrict__ vrec,
                                                                   const long long *__restrict__ vert_first,
                                                                   const long long *__restrict__ face_first,
                                                                   unsigned long long *__restrict__ keys) {
  const int row = blockIdx.x * MESH_THREADS + threadIdx.x;  // the grid covers sum_f < 2^31 exactly once
  const auto setup = [&](int bm, int brow, MeshItem &it) {   // the lane's own row and mesh, or broadcast ones
    it.keys = keys + (size_t)bm * h * w;
    it.id = (unsigned int)(brow - face_first[bm]);   // loaded before the set-up can refuse the face: measured faster than after it
    return face_setup(faces, vrec, brow, vert_first[bm], vert_first[bm + 1] - vert_first[bm], cull, it.f);
  };
  MeshItem it;
  int m = 0, xa = 0, xb = -1, ya = 0, yb = -1;
  bool live = row < sum_f;   // no lane leaves before the walk: its wave may hold large faces, and faces of several meshes
  if (live) {
    m = mesh_of_row(face_first, b, row);
    live = setup(m, row, it) && tri_box(it.f.t, w, h, xa, xb, ya, yb);
  }
  // a large face is set up again from its broadcast row and mesh
  tri_walk_boxes(live, xa, xb, ya, yb, it, [&](int src, MeshItem &g) { return setup(__shfl(m, src), __shfl(row, src), g); },
                 [&](const MeshItem &g, int xi, int yi) { mesh_try_pixel(g, xi, yi, ortho, w); });
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
  Carve c{(char *)ws, 0};
  MeshWs m;
  m.keys = c.take<unsigned long long>((size_t)b * h * w);   // padded to 16 bytes: the records are loaded 16 bytes at a time
  m.vrec = c.take<int4>((size_t)sum_v);
  m.vert_first = c.take_offsets(b), m.face_first = m.vert_first + (b + 1);
  m.bytes = c.o;
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
