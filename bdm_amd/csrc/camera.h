// camera.h -- the one definition of the camera model shared by the rasterisers (sampler_ops.hip, render.hip, mesh_render.hip), so
// that a point lands on the same pixel whichever kernel projects it:
//   row-vector convention X_view = X_world R + T;  perspective ndc = focal * X_view.xy / X_view.z + pp;  orthographic ndc =
//   focal * X_view.xy + pp;  pixel i of an axis of `size` pixels has its centre at ndc 1 - (2 i + 1) / size  (+X left, +Y up).
// The results define pixels and depth keys: every body is written operation by operation and carries `#pragma clang fp contract(off)`
// itself.  The division is whatever the including translation unit's flags make it (mesh_render.hip is built with correctly rounded
// division, the others are not): nothing here chooses one.
#pragma once
#include <hip/hip_runtime.h>

namespace bdm {

// a camera travels as 16 packed floats: R (3 x 3, row-major) at 0, T at 9, focal (x, y) at 12, principal point (x, y) at 14.
// A view, not a copy: each function reads the entries it needs.
struct Camera { const float *c; };

__device__ __forceinline__ Camera load_camera(const float *__restrict__ cams, size_t index) { return Camera{cams + index * 16}; }

__device__ __forceinline__ void view_transform(const Camera &cam, float x, float y, float z, float &xv, float &yv, float &zv) {
#pragma clang fp contract(off)
  const float *c = cam.c;
  xv = x * c[0] + y * c[3] + z * c[6] + c[9];
  yv = x * c[1] + y * c[4] + z * c[7] + c[10];
  zv = x * c[2] + y * c[5] + z * c[8] + c[11];
}

__device__ __forceinline__ void ndc_project(const Camera &cam, float xv, float yv, float zv, int ortho, float &u, float &v) {
#pragma clang fp contract(off)
  const float *c = cam.c;
  if (ortho) {
    u = c[12] * xv + c[14];
    v = c[13] * yv + c[15];
  } else {
    u = c[12] * xv / zv + c[14];
    v = c[13] * yv / zv + c[15];
  }
}

// world point -> (ndc u, ndc v, view depth)
__device__ __forceinline__ void project_point(const Camera &c, float x, float y, float z, int ortho, float &u, float &v, float &zv) {
  float xv, yv;
  view_transform(c, x, y, z, xv, yv, zv);
  ndc_project(c, xv, yv, zv, ortho, u, v);
}

__device__ __forceinline__ float pixel_centre(int i, int size) {
#pragma clang fp contract(off)
  return 1.f - (2.f * i + 1.f) / size;
}

}  // namespace bdm
