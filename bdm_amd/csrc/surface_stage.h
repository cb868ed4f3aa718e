// What the two grid entries of the mesher share (surface.hip: bdm_surface_grid; surface_poisson.hip: bdm_surface_poisson_grid): the
// section-12 workspace layout, the limits, and the two host functions of surface.hip that launch the frame and the mark stage.
#pragma once
#include "common.h"

namespace bdm {

constexpr int SRF_THREADS = 256;             // workgroup of the per-node kernels: one count per workgroup
constexpr int SRF_WAVES = SRF_THREADS / 64;
constexpr int SRF_WIDE = 1024;               // workgroup of the per-cloud kernels (box, scan)
constexpr int SRF_PAR = 8;                   // words per cloud: cx, cy, cz, inv, live, 3 unused
constexpr int SRF_N_MAX = 65536, SRF_R_MIN = 16, SRF_R_MAX = 256, SRF_S_MIN = 2, SRF_S_MAX = 4;
constexpr unsigned SRF_GRID_Y = 32768;       // clouds beyond it are reached by the stride loop over blockIdx.y

struct SurfWs {
  int *sw, *su, *cell;      // [b][r3] each
  int *cell_bc, *edge_bc;   // [b][nb], [b][3][nb]: counts per workgroup, then their exclusive scan
  float *par;               // [b][SRF_PAR]
  unsigned char *eflag;     // [b][3][r3]
  int r3, nb;
};

static inline size_t surf_ws_ints(int b, int r3, int nb) { return (size_t)b * (3 * (size_t)r3 + 4 * (size_t)nb + SRF_PAR); }

static inline size_t surf_ws_bytes(int b, int r) {
  const int r3 = r * r * r;
  return surf_ws_ints(b, r3, cdiv(r3, SRF_THREADS)) * sizeof(int) + 3 * (size_t)b * r3;
}

static inline SurfWs surf_ws(void *ws, int b, int r) {
  SurfWs w;
  w.r3 = r * r * r, w.nb = cdiv(w.r3, SRF_THREADS);
  w.sw = (int *)ws;
  w.su = w.sw + (size_t)b * w.r3;
  w.cell = w.su + (size_t)b * w.r3;
  w.cell_bc = w.cell + (size_t)b * w.r3;
  w.edge_bc = w.cell_bc + (size_t)b * w.nb;
  w.par = (float *)(w.edge_bc + (size_t)b * 3 * w.nb);
  w.eflag = (unsigned char *)(w.par + (size_t)b * SRF_PAR);
  return w;
}

bool surf_sizes_ok(int b, int n, int r, int s);
int surf_check_sizes(const char *what, int b, int n, int r, int s);

// surf_box_kernel: c, inv = float(r - 1 - 2 margin) / (2 half), the live flag, counts = {0, 0, 0, valid}
void surf_launch_frame(int b, int n, int r, int margin, const float *points, const float *normals, const SurfWs &w, int *counts,
                       hipStream_t st);
// surf_cell_kernel ... surf_rank_kernel on the SW, SU of the workspace: cell map, edge codes, scanned counts, counts[0 .. 2]
void surf_launch_mark(int b, int r, int thr, const SurfWs &w, int *counts, hipStream_t st);

}  // namespace bdm
