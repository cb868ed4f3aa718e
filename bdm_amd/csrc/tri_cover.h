// tri_cover.h -- which grid centres a snapped triangle covers, and how a wave shares that work: what the mesh rasteriser (mesh_render.hip:
// pixel centres) and the solid voxeliser (mesh_voxel.hip: column centres of a projection plane) share.  Integer
// device code only: what a covered centre is worth, and every float, stay with the operator behind its own `fp contract(off)`.
// Coordinates are snapped to 1 / TRI_SNAP of a grid step; the centre of step i sits at TRI_SNAP i + TRI_SNAP / 2.
#pragma once

namespace bdm {

constexpr int TRI_SNAP = 256, TRI_SNAP_SHIFT = 8;   // snapped positions per grid step (pixel, cell); tri_span divides by shifting
static_assert((1 << TRI_SNAP_SHIFT) == TRI_SNAP, "tri_span shifts by TRI_SNAP_SHIFT where it means a division by TRI_SNAP");
constexpr int TRI_SMALL_BOX = 16;                   // boxes up to 16 x 16 centres are walked by the item's own lane

__device__ __forceinline__ long long tri_edge(int ax, int ay, int bx, int by, long long px, long long py) {
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}
__device__ __forceinline__ long long tri_centre(int i) { return (long long)TRI_SNAP * i + TRI_SNAP / 2; }

// centres inside [lo, hi] (snapped coordinates), clamped to [0, size): first and last index, first > last = none
__device__ __forceinline__ void tri_span(int lo, int hi, int size, int &first, int &last) {
  first = max((lo + (TRI_SNAP / 2 - 1)) >> TRI_SNAP_SHIFT, 0);   // ceil((lo - 128) / 256); >> on a negative int is arithmetic
  last = min((hi - TRI_SNAP / 2) >> TRI_SNAP_SHIFT, size - 1);   // floor((hi - 128) / 256)
}

struct Tri2 { int ax, ay, bx, by, cx, cy; };   // wound positive: edge(a, b, c) > 0
// Corner records a, b, c (snapped .x, .y and whatever else rides along): b and c are swapped whole when the area is negative, t is
// (a, b, c) after that -> the area as given (0: t covers nothing).  Whole records, so that a caller's 16-byte loads stay whole.
template <class P>
__device__ __forceinline__ long long tri_wind(Tri2 &t, const P &a, P &b, P &c) {
  const long long area = tri_edge(a.x, a.y, b.x, b.y, c.x, c.y);
  if (area < 0) { const P s = b; b = c; c = s; }
  t = Tri2{a.x, a.y, b.x, b.y, c.x, c.y};
  return area;
}
// the box of centres t can cover, clamped to [0, size_x) x [0, size_y) -> whether it holds a centre
__device__ __forceinline__ bool tri_box(const Tri2 &t, int size_x, int size_y, int &x0, int &x1, int &y0, int &y1) {
  tri_span(min(t.ax, min(t.bx, t.cx)), max(t.ax, max(t.bx, t.cx)), size_x, x0, x1);
  tri_span(min(t.ay, min(t.by, t.cy)), max(t.ay, max(t.by, t.cy)), size_y, y0, y1);
  return x0 <= x1 && y0 <= y1;
}

// A centre ON an edge with vector (dx, dy) belongs to the triangle on one side of the edge only, so that two triangles sharing the
// edge cover it once.  Moving the centre by (sx, sy) changes the edge function by dx sy - dy sx.  Y_DOWN = false, the voxeliser: the
// centre moved by (eps_x, eps_y), eps_x >> eps_y > 0 (u comes before v in x, y, z) is inside, i.e. dy < 0, or dy == 0 and dx > 0:
// both axes of its plane run upwards and the rule is the perturbation's, as in its crossing rule.  Y_DOWN = true, the rasteriser:
// its image y runs downwards (pixel row 0 is the top), so its top-left rule reads dy > 0 in its snapped coordinates.  The two agree
// with their own conventions and disagree with each other; the voxeliser's restatement holds the other rule as a mutant.
template <bool Y_DOWN>
__device__ __forceinline__ bool tri_owns(int dx, int dy) { return (Y_DOWN ? dy > 0 : dy < 0) || (dy == 0 && dx > 0); }

// whether t covers the centre (i, j); e0, e1, e2: the edge functions there opposite a, b, c (their sum is the area)
template <bool Y_DOWN>
__device__ __forceinline__ bool tri_covers(const Tri2 &t, int i, int j, long long &e0, long long &e1, long long &e2) {
  const long long px = tri_centre(i), py = tri_centre(j);
  e0 = tri_edge(t.bx, t.by, t.cx, t.cy, px, py);
  e1 = tri_edge(t.cx, t.cy, t.ax, t.ay, px, py);
  e2 = tri_edge(t.ax, t.ay, t.bx, t.by, px, py);
  if (e0 < 0 || e1 < 0 || e2 < 0) return false;
  if (e0 == 0 && !tri_owns<Y_DOWN>(t.cx - t.bx, t.cy - t.by)) return false;
  if (e1 == 0 && !tri_owns<Y_DOWN>(t.ax - t.cx, t.ay - t.cy)) return false;
  return e2 != 0 || tri_owns<Y_DOWN>(t.bx - t.ax, t.by - t.ay);
}

// Every centre (i, j) of this lane's box [x0, x1] x [y0, y1] (live: it has one) through visit(item, i, j).  A box up to TRI_SMALL_BOX x
// TRI_SMALL_BOX is walked by its lane with `mine`; after those the wave takes its larger boxes one at a time, lowest lane first, all
// 64 lanes striding over the box, so a triangle across the grid costs a wave and not a thread.  Their items are not broadcast but
// built again: redo(src, item) -> bool makes the item of lane src from values it broadcasts itself (__shfl(.., src); uniform loads).
// EVERY lane of the wave calls this in converged control flow (ballot, shuffles): a kernel may leave before the call only as a whole
// workgroup, and a lane without work passes live = false.  redo runs converged; visit does not and must not shuffle.
template <class Item, class Redo, class Visit>
__device__ __forceinline__ void tri_walk_boxes(bool live, int x0, int x1, int y0, int y1, const Item &mine, Redo redo, Visit visit) {
  const bool large = live && (x1 - x0 >= TRI_SMALL_BOX || y1 - y0 >= TRI_SMALL_BOX);
  if (live && !large)
    for (int j = y0; j <= y1; ++j)        // at most 16 x 16 trips
      for (int i = x0; i <= x1; ++i) visit(mine, i, j);
  unsigned long long todo = __ballot(large);
  const int lane = threadIdx.x & 63;
  for (int trip = 0; trip < 64 && todo; ++trip) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int bx0 = __shfl(x0, src), bx1 = __shfl(x1, src), by0 = __shfl(y0, src), by1 = __shfl(y1, src);
    Item g;
    if (!redo(src, g)) continue;   // (it passed once)
    const int width = bx1 - bx0 + 1, count = width * (by1 - by0 + 1);   // <= size_x size_y
    for (int e = lane; e < count; e += 64) visit(g, bx0 + e % width, by0 + e / width);
  }
}

}  // namespace bdm
