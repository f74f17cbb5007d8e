// footprint.h — the vehicle outline against the occupancy grid, as validate.hip, replan.hip, shot.hip and search.hip share it.
//
//   SemanticMapManager::CheckCollisionUsingPosAndYaw   semantic_map_manager.cc:639-662
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox  common/src/common/basics/shapes.cc:110-149
//   GridMapND::CheckIfEqualUsingGlobalPosition         common/src/common/basics/semantics.cc:169-179, 214-221
//
// (corridor.hip's cell_occupied<BITS> is another probe -- a bit map, the quotient from a reciprocal -- and only takes its
// grid fields from DevGrid.)
#pragma once

namespace dftpav {

struct DevGrid { // the handle's occupancy map on the device
  const unsigned char *cells;
  int size_x, size_y;
  double resolution, origin_x, origin_y;
};
struct DevFootprint { // the vehicle, and the spacing of its outline points as the reference's running sum
  double width, length, dcr;
  const double *v_tab; // res, res + res, ...
  int n_v;
};

// coord = round((p - origin) / resolution); out of range counts as free; 80 is GridMapND::OCCUPIED
__device__ inline bool grid_occupied(const DevGrid &g, double x, double y) {
  const double cx = round((x - g.origin_x) / g.resolution), cy = round((y - g.origin_y) / g.resolution);
  if (!(cx >= 0.0 && cx < (double)g.size_x && cy >= 0.0 && cy < (double)g.size_y)) return false;
  return g.cells[(int)cx + g.size_x * (int)cy] == 80;
}
// the dense vertices of one edge a -> b (its end points are the corners, probed by footprint_hits)
__device__ inline bool edge_hits(const DevGrid &g, const DevFootprint &fp, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  const double norm = sqrt(dx * dx + dy * dy);
  for (int j = 0; j < fp.n_v; j++) {
    const double dl = fp.v_tab[j];
    if (!(dl < norm)) break;
    const double f = dl / norm;
    if (grid_occupied(g, f * dx + ax, f * dy + ay)) return true;
  }
  return false;
}
// CheckCollisionUsingPosAndYaw for the pose (px, py) whose yaw has the cosine cs and the sine sn (the caller's: shot.hip is
// held to the portable pair, the others to cr_trig.h's): the obb centre, its four corners, the four edges, then the corners
__device__ inline bool footprint_hits(const DevGrid &g, const DevFootprint &fp, double px, double py, double cs, double sn) {
  const double W = fp.width, Lv = fp.length;
  const double x = px + fp.dcr * cs, y = py + fp.dcr * sn;
  const double c1x = x + 0.5 * Lv * cs + 0.5 * W * sn, c1y = y + 0.5 * Lv * sn - 0.5 * W * cs;
  const double c2x = x + 0.5 * Lv * cs - 0.5 * W * sn, c2y = y + 0.5 * Lv * sn + 0.5 * W * cs;
  const double c3x = x - 0.5 * Lv * cs - 0.5 * W * sn, c3y = y - 0.5 * Lv * sn + 0.5 * W * cs;
  const double c4x = x - 0.5 * Lv * cs + 0.5 * W * sn, c4y = y - 0.5 * Lv * sn - 0.5 * W * cs;
  return edge_hits(g, fp, c1x, c1y, c2x, c2y) || edge_hits(g, fp, c2x, c2y, c3x, c3y) || edge_hits(g, fp, c3x, c3y, c4x, c4y) ||
         edge_hits(g, fp, c4x, c4y, c1x, c1y) || grid_occupied(g, c1x, c1y) || grid_occupied(g, c2x, c2y) ||
         grid_occupied(g, c3x, c3y) || grid_occupied(g, c4x, c4y);
}

// The same probe points against the distance field d2 of g.cells (distfield.hip) instead of the cells: the smallest d2 over them.
// A point outside the grid is skipped, as "out of range counts as free"; INT32_MAX where every point is.  Every point is visited.
__device__ inline int grid_d2(const DevGrid &g, const int *d2, double x, double y) {
  const double cx = round((x - g.origin_x) / g.resolution), cy = round((y - g.origin_y) / g.resolution);
  if (!(cx >= 0.0 && cx < (double)g.size_x && cy >= 0.0 && cy < (double)g.size_y)) return 0x7fffffff;
  return d2[(size_t)(int)cx + (size_t)g.size_x * (size_t)(int)cy];
}
__device__ inline int edge_min_d2(const DevGrid &g, const int *d2, const DevFootprint &fp, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  const double norm = sqrt(dx * dx + dy * dy);
  int m = 0x7fffffff;
  for (int j = 0; j < fp.n_v; j++) {
    const double dl = fp.v_tab[j];
    if (!(dl < norm)) break;
    const double f = dl / norm;
    m = min(m, grid_d2(g, d2, f * dx + ax, f * dy + ay));
  }
  return m;
}
__device__ inline int footprint_min_d2(const DevGrid &g, const int *d2, const DevFootprint &fp, double px, double py, double cs, double sn) {
  const double W = fp.width, Lv = fp.length;
  const double x = px + fp.dcr * cs, y = py + fp.dcr * sn;
  const double c1x = x + 0.5 * Lv * cs + 0.5 * W * sn, c1y = y + 0.5 * Lv * sn - 0.5 * W * cs;
  const double c2x = x + 0.5 * Lv * cs - 0.5 * W * sn, c2y = y + 0.5 * Lv * sn + 0.5 * W * cs;
  const double c3x = x - 0.5 * Lv * cs - 0.5 * W * sn, c3y = y - 0.5 * Lv * sn + 0.5 * W * cs;
  const double c4x = x - 0.5 * Lv * cs + 0.5 * W * sn, c4y = y - 0.5 * Lv * sn - 0.5 * W * cs;
  int m = min(min(edge_min_d2(g, d2, fp, c1x, c1y, c2x, c2y), edge_min_d2(g, d2, fp, c2x, c2y, c3x, c3y)),
              min(edge_min_d2(g, d2, fp, c3x, c3y, c4x, c4y), edge_min_d2(g, d2, fp, c4x, c4y, c1x, c1y)));
  m = min(min(m, grid_d2(g, d2, c1x, c1y)), min(grid_d2(g, d2, c2x, c2y), min(grid_d2(g, d2, c3x, c3y), grid_d2(g, d2, c4x, c4y))));
  return m;
}

} // namespace dftpav
