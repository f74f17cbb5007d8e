// render_args.h — what the host half of dftpav_grid_render hands the kernels of render.hip.  The host snaps every world coordinate to
// its cell coordinate (rint((p - origin) / resolution), the refusals need them anyway), so the kernels see integers alone.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dftpav_hip.h"

namespace dftpav {

enum { kRenderMaxChunks = 64 }; // the most workgroups (of four waves) that share the rows of one polygon or circle

struct RenderArgs {
  unsigned char *cells; // the map [size_y][size_x]
  int size_x, size_y;
  unsigned char background;
  // polygons: edge e of polygon p is edges[poly_off[p] + e] = (X0, Y0, X1, Y1), from vertex e to vertex e + 1, cyclic
  int n_poly, n_vert;
  const int *poly_off;  // [n_poly + 1]
  const int4 *poly_box; // [n_poly] minX, maxX, minY, maxY of the snapped vertices (not read for a polygon without vertices)
  const int4 *edges;    // [n_vert]
  int poly_chunks;      // workgroups per polygon: 1 ..= kRenderMaxChunks
  // circles: (cx, cy, r, 0) in cells
  int n_circle;
  const int4 *circles;
  int circle_chunks;
  // points: (x, y) in cells
  int n_point;
  const int2 *points;
};

} // namespace dftpav
