// goalfield_args.h — what the host half of the goal-field calls (dftpav_grid_goal_field, the search heuristic of
// dftpav_set_search_heuristic) hands the kernel of goalfield.hip.
#pragma once
#include "../../include/dftpav_hip.h"

namespace dftpav {

enum { kGfThreads = 256 };                 // one workgroup per field
enum { kGfTileX = 64, kGfTileY = 32 };     // a tile of the field in LDS ...
enum { kGfStride = kGfTileX + 2, kGfRows = kGfTileY + 2 }; // ... with its one-cell halo: 66 x 34 words, 8976 bytes
enum { kGfAxial = 5, kGfDiagonal = 7 };    // step costs

// goal_field_kernel: block g builds fields[g] from goal_cell[g].  The host has set every field to DFTPAV_FIELD_UNREACHED and every
// dirty word to 0, and hands over only goals inside the grid.
//
// The windowed instance (window != nullptr; dftpav_goal_window, docs/NEXT_ROWS.md §4.22): block g builds the field of the window
// window[g] = (X0, Y0, WX, WY) -- a rectangle of the whole-map field's own tiles, X0 a multiple of kGfTileX, Y0 of kGfTileY, the
// goal cell inside it -- compactly as [WY][WX] at fields + offset[g]; its dirty map, one word per tile of the window, is at
// dirty + g * dirty_stride.  tiles_x and tiles_y are not read.
struct GoalFieldArgs {
  const int *d2; // the distance field of the map (distfield.hip), [size_y][size_x]
  int size_x, size_y;
  int T;         // a cell is blocked iff d2 <= T
  int tiles_x, tiles_y;
  const int *goal_cell; // [n][2] (ix, iy), grid coordinates
  int *fields;          // [n][size_y][size_x]; windowed: field g is [WY][WX] at offset[g]
  int *dirty;           // [n][tiles_y * tiles_x], one word per tile
  int *n_reached;       // [n]
  const int *window;       // [n][4], or nullptr: every field covers the grid
  const long long *offset; // [n] where field g starts in `fields`, in ints (windowed only)
  int dirty_stride;        // words between the dirty maps of two fields (windowed only)
};

} // namespace dftpav
