// stamp_args.h — what the host half of the stamp calls (dftpav_grid_stamp_poses, dftpav_planner_stamp_slots, dftpav_grid_clear_stamps,
// dftpav_grid_read_cells) hands the kernels of stamp.hip.
#pragma once
#include "../../include/dftpav_hip.h"

namespace dftpav {

enum { kStampCountBlocks = 256 }; // the most partial counts of stamp_count_kernel (the host adds them in order)

// stamp_box_kernel: one wave per box.  The boxes lie as four arrays [n_boxes]; in the slot form these are the pose arrays of
// conflict_pose_kernel, [K][S_pad], and box b belongs to slot b % S_pad.
struct StampBoxArgs {
  unsigned char *cells; // the working map [size_y][size_x]
  unsigned *bits;       // its bit map (bit ix + size_x * iy), or null
  int size_x, size_y;
  double resolution, origin_x, origin_y;
  const double *cx, *cy, *cs, *sn;
  int n_boxes;
  const unsigned char *select; // [S_pad] 0: the slot's boxes stamp nothing; null: every box stamps
  int S_pad;                   // read with select alone
  double hl, hw;               // 0.5 * veh_length + inflate, 0.5 * veh_width + inflate
};

// stamp_bits_kernel: the bit map made again from the bytes, a thread per word
struct StampBitsArgs {
  const unsigned char *cells;
  unsigned *bits;
  size_t n_cells;
};

// stamp_count_kernel: the cells that are 80 in `cells` and not in `base`, a partial count per workgroup
struct StampCountArgs {
  const unsigned char *cells, *base;
  size_t n_cells;
  unsigned *partial; // [gridDim.x]
};

} // namespace dftpav
