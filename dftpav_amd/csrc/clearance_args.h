// clearance_args.h — what the host half of the clearance calls (dftpav_grid_distance_field, dftpav_batch_check_clearance,
// dftpav_planner_check_clearance, the clearance filter) hands the kernels of distfield.hip and clearance.hip.
#pragma once
#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "footprint.h"
#include "piece_eval.h"
#include "plan_args.h"

namespace dftpav {

enum { kDistMaxSide = 16384 }; // a map side: g * g + dy * dy <= 2 * 16383^2 < 2^31 - 1
enum { kDistTileX = 64, kDistTileY = 4 }; // a workgroup of either field pass: one wave along x, four rows

// distfield.hip: cells [size_y][size_x] -> g (the distance along x) -> d2 (the squared Euclidean distance), both [size_y][size_x]
struct DistFieldArgs {
  const unsigned char *cells;
  int size_x, size_y;
  int *g;
  int *d2;
};

// what both clearance kernels share: the map with its field, the vehicle, the sample times and the result rows
struct ClearanceCommon {
  DevGrid grid;
  const int *d2; // the field of grid.cells
  DevFootprint fp;
  SampleTable tab;   // (validation_table)
  int *min_d2, *arg; // [rows]
  double *clearance; // [rows]
};

// clearance_batch_kernel: the first B trajectories of a solved batch
struct ClearanceBatchArgs {
  ClearanceCommon C;
  const double *coeffs;   // [B][Ntot][6][2]
  const double *piece_dt; // [B][M]
  DevLayout L;
  int B;
  const int *members; // nullptr: trajectory b writes row b; else row members[b / R] * R + b % R (the [Q][R] rows of a call)
  int R;
  int *reject;          // [B] or nullptr (the read-out call); the filter: set to 1 unless clearance >= min_clearance, never read or cleared
  double min_clearance;
};

// clearance_table_kernel: every slot of the executing table (read only)
struct ClearanceTableArgs {
  ClearanceCommon C;
  ExecTable T;
};

} // namespace dftpav
