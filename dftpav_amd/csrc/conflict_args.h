// conflict_args.h — what the host half of the conflict calls (dftpav_planner_check_conflicts, dftpav_planner_sample_poses) hands the
// kernels of conflict.hip.
#pragma once
#include <cstddef>

#include "../../include/dftpav_hip.h"
#include "piece_eval.h"
#include "plan_args.h"

namespace dftpav {

enum { kConflictTile = 64 }; // slots of a tile: one wave, a lane per slot

// The poses of every slot at every clock, sample-major: four arrays [K][S_pad], S_pad the slots rounded up to whole tiles.  An empty
// slot and the padding behind the last slot hold NaN.
struct ConflictPoses {
  double *cx, *cy, *cs, *sn;
  unsigned char *occupied; // [S_pad] 1: the slot holds a plan
  int K, S_pad;
};

// conflict_pose_kernel
struct ConflictPoseArgs {
  ExecTable T; // read only
  ConflictPoses P;
  double t0, dt;
  double dcr; // veh_d_cr
};

// The lexicographic minima of one slot, over one J-tile (the partial rows [tiles][S_pad]) or over all of them (the outputs [slots])
struct ConflictRows {
  double *min_sep;
  int *sep_sample, *sep_partner, *conflict_sample, *conflict_partner;
};

// The vehicle and the two distances of every pair kernel of the family (conflict.hip, cand_conflict.hip, joint_select.hip,
// conflict_trigger.hip); the host forms them in one place (pair_consts, capi_conflicts.cpp)
struct PairConsts {
  double half_l, half_w; // 0.5 * veh_length, 0.5 * veh_width
  double margin;
  double reach2; // R * R of the broad phase, R = range + 2 * the footprint's circumradius
};

// conflict_pair_kernel: workgroup (I-tile, J-tile) writes the partial row jt * S_pad + i of every slot i of its I-tile
struct ConflictPairArgs {
  ConflictPoses P; // read only
  ConflictRows part;
  PairConsts V;
};
static_assert(offsetof(ConflictPairArgs, V) == sizeof(ConflictPoses) + sizeof(ConflictRows) && sizeof(ConflictPairArgs) == offsetof(ConflictPairArgs, V) + 32,
              "the four doubles lie where they lay");

// conflict_reduce_kernel: slot i's partial rows merged into its output row
struct ConflictReduceArgs {
  ConflictRows part, out;
  int n_slots, S_pad, tiles;
};

} // namespace dftpav
