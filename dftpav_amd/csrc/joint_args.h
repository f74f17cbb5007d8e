// joint_args.h — what the host half of joint selection (dftpav_planner_set_joint_selection, the joint stage of dftpav_plan_queries,
// dftpav_debug_joint_select) hands the kernels of joint_select.hip.  docs/NEXT_ROWS.md §4.28.
#pragma once
#include "../../include/dftpav_hip.h"
#include "cand_conflict_args.h"

namespace dftpav {

// The candidates of a call in query order, candidate i = q * R + r, C = Q * R of them, C_pad = C rounded up to whole tiles of 64.
// Poses are ConflictPoses' shape with C_pad for S_pad: four arrays [K][C_pad]; the padding and the candidates of a query outside
// every layout group hold NaN.
struct JointPoses {
  double *cx, *cy, *cs, *sn;
  int K, C_pad;
};

// what the selection reads per candidate, in query order (joint_pose_kernel gathers it from a group's batch)
struct JointCands {
  double *cost;  // [C]
  int *eligible; // [C] succeeded, not colliding, no reject flag, cost not NaN; 0 for a query outside every group
  int *flag;     // [C] the index of the candidate's reject flag in the call's flag array, -1: none
};

// joint_pose_kernel: the first nm * R trajectories of a group's batch into the call-wide arrays, through members
struct JointPoseArgs {
  CandBatch C;
  JointPoses P;
  JointCands J;
  const int *members; // [nm] the group's queries
  int R;
  int flag0;            // the group's first flag: trajectory c owns flag flag0 + c
  const double *f;      // [nm * R] the solve's final cost
  const int *success;   // [nm * R]
  const int *collision; // [nm * R]
  const int *reject;    // [nm * R], the filters' flags of the group
};

// joint_pair_kernel: workgroup (it, jt) writes word i * tiles + jt of every candidate i of I-tile it: bit j, conf(i, 64 jt + j)
struct JointPairArgs {
  JointPoses P; // read only
  unsigned long long *bits; // [C_pad][tiles]
  int C, R, tiles;
  PairConsts V;
};
static_assert(offsetof(JointPairArgs, V) == offsetof(JointPairArgs, tiles) + 8 && sizeof(JointPairArgs) == offsetof(JointPairArgs, V) + 32,
              "the four doubles lie where they lay");

// joint_greedy_kernel: one workgroup walks the queries in order
struct JointGreedyArgs {
  const unsigned long long *bits;
  JointCands J; // read only
  const int *minit; // [Q] or nullptr: a query whose flag is set has no eligible restart
  int Q, R, tiles;
  int *winner;  // [Q] w(q), -1: none
  int *wcand;   // [Q] q * R + w(q), -1: none
  int *blocked; // [C]
  int *reject;  // the call's flag array or nullptr; flag[i] of a blocked candidate is set to 1, by the lane that owns it
};

// joint_rows_kernel: workgroup g takes the candidates [64 g, 64 g + 64) against the winners of the queries below their own
struct JointRowsArgs {
  JointPoses P; // read only
  const int *wcand;
  ConflictRows rows; // [C]; the partner index is the query index
  int C, Q, R;
  PairConsts V;
};
static_assert(offsetof(JointRowsArgs, V) == offsetof(JointRowsArgs, R) + 8 && sizeof(JointRowsArgs) == offsetof(JointRowsArgs, V) + 32,
              "the four doubles lie where they lay");

} // namespace dftpav
