// cand_conflict_args.h — what the host half of the candidate conflict calls (dftpav_batch_check_conflicts, dftpav_batch_sample_poses,
// the conflict filter of dftpav_plan_queries) hands the kernels of cand_conflict.hip.
#pragma once
#include "../../include/dftpav_hip.h"
#include "conflict_args.h"
#include "device_types.h"

namespace dftpav {

// the candidates: the first B trajectories of a batch, as dftpav_batch_coeffs returns them, all starting at t_start
struct CandBatch {
  const double *coeffs;   // [B][Ntot][6][2]
  const double *piece_dt; // [B][M]
  DevLayout L;
  int B;
  double t_start;
  double t0, dt; // the clocks t0 + (double)k * dt
  double dcr;    // veh_d_cr
};

// cand_pose_kernel: the candidates' poses alone, [K][B][4] = cx, cy, cs, sn
struct CandPoseArgs {
  CandBatch C;
  int K;
  double *poses;
};

// cand_pair_kernel: workgroup g takes the candidates [64 g, 64 g + 64) against every J-tile of the table's poses
struct CandPairArgs {
  CandBatch C;
  ConflictPoses P;   // the table's poses at the same clocks (conflict_pose_kernel's), read only
  ConflictRows rows; // candidate c writes row c, or with members row members[c / R] * R + c % R (the [Q][R] rows of a call)
  const int *members;
  int R;
  const int *own; // nullptr: none; else the own slot (-1: none) of row c (no members) or of query members[c / R]
  int *reject;    // [B] or nullptr (the read-out); the filter: set to 1 where conflict_sample >= 0, never read or cleared
  PairConsts V;
};
static_assert(offsetof(CandPairArgs, V) == offsetof(CandPairArgs, reject) + 8 && sizeof(CandPairArgs) == offsetof(CandPairArgs, V) + 32,
              "the four doubles lie where they lay");

} // namespace dftpav
