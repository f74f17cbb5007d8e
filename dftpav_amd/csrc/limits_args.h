// limits_args.h — what the host half of dftpav_batch_check_limits / dftpav_planner_check_limits hands the kernels of limits.hip.
#pragma once
#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "piece_eval.h"
#include "plan_args.h"

namespace dftpav {

enum { kLimVel = 0, kLimAcc, kLimLatAcc, kLimCur, kLimSteer, kLimQ }; // the columns of dftpav_limits_out

// what both kernels share: the sample times, the limits and the result rows
struct LimitsCommon {
  SampleTable tab; // (validation_table)
  double wheel_base;
  double lim[kLimQ][2]; // [quantity][0] forward (singul > 0), [1] backward; one value twice where the limit has no direction
  double *max_abs;      // [rows][5]
  int *arg, *violated;  // [rows][5]
  int *feasible;        // [rows]
};

// limits_batch_kernel: the first B trajectories of a solved batch
struct LimitsBatchArgs {
  LimitsCommon C;
  const double *coeffs;   // [B][Ntot][6][2]
  const double *piece_dt; // [B][M]
  DevLayout L;
  int B;
  const int *members; // nullptr: trajectory b writes row b; else row members[b / R] * R + b % R (the [Q][R] rows of a call)
  int R;
  int *reject; // [B] or nullptr (the read-out call); the filter: set to 1 where the trajectory is not feasible, never read or cleared
};

// limits_table_kernel: every slot of the executing table (read only)
struct LimitsTableArgs {
  LimitsCommon C;
  ExecTable T;
};

} // namespace dftpav
