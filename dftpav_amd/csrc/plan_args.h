// plan_args.h — what the host half of dftpav_plan_queries (capi.cpp) hands the kernels of plan.hip.
#pragma once
#include "../../include/dftpav_hip.h"
#include "device_types.h"

namespace dftpav {

// plan_pack_kernel: the queries of one layout group, out of the padded front-end arrays into the group's batch
struct PlanPackArgs {
  DevLayout L;
  dftpav_frontend_out fe; // device pointers: the padded arrays of every query of the call
  const int *members;     // [n_members] query index (in the call) of each member of the group
  int n_members, n_restarts;
  double sigma, lo, hi; // the restart sampler's (restart.hip)
  unsigned long long seed;
  double mini_T, max_vel[2], max_acc[2]; // [0] forward, [1] backward (traj_optimizer.cpp:30-33, 65-76)
  double *x0, *iniS, *finS;              // the batch's arrays, trajectory t = member * n_restarts + restart
  double *poses;                         // [n_members][Npts][3] constraint-point poses of the hypotheses
  int *mini_t_flag;                      // [Q] set where a restart of the query fails the mini_T test
};

// plan_select_kernel: per member the cheapest restart that succeeded and does not collide; trajectory t = member * R + restart
struct PlanSelectArgs {
  const double *cost;                 // [n_members * R]
  const int *success, *collision;     // [n_members * R]
  const int *status, *iters, *evals, *first_sample; // [n_members * R], may be nullptr (then nothing per restart is copied)
  const double *x, *coef, *dt;        // [..][n], [..][n_coef], [..][M]; may be nullptr
  int n, n_coef, M;
  const int *members; // [n_members] query of each member; nullptr: member m is query m
  int n_members, R;
  // compact outputs, indexed by query
  int *winner;
  double *w_cost;
  int *w_iters;
  double *w_x, *w_coef, *w_dt;
  int x_stride, coef_stride, dt_stride;
  double *r_cost; // [Q][R]
  int *r_status, *r_success, *r_iters, *r_evals, *r_collision, *r_first_sample;
};

} // namespace dftpav
