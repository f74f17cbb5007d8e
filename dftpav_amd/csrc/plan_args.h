// plan_args.h — what the host half of dftpav_plan_queries (capi.cpp) hands the kernels of plan.hip.
#pragma once
#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "footprint.h"
#include "piece_eval.h"

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

// plan_select_kernel: per member the cheapest restart that succeeded, does not collide and is not rejected; trajectory t = member * R + restart
struct PlanSelectArgs {
  const double *cost;                 // [n_members * R]
  const int *success, *collision;     // [n_members * R]; collision is the re-check's own output and is copied to r_collision as it is
  const int *reject;                  // [n_members * R] or nullptr: what the post-solve filters set (limits.hip, clearance.hip, the penalty gate)
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

// penalty_gate_kernel: one thread per trajectory t = member * R + restart of a group; row = (query, restart)
struct PenaltyGateArgs {
  const double *terms;    // [n][5] the terms of the cost per trajectory (CostTerm)
  const int *members;     // [n / R] query of each member; nullptr: row = t
  int n, R;
  double cap_corridor, cap_surround, cap_feas;
  double *r_terms;        // [rows][5] or nullptr
  int *r_rejected;        // [rows] or nullptr
  int *reject;            // [n] or nullptr: set to 1 where rejected, never read or cleared
};

// the executing table of a planner (capi.cpp: dftpav_planner_install / _adopt): one row per slot, device pointers.  n_seg == 0: empty.
// Padded as dftpav_plan_out: the pieces of a slot's segments follow one another in `coeffs`.
struct ExecTable {
  int n_slots, max_seg, max_pieces;
  int *n_seg;                              // [slots]
  int *singul, *piece_nums;                // [slots][max_seg]
  double *coeff_dt;                        // [slots][max_seg] duration of a piece of each segment
  double *coeffs;                          // [slots][max_seg * max_pieces][6][2]
  double *duration, *start_time, *end_time; // [slots][max_seg] (traj_container.hpp:58-73)
  double *end_state;                       // [slots][4] the goal the plan was made for
  double *hist;                            // [slots][2] previous desired state: time stamp, angle
  int *have_hist;                          // [slots]
};

// the publisher's state of every slot of the table (TrajPlannerServer::PublishData, traj_server_ros.cpp:195-318), beside the table: the
// kernels that take an ExecTable by value do not see it
struct PubTable {
  int *exe_index; // [slots] exe_traj_index_
  double *hist;   // [slots][2] ctrl_state_hist_.back(): time stamp, angle
  int *have;      // [slots] ctrl_state_hist_ is not empty
};

// exec_adopt_kernel: the winners of the last dftpav_plan_queries call into slots of the table, device to device
struct ExecAdoptArgs {
  ExecTable T;
  const int *pairs;         // [n][2] query, slot
  int n;
  const int *q_n_seg, *q_singul, *q_piece_nums; // the front end's rows of the call, by query
  const double *q_dt, *q_coeffs;                // the winners' piece durations [Q][max_seg] and pieces [Q][max_seg * max_pieces][12]
  const double *q_goal;                         // [Q][4]
  const double *desired;                        // [slots][8] or nullptr: the slot's new filter history (stamp, angle); nullptr: none
  double t_start;
};

// replan_check_kernel (replan.hip)
enum { kRcOccupied = 0, kRcComplete, kRcExeIndex, kRcCloseTurn, kRcNear, kRcTargetMoved, kRcCollision, kRcFirstSample, kRcReplan, kRcInts };
struct ReplanArgs {
  ExecTable T;
  DevGrid grid;
  DevFootprint fp;
  double wheel_base;
  SampleTable tab;
  double t_now, budget;
  const double *goals; // [slots][4] or nullptr: the stored goals
  const double *ego;   // [slots][6] x, y, angle, v, steer, acc, or nullptr
  int *o_int;          // [kRcInts][slots]
  double *desired, *start_state, *start_ctrl; // [slots][8], [slots][4], [slots][2]
};

// publish_kernel (replan.hip): K publisher ticks for every slot
enum { kPubChunk = DFTPAV_PUBLISH_CHUNK }; // ticks a workgroup takes at a time (its size)
struct PublishArgs {
  ExecTable T; // read only
  PubTable P;  // read, and written back at the end
  int K;
  const double *t; // [K] the clocks
  double wheel_base;
  double *states; // [K][slots][8]
  int *published; // [K][slots]
};

// pub_reset_kernel: the publisher's state of the slots an adoption fills (traj_server_ros.cpp:177)
enum { kPubKeep = 0, kPubDrop = 1, kPubSeed = 2 };
struct PubResetArgs {
  PubTable P;
  const int *pairs; // [n][2] query, slot (the adoption's)
  const int *mode;  // [n] kPubKeep: exe_index = 0, the history stays; kPubDrop: and no history; kPubSeed: the history from `desired`
  int n;
  const double *desired; // [slots][8], read for kPubSeed: time stamp, ., ., angle
};

} // namespace dftpav
