// capi_internal.h — what the host translation units behind libdftpav_hip.so share (capi*.cpp; no kernel file includes it): the
// objects behind the C-ABI's opaque pointers, the kernels' launch functions, and the helpers that more than one unit calls.
//   capi.cpp          parameters, handle, moving obstacles, batch create / upload / order / solve / results / trace
//   capi_steps.cpp    the steps around a solve: restarts, resampling, shots, search, map, corridor, re-check, read-out, plan cycle
//   capi_planner.cpp  dftpav_plan_queries, the executing table, the replan check / tick, the publisher, the limit / penalty / clearance
//                     filters, the stamps of the executing plans
//   capi_conflicts.cpp  the footprint conflicts: between executing plans, of candidates against them (the conflict filter), joint
//                     selection, the conflict trigger
//   capi_comm.cpp     RCCL                capi_wire.cpp     the "DPTJ" serialisation
// There is deliberately no CPU fallback: without a usable HIP device every entry point that needs one fails with DFTPAV_E_NO_DEVICE.
// Device times are taken with EventMarks<N> (below) alone: the events exist from their first record on, complete(k) is the one flag a
// read-out tests before it asks for elapsed(), and the owner's `delete` releases them (dftpav_destroy: in front of the stream).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <vector>

#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "e4_plan.h"
#include "traj_math.h"
#include "cr_trig.h"
#include "rs_math.h"
#include "step_args.h"
#include "search_args.h"
#include "plan_args.h"
#include "limits_args.h"
#include "clearance_args.h"
#include "conflict_args.h"
#include "cand_conflict_args.h"
#include "conflict_trigger_args.h"
#include "joint_args.h"
#include "stamp_args.h"
#include "render_args.h"
#include "goalfield_args.h"

namespace dftpav {
hipError_t launch_solver(const DevBatch &D, const DevBatch *d_dev, int mode, int threads, int grid, SchedArgs sched,
                         hipStream_t stream);
hipError_t launch_corridor(const CorridorArgs &A, hipStream_t stream); // (A.res_rcp is set there)
hipError_t launch_frontend(const dftpav_frontend_params &fp, const double *paths, const int *path_len, int max_path,
                           const double *start_states, const double *end_states, const double *start_ctrl, int n_hyp,
                           const dftpav_frontend_out &out, hipStream_t stream);
hipError_t launch_restarts(const double *inner, const double *durs, int n_hyp, int n_restarts, int n_inner, int M, double sigma,
                           double lo, double hi, unsigned long long seed, double *out_inner, double *out_durs, hipStream_t stream);
hipError_t launch_fit(const double *states, int S, int n_states, const double *opM, double *dur, double *coef, double *total,
                      double *start, hipStream_t stream);
hipError_t launch_validate(const ValidateArgs &A, hipStream_t stream);
hipError_t launch_states(const double *coeffs, const double *piece_dt, const DevLayout &L, int B, double wheel_base, double t0,
                         double sample_dt, int n_samples, int filter, double *states, int *n_valid, hipStream_t stream);
hipError_t launch_shots(const ShotArgs &A, hipStream_t stream);
hipError_t launch_search(const SearchArgs &A, int blocks, hipStream_t stream);
// plan.hip: the kernels between the stages of dftpav_plan_queries
hipError_t launch_plan_paths(const int *status, const int *path_len, const int *skip, int n, int max_path, double *paths, int *fe_len,
                             hipStream_t stream);
hipError_t launch_plan_pack(const PlanPackArgs &A, hipStream_t stream);
hipError_t launch_plan_select(const PlanSelectArgs &A, hipStream_t stream);
hipError_t launch_penalty_gate(const PenaltyGateArgs &A, hipStream_t stream);
hipError_t launch_replan_check(const ReplanArgs &A, hipStream_t stream);
hipError_t launch_exec_adopt(const ExecAdoptArgs &A, hipStream_t stream);
hipError_t launch_publish(const PublishArgs &A, hipStream_t stream);
hipError_t launch_pub_reset(const PubResetArgs &A, hipStream_t stream);
// limits.hip: solved plans against the kinematic limits
hipError_t launch_limits_batch(const LimitsBatchArgs &A, hipStream_t stream);
hipError_t launch_limits_table(const LimitsTableArgs &A, hipStream_t stream);
// distfield.hip, clearance.hip: the distance field of the map, the clearance of solved plans
hipError_t launch_dist_field(const DistFieldArgs &A, hipStream_t stream);
hipError_t launch_clearance_batch(const ClearanceBatchArgs &A, hipStream_t stream);
hipError_t launch_clearance_table(const ClearanceTableArgs &A, hipStream_t stream);
// conflict.hip: the poses of the executing plans at K clocks, their pairwise separation per (I-tile, J-tile), the rows per slot
hipError_t launch_conflict_poses(const ConflictPoseArgs &A, hipStream_t stream);
hipError_t launch_conflict_pairs(const ConflictPairArgs &A, hipStream_t stream);
hipError_t launch_conflict_reduce(const ConflictReduceArgs &A, hipStream_t stream);
// cand_conflict.hip: the poses of a batch's candidates at K clocks; their separation from the table's poses, the rows per candidate
hipError_t launch_cand_poses(const CandPoseArgs &A, hipStream_t stream);
hipError_t launch_cand_pairs(const CandPairArgs &A, hipStream_t stream);
// joint_select.hip: the candidates of a call against each other: their poses per group, the conflict bits per (I-tile, J-tile), the
// greedy walk over the queries, the rows per candidate
hipError_t launch_joint_poses(const JointPoseArgs &A, hipStream_t stream);
hipError_t launch_joint_pairs(const JointPairArgs &A, hipStream_t stream);
hipError_t launch_joint_greedy(const JointGreedyArgs &A, hipStream_t stream);
hipError_t launch_joint_rows(const JointRowsArgs &A, hipStream_t stream);
// conflict_trigger.hip: behind launch_conflict_poses, the pair-samples that make a slot yield per (I-tile, J-tile), the rows per slot
hipError_t launch_trigger_pairs(const TriggerPairArgs &A, hipStream_t stream);
hipError_t launch_trigger_reduce(const TriggerReduceArgs &A, hipStream_t stream);
// stamp.hip: boxes into the working map, the bit map from the bytes again, the cells stamped since the base copy
hipError_t launch_stamp_boxes(const StampBoxArgs &A, hipStream_t stream);
hipError_t launch_stamp_bits(const StampBitsArgs &A, hipStream_t stream);
hipError_t launch_stamp_count(const StampCountArgs &A, hipStream_t stream);
int stamp_count_blocks(size_t n_cells); // the partial counts launch_stamp_count writes
// render.hip: the background, then the polygons (interior, outline), circles and points of an obstacle set into the map
hipError_t launch_render(const RenderArgs &A, hipStream_t stream);
// goalfield.hip: the cost-to-go fields of n goal cells, one workgroup each
hipError_t launch_goal_fields(const GoalFieldArgs &A, int n, hipStream_t stream);
// rstable.hip: every entry of the Reeds-Shepp cost-to-go table
hipError_t launch_rs_table(const RsTableArgs &A, hipStream_t stream);
hipError_t launch_corridor_layout(const double *raw, double *out, int B, int Npts, int H, int NptsPad, hipStream_t stream);
hipError_t launch_adopt(const DevBatch &D, const DevBatch &prev, hipStream_t stream);
// solver_ref.hip: the same path in the reference's own floating-point order
bool reference_order_supported(const DevLayout &L, const DevParams &P, int S);
size_t reference_order_scratch_doubles(const DevLayout &L, int B, int S);
size_t reference_order_table_doubles(int N);
void reference_order_pack_tables(int N, const double *full, double *packed);
int reference_order_interior_mask(int sweep, int row_mod_6);
RefPlan reference_order_plan(const DevLayout &L, const DevParams &P, int S, int B, int n_cu, bool throughput, const RefOptions &o);
hipError_t launch_ring_reset(const DevBatch &D, hipStream_t stream);
hipError_t launch_solver_ref(const DevBatch &D, const DevBatch *d_dev, int mode, const double *tabs, double *scratch, const RefPlan &pl, int scheduled,
                             hipStream_t stream);
hipError_t prepare_solver_quad(const RefPlan &pl); // once per plan, in front of its first launch_solver_quad
hipError_t launch_solver_quad(const DevBatch &D, const DevBatch *d_dev, int mode, const double *tabs, const double *cor_t, bool rect, double *scratch,
                              const RefPlan &pl, int scheduled, bool alone, hipStream_t stream);
// the QUAD shapes' copy of the corridor (solver_ref4.hip: one gear segment, solver_ref4m.hip: several)
size_t reference_order_quad_corridor_doubles(const DevLayout &L, int B);
hipError_t launch_quad_corridor(const DevBatch &D, double *cor_t, bool rect, hipStream_t stream);
hipError_t launch_quad_rect_check(const double *corridor, int B, int Npts, int NptsPad, int *d_flag, hipStream_t stream);
hipError_t launch_quadm_corridor(const DevBatch &D, double *cor_t, hipStream_t stream);
}
using namespace dftpav;

// N marks on a stream and the time between any two of them.  A chain of enqueued work records mark k in front of or behind its
// kernels; reset() at its start and complete(k) at its end -- "the last chain that used these marks ran up to mark k" -- make the
// flag that a read-out tests with reached(k).  A chain that never calls reset() keeps reporting its last complete run.  The events
// are created by their first record and destroyed with the object: the owner is deleted with its device current and, where it
// owns the stream, in front of the stream's destruction.
template <int N> struct EventMarks {
  hipEvent_t ev[N] = {};
  int done = 0; // marks [0, done) are those of a complete chain
  EventMarks() = default;
  EventMarks(const EventMarks &) = delete;
  EventMarks &operator=(const EventMarks &) = delete;
  ~EventMarks() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t record(int k, hipStream_t stream) {
    if (!ev[k])
      if (hipError_t e = hipEventCreate(&ev[k])) return e;
    return hipEventRecord(ev[k], stream);
  }
  void reset() { done = 0; }
  void complete(int k = N - 1) { done = k + 1; }
  bool reached(int k = N - 1) const { return done > k; }
  // ms from mark a to mark b.  wait: synchronises on mark b first -- for the chains that return without a wait for the stream; the
  // read-outs of chains that end with one pass false.  The caller has tested reached(b).
  hipError_t elapsed(float *ms, int a, int b, bool wait) const {
    if (wait)
      if (hipError_t e = hipEventSynchronize(ev[b])) return e;
    return hipEventElapsedTime(ms, ev[a], ev[b]);
  }
};

struct CommShared; // capi_comm.cpp: an RCCL communicator and its holders

struct dftpav_handle {
  dftpav_params params;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // moving obstacles (device copies)
  int S = 0;
  int sur_pieces = 0; // pieces of all obstacles together
  int sur_version = 0; // bumped by dftpav_set_surround so batches refresh their device descriptor
  int *d_sur_off = nullptr;
  double *d_sur_dur = nullptr, *d_sur_coef = nullptr, *d_sur_total = nullptr, *d_sur_start = nullptr, *d_sur_theta = nullptr, *d_sur_bbox = nullptr;
  // obstacle map of the corridor generator (device copy) and the table of sample offsets along a line
  dftpav_grid_map map{};
  unsigned char *d_cells = nullptr;
  unsigned *d_bits = nullptr; // one bit per cell, when the whole map fits in a quarter of the LDS
  double *d_dl = nullptr;
  int n_dl = 0;
  EventMarks<2> cor_ev;                    // around the last kernel of the corridor family (dftpav_corridor_last_ms)
  hipEvent_t mark[2] = {nullptr, nullptr}; // dftpav_mark
  EventMarks<2> lim_ev;                    // around the last limits kernel of a check_limits call
  // the distance field of the map (distfield.hip): built by the first clearance call after a dftpav_set_grid_map, never otherwise
  int *d_dist = nullptr; // one allocation: d2 [cells], then the row pass's g [cells]
  size_t dist_cells = 0; // what d_dist holds room for
  bool dist_stale = true;
  EventMarks<2> field_ev, clr_ev; // around the last field build / the last clearance kernel of a check call
  EventMarks<3> conf_ev; // conflict.hip: in front of the pose kernel, between it and the pair kernel, behind the reduce kernel; of the
                         // last dftpav_planner_sample_poses (complete to mark 1) / _check_conflicts (to mark 2) call
  EventMarks<3> cand_ev; // cand_conflict.hip: in front of the pose kernel (the table's; dftpav_batch_sample_poses: the candidates'), between it
                         // and the pair kernel, behind the pair kernel; of the last dftpav_batch_sample_poses (complete to mark 1) /
                         // dftpav_batch_check_conflicts (to mark 2) call
  EventMarks<4> joint_ev; // joint_select.hip: in front of the pose kernels, behind them, behind the pair kernel, behind the greedy and row
                          // kernels; of the last dftpav_plan_queries call with joint selection or dftpav_debug_joint_select (marks 1 to 3)
  bool joint_posed = false; // that chain ran the pose kernels
  EventMarks<3> trig_ev; // conflict_trigger.hip: in front of the pose kernel, between it and the pair kernel, behind the reduce kernel; of the
                         // last dftpav_planner_check_yield, dftpav_replan_tick with the trigger on, or dftpav_debug_conflict_trigger
  bool trig_posed = false; // that chain ran the pose kernel (the debug hook records marks 1 and 2)
  // the stamps (stamp.hip): nothing of it exists until a stamp call.  d_cells stays the working map every call reads
  unsigned char *d_cells_base = nullptr; // the map as uploaded: copied by the first stamp after a dftpav_set_grid_map, which drops it
  unsigned char *d_stamp_ws = nullptr;   // dftpav_planner_stamp_slots: the poses 4 x [K][S_pad], occupied [S_pad], select [S_pad];
  size_t stamp_ws_bytes = 0;             // kept from call to call, so the call waits for nothing
  std::vector<unsigned char> stamp_sel;  // the host source of select's asynchronous copy, and the event behind that copy: the
  hipEvent_t stamp_sel_ev = nullptr;     // next call waits for it before it writes the vector again
  EventMarks<3> stamp_ev; // of the last stamp call: in front of the pose kernel, between it and the box kernel, behind the box kernel
  bool stamp_posed = false; // that call ran the pose kernel (dftpav_planner_stamp_slots); dftpav_grid_stamp_poses records marks 1 and 2
  // the rendered map (render.hip): nothing of it exists until a dftpav_grid_render
  unsigned char *d_render_ws = nullptr; // the snapped obstacle set of one call: poly_off | boxes | edges | circles | points; kept from
  size_t render_ws_bytes = 0;           // call to call (every call ends with a wait, so the next finds it idle)
  EventMarks<2> render_ev;              // in front of the background kernel, behind the last kernel of the last render
  // the search heuristic (dftpav_set_search_heuristic) and the workspace of the goal fields (goalfield.hip): nothing of it is
  // allocated or launched until a call asks for a field
  dftpav_goal_field_params heu{0, 0.0, 0.0};
  double heu_margin = -1.0; // dftpav_set_search_heuristic_window; < 0: whole-map fields.  Read only while heu.enabled
  int *d_gf = nullptr;      // the fields of one turn [goals][cells], then their dirty maps [goals][tiles]; windowed: each field
                            // [WY][WX] at its offset, then the dirty maps at the stride of the turn's largest
  size_t gf_ints = 0;
  int *d_gf_meta = nullptr; // of a whole call: field_of [queries], goal cells [goals][2], (windowed: windows [goals][4], a pad to an
                            // even count, offsets [goals] as 64-bit,) n_reached [goals]
  size_t gf_meta_ints = 0;
  std::vector<int> gf_host; // the host copy of all of it but n_reached (the source of an asynchronous copy)
  std::deque<EventMarks<2>> gf_ev; // a pair around every turn's build
  int gf_timed = 0;                // pairs recorded by the last call that built fields
  // the Reeds-Shepp term of the search heuristic (dftpav_set_search_rs_heuristic) and its table (rstable.hip): built in front of
  // the first search launch that needs it, kept until a call asks for another key (rho, n_yaw, extent, cell)
  dftpav_rs_heuristic_params rsh{0, 0, 0.0, 0.0, 0.0};
  double *d_rs = nullptr;
  size_t rs_doubles = 0;
  double rs_rho = 0.0, rs_extent = 0.0, rs_cell = 0.0; // the key of what d_rs holds; rs_n_yaw == 0: nothing
  int rs_n_yaw = 0;
  int rs_builds = 0; // launches of rs_table_kernel over the handle's life
  EventMarks<2> rs_ev; // around the last build
  std::vector<struct dftpav_batch *> batches; // every live batch of this handle (obstacle changes finish their chained stragglers)
  // RCCL communicator of dftpav_comm_create (one rank per handle = per GPU), and the staging block of this rank's records
  void *comm = nullptr;
  struct CommShared *comm_ref = nullptr; // the communicator's holders (dftpav_comm_share): destroyed when the last one lets go
  int comm_ranks = 0, comm_rank = 0;
  unsigned char *d_comm_send = nullptr;
  size_t comm_send_bytes = 0;
  // workspace of dftpav_kino_search (node pools, heaps, hash tables of the queries in flight), grown on demand
  void *d_search_ws = nullptr;
  size_t search_ws_bytes = 0;
};

struct dftpav_batch {
  dftpav_handle *h = nullptr;
  int B = 0;
  int n_active = 0; // dftpav_plan_queries: the leading trajectories in use this call (0: all B); the kernels see it as the batch size
  DevLayout L{};
  DevParams P{};
  int threads = 0;
  bool op_in_lds = false, cor_in_lds = false;
  bool have_corridor = false; // set by dftpav_batch_upload (host corridor) or dftpav_batch_corridor_from_states
  // time-sliced scheduling (batches larger than the device holds at once): the queue launch runs in the
  // shape above, the stragglers it hands over finish in the latency shape below
  bool sched = false;
  int slots = 0, slice = 0, hand_over = 0;
  int threads2 = 0;
  bool op_in_lds2 = false, cor_in_lds2 = false;
  int *d_queue = nullptr, *d_stragglers = nullptr, *d_stragglers2 = nullptr, *d_sflag = nullptr, *d_iota = nullptr;
  int qcap = 0;
  bool pending = false; // a chained solve left this batch's stragglers for the next chained solve (or dftpav_batch_finish)
  unsigned *d_qctl = nullptr;
  double *d_state = nullptr;
  DevBatch *d_dev2 = nullptr;
  // E4 lane plans (e4_plan.h) of the two launch shapes: host copies of the sizes, device tables
  E4Sizes e4{}, e4b{};
  int *d_e4[2][5] = {{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}}; // gtab, ltab, wave, round, piece
  int NptsPad = 0;
  std::vector<double> x0_host;
  bool uploaded = false;
  double t_now = 0.0, epis = 0.0;
  // device buffers
  double *d_x0 = nullptr, *d_iniS = nullptr, *d_finS = nullptr, *d_corridor = nullptr;
  int16_t *d_pt_piece = nullptr, *d_pt_j = nullptr;
  double *d_opM[kMaxSeg] = {nullptr}, *d_opMT[kMaxSeg] = {nullptr};
  double *d_histS = nullptr, *d_histY = nullptr, *d_histU = nullptr, *d_histV = nullptr, *d_histR = nullptr;
  double *d_histM = nullptr; // QUAD shape of the reference order: the mirrored ends of the history rings (DevBatch::histM)
  double *d_x_in = nullptr, *d_x_out = nullptr, *d_f = nullptr, *d_g = nullptr;
  int *d_status = nullptr, *d_success = nullptr, *d_iters = nullptr, *d_evals = nullptr;
  long long *d_hist = nullptr, *d_ticks = nullptr, *d_prof = nullptr;
  unsigned char *d_records = nullptr; // [B + 1][16] result records written by the solver's epilogue (+ one zero record of padding)
  unsigned char *h_records = nullptr; // [B][16] the same in pinned host memory, written by the epilogues too (DevBatch::records_host)
  DevBatch *d_dev = nullptr; // device copy of the launch descriptor
  int dev_version = -1;
  // pinned host staging of the two descriptors and the event behind their last copy: refreshing the device copies then
  // needs no stream synchronisation (dftpav_plan_cycle enqueues the corridor kernel in front of the solve and must not wait for it)
  DevBatch *h_stage = nullptr;
  hipEvent_t stage_ev = nullptr;
  bool stage_busy = false;
  bool prof_on = false;
  double *d_coef = nullptr, *d_dt = nullptr;
  double *d_f_eval = nullptr; // costs of dftpav_batch_eval (kept apart from the solve's final costs)
  double *d_terms = nullptr;  // dftpav_batch_cost_terms: terms [B][5], then seg_terms [B][M][5]
  double *d_trace = nullptr;  // dftpav_batch_trace
  double *d_cor_raw = nullptr; // the caller's hPoly columns as uploaded (normalised and laid out on the device)
  // dftpav_batch_set_order(DFTPAV_ORDER_REFERENCE): the substitution tables of the band system and the term records (solver_ref.hip)
  int order = DFTPAV_ORDER_DEVICE;
  int ref_S = 0; // moving obstacles on the handle when the reference order was chosen (the term records are sized for them)
  double *d_ref_tab = nullptr, *d_ref_scratch = nullptr;
  RefPlan ref_plan{}; // its launch plan (chosen with the order)
  double *d_cor_t = nullptr; // QUAD shapes: the corridor as [B][4 H][Kmax + 1][16] (solver_ref4.hip), refreshed when the corridor changes
  bool cor_t_dirty = true;
  // Rectangles (solver_ref4.hip: RECT).  cor_rect: every corridor in d_corridor is known to be one -- learned by dftpav_batch_upload,
  // which waits for the device anyway; the corridors the device makes from the map (dftpav_batch_corridor_from_hypotheses,
  // dftpav_plan_cycle: no wait, none added) leave it false and run the sixteen-double layout.  cor_t_rect: the layout d_cor_t is in.
  bool cor_rect = false, cor_t_rect = false;
  int *d_rect_flag = nullptr;
  bool coef_override = false; // test hook dftpav_debug_batch_set_coeffs: validate / sample_states take the coefficients as they are
  int residency = -1; // the caller's residency hint (dftpav_batch_create_shaped); 2 = many such batches in flight: the throughput shapes whatever B
  // dftpav_plan_cycle: work buffers that live from the call to dftpav_plan_cycle_fetch (reused by the next cycle)
  struct PlanCycle {
    double *d_poses = nullptr, *d_tab = nullptr, *d_rd = nullptr; // d_tab: the validation_table of the re-check
    int *d_col = nullptr, *d_first = nullptr, *d_valid = nullptr;
    size_t n_poses = 0, n_tab = 0, n_rd = 0;
    std::vector<double> poses, tab; // host sources of the asynchronous copies
    int n_samples = 0;
    bool in_flight = false;
  } pc;
  int trace_b = -1, trace_cap = 0, trace_n = 0;
  EventMarks<2> solve_ev; // around the last solve; complete once one was enqueued
  bool solved = false; // results of a solve of the CURRENT inputs exist (cleared by dftpav_batch_upload)
};

#define HIPCHK(h, call)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
      return DFTPAV_E_HIP;                                                               \
    }                                                                                    \
  } while (0)

// the handle's map and vehicle as the kernels take them (footprint.h); v_tab: the spacings of the outline points on the device
inline DevGrid dev_grid(const dftpav_handle *h) {
  return DevGrid{h->d_cells, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y};
}
inline DevFootprint dev_footprint(const dftpav_handle *h, const double *v_tab, int n_v) {
  return DevFootprint{h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, v_tab, n_v};
}

// What a launch of the search needs besides the queries and the outputs: the checked parameters, the tables of the running sums
// (inputs, outline point spacing, shot sample offsets; `tabs` is their host copy, in_tab | v_tab | l_tab) and the handle's
// workspace for `slots` queries in flight.  Shared by dftpav_kino_search and dftpav_plan_queries.
struct SearchSetup {
  SearchArgs S{};
  std::vector<double> tabs;
  size_t n_in_tab = 0, n_vv = 0, n_ll = 0;
  int slots = 0;
};

// a validation_table kept on the device by a selection filter, and the check_dt it was tabulated for
struct CachedTable {
  double *d = nullptr;
  int n_t = 0, n_v = 0;
  double dt = 0.0;
};

// The goal fields of one call's queries (the heuristic on): which field each query reads and which cells are built, turn by turn.
// A turn is one launch of the search over `per_turn` queries (the search's slots, or fewer where the workspace cap holds fewer
// fields); its distinct goal cells are goals [turn_off[t], turn_off[t + 1]) and field_of is relative to the turn.
// Windowed (dftpav_set_search_heuristic_window, dftpav_grid_goal_field_windowed): a field belongs to a (goal cell, window) pair,
// win / off are every field's window and its offset in ints inside its turn's workspace, and a turn uses turn_ints[t] ints of
// fields and a dirty map of turn_tiles[t] words per field behind them.
struct GoalFieldPlan {
  int per_turn = 0, T = 0;
  std::vector<int> turn_off;
  size_t n_goals = 0;
  const int *d_field_of = nullptr, *d_cells = nullptr;
  int *d_reached = nullptr;
  double unit = 0.0;
  bool windowed = false;
  std::vector<int> win;       // [n_goals][4]
  std::vector<long long> off; // [n_goals]
  std::vector<size_t> turn_ints;
  std::vector<int> turn_tiles;
  const int *d_win = nullptr;
  const long long *d_off = nullptr;
};

// n rows of a limits check wired into C: max_abs [n][5] at d_max, then arg [n][5] | violated [n][5] | feasible [n] from d_int on
inline void limit_rows(LimitsCommon &C, double *d_max, int *d_int, size_t n) {
  C.max_abs = d_max;
  C.arg = d_int;
  C.violated = d_int + kLimQ * n;
  C.feasible = d_int + 2 * kLimQ * n;
}

// five rows [n] wired from their two bases: min_sep at d_sep; sep_sample | sep_partner | conflict_sample | conflict_partner from d_int on
inline ConflictRows conflict_rows(double *d_sep, int *d_int, size_t n) {
  return ConflictRows{d_sep, d_int, d_int + n, d_int + 2 * n, d_int + 3 * n};
}

// The selection filters of dftpav_plan_queries: four structs of one shape (capi_planner.cpp; the conflict filter, joint selection and
// the trigger behind it: capi_conflicts.cpp).  Each holds its switch (`on`, and
// `last`: the last dftpav_plan_queries call ran with it), its parameters and its one allocation `d` -- the sample table at its head
// where the filter has one, then the rows [cap = max_queries * R] of a call -- and states the same operations once:
//   configure  the set_*_filter entry behind its argument checks: allocates on first use, switches on; a refusal changes nothing
//   clear      the rows of a call (rows = Q * R) as a trajectory that no kernel visits reports them
//   run        one group's launch: the batch's first nm * R trajectories into the rows of `members`, `reject` set where it rejects
//   fetch      the rows of the last call into the caller's arrays (nothing waits)
//   release    the allocation (dftpav_planner_destroy)
// Off by default, and then a call allocates, clears and launches nothing of it.
struct LimitFilter {
  bool on = false, last = false;
  dftpav_limits lim{};
  unsigned char *d = nullptr;
  CachedTable tab; // (its dt is the filter's check_dt)
  size_t cap = 0;
  double *d_max = nullptr; // max_abs
  int *d_int = nullptr;    // arg | violated | feasible (limit_rows)
  LimitsCommon rows() const { LimitsCommon C{}; limit_rows(C, d_max, d_int, cap); return C; } // the rows alone: the one place they are wired
  bool common(const dftpav_handle *h, LimitsCommon &C) const; // limits, sample table and rows; false: limits_common refused
  int configure(dftpav_handle *h, size_t rows_cap, const dftpav_limits &l, double check_dt);
  int clear(dftpav_handle *h, size_t rows);
  int run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject);
  int fetch(dftpav_handle *h, const dftpav_limits_out *out, size_t rows);
  void release() { if (d) (void)hipFree(d); }
};
struct PenaltyFilter {
  bool on = false, last = false;
  dftpav_penalty_caps caps{};
  unsigned char *d = nullptr;
  double *d_terms = nullptr;
  int *d_rej = nullptr;
  int configure(dftpav_handle *h, size_t rows_cap, const dftpav_penalty_caps &c);
  int clear(dftpav_handle *h, size_t rows);
  int run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject);
  int fetch(dftpav_handle *h, double *r_terms, int *r_rejected, size_t rows);
  void release() { if (d) (void)hipFree(d); }
};
struct ClearanceFilter {
  bool on = false, last = false;
  double min = -1.0;
  unsigned char *d = nullptr;
  CachedTable tab; // (both tables; its dt is the filter's check_dt)
  double *d_m = nullptr;
  int *d_d2 = nullptr, *d_arg = nullptr;
  std::vector<double> h_inf; // +inf, the rows' clearance before a call's kernels run
  int configure(dftpav_handle *h, size_t rows_cap, double min_clearance, double check_dt);
  int clear(dftpav_handle *h, size_t rows);
  int run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject);
  int fetch(dftpav_handle *h, const dftpav_clearance_out *out, size_t rows);
  void release() { if (d) (void)hipFree(d); }
};

// The conflict filter: rejects a trajectory that comes within `margin` of an executing plan at one of the K clocks t_now + k dt
// (cand_conflict.hip).  Its allocation holds the table's poses at the call's clocks (4 x [K][S_pad], occupied [S_pad]), the own
// slots [max_queries] and the rows.  clear also uploads the call's own slots and launches conflict_pose_kernel, once per call; with a
// table never filled or all empty it launches nothing, and run then launches nothing either: the cleared rows stand.
struct ConflictFilter {
  bool on = false, last = false;
  double margin = -1.0, range = 0.0, dt = 0.0;
  int K = 0;
  unsigned char *d = nullptr;
  int cap_K = 0; // the K the allocation was made for
  double *d_pose = nullptr, *d_sep = nullptr;
  unsigned char *d_occupied = nullptr;
  int *d_own = nullptr, *d_int = nullptr; // d_int: sep_sample | sep_partner | conflict_sample | conflict_partner, each [cap]
  size_t cap = 0;
  std::vector<double> h_inf; // +inf, the rows' min_sep before a call's kernels run
  std::vector<int> h_own;    // the host source of the own slots' copy
  ConflictPoses P{};         // the table's poses of the running call
  double t_call = 0.0;       // its t_now
  bool have_table = false;   // it found an occupied slot
  ConflictRows rows() const { return conflict_rows(d_sep, d_int, cap); }
  int configure(struct dftpav_planner *p, double margin_, double range_, double dt_, int K_);
  int clear(struct dftpav_planner *p, size_t n_rows, double t_now, const std::vector<int> &own);
  int run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject);
  int fetch(dftpav_handle *h, const dftpav_conflict_out *out, size_t n_rows);
  void release() { if (d) (void)hipFree(d); }
};

// Joint selection, an option of the conflict filter (joint_select.hip): the candidates of a call against each other, the queries in
// call order.  One allocation: the poses 4 x [cap_K][C_pad], the conflict bits [C_pad][C_pad / 64], per candidate cost, eligibility,
// flag index, blocked and the five rows, per query the winner and its candidate index.  The filters' shape: configure, clear, run
// (the joint stage of a call, behind the last group), fetch, release.  It runs only with the conflict filter on.
struct JointSelect {
  bool on = false, last = false;
  unsigned char *d = nullptr;
  size_t cap = 0, cap_pad = 0; // candidates max_queries * R, and rounded up to whole tiles
  int cap_K = 0;               // the K the allocation was made for
  double *d_pose = nullptr, *d_cost = nullptr, *d_sep = nullptr;
  unsigned long long *d_bits = nullptr;
  int *d_elig = nullptr, *d_flag = nullptr, *d_blocked = nullptr, *d_winner = nullptr, *d_wcand = nullptr;
  int *d_int = nullptr; // sep_sample | sep_partner | conflict_sample | conflict_partner, each [cap]
  std::vector<double> h_inf; // +inf, the rows' min_sep before a call's kernels run
  JointPoses P{};            // the poses of the running call
  ConflictRows rows() const { return conflict_rows(d_sep, d_int, cap); }
  JointCands cands() const { return JointCands{d_cost, d_elig, d_flag}; }
  static bool fits(size_t candidates, int K) {
    return candidates <= (size_t)DFTPAV_JOINT_MAX_CANDIDATES && candidates * (size_t)(K > 0 ? K : 1) <= ((size_t)1 << 22);
  }
  int configure(struct dftpav_planner *p, int K); // DFTPAV_E_UNSUPPORTED beyond the two design bounds, and nothing changed
  int clear(struct dftpav_planner *p, int Q, int K);
  int pose_group(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int flag0, const int *col, const int *reject,
                 double t_call, double dt);
  int run(struct dftpav_planner *p, int Q, double margin, double range); // pair bits, greedy, rows
  int fetch(dftpav_handle *h, const dftpav_conflict_out *out, int *blocked, size_t n_rows);
  void release() { if (d) (void)hipFree(d); }
};

// The conflict trigger of the tick (conflict_trigger.hip): which executing plans meet at the adoption clock, and which of the two
// slots gives way.  One allocation, made by configure: the table's poses 4 x [cap_K][S_pad], occupied [S_pad], the partial rows
// sample | partner, each [tiles][S_pad], and the rows yield | sample | partner, each [max_queries].  A tick allocates nothing.
struct ConflictTrigger {
  bool on = false, last = false; // last: the last tick ran with it, and d_rows holds that tick's rows
  double margin = -1.0, range = 0.0, dt = 0.0;
  int K = 0;
  unsigned char *d = nullptr;
  int cap_K = 0; // the K the allocation was made for
  double *d_pose = nullptr;
  unsigned char *d_occupied = nullptr;
  int *d_part = nullptr, *d_rows = nullptr;
  std::vector<int> h_yield; // the tick's copy of yield [max_queries] (the planner's: a failing call leaves nothing the stream still writes)
  int configure(struct dftpav_planner *p, double margin_, double range_, double dt_, int K_);
  int run(struct dftpav_planner *p, double t_now, double t0); // poses at t0 + k dt, pairs, rows: enqueued, nothing waits
  int fetch(struct dftpav_planner *p, const dftpav_yield_out *out);
  void release() { if (d) (void)hipFree(d); }
};

struct dftpav_planner {
  dftpav_handle *h = nullptr;
  int max_queries = 0, R = 0;
  struct Entry {
    std::vector<int> key; // M, singul[M], piece_nums[M]
    dftpav_batch *b;
  };
  std::vector<Entry> cache; // one batch per layout met so far
  // device work buffers: one allocation, carved up for the paddings of the last call (kept while they do not change)
  unsigned char *d_arena = nullptr;
  size_t arena_bytes = 0;
  long long sig[6] = {0, 0, 0, 0, 0, 0}; // max_seg, max_pieces, max_path, max_states, doubles of the search tables, of the validation tables
  double *d_st = nullptr, *d_en = nullptr, *d_ct = nullptr, *d_tabs = nullptr, *d_paths = nullptr, *d_vt = nullptr;
  int *d_skip = nullptr, *d_sints = nullptr, *d_fe_len = nullptr, *d_members = nullptr, *d_minit = nullptr, *d_col = nullptr, *d_first = nullptr;
  // what the selection filters set, indexed like d_col (trajectory order, a group at g_off[g] * R): cleared once per call that runs with a
  // filter, written by the filters' kernels only where they reject, read by the selection beside d_col.  Never touched with every filter off.
  int *d_reject = nullptr;
  dftpav_frontend_out fe{}; // device pointers
  double *d_poses = nullptr;
  size_t fe_zero_bytes = 0; // the front-end outputs are one stretch of the arena, zeroed per call (as dftpav_frontend_resample does)
  unsigned char *d_fe0 = nullptr;
  // compact outputs (zeroed per call): one stretch too
  unsigned char *d_out0 = nullptr;
  size_t out_zero_bytes = 0;
  int *d_winner = nullptr, *d_witers = nullptr, *d_rint[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double *d_wcost = nullptr, *d_wx = nullptr, *d_wcoef = nullptr, *d_wdt = nullptr, *d_rcost = nullptr;
  EventMarks<4> plan_ev; // dftpav_plan_queries: in front of the search, behind it, behind the resampling, at the end
  std::vector<int> group_sizes;
  // host staging of the tables that decide the grouping
  std::vector<int> h_sints, h_nseg, h_singul, h_pn, h_nstates, h_skip, h_members, h_minit;
  std::vector<double> h_dt, h_vt;
  // the host side of every copy from the device that a planner call enqueues and is not the caller's own memory lives here, not in
  // the call's scope: a call that leaves early leaves nothing behind that the stream still writes.  The winners of a call are
  // fetched into last_winner (below); these are the tick's: the replan flags [slots], the start states [slots][4], controls [slots][2]
  std::vector<int> h_rc_flag;
  std::vector<double> h_rc_st, h_rc_ct;
  // ---- the replan loop (dftpav_planner_install ... dftpav_replan_tick)
  // what the last dftpav_plan_queries call left behind for dftpav_planner_adopt: its size and paddings, per query the final
  // plan_status and winner, and the goals (read only while last_Q > 0: a call that fails leaves them half written)
  int last_Q = 0, last_MS = 0, last_MP = 0;
  std::vector<int> last_status, last_winner;
  std::vector<double> last_goal;
  // the executing table: one allocation of its own (the arena above is carved again when the paddings of a call change)
  unsigned char *d_exec = nullptr;
  ExecTable T{};
  std::vector<int> h_occupied;  // host mirror: n_seg of every slot
  std::vector<double> h_goal;   // host mirror: the stored goals [slots][4]
  // outputs of the check, its two tables and its inputs: one allocation
  unsigned char *d_rc = nullptr;
  int *d_rc_int = nullptr, *d_pairs = nullptr;
  double *d_rc_des = nullptr, *d_rc_st = nullptr, *d_rc_ct = nullptr, *d_rc_goal = nullptr, *d_rc_ego = nullptr, *d_rc_tab = nullptr;
  int rc_n_t = 0, rc_n_v = 0;
  double rc_dt = 0.0, rc_res = 0.0; // what d_rc_tab was tabulated for
  EventMarks<2> check_ev, tick_ev; // around the last check kernel / the last tick
  // ---- the publisher (dftpav_planner_publish): its state per slot lives in d_exec beside the table; clocks and outputs grow on demand
  PubTable P{};
  int *d_pub_mode = nullptr; // [slots] of d_rc: what an adoption does to the control history of each adopted pair
  unsigned char *d_pub = nullptr;
  size_t pub_ticks = 0; // d_pub holds the clocks and outputs of this many ticks
  double *d_pub_t = nullptr, *d_pub_states = nullptr;
  int *d_pub_code = nullptr;
  EventMarks<2> pub_ev; // around the last publish kernel
  // ---- the selection filters (dftpav_planner_set_limit_filter / _penalty_filter / _clearance_filter / _conflict_filter)
  LimitFilter lim;
  PenaltyFilter pen;
  ClearanceFilter clr;
  ConflictFilter cnf;
  JointSelect jnt; // dftpav_planner_set_joint_selection
  ConflictTrigger trg; // dftpav_planner_set_conflict_trigger
  std::vector<int> own_next; // dftpav_planner_set_own_slots: the own slots [Q] of the next dftpav_plan_queries call, which consumes them
};

namespace dftpav {
// ---- capi.cpp
int finish_pending(dftpav_batch *b);                          // finishes the stragglers a chained solve left suspended (no-op otherwise)
int solve_impl(dftpav_batch *b, dftpav_batch *prev, bool chained);
int sync_dev(dftpav_batch *b, DevBatch &D);                   // refreshes the device copy of the launch descriptor
hipError_t launch_for(dftpav_batch *b, const DevBatch &D, int mode);
int cost_terms_on_stream(dftpav_batch *b, const double *d_x); // the terms of the cost into b->d_terms; nothing waits
void fill_dev_layout(const dftpav_layout &layout, int K, int Kd, DevLayout &L);
void fill_dev_params(const dftpav_params &p, DevParams &P);
// ---- capi_steps.cpp
int search_setup(dftpav_handle *h, const dftpav_search_params *sp, int n, SearchSetup &U);
// the outputs of a search wired into U.S: the tables in d_tabs (in_tab | v_tab | l_tab), the queries, the eight int rows [n] of d_ints
// in the order of dftpav_search_out, and the node / path lists (null with a padding of 0)
void wire_search(SearchSetup &U, double *d_tabs, double *d_start, double *d_end, int *d_ints, size_t n, int max_nodes, double *d_nodes,
                 int max_path, double *d_paths);
// The two running sums of the collision re-check, tabulated into `tab`: 4096 sample times t += check_dt from 0.0
// (traj_server_ros.cpp:387), then the spacings of the outline points dl += vertex_res while dl < max(veh_length, veh_width) + 1.0
// (shapes.cc:128), one entry vertex_res if that leaves none.  max_spacings > 0: DFTPAV_E_UNSUPPORTED where that many or more are needed.
int validation_table(const dftpav_params &p, double check_dt, double vertex_res, int max_spacings, std::vector<double> &tab, int *n_t, int *n_v);
// rectangles of n_poses poses (device) from the handle's map into the batch's corridor, each `replicate` times.  Nothing waits for the
// device: the batch keeps the sixteen-double layout (dftpav_batch::cor_rect)
int corridor_into_batch(dftpav_batch *b, const double *d_poses, int n_poses, int replicate);
// coefficients and piece durations of the solutions, regenerated on the device from x (unless the test hook overrode them)
int ensure_coeffs(dftpav_batch *b, DevBatch &D);
// the collision re-check of the first n_traj trajectories against the handle's map; d_tab: a validation_table on the device
int validate_on_stream(dftpav_batch *b, int n_traj, const double *d_tab, int n_t, int n_v, double check_dt, int *d_col, int *d_first);
// dftpav_limits as the kernels of limits.hip read it; false: a limit that is not > 0 (a NaN included)
bool limits_common(const dftpav_params &p, const dftpav_limits &l, LimitsCommon &C);
// The part the batch and the table form of a check share.  check_limits_rows: C from limits_common; the sample times of check_dt
// are tabulated and uploaded, n rows max_abs | arg | violated | feasible allocated and wired into C, `launch` runs with the finished
// C between the marks of h->lim_ev, the rows are fetched into out, and the call waits.  check_clearance_rows likewise: the distance
// field is ensured, `launch` gets clearance_common with n rows min_d2 | arg | clearance, between the marks of h->clr_ev.
int check_limits_rows(dftpav_handle *h, double check_dt, size_t n, const dftpav_limits_out *out, LimitsCommon C,
                      const std::function<hipError_t(const LimitsCommon &)> &launch);
int check_clearance_rows(dftpav_handle *h, double check_dt, size_t n, const dftpav_clearance_out *out,
                         const std::function<hipError_t(const ClearanceCommon &)> &launch);
// copies of n rows to the host on the handle's stream, each unless the caller did not ask for it (nothing waits)
int fetch_limits(dftpav_handle *h, const dftpav_limits_out *out, const LimitsCommon &C, size_t n);
int fetch_clearance(dftpav_handle *h, const dftpav_clearance_out *out, const int *d_d2, const int *d_arg, const double *d_m, size_t n);
// the distance field of the handle's map, built on the handle's stream if the map changed since the last build (nothing waits);
// DFTPAV_E_INVALID without a map, DFTPAV_E_UNSUPPORTED for a side above 16384 cells
int ensure_dist_field(dftpav_handle *h);
// The boxes (four device arrays [n_boxes]; select [S_pad] on the device or null) stamped into the working map on the handle's stream,
// between marks 1 and 2 of h->stamp_ev: the base copy is made if the map has none, the distance field goes stale.  Nothing waits.
// The caller has checked the map and inflate.
int stamp_boxes_on_stream(dftpav_handle *h, const double *cx, const double *cy, const double *cs, const double *sn, int n_boxes,
                          const unsigned char *d_select, int S_pad, double inflate);
// the outline spacing of the clearance calls: the reference's own (shapes.h:200-201), which dftpav_batch_validate's callers pass as 0.1
constexpr double kClearanceVertexRes = 0.1;
// the map, its field, the vehicle and the tables (d_tab: a validation_table of kClearanceVertexRes on the device) as clearance.hip reads them
ClearanceCommon clearance_common(const dftpav_handle *h, const double *d_tab, int n_t, int n_v, double check_dt);
// The goal fields of n goals (xy: their x, y at a stride of `stride` doubles), blocked by inflate_radius, planned in turns of at most
// `slots` queries: the distance field is ensured, the workspace grown, field_of and the cells uploaded on the handle's stream.
// margin >= 0: windowed, every query's field limited to dftpav_goal_window of its start (start_xy, at the same stride) and goal;
// margin < 0: whole-map fields, and start_xy is not read.
int goal_field_plan(dftpav_handle *h, const double *start_xy, const double *xy, int stride, int n, int slots, double inflate_radius,
                    double margin, GoalFieldPlan &G);
// builds turn t's fields on the handle's stream (nothing waits) and returns their base; with S, wires them into a search launch
int goal_field_turn(dftpav_handle *h, const GoalFieldPlan &G, int t, SearchArgs *S, int **fields);
// search_setup's slots with the heuristic: a plan for the queries' goals when it is on (G.per_turn replaces U.slots), nothing otherwise
int search_heuristic_plan(dftpav_handle *h, const double *start_states, const double *end_states, int n, SearchSetup &U, GoalFieldPlan &G);
// The Reeds-Shepp table.  rs_geometry: the checked geometry of a parameter set (DFTPAV_E_INVALID / _UNSUPPORTED as the header
// says).  ensure_rs_table: the table of (rho, gp) on the device, built on the handle's stream if the handle holds another.
// search_rs_plan: with the heuristic on, the table of the launch's rho wired into U.S; off, nothing.
int rs_geometry(const dftpav_rs_heuristic_params &gp, RsGeometry &g, size_t &entries);
int ensure_rs_table(dftpav_handle *h, double rho, const dftpav_rs_heuristic_params &gp, RsGeometry &g);
int search_rs_plan(dftpav_handle *h, SearchSetup &U);
// ---- capi_conflicts.cpp (hidden: the split adds nothing to the library's dynamic symbols)
#define DFTPAV_HIDDEN __attribute__((visibility("hidden")))
// the K clocks t0 + k dt of a conflict call: 1 <= K <= DFTPAV_CONFLICT_MAX_SAMPLES, dt > 0 and finite, t0 finite
DFTPAV_HIDDEN bool conflict_clocks_ok(double t0, double dt, int K);
// the planner's slots rounded up to whole tiles of kConflictTile
DFTPAV_HIDDEN int conflict_s_pad(const dftpav_planner *p);
// the poses of every slot at the K clocks into d_pose (4 x [K][S_pad]) and d_occupied [S_pad], wired into P, on the handle's stream
// between marks 0 and 1 of `ev` (nullptr: no marks; nothing waits)
DFTPAV_HIDDEN int conflict_poses_into(dftpav_planner *p, double *d_pose, unsigned char *d_occupied, EventMarks<3> *ev, double t0, double dt,
                                      int K, ConflictPoses &P);

// One allocation for many arrays, measured and carved by the same list: fields(take) names every array in order, take(bytes) is its
// address -- null while `base` is null, the measuring pass -- and advances by the size rounded up to 256 bytes.  Returns the bytes used.
template <class F> size_t carve(unsigned char *base, F &&fields) {
  size_t used = 0;
  auto take = [&](size_t bytes) {
    void *r = base ? (void *)(base + used) : nullptr;
    used += (bytes + 255) / 256 * 256;
    return r;
  };
  fields(take);
  return used;
}

// A carved allocation `d` made, or made again for a larger `fields`: measured, allocated, and only then the old block freed, behind a
// wait for the handle's stream (nothing of it is in flight after that); carved, d set.  A refused allocation leaves d and its block
// alone -- a caller that must stay as it was lets `fields` write locals and copies them behind a success.
template <class F> int regrow(dftpav_handle *h, unsigned char *&d, F &&fields) {
  unsigned char *fresh = nullptr;
  HIPCHK(h, hipMalloc(&fresh, carve(nullptr, fields)));
  if (d) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(d);
  }
  carve(fresh, fields);
  d = fresh;
  return DFTPAV_OK;
}

// The temporary device buffers of one call.  They are freed when the call ends, after a wait for the handle's stream: whatever the
// call enqueued -- a copy into the caller's memory included -- has ended by then, on the error paths too.
struct DevScratch {
  dftpav_handle *h;
  std::vector<void *> ptrs;
  explicit DevScratch(dftpav_handle *h_) : h(h_) {}
  DevScratch(const DevScratch &) = delete;
  DevScratch &operator=(const DevScratch &) = delete;
  ~DevScratch() {
    if (ptrs.empty()) return;
    (void)hipStreamSynchronize(h->stream);
    for (void *p : ptrs) (void)hipFree(p);
  }
  hipError_t alloc_bytes(void **p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) ptrs.push_back(*p);
    else *p = nullptr;
    return e;
  }
  template <class T> hipError_t alloc(T *&p, size_t n) {
    void *v = nullptr;
    const hipError_t e = alloc_bytes(&v, sizeof(T) * n);
    p = (T *)v;
    return e;
  }
  void keep() { ptrs.clear(); } // the buffers now belong to the caller
};

// a copy to the host on the handle's stream, unless the caller did not ask for that output
inline hipError_t fetch_async(dftpav_handle *h, void *dst, const void *src, size_t bytes) {
  return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}

// a work buffer that lives from call to call: reallocated only when it is too small (contents are not kept)
template <class T> int grow(dftpav_handle *h, T *&p, size_t &have, size_t want) {
  if (have >= want && p) return DFTPAV_OK;
  if (p) HIPCHK(h, hipFree(p));
  p = nullptr;
  HIPCHK(h, hipMalloc(&p, sizeof(T) * want));
  have = want;
  return DFTPAV_OK;
}
} // namespace dftpav
