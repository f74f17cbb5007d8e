/*
 * dftpav_hip.h — C-ABI of the MI355X-native batched MINCO / L-BFGS trajectory solver.
 *
 * This is the drop-in boundary for Dftpav's traj_planner solve path.  The
 * reference has no FFI layer: the boundary there is the C++ class
 * PolyTrajOptimizer (traj_planner/include/plan_manage/traj_optimizer.h:100-120)
 * plus the L-BFGS callback typedef (include/geo_utils2d/lbfgs.hpp:200-202).
 * Every entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C PODs, caller-allocated buffers, no exceptions, no logging.
 *   - all reals are IEEE fp64 (the reference computes in double throughout,
 *     common/basics/basics.h:29 `decimal_t = double`).
 *   - 2x3 boundary states are column-major [px,py, vx,vy, ax,ay]
 *     (Eigen::MatrixXd(2,3) default storage, traj_optimizer.cpp:8).
 *   - return value: DFTPAV_OK (0) or a negative DFTPAV_E_* code.  Per-trajectory
 *     solver status uses the reference's lbfgs enum values (lbfgs.hpp:135-184).
 *   - one handle = one HIP stream + its device buffers; single owner thread
 *     (PolyTrajOptimizer is not re-entrant either, traj_optimizer.h:80-92).
 */
#ifndef DFTPAV_HIP_H
#define DFTPAV_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library return codes ------------------------------------------------ */
#define DFTPAV_OK 0
#define DFTPAV_E_INVALID (-1)     /* bad argument / size mismatch (traj_optimizer.cpp:26-48) */
#define DFTPAV_E_MINI_T (-2)      /* initTs.min < mini_T          (traj_optimizer.cpp:30-33) */
#define DFTPAV_E_ONE_PIECE (-3)   /* a segment with <2 pieces     (traj_optimizer.cpp:38-41) */
#define DFTPAV_E_NO_DEVICE (-4)   /* no HIP device / kernel image not loadable: never falls back to CPU */
#define DFTPAV_E_HIP (-5)         /* a HIP runtime call failed (see dftpav_last_error) */
#define DFTPAV_E_UNSUPPORTED (-6) /* layout exceeds a compiled limit */
#define DFTPAV_E_COMM (-7)        /* RCCL is not loadable, or one of its calls failed (see dftpav_last_error) */

/* ---- per-trajectory solver status: values of lbfgs.hpp:135-184 ----------- */
enum {
  DFTPAV_LBFGS_CONVERGENCE = 0,
  DFTPAV_LBFGS_STOP = 1,
  DFTPAV_LBFGS_CANCELED = 2,
  DFTPAV_LBFGSERR_UNKNOWNERROR = -1024,
  DFTPAV_LBFGSERR_INVALID_N = -1023,
  DFTPAV_LBFGSERR_INVALID_MEMSIZE = -1022,
  DFTPAV_LBFGSERR_INVALID_GEPSILON = -1021,
  DFTPAV_LBFGSERR_INVALID_TESTPERIOD = -1020,
  DFTPAV_LBFGSERR_INVALID_DELTA = -1019,
  DFTPAV_LBFGSERR_INVALID_MINSTEP = -1018,
  DFTPAV_LBFGSERR_INVALID_MAXSTEP = -1017,
  DFTPAV_LBFGSERR_INVALID_FDECCOEFF = -1016,
  DFTPAV_LBFGSERR_INVALID_SCURVCOEFF = -1015,
  DFTPAV_LBFGSERR_INVALID_MACHINEPREC = -1014,
  DFTPAV_LBFGSERR_INVALID_MAXLINESEARCH = -1013,
  DFTPAV_LBFGSERR_INVALID_FUNCVAL = -1012,
  DFTPAV_LBFGSERR_MINIMUMSTEP = -1011,
  DFTPAV_LBFGSERR_MAXIMUMSTEP = -1010,
  DFTPAV_LBFGSERR_MAXIMUMLINESEARCH = -1009,
  DFTPAV_LBFGSERR_MAXIMUMITERATION = -1008,
  DFTPAV_LBFGSERR_WIDTHTOOSMALL = -1007,
  DFTPAV_LBFGSERR_INVALIDPARAMETERS = -1006,
  DFTPAV_LBFGSERR_INCREASEGRADIENT = -1005
};

/* ---- constants of the optimiser ------------------------------------------
 * Replaces PolyTrajOptimizer::setParam (traj_optimizer.cpp:1713-1781), the
 * protobuf OptCfg (proto/minco_config.proto:67-99, values
 * config/minco_config.pb.txt:65-100), common::VehicleParam defaults
 * (common/basics/semantics.h:66-76) and the constants hard-coded in
 * traj_optimizer.h:68 / traj_optimizer.cpp:127-134,197. */
typedef struct dftpav_params {
  int traj_resolution;      /* K   : samples-1 on interior pieces        (pb.txt:66) */
  int des_traj_resolution;  /* K_d : samples-1 on first/last piece       (pb.txt:67) */
  double wei_obs;           /* wei_sta_obs  1000                         (pb.txt:68) */
  double wei_surround;      /* wei_dyn_obs  5000                         (pb.txt:69) */
  double wei_feas;          /* 2500                                      (pb.txt:70) */
  double wei_sqrvar;        /* read, unused by the live path             (pb.txt:71) */
  double wei_time;          /* 500                                       (pb.txt:72) */
  double surround_clearance;/* dyn_obs_clearance 0.4                     (pb.txt:73) */
  double half_margin;       /* 0.15 footprint inflation                  (pb.txt:74) */
  double max_forward_vel, max_forward_acc, max_forward_cur;   /* 5 8 1 (pb.txt:83-85) */
  double max_backward_vel, max_backward_acc, max_backward_cur;/* 2 4 1 (pb.txt:87-89) */
  double max_latacc;        /* computed, penalty disabled in the reference (traj_optimizer.cpp:666-678) */
  double max_phidot;        /* idem                                        (traj_optimizer.cpp:707-773) */
  int gear_opt;             /* GearOpt true                              (pb.txt:95) */
  double non_sinv;          /* 0.24, hard-coded traj_optimizer.h:68 */
  double mini_T;            /* 0.1                                       (pb.txt:99) */
  double fail_cost;         /* 50000, traj_optimizer.cpp:197 */
  /* raw vehicle (semantics.h:66-76); inflated by 2*half_margin inside, as setParam does */
  double veh_width, veh_length, veh_wheel_base, veh_d_cr;
  /* L-BFGS (lbfgs.hpp:15-129 defaults overridden at traj_optimizer.cpp:127-134) */
  int lbfgs_mem_size;       /* 256 (pb.txt:96) */
  int lbfgs_past;           /* 3   (pb.txt:97) */
  double lbfgs_delta;       /* 1e-4 (pb.txt:98) */
  double lbfgs_g_epsilon;   /* 1e-16 */
  int lbfgs_max_iterations; /* 12000 */
  int lbfgs_max_linesearch; /* 64 */
  double lbfgs_min_step;    /* 1e-32 */
  double lbfgs_max_step;    /* 1e20 */
  double lbfgs_f_dec_coeff; /* 1e-4 */
  double lbfgs_s_curv_coeff;/* 0.9 */
  double lbfgs_cautious_factor; /* 1e-6 */
  double lbfgs_machine_prec;    /* 1e-16 */
} dftpav_params;

/* Fills the live values of the reference (files cited on each field above). */
void dftpav_default_params(dftpav_params *p);

/* ---- moving obstacles ----------------------------------------------------
 * Replaces PolyTrajOptimizer::setSurroundTrajs(SurroundTrajData*)
 * (traj_optimizer.h:108, traj_optimizer.cpp:1916) and the fields of
 * plan_utils::LocalTrajData the hot path reads (traj_container.hpp:28-38):
 * traj (pieces), duration, start_time.  A piece is {duration, 2x6 coeffMat}
 * with column 0 multiplying t^5 (poly_traj_utils.hpp:77-87,993); coeffs are
 * stored column-major per piece: [x5,y5, x4,y4, ... x0,y0]. All obstacles of
 * one set share `n_pieces` rows in the flattened arrays via piece_offsets. */
typedef struct dftpav_surround {
  int S;                       /* number of moving obstacles (0 = none) */
  const int *piece_offsets;    /* [S+1] prefix offsets into durations/coeffs */
  const double *durations;     /* [piece_offsets[S]] */
  const double *coeffs;        /* [piece_offsets[S]][12] */
  const double *total_duration;/* [S]  LocalTrajData::duration */
  const double *start_time;    /* [S]  LocalTrajData::start_time */
} dftpav_surround;

/* ---- structure shared by every trajectory of a batch ----------------------
 * M gear segments (`trajnum`), N_i pieces each, singul_i = +1 forward / -1
 * reverse (traj_optimizer.cpp:13-23).  n = 2*sum(N_i-1) + M + 3*(M-1)
 * decision variables laid out [P_0..P_{M-1} | tau | gear xy | gear angle]
 * (traj_optimizer.cpp:80-115). */
typedef struct dftpav_layout {
  int M;
  const int *piece_nums; /* [M] */
  const int *singuls;    /* [M] */
  int H;                 /* half-planes per constraint point (4 on the live path, traj_manager.cpp:1225) */
} dftpav_layout;

/* ---- inputs of OptimizeTrajectory for B trajectories ----------------------
 * Replaces the argument list of PolyTrajOptimizer::OptimizeTrajectory
 * (traj_optimizer.h:118-120).  Every array is trajectory-major. */
typedef struct dftpav_batch_data {
  const double *ini_states; /* [B][M][6]  iniStates   */
  const double *fin_states; /* [B][M][6]  finStates   */
  const double *inner_pts;  /* [B][2*sum(N_i-1)] initInnerPts, segment after segment, (x,y) per waypoint */
  const double *init_Ts;    /* [B][M]     initTs (segment totals, each >= mini_T) */
  const double *corridor;   /* [B][Npts][H][4] hPoly columns (n_x,n_y,p_x,p_y), outward normal,
                               NOT necessarily unit (normalised inside, traj_optimizer.cpp:49-52);
                               Npts = sum_i (N_i-2)(K+1)+2(K_d+1) in sampling order */
  double t_now;             /* `now`  (traj_optimizer.h:120) */
  double help_eps;          /* `help_eps` -> epis (live value 0.0, traj_manager.cpp:610) */
} dftpav_batch_data;

typedef struct dftpav_handle dftpav_handle;
typedef struct dftpav_batch dftpav_batch;

/* number of decision variables / constraint points of a layout */
int dftpav_num_vars(const dftpav_layout *l);
int dftpav_num_points(const dftpav_params *p, const dftpav_layout *l);

/* Replaces PolyTrajOptimizer construction + setParam (traj_optimizer.h:100).
 * device: HIP ordinal.  Fails with DFTPAV_E_NO_DEVICE when no gfx950 device
 * is usable — there is no CPU fallback in this library. */
int dftpav_create(const dftpav_params *params, int device, dftpav_handle **out);
void dftpav_destroy(dftpav_handle *h);
const char *dftpav_last_error(const dftpav_handle *h);

/* Replaces setSurroundTrajs (traj_optimizer.h:108). s==NULL or s->S==0 clears
 * it (surround_trajs_ == NULL, traj_optimizer.cpp:636). Data is copied.
 * Limits (the reference loops over surround_trajs_->size() without one): at most DFTPAV_MAX_SURROUND obstacles with
 * DFTPAV_MAX_SURROUND_PIECES pieces in all -- a larger set is refused here and by dftpav_set_surround_wire
 * (DFTPAV_E_UNSUPPORTED, the installed set is kept); and (constraint points of the layout) x S <= 65535, which only a
 * solve / eval / validation of a batch can check (DFTPAV_E_UNSUPPORTED there).  dftpav_fit_surround fits and installs
 * a set of any size (its result can be read back with dftpav_get_surround); beyond the limits above the solver refuses
 * it in the same way. */
#define DFTPAV_MAX_SURROUND 16
#define DFTPAV_MAX_SURROUND_PIECES 512
int dftpav_set_surround(dftpav_handle *h, const dftpav_surround *s);

/* ---- front-end resampling: from a searched path to the solver's arguments ----
 * Replaces KinoAstar::getKinoNode from SampleTraj on (kino_astar.cpp:606-743:
 * gear segmentation, trapezoid time allocation, flat boundary states) and the
 * resampling of TrajPlanner::RunMINCOParking (traj_manager.cpp:531-568, through
 * KinoAstar::evaluatePos, kino_astar.cpp:468-521) for n_hyp hypotheses. */
typedef struct dftpav_frontend_params {
  double max_forward_vel, max_forward_acc;   /* 5.0, 8.0  (minco_config.pb.txt:77-78) */
  double max_backward_vel, max_backward_acc; /* 2.0, 4.0  (pb.txt:79-80) */
  double non_siguav;                         /* 0.2       (kino_astar.h:207) */
  double wheel_base;                         /* 2.85      (semantics.h:68) */
  double piece_duration;                     /* 1.0       (pb.txt:76 traj_piece_duration) */
  int traj_res, dense_traj_res;              /* samples per piece: inner pieces / first and last piece (pb.txt:66-67) */
} dftpav_frontend_params;
/* Caller-allocated outputs, padded: per hypothesis up to max_seg gear segments,
 * per segment up to max_pieces pieces and max_states constraint-point poses. */
typedef struct dftpav_frontend_out {
  int max_seg, max_pieces, max_states;
  int *n_seg;         /* [n_hyp]  segments found (may exceed max_seg: then only the first max_seg are written) */
  int *singul;        /* [n_hyp][max_seg]  +1 forward / -1 reverse */
  int *piece_nums;    /* [n_hyp][max_seg] */
  double *piece_dt;   /* [n_hyp][max_seg]  timePerPiece; initTs = piece_dt * piece_nums */
  double *ini_states; /* [n_hyp][max_seg][6]  col-major 2x3 flat state (p, v, a) */
  double *fin_states; /* [n_hyp][max_seg][6] */
  double *inner_pts;  /* [n_hyp][max_seg][max_pieces-1][2] */
  int *n_states;      /* [n_hyp][max_seg]  poses produced (may exceed max_states: then only the first are written) */
  double *states;     /* [n_hyp][max_seg][max_states][3]  statelist of getRectangleConst: (x, y, yaw) */
} dftpav_frontend_out;
/* paths: [n_hyp][max_path][3] poses (x, y, yaw in (-pi, pi]) of which path_len[h] >= 2 are used;
 * start_states / end_states: [n_hyp][4] (x, y, yaw, v); start_ctrl: [n_hyp][2] (steer, acceleration). */
int dftpav_frontend_resample(dftpav_handle *h, const dftpav_frontend_params *fp, const double *paths, const int *path_len,
                             int max_path, const double *start_states, const double *end_states, const double *start_ctrl,
                             int n_hyp, const dftpav_frontend_out *out);

/* ---- seeded restart sampler: the batch axis (SURVEY.md §8(d) "Restarts", §8(f)-3) ----
 * No reference counterpart (the reference plans one trajectory per cycle).  Every
 * hypothesis h (inner waypoints [n_inner] = x0, y0, x1, y1, ...; M segment
 * durations) yields n_restarts trajectories, b = h * n_restarts + r: r == 0 is the
 * hypothesis itself, r > 0 has its waypoints moved by N(0, sigma^2) per coordinate
 * and every duration scaled by U[dur_lo, dur_hi].  The generator (SplitMix64
 * streams keyed by (seed, h, r), Box-Muller) is defined in
 * dftpav_amd/csrc/restart.hip; the same (seed, h, r) gives the same bits anywhere. */
int dftpav_sample_restarts(dftpav_handle *h, const double *inner_pts, const double *durations, int n_hyp, int n_restarts,
                           int n_inner, int M, double sigma, double dur_lo, double dur_hi, unsigned long long seed,
                           double *out_inner_pts, double *out_durations);

/* ---- moving-obstacle trajectory fitting ----
 * Replaces TrajPlanner::ConverSurroundTrajFromPoints (traj_manager.cpp:743-789,
 * with state_to_flat_output :139-158) followed by setSurroundTrajs: S predicted
 * state sequences, states [S][n_states][7] = (x, y, angle, velocity,
 * acceleration, curvature, time_stamp) per state, are each fitted on the device
 * with a uniform-time minimum-jerk trajectory of n_states - 1 pieces and
 * installed as the handle's moving obstacles (S == 0 clears them). */
int dftpav_fit_surround(dftpav_handle *h, const double *states, int S, int n_states);
/* Reads back the installed moving obstacles in the layout of dftpav_surround
 * (any pointer may be NULL; call once with the arrays NULL to get S and the
 * total number of pieces). */
int dftpav_get_surround(dftpav_handle *h, int *S, int *n_pieces, int *piece_offsets, double *durations, double *coeffs,
                        double *total_duration, double *start_time);

/* ---- safe-corridor generation, the step before the solve ----
 * Replaces map_itf_->GetObstacleMap + the map queries of getRectangleConst
 * (traj_manager.cpp:1216-1217, map_adapter.cpp:93-97, semantics.h:351-358):
 * a GridMapND<uint8_t, 2>, cell (ix, iy) at cells[ix + size_x * iy], centred at
 * origin + (ix, iy) * resolution, 80 = OCCUPIED.  The cells are copied. */
typedef struct dftpav_grid_map {
  const unsigned char *cells;
  int size_x, size_y;
  double resolution;
  double origin_x, origin_y;
} dftpav_grid_map;
int dftpav_set_grid_map(dftpav_handle *h, const dftpav_grid_map *map);

/* Replaces TrajPlanner::getRectangleConst (traj_manager.cpp:1213-1469): one
 * vehicle-aligned rectangle per state (x, y, yaw), grown cell by cell on the
 * map of dftpav_set_grid_map with the raw vehicle size of dftpav_params.
 * hpoly: [n_states][4][4], per state the four columns (n_x, n_y, p_x, p_y) of
 * hPoly (traj_manager.cpp:1442-1465) — the layout dftpav_batch_data.corridor
 * takes for H = 4. */
int dftpav_corridor_rectangles(dftpav_handle *h, const double *states, int n_states, double *hpoly);
/* Duration of the last corridor kernel on the device (HIP events), without the copies. */
int dftpav_corridor_last_ms(dftpav_handle *h, float *ms);

/* Device-resident batch of B trajectories with a common layout.  The launch shape (threads per trajectory, workgroups per
 * CU, what is staged in LDS) is chosen here, for layouts with many constraint points with the obstacle set that is
 * installed on the handle at this moment (dftpav_set_surround / dftpav_fit_surround before dftpav_batch_create); a set
 * installed later still works, with the shape chosen without it. */
int dftpav_batch_create(dftpav_handle *h, const dftpav_layout *layout, int B, dftpav_batch **out);
/* The same with the residency plan chosen by the caller instead of by B: 0 = one workgroup per CU, the trajectory's
 * half-planes and the MINCO operators staged in LDS (lowest latency of one solve; the default for B <= #CUs), 1 = two per
 * CU, 2 = four per CU (highest throughput; the default for large B), -1 = by B.  For callers that keep several small
 * batches in flight on several handles (a PolyTrajOptimizer per planner thread, traj_optimizer.h:80-92). */
int dftpav_batch_create_shaped(dftpav_handle *h, const dftpav_layout *layout, int B, int residency, dftpav_batch **out);
void dftpav_batch_destroy(dftpav_batch *b);

/* The setup half of OptimizeTrajectory (traj_optimizer.cpp:26-115): validates,
 * normalises corridor normals, clamps boundary |v|,|a|, packs x0, uploads to
 * HBM.  After this call the batch is resident; solve/eval touch no host data. */
int dftpav_batch_upload(dftpav_batch *b, const dftpav_batch_data *d);

/* The floating-point order of the solve path for this batch (eval, solve, coeffs; default DFTPAV_ORDER_DEVICE).
 *
 * DFTPAV_ORDER_DEVICE: the throughput kernels.  They reassociate three sums of the reference -- the per-piece sums of the
 *   penalty gradient, the MINCO solves (a dense operator for the banded substitution) and the dot products of L-BFGS --
 *   so a single evaluation equals the reference's to rounding (<= 1e-11) and, the solver being chaotic, a whole solve
 *   equals it statistically.
 * DFTPAV_ORDER_REFERENCE: every sum in the order PolyTrajOptimizer executes it (traj_optimizer.cpp:486-705 sample ->
 *   vertex -> plane accumulation, poly_traj_utils.hpp:805-852 banded substitutions, lbfgs.hpp:716-739 two-loop with
 *   sequential dot products), no fused multiply-adds: the mode of a drop-in that must reproduce the CPU planner's
 *   decision exactly, and the parity proof of the other one.  THE CONTRACT, precisely: final x, cost, status, iterations
 *   and evaluations are bit-equal to those of the reference's PROGRAM evaluated with sequential reductions (dot products,
 *   norms and matrix products as one chain from their first term), no FMA contraction and -- where the program calls libm --
 *   correctly rounded calls.  That program is what the CPU restatement executes (oracle/dftpav_oracle.c, orders 0 / 2: test
 *   infrastructure).  The reference itself cannot be built in this project's image (it needs Eigen, ROS and protobuf-generated
 *   code) and holds no golden vectors: PARITY IS UNPINNED against an upstream binary.  Such a binary, built against a real
 *   Eigen, vectorises reductions into 2- or 4-lane partial sums and WILL differ in last bits -- as two such builds differ from
 *   each other -- and this solver turns a last-bit difference into a different, statistically equal answer.
 *     - one gear segment, no moving obstacles: the reference's program has no libm call inside the loop; this mode
 *       returns the bits of the restatement's order 0;
 *     - gear shifts: the reference calls libm's cos / sin of every junction angle per evaluation
 *       (traj_optimizer.cpp:273-282, 311-318), whose bits depend on the host (glibc's are not correctly rounded and are
 *       IFUNC-dispatched by CPU model): this mode uses the CORRECTLY ROUNDED cos / sin (cr_trig.h); it equals the
 *       result of the same program over a host libm whenever that libm rounded every junction angle's cos / sin correctly;
 *     - moving obstacles: libm's exp (40 times) and log (9 times) per (constraint point, obstacle) pair and pow(|v|, 3)
 *       (traj_optimizer.cpp:1686-1707, poly_traj_utils.hpp:109) are likewise the correctly rounded exp / log / x^3;
 *     - gear shifts TOGETHER WITH moving obstacles -- the reference's live call, traj_manager.cpp:604-610 -- are covered,
 *       including trajtimes[i] = duration of segment i - 1 (traj_optimizer.cpp:230-234) and the extra gdT addends per
 *       previous segment (:1674-1676);
 *     - with libm calls in the loop the yardstick is the restatement's order 2 (the same statements with exp / log / pow / sin /
 *       cos from binary128): whole solves of this mode are bit-equal to it on all of the three cases above;
 *     - limits: n <= 256 variables, H <= 12 half-planes, 5 H + S + 4 <= 64 terms per constraint point, every gear segment
 *       >= 2 pieces, 159 KB of LDS for one trajectory's state; otherwise DFTPAV_E_UNSUPPORTED, order unchanged.  (n > 64 or H > 5 --
 *       a plan of more than 32 pieces, corridors that are not rectangles -- run in a slow generic kernel: the plain L-BFGS step
 *       over vectors in LDS, twelve plane slots per point.)  Choose the order again after the number of
 *       obstacles on the handle changed.  dftpav_batch_trace* is a device-order facility (DFTPAV_E_UNSUPPORTED here).
 *     - one step of the path is bit-equal by MEASUREMENT, not by proof: a division by a stored quantity (the diagonals of the
 *       band factorisation, y.s of a stored pair) is a multiplication by its reciprocal with one residual correction, which
 *       is the correctly rounded quotient whenever the first product is a faithful rounding of it (Markstein); no
 *       counter-example in 2^31 random pairs nor in any solve compared with the restatement, none ruled out.  The
 *       environment variable DFTPAV_REF_EXACT_DIV=1 makes the recursion divide (slower; the bits have never differed).
 *   Launch shape by batch size (or by the residency hint of dftpav_batch_create_shaped: 2 = many batches in flight): up to five
 *   trajectories per CU one workgroup each (lowest latency); beyond, one gear segment of <= 16 pieces and n <= 32 without moving
 *   obstacles -- BASELINE configs[2] / [3] -- takes the QUAD shape (solver_ref4.hip): FOUR trajectories per wave, one per row of
 *   16 lanes, a piece per lane, 16 trajectories per CU, the rows popping trajectories from the batch's ring (35-38 k solves/s on a
 *   stream of 4096-batches on MI355X); up to four gear segments of <= 16 pieces in all and n <= 48 without moving obstacles -- BASELINE
 *   configs[1], the reference's live layouts -- the same shape with the segments' pieces side by side on a row (solver_ref4m.hip;
 *   22-25 k solves/s on such a stream); everything else one WAVE per trajectory, eight per CU (solver_ref.hip).  A batch that has
 *   the device to itself (the default; dftpav_batch_set_hand_over(b, 0) announces others behind it) takes every wave slot and
 *   hands its last trajectories to the WAVE shape.  Every shape returns the same bits.
 *   The launch plan is chosen here, once, and every later launch of the batch follows it.  The developer options of this mode
 *   (DFTPAV_REF_SHAPE, _WAVES, _THREADS, _QUAD_WAVES, _QUAD_HANDOVER, _SLICE, _SLOTS, _EXACT_DIV and DFTPAV_VERBOSE) are read
 *   then: a change of them applies from the next call that chooses the reference order (a call that finds the batch in it, with
 *   the same number of obstacles, changes nothing).  On an error the batch keeps its order and plan as they were. */
#define DFTPAV_ORDER_DEVICE 0
#define DFTPAV_ORDER_REFERENCE 1
int dftpav_batch_set_order(dftpav_batch *b, int order);
int dftpav_batch_get_order(const dftpav_batch *b);

/* Decision vectors x0 packed by upload ([B][n], host copy). */
/* RunMINCOParking's pair getRectangleConst(statelist) -> OptimizeTrajectory(..., hPoly_container, ...)
 * (traj_manager.cpp:569-610) without the rectangles leaving the device: the
 * corridor of every trajectory of the batch is generated from its constraint-
 * point poses, states [B][Npts][3] (x, y, yaw), straight into the solver's own
 * layout.  Use with dftpav_batch_upload(d) where d->corridor == NULL.  H must be 4.
 * ORDER: dftpav_batch_upload first, then this call, then solve / eval.  Every upload with d->corridor == NULL
 * invalidates the half-planes of the previous cycle on purpose (they belong to the previous poses): a solve that
 * follows an upload without a new corridor returns DFTPAV_E_INVALID rather than using stale half-planes. */
int dftpav_batch_corridor_from_states(dftpav_batch *b, const double *states);
/* The same when the batch is n_restarts restarts of each hypothesis (trajectory
 * t = hypothesis * n_restarts + restart, as dftpav_sample_restarts lays them out)
 * and the restarts share their hypothesis' corridor, as the path they were
 * sampled from does: states [B / n_restarts][Npts][3]. */
int dftpav_batch_corridor_from_hypotheses(dftpav_batch *b, const double *states, int n_restarts);

int dftpav_batch_get_x0(dftpav_batch *b, double *x0);

/* L1 cut (unit-test boundary) == PolyTrajOptimizer::costFunctionCallback
 * (traj_optimizer.cpp:206-350, type lbfgs.hpp:200-202) for B decision
 * vectors at once: x [B][n] -> f [B], g [B][n].  Host buffers. */
int dftpav_batch_eval(dftpav_batch *b, const double *x, double *f, double *g);

/* The cost of dftpav_batch_eval term by term.  The reference forms it as a sum of five (traj_optimizer.cpp:292-297 per gear
 * segment: the jerk energy, and costs(0) corridor, costs(1) moving obstacles, costs(2) feasibility -- velocity, longitudinal
 * acceleration, curvature; :328-344 the time term and the total) and prints the per-segment jerk cost after a solve
 * (traj_manager.cpp:623); the terms are the operands of those very sums, taken from the evaluation kernel's own per-segment
 * records (solver_ref.hip) -- no second penalty integral:
 *   seg_terms [B][M][5]  per gear segment: jerk energy, T * wei_time, costs(0), costs(1), costs(2)
 *   terms     [B][5]     each column chained over the segments in order from 0.0
 * so that  f == terms[SMOOTH] + terms[TIME] + sum over segments in order of ((costs(0) + costs(1)) + costs(2))  in the bits of
 * dftpav_batch_eval.  x [B][n], or NULL: the solution of the last solve (DFTPAV_E_INVALID if there is none).  Either output may be
 * NULL.  DFTPAV_ORDER_REFERENCE only: DFTPAV_E_UNSUPPORTED in the device order, whose sums do not keep the penalty classes apart.
 * Refuses what dftpav_batch_eval refuses; a refused call changes nothing.  Every launch shape of the order is served by the
 * TEAM / WAVE kernel, as dftpav_batch_coeffs is; the results of a solve are not touched. */
#define DFTPAV_TERM_SMOOTH 0
#define DFTPAV_TERM_TIME 1
#define DFTPAV_TERM_CORRIDOR 2
#define DFTPAV_TERM_SURROUND 3
#define DFTPAV_TERM_FEAS 4
#define DFTPAV_COST_TERMS 5
int dftpav_batch_cost_terms(dftpav_batch *b, const double *x, double *terms, double *seg_terms);

/* Observation of one trajectory's solve, the role of lbfgs_progress_t
 * (lbfgs.hpp:242-249; the reference passes NULL, traj_optimizer.cpp:164) at
 * the granularity of the evaluation callback (lbfgs.hpp:200-202): during the
 * following solves every cost/gradient evaluation of trajectory `traj` is
 * recorded, up to max_evals of them (0 switches it off).  dftpav_batch_get_trace
 * returns n_evals rows of 3 n + 4 doubles: the evaluated x [n], its gradient
 * g [n], the search direction d [n] in force, then f, the trial step stp, the
 * iteration k and the evaluation's number within its line search (row 0 is the
 * evaluation of x0: d, stp and the count are 0).  Used by the lockstep parity
 * test against the reference's line search and two-loop recursion. */
int dftpav_batch_trace(dftpav_batch *b, int traj, int max_evals);
int dftpav_batch_get_trace(dftpav_batch *b, double *rows, int *n_evals);
/* The same for `count` consecutive trajectories from `first` at once (one block of records each), and the read-out of one
 * of them.  Device-order solves only (a reference-order solve needs no such check: it is the reference's sequence). */
int dftpav_batch_trace_range(dftpav_batch *b, int first, int count, int max_evals);
int dftpav_batch_get_trace_of(dftpav_batch *b, int traj, double *rows, int *n_evals);

/* L2 cut (production) == lbfgs::lbfgs_optimize driven from
 * OptimizeTrajectory (traj_optimizer.cpp:159-166, lbfgs.hpp:440-751): one
 * persistent kernel launch runs every trajectory's whole L-BFGS solve on the
 * device, starting from the resident x0.  Asynchronous on the handle's stream. */
int dftpav_batch_solve_async(dftpav_batch *b);
int dftpav_batch_sync(dftpav_batch *b);

/* Results (any pointer may be NULL):
 *   x          [B][n]  final decision vectors (x after lbfgs_optimize returns)
 *   final_cost [B]     `final_cost` (traj_optimizer.cpp:160)
 *   status     [B]     lbfgs_optimize return code (enum above)
 *   success    [B]     flag_success of OptimizeTrajectory (traj_optimizer.cpp:176-201)
 *   iters      [B]     L-BFGS iterations k
 *   evals      [B]     cost/gradient evaluations (iter_num_, traj_optimizer.cpp:334)
 *   hist_sum   [B]     sum over iterations of the history depth used by the
 *                      two-loop recursion (input of the bytes model)
 *   latency_us [B]     in-kernel wall time of each trajectory's solve (100 MHz
 *                      constant counter; OPT.cpp:157-169 computes the same and drops it) */
int dftpav_batch_results(dftpav_batch *b, double *x, double *final_cost, int *status,
                         int *success, int *iters, int *evals, long long *hist_sum,
                         double *latency_us);

/* Chained solves: throughput mode for a stream of equally shaped batches (restarts of successive planning
 * cycles).  The iteration counts of a batch are heavy-tailed: when its queue launch is down to the last
 * trajectories, a plain solve finishes them on a nearly empty device.  dftpav_batch_solve_chained(b, prev) starts
 * b like dftpav_batch_solve_async but (1) leaves b's own last trajectories suspended and (2) takes over the ones
 * `prev` left suspended, so that they are worked off inside b's full-occupancy phase.  Results are bit-identical
 * to a plain solve.  `prev` is complete when this call's work is (stream order); b is complete after the next
 * chained solve that names it as `prev`, or after dftpav_batch_finish(b) -- which dftpav_batch_sync / _results /
 * _pack_results / _coeffs / _validate / _sample_states call by themselves.  b and prev must be different batches
 * of the same handle with the same layout, size, parameters and plan; otherwise (or with prev == NULL, or for
 * batches too small to be scheduled) the call degrades to finishing prev and solving b unchained.  New inputs
 * for a batch (dftpav_batch_upload, dftpav_batch_corridor_from_*) discard what it still had suspended. */
int dftpav_batch_solve_chained(dftpav_batch *b, dftpav_batch *prev);
int dftpav_batch_finish(dftpav_batch *b);

/* Timing across solves and handles: dftpav_mark records one of a handle's two marker events on its stream,
 * dftpav_marks_elapsed_ms returns the device time between a marker of one handle and a marker of another (same
 * device) after waiting for the second -- the HIP-event clock bench.py puts around its timed region. */
int dftpav_mark(dftpav_handle *h, int slot);
int dftpav_marks_elapsed_ms(dftpav_handle *from, int from_slot, dftpav_handle *to, int to_slot, float *ms);

/* The end game of a scheduled solve: once no more than `hand_over` trajectories of the batch are unfinished they
 * leave the queue launch and finish in the latency shape (default: one per CU; negative restores it).  0 keeps every
 * trajectory in the queue launch to its end -- the setting for a stream of batches solved alternately on TWO handles
 * (two HIP streams): the queue launch of the next batch then fills the workgroup slots the previous one frees while
 * it thins out, which keeps the device full without any hand-over (bench.py's default). */
int dftpav_batch_set_hand_over(dftpav_batch *b, int hand_over);

/* Multi-GPU hand-off: one 16-byte record {f64 final_cost, i32 status, i32 iters} per trajectory — what the single
 * all-gather of SURVEY §8(e) carries.  The solve kernels write a trajectory's record in their epilogue, the moment it
 * finishes; there is no packing kernel between the solve and the collective (it used to wait up to 110 ms for a workgroup
 * slot behind the other stream's persistent workgroups).
 *   dftpav_batch_pack_results: copies the records into caller-owned DEVICE memory, asynchronously on the handle's stream.
 *   dftpav_batch_records:      waits for the solve and hands them over in HOST memory [B][16]: the epilogues write every record a
 *                              second time into pinned host memory of the batch, so nothing runs on the device behind the solve (the
 *                              runtime's device-to-host copy is a blit kernel that queues behind other streams' persistent waves). */
int dftpav_batch_pack_results(dftpav_batch *b, void *device_dst);
int dftpav_batch_records(dftpav_batch *b, void *host_dst);

/* The collective itself behind the C-ABI, for a C++ host (the reference's caller is one: TrajPlanner::RunMINCOParking,
 * traj_manager.cpp:608-610) that shards its restarts / hypotheses over the GPUs of a node, one process (or thread) and one
 * dftpav_handle per GPU: ONE RCCL all-gather of the 16-byte records over xGMI, enqueued on the handle's stream.
 *   dftpav_comm_available   1 where RCCL is loadable (dlopen only; every rank may ask), else 0
 *   dftpav_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId) and hands the bytes to the other ranks by whatever
 *                           channel the host has (MPI, a socket, torch.distributed ...)
 *   dftpav_comm_create      every rank, collectively: ncclCommInitRank on the handle's device
 *   dftpav_comm_share       another handle (= HIP stream) of the same process and device uses the owner's communicator: a host
 *                           with k batches in flight on k handles sets up one communicator per rank, not k.  The communicator
 *                           is held by all of them and destroyed when the last lets go (dftpav_comm_destroy / dftpav_destroy,
 *                           any order); every rank issues its collectives in the same order (round-robin over the handles does).
 *                           The holders may live on different host threads: the library serialises its calls on the shared
 *                           communicator with a lock (RCCL takes no concurrent enqueues); the ORDER is still the host's to keep
 *   dftpav_comm_layout      the contiguous shard [first, first + count) of a rank out of global_B trajectories, and `block` =
 *                           the largest shard: the gathered buffer holds nranks blocks of `block` records, rank r's shard at
 *                           the start of block r (the pad, at most one record, is zero)
 *   dftpav_batch_allgather_results   all-gathers this rank's records (written by the solve kernels' epilogues: the send
 *                           buffer is the batch's own record array) into all_records (DEVICE memory, nranks * block * 16 bytes);
 *                           asynchronous: the caller synchronises the handle's stream (dftpav_batch_sync)
 * RCCL is loaded on first use (librccl.so.1); DFTPAV_E_COMM where it is absent or a call fails.
 *
 * HARD REQUIREMENT for more than four handles with work in flight in one process (strong scaling keeps up to 16 steps in
 * flight per GPU): the environment variable GPU_MAX_HW_QUEUES must be set to at least that number BEFORE the HIP runtime
 * starts (the default is 4 hardware queues per process: the fifth stream's launch waits for one of the first four to drain,
 * which halves the throughput of 8 batches in flight and lets a collective queue behind an unrelated batch). */
#define DFTPAV_UNIQUE_ID_BYTES 128
int dftpav_comm_available(void);
int dftpav_comm_unique_id(void *id128);
int dftpav_comm_create(dftpav_handle *h, int nranks, int rank, const void *id128);
int dftpav_comm_destroy(dftpav_handle *h);
int dftpav_comm_share(dftpav_handle *h, dftpav_handle *owner);
int dftpav_comm_layout(int global_B, int nranks, int rank, int *first, int *count, int *block);
int dftpav_batch_allgather_results(dftpav_batch *b, int global_B, void *all_records);

/* Replaces getMinJerkOptPtr()[i].getCoeffs()/getDt() (traj_optimizer.h:112,
 * poly_traj_utils.hpp:1069-1074): regenerates the piece coefficients from the
 * final x on the device.  coeffs [B][Ntot][6][2] (row k multiplies s^k, then
 * x/y), piece_dt [B][M]. */
int dftpav_batch_coeffs(dftpav_batch *b, double *coeffs, double *piece_dt);

/* Duration in ms of the last solve of this batch, measured with HIP events recorded
 * on the handle's stream around its launches.  After dftpav_batch_solve_chained(b, prev)
 * this is the GPU time of the call: b's queue launch, including the trajectories adopted
 * from prev; a later dftpav_batch_finish(b) or adoption of b's stragglers moves the end
 * event to where b became complete. */
int dftpav_batch_last_solve_ms(dftpav_batch *b, float *ms);

/* ---- validation of the result, the step after the solve ----
 * Replaces the collision re-check of TrajPlannerServer::CheckReplan
 * (traj_server_ros.cpp:385-397) for every trajectory of a solved batch: each
 * segment is sampled at t = 0, sample_dt, ... < duration (0.05 in the
 * reference), the vehicle outline at spacing vertex_res (0.1, shapes.h:201)
 * is tested against the map of dftpav_set_grid_map
 * (semantic_map_manager.cc:639-662).  collision[t] = 1 if any sample of
 * trajectory t collides, first_sample[t] = index of the first such sample
 * counted over the segments in order (-1 if none).  Either output may be NULL.
 * dftpav_corridor_last_ms reports the kernel's duration afterwards. */
int dftpav_batch_validate(dftpav_batch *b, double sample_dt, double vertex_res, int *collision, int *first_sample);

/* ---- read-out of the result: Trajectory::GetState over a time grid ----
 * Replaces Trajectory::GetState (poly_traj_utils.hpp:378-406, with
 * Piece::getStateExpPos :303-340) called the way the server plays a plan back
 * (TrajPlannerServer::PublishData, traj_server_ros.cpp:244-259): the gear
 * segments of a trajectory follow one another in time as
 * TrajContainer::addSingulTraj chains them (traj_container.hpp:58-73,
 * traj_manager.cpp:617-624; time 0 = start of the first segment), sample k
 * carries the time stamp t0 + k * sample_dt and is read from the first segment
 * whose end_time is not <= that time; past the last segment nothing is
 * published.  states [B][n_samples][8] = {time_stamp, x, y, angle, curvature,
 * velocity, acceleration, steer} (the fields of common::State the server
 * publishes), rows past n_valid[t] are zero; n_valid [B] may be NULL.
 * filter_singularity != 0 applies TrajPlannerServer::FilterSingularityState
 * (traj_server_ros.cpp:335-356) along each trajectory, the history being the
 * previous sample.  Needs a solved batch. */
int dftpav_batch_sample_states(dftpav_batch *b, double t0, double sample_dt, int n_samples, int filter_singularity,
                               double *states, int *n_valid);

/* ---- one planning cycle, stream-ordered ------------
 * Replaces the body of TrajPlanner::RunMINCOParking from getRectangleConst on
 * (traj_manager.cpp:551-626) together with the consumers of its result: the
 * collision re-check of CheckReplan (traj_server_ros.cpp:385-397) and the state
 * playback (traj_server_ros.cpp:244-259,335-356).  After the boundary states,
 * waypoints and durations of `d` are uploaded (d->corridor is ignored), every
 * stage is enqueued on the handle's stream without the host in between:
 *   rectangles of every hypothesis from the installed map
 *     (states [B / n_restarts][Npts][3], as dftpav_batch_corridor_from_hypotheses)
 *   -> solve -> coefficients of the solutions
 *   -> collision re-check every check_dt seconds (outline points every vertex_res m)
 *   -> states at t0 + k * state_dt, k < n_samples (as dftpav_batch_sample_states).
 * dftpav_plan_cycle returns once everything is enqueued; dftpav_plan_cycle_fetch
 * waits for the stream and copies out whatever is asked for (any pointer may be
 * NULL): the arrays of dftpav_batch_results, dftpav_batch_validate and
 * dftpav_batch_sample_states, bit for bit what the separate calls return. */
int dftpav_plan_cycle(dftpav_batch *b, const dftpav_batch_data *d, const double *states, int n_restarts, double check_dt,
                      double vertex_res, double t0, double state_dt, int n_samples, int filter_singularity);
int dftpav_plan_cycle_fetch(dftpav_batch *b, double *x, double *final_cost, int *status, int *success, int *iters, int *collision,
                            int *first_sample, double *states, int *n_valid);

/* ---- serialised form of a trajectory -----------------------
 * The reference declares traj_planner/msg/PolyTraj.msg:1-9 (drone_id, traj_id,
 * start_time, order, float32 coefficients, durations) and never uses it; plans
 * and predicted obstacle motions travel as plan_utils::LocalTrajData
 * (traj_container.hpp:28-38) inside one process.  This is the same content as
 * bytes, in fp64 so that a trajectory survives the trip bit for bit
 * (little-endian, every field naturally aligned):
 *
 *   header  (32 B)  char magic[4] = "DPTJ"; u16 version = 1; u8 order = 5; u8 dim = 2;
 *                   i32 drone_id; i32 traj_id; i32 n_segments; i32 reserved = 0; f64 start_time
 *   segment (24 B)  i32 singul; i32 n_pieces; f64 start_time; f64 duration   (LocalTrajData of one gear segment,
 *                   start/duration as addSingulTraj computes them from header.start_time)
 *   piece  (104 B)  f64 duration; f64 coeff[12]   CoefficientMat column-major, column 0 multiplies t^5:
 *                   x5,y5, x4,y4, ... x0,y0 (poly_traj_utils.hpp:77-87, 993) — the layout of dftpav_surround.coeffs
 *
 * dftpav_wire_size: bytes of a trajectory with these segments (0 on bad input).
 * dftpav_wire_pack: one trajectory from the arrays dftpav_batch_coeffs returns for it (coeffs [Ntot][6][2], piece_dt [M]).
 * dftpav_wire_info: validates a blob, returns its header fields and the total piece count (any output may be NULL).
 * dftpav_wire_unpack: singuls/piece_nums/seg_start/seg_duration [n_segments], durations [pieces], coeffs [pieces][12].
 * dftpav_set_surround_wire: installs S blobs as the moving obstacles (== dftpav_set_surround; the segments of a
 *   blob are joined into one obstacle trajectory that starts at the blob's start_time).  The reference builds its
 *   obstacle model with getTraj(1) (traj_manager.cpp:726,775), so a blob with a reverse segment is refused.
 * Pure host code except the last one. */
size_t dftpav_wire_size(int n_segments, const int *piece_nums);
int dftpav_wire_pack(const dftpav_layout *layout, const double *coeffs, const double *piece_dt, int drone_id, int traj_id,
                     double start_time, void *buf, size_t capacity, size_t *written);
int dftpav_wire_info(const void *buf, size_t size, int *drone_id, int *traj_id, double *start_time, int *n_segments,
                     int *n_pieces);
int dftpav_wire_unpack(const void *buf, size_t size, int *singuls, int *piece_nums, double *seg_start, double *seg_duration,
                       double *durations, double *coeffs);
int dftpav_set_surround_wire(dftpav_handle *h, const void *const *bufs, const size_t *sizes, int S);

/* ---- Reeds-Shepp shots: analytic hypotheses ------------------
 * Replaces KinoAstar::computeShotTraj and is_shot_sucess (kino_astar.cpp:304-345) for n (from, to) pose
 * pairs (x, y, yaw): the shortest Reeds-Shepp path of turning radius 1 / max_cur
 * (ompl::base::ReedsSheppStateSpace, kino_astar.cpp:423 -- OMPL is not part of the reference tree; the
 * published algorithm is restated in dftpav_amd/csrc/rs_math.h), its length (ReedsSheppStateSpace::distance),
 * word (type 0..17, the rows of OMPL's reedsSheppPathType table) and signed segment lengths in units of the
 * turning radius, the poses at l = 0, checkl, checkl + checkl, ... <= length (ReedsSheppStateSpace::
 * interpolate; 0.2 in the reference, minco_config.pb.txt:59) and, if `collides` is given, whether any of
 * them collides on the map of dftpav_set_grid_map (CheckCollisionUsingPosAndYaw, outline spacing vertex_res).
 * samples [n][max_samples][3]: at most max_samples poses are stored per pair, n_samples reports how many the
 * loop visits.  Any output may be NULL.  The sampled path is what dftpav_frontend_resample takes as a searched
 * path (the reference appends it to the searched prefix, kino_astar.cpp:585-599). */
int dftpav_reeds_shepp_shots(dftpav_handle *h, const double *from, const double *to, int n, double max_cur, double checkl,
                             int max_samples, double vertex_res, double *length, int *type, double *seg, double *samples,
                             int *n_samples, int *collides);

/* ---- hybrid A* front-end search: a start pose and a goal to the searched path --------
 * Replaces TrajPlanner::getKinoPath (traj_manager.cpp:69-117): KinoAstar::search (kino_astar.cpp:37-301) with its
 * 3D-then-2D retry, then getKinoNode up to SampleTraj (kino_astar.cpp:554-612), for n independent queries on the map of
 * dftpav_set_grid_map (cells outside the grid are free).  One deviation: the reference's wall-clock budget
 * max_search_time (1.0 s, minco_config.pb.txt:50) is the iteration budget max_iters; when iter_num_ reaches it the
 * reference's time-out branch is taken (kino_astar.cpp:115-132).  The default max_iters is a chosen number, not derived
 * from the 1 s. */
typedef struct dftpav_search_params {
  double map_size_x, map_size_y;   /* 1000, 1000: origin_ = -0.5 map_size, the search's index frame (pb.txt:14-15, KA:404-409) */
  double map_resl;                 /* 0.3   (pb.txt:57) */
  double phi_grid_resolution;      /* 0.3   (pb.txt:51) */
  double lambda_heu;               /* 5.0   (pb.txt:47) */
  double tie_breaker;              /* 1 + 1 / 10000 (kino_astar.h:167) */
  int allocate_num;                /* 100000 nodes (pb.txt:48) */
  int check_num;                   /* 5     (pb.txt:49) */
  double step_arc;                 /* 0.9   (pb.txt:58) */
  double max_frontend_cur;         /* 1.0   (pb.txt:81): max_steer = atan(wheel_base * max_cur), shot radius 1 / max_cur */
  double checkl;                   /* 0.2   (pb.txt:59) */
  double traj_forward_penalty;     /* 1.0   (pb.txt:52) */
  double traj_back_penalty;        /* 2.5   (pb.txt:53) */
  double traj_gear_switch_penalty; /* 15.0  (pb.txt:54) */
  double traj_steer_penalty;       /* 0.5   (pb.txt:55) */
  double traj_steer_change_penalty;/* 0.0   (pb.txt:56) */
  double veh_width, veh_length;    /* 1.90 + 0.2, 4.88 + 0.2: vp_ with its margin (semantics.h, kino_astar.cpp:426-427) */
  double veh_d_cr, wheel_base;     /* 1.015, 2.85 (semantics.h) */
  double vertex_res;               /* 0.1   outline point spacing (shapes.h:201) */
  int max_iters;                   /* 20000 pops: stands for max_search_time (chosen, see above) */
  int use3d;                       /* 1: the first search keys nodes on (x, y, yaw) cells (getKinoPath: true) */
  int retry_2d;                    /* 1: a NO_PATH of a 3D search is searched again in 2D (traj_manager.cpp:87-103) */
} dftpav_search_params;
void dftpav_default_search_params(dftpav_search_params *sp);
#define DFTPAV_SEARCH_REACH_END 2 /* KinoAstar's enum, kino_astar.h:234 */
#define DFTPAV_SEARCH_NO_PATH 3
/* Caller-allocated outputs, per query q (every pointer required when its size is > 0). */
typedef struct dftpav_search_out {
  int max_nodes, max_path;
  int *status;       /* [n] DFTPAV_SEARCH_REACH_END or DFTPAV_SEARCH_NO_PATH */
  int *shot_success; /* [n] the search ended on a free shot (is_shot_succ_) */
  int *used_3d;      /* [n] the answer comes from a 3D search */
  int *budget_hit;   /* [n] the search ended at max_iters (the time-out branch) */
  int *iters;        /* [n] iter_num_ of the answering search */
  int *nodes_used;   /* [n] use_node_num_ of the answering search */
  int *n_nodes;      /* [n] path nodes, start to terminal (0 for NO_PATH; may exceed max_nodes: only the first are written) */
  double *nodes;     /* [n][max_nodes][6] x, y, yaw (as searched, not normalised), steer, arc, singul */
  int *path_len;     /* [n] SampleTraj poses (0 for NO_PATH; may exceed max_path: only the first are written) */
  double *paths;     /* [n][max_path][3] SampleTraj: the layout dftpav_frontend_resample takes */
} dftpav_search_out;
/* start_states / end_states [n][4] (x, y, yaw, v); start_ctrl [n][2] (steer, acceleration: search keeps it for
 * getKinoNode's flat states, i.e. for dftpav_frontend_resample).  DFTPAV_E_INVALID without a map;
 * DFTPAV_E_UNSUPPORTED for parameters beyond the kernel's bounds (more than 32 inputs per expansion, check_num > 8,
 * inputs x check_num > 256, a shot longer than its sample table).  dftpav_corridor_last_ms reports the kernel time. */
int dftpav_kino_search(dftpav_handle *h, const dftpav_search_params *sp, const double *start_states, const double *start_ctrl,
                       const double *end_states, int n, const dftpav_search_out *out);
/* Test hook, pure host code: the workspace arithmetic of a search of n queries.  bytes_per_query: node pool, heap, path list
 * and hash table of one query in flight; slots: the queries in flight at once, n or as many as 6 GiB of workspace hold (at
 * least 1) -- the queries beyond run in further launches over the same slots.  Either pointer may be NULL.
 * DFTPAV_E_INVALID for n < 1 or allocate_num < 2. */
int dftpav_debug_search_slots(const dftpav_search_params *sp, int n, int *slots, size_t *bytes_per_query);
/* Test hook, pure host code: the two tables every collision re-check reads (dftpav_batch_validate, dftpav_plan_cycle,
 * dftpav_plan_queries, dftpav_replan_check), out = 4096 sample times (the running sum t += check_dt from 0.0) | the spacings of
 * the outline points (the running sum dl += vertex_res while dl < max(veh_length, veh_width) + 1.0; one entry vertex_res if that
 * leaves none); *n_t and *n_v their counts.  max_spacings > 0: DFTPAV_E_UNSUPPORTED where that many spacings or more are needed
 * (dftpav_replan_check: 4096); 0: no cap, and DFTPAV_E_UNSUPPORTED for a table beyond out's 8192 doubles.  DFTPAV_E_INVALID for
 * a NULL pointer, increments that are not positive, or max_spacings < 0. */
int dftpav_debug_validation_table(const dftpav_params *p, double check_dt, double vertex_res, int max_spacings, double *out /*[8192]*/,
                                  int *n_t, int *n_v);

/* ---- a batch of start / goal queries to their plans, mixed layouts included --------------
 * Replaces TrajPlanner::RunOnceParking from the arrival test on (traj_manager.cpp:194-217): per query the
 * arrival test (:196), getKinoPath (:69-117, as dftpav_kino_search), getKinoNode from SampleTraj on and the
 * resampling of RunMINCOParking (as dftpav_frontend_resample), n_restarts seeded restarts of the searched
 * hypothesis (as dftpav_sample_restarts, keyed by (seed, query index in the call, restart)), getRectangleConst,
 * OptimizeTrajectory in DFTPAV_ORDER_REFERENCE, the coefficients and the collision re-check of CheckReplan
 * (traj_server_ros.cpp:385-397), and the choice of the cheapest collision-free restart.  The map is the one of
 * dftpav_set_grid_map, the moving obstacles those installed on the handle.
 *
 * Searched paths of different goals come back with different layouts (gear segments, pieces, directions).  The
 * queries are grouped by layout (dftpav_plan_group_layouts); every layout has a batch of its own in the planner,
 * created on first use with room for max_queries * n_restarts trajectories and kept for later calls.  The stages
 * run on the handle's stream from device memory; the host reads the small tables that decide the grouping once,
 * after the resampling, and the compact results at the end.  Bit for bit what the separate calls return.
 * A query without a plan does not disturb the others.  A restart that fails the mini_T test of
 * traj_optimizer.cpp:30-33 makes its query DFTPAV_PLAN_NO_VALID_RESTART (OptimizeTrajectory refuses it).
 * Destroy a planner before its handle. */
typedef struct dftpav_planner dftpav_planner;
#define DFTPAV_PLAN_OK 0
#define DFTPAV_PLAN_NO_PATH 1            /* the search found none (DFTPAV_SEARCH_NO_PATH) */
#define DFTPAV_PLAN_TOO_MANY_SEGMENTS 2  /* more segments, pieces, poses or path poses than the padding holds */
#define DFTPAV_PLAN_LAYOUT_UNSUPPORTED 3 /* outside the limits of DFTPAV_ORDER_REFERENCE (dftpav_batch_set_order) */
#define DFTPAV_PLAN_NO_VALID_RESTART 4   /* every restart failed or collides */
#define DFTPAV_PLAN_ARRIVED 5            /* closer to the goal than 1.0 m (traj_manager.cpp:196): nothing is planned */
#define DFTPAV_PLAN_MAX_VARS 256         /* decision variables of a plan at most (the reference order's limit) */
typedef struct dftpav_plan_params {
  dftpav_search_params search;     /* dftpav_default_search_params */
  dftpav_frontend_params frontend; /* as dftpav_frontend_resample; traj_res / dense_traj_res must equal the handle's
                                      traj_resolution / des_traj_resolution */
  double sigma, dur_lo, dur_hi;    /* 0.3, 0.8, 1.25: the restart sampler (dftpav_sample_restarts) */
  unsigned long long seed;         /* 0 */
  double check_dt, vertex_res;     /* 0.05, 0.1: the collision re-check (dftpav_batch_validate) */
  int max_seg, max_pieces, max_path; /* 8, 64, 4096: padding of the front end (max_seg <= 8); a segment holds up to
                                      (max_pieces - 2) (traj_res + 1) + 2 (dense_traj_res + 1) poses */
} dftpav_plan_params;
void dftpav_default_plan_params(dftpav_plan_params *pp);
/* Caller-allocated outputs.  Q queries, R = the planner's n_restarts, padded with max_seg / max_pieces of the
 * parameters.  Every pointer may be NULL.  Rows of queries without a plan are zero (winner: -1). */
typedef struct dftpav_plan_out {
  int *plan_status;     /* [Q] DFTPAV_PLAN_* */
  int *n_seg;           /* [Q] gear segments found (as dftpav_frontend_out; 0 where nothing was searched or resampled) */
  int *singul;          /* [Q][max_seg] */
  int *piece_nums;      /* [Q][max_seg] */
  double *piece_dt;     /* [Q][max_seg] of the searched hypothesis */
  int *winner;          /* [Q] restart index, -1 if none */
  double *final_cost;   /* [Q] the winner's */
  int *iters;           /* [Q] */
  double *x;            /* [Q][DFTPAV_PLAN_MAX_VARS] the winner's decision vector (dftpav_num_vars of its layout are used) */
  double *coeffs;       /* [Q][max_seg * max_pieces][6][2] the winner's pieces, as dftpav_batch_coeffs / dftpav_wire_pack take them */
  double *coeff_dt;     /* [Q][max_seg] the winner's piece durations (piece_dt of dftpav_batch_coeffs) */
  double *r_final_cost; /* [Q][R] per restart, as dftpav_batch_results / dftpav_batch_validate */
  int *r_status, *r_success, *r_iters, *r_evals, *r_collision, *r_first_sample; /* [Q][R] */
  int *search_status, *search_iters, *search_path_len;                          /* [Q] as dftpav_search_out */
} dftpav_plan_out;
int dftpav_planner_create(dftpav_handle *h, int max_queries, int n_restarts, dftpav_planner **out);
void dftpav_planner_destroy(dftpav_planner *p);
/* start_states / end_states [Q][4] (x, y, yaw, v), start_ctrl [Q][2]; t_now: `now` of OptimizeTrajectory.
 * DFTPAV_E_INVALID without a map, for Q > max_queries or bad parameters; the planner stays usable. */
int dftpav_plan_queries(dftpav_planner *p, const dftpav_plan_params *pp, const double *start_states, const double *start_ctrl,
                        const double *end_states, int Q, double t_now, const dftpav_plan_out *out);
/* n_batches: batches the planner holds (one per layout met so far); n_groups / group_sizes [max_queries]: the layout groups of
 * the last call, in order of first appearance; stage_ms [4]: device time of the last call's search, resampling, groups
 * (pack to selection) and everything together.  Any pointer may be NULL. */
int dftpav_planner_info(dftpav_planner *p, int *n_batches, int *n_groups, int *group_sizes, float *stage_ms);
/* The grouping rule, pure host code: query q with search_status[q] == DFTPAV_SEARCH_REACH_END and 1 <= n_seg[q] <= max_seg
 * joins the group of the first query with the same n_seg, singul[0 .. n_seg) and piece_nums[0 .. n_seg) (rows of max_seg
 * ints); group[q] = its index in order of first appearance, group_first[g] = that first query.  Otherwise group[q] = -1 and
 * plan_status[q] = DFTPAV_PLAN_NO_PATH (not REACH_END) or DFTPAV_PLAN_TOO_MANY_SEGMENTS; grouped queries get DFTPAV_PLAN_OK.
 * plan_status may be NULL.  n_groups receives the number of groups. */
int dftpav_plan_group_layouts(int Q, int max_seg, const int *search_status, const int *n_seg, const int *singul,
                              const int *piece_nums, int *group, int *group_first, int *n_groups, int *plan_status);
/* Test hook: the selection rule on caller-supplied arrays [n_query][n_restarts]: among restarts with success != 0 and
 * collision == 0 the smallest cost (a NaN never wins), ties to the lowest index, -1 if none. */
int dftpav_debug_plan_select(dftpav_handle *h, int n_query, int n_restarts, const double *cost, const int *success,
                             const int *collision, int *winner_out);

/* ---- the replan loop: a table of executing plans, checked and planned again once per tick ----------
 * Replaces the 20 Hz loop of TrajPlannerServer for as many plans as the planner has slots (max_queries of
 * dftpav_planner_create): PlanCycleCallback's completion test (traj_server_ros.cpp:149-158), CheckReplan (:359-402),
 * the desired state of Replan (:414, :445-461, with Trajectory::GetState, poly_traj_utils.hpp:378-406, and
 * FilterSingularityState, :335-356), the hand-over of that state to the planner (getKinoPath, traj_manager.cpp:74-75) and
 * the swap of the new plan for the executing one (:171-178).  A slot is empty or holds one executing plan in device memory:
 * its layout, pieces and piece durations padded as dftpav_plan_out, per gear segment duration / start_time / end_time
 * chained as TrajContainer::addSingulTraj does (traj_container.hpp:58-73, traj_manager.cpp:618-625: duration = the piece
 * durations summed in order, segment 0 starts at t_start, end_time = start_time + duration, the next segment starts at that
 * end_time), the goal the plan was made for, and the previous desired state of the singularity filter (time stamp, angle).
 * The padding (max_seg <= 8, max_pieces) is fixed by the first call that fills the table; another padding later is
 * DFTPAV_E_INVALID.  Slots named twice in one call, slots outside [0, max_queries), n_seg outside [1, max_seg] and
 * piece_nums outside [1, max_pieces] are DFTPAV_E_INVALID; a refused call changes nothing.
 * NOT reproduced: Replan's busy-wait until the budget has passed with its "exceed time budget"
 * refusal (traj_server_ros.cpp:472-484) -- wall clock belongs to the caller --, the restamping of the first plan
 * (traj_manager.cpp:631-637), the refusal of a new plan whose first segment lasts <= 1e-5 s (traj_server_ros.cpp:496-499)
 * and the reset of the filter history to the map message's ego state after a first plan (:436-437: the tick stores
 * (t_now + budget, the ego angle) instead).
 *
 * dftpav_planner_install: n plans from host arrays (TrajContainer::addSingulTraj, traj_container.hpp:58-73) into `slots`
 *   [n]: n_seg [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs [n][max_seg * max_pieces][6][2] (the pieces of a
 *   plan's segments one after another), end_states [n][4].  The times are chained on the host.  The slots start without
 *   filter history.
 * dftpav_planner_adopt: the winners of the LAST dftpav_plan_queries call of this planner become the executing plans
 *   (executing_traj_ = std::move(next_traj_), traj_server_ros.cpp:171-178): query queries[i] into slot slots[i], a
 *   device-to-device gather by one small kernel, the times chained there by the same additions.  A query without a winner
 *   leaves its slot untouched; adopted [n] (may be NULL) reports 1 / 0.  The goal stored is the query's end state.
 * dftpav_planner_set_history: the previous desired state of `slots` [n] (desired_state_hist_.back(), :460-461): time stamps
 *   and angles [n].  An empty slot is DFTPAV_E_INVALID.
 * dftpav_planner_clear: empties `slots` [n] (executing_traj_.release(), :154).
 * dftpav_planner_executing: reads a slot back; any pointer may be NULL.  n_seg 0: empty (the arrays are then zero).
 *   singul / piece_nums / coeff_dt / duration / start_time / end_time [max_seg], coeffs [max_seg * max_pieces][6][2],
 *   end_state [4], hist [2] (time stamp, angle), have_hist [1].  Size them by dftpav_planner_padding.
 * dftpav_planner_padding: the table's padding (max_seg, max_pieces), 0 and 0 before the first call that fills the table
 *   (dftpav_planner_executing then writes n_seg and have_hist only).  Either pointer may be NULL. */
int dftpav_planner_install(dftpav_planner *p, int n, const int *slots, int max_seg, int max_pieces, const int *n_seg,
                           const int *singul, const int *piece_nums, const double *coeff_dt, const double *coeffs,
                           const double *end_states, double t_start);
int dftpav_planner_adopt(dftpav_planner *p, int n, const int *queries, const int *slots, double t_start, int *adopted);
int dftpav_planner_set_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles);
int dftpav_planner_clear(dftpav_planner *p, int n, const int *slots);
int dftpav_planner_executing(dftpav_planner *p, int slot, int *n_seg, int *singul, int *piece_nums, double *coeff_dt,
                             double *coeffs, double *duration, double *start_time, double *end_time, double *end_state,
                             double *hist, int *have_hist);
int dftpav_planner_padding(dftpav_planner *p, int *max_seg, int *max_pieces);

/* Caller-allocated outputs of the check, one row per slot; every pointer may be NULL.  Rows of empty slots without an ego
 * state and of completed slots are zero apart from occupied / complete (first_sample: -1). */
typedef struct dftpav_replan_out {
  int *occupied;           /* [slots] the slot holds a plan */
  int *complete;           /* [slots] t_now > end_time of the last segment (traj_server_ros.cpp:150) */
  int *exe_index;          /* [slots] first segment whose end_time is not <= t_now (:248-252); at t_now == the last end_time the last */
  int *is_close_turnpoint; /* [slots] :373-377 */
  int *is_near;            /* [slots] :379 */
  int *target_moved;       /* [slots] (localTarget - end_state.head(2)).norm() > 0.1 (:367, :381) */
  int *collision;          /* [slots] the loop of :385-397, as dftpav_batch_validate */
  int *first_sample;       /* [slots] as dftpav_batch_validate (-1: none) */
  int *replan;             /* [slots] is_near && !is_close_turnpoint && target_moved, or collision; 1 for an empty slot with an ego state */
  double *desired;         /* [slots][8] time_stamp, x, y, angle, curvature, velocity, acceleration, steer at t_now + budget */
  double *start_state;     /* [slots][4] x, y, angle, velocity (traj_manager.cpp:74) */
  double *start_ctrl;      /* [slots][2] steer, acceleration (traj_manager.cpp:75) */
} dftpav_replan_out;

/* One kernel (replan.hip), one workgroup per slot, whatever the layouts: completion, CheckReplan and Replan's desired state
 * (see above) for every slot at clock t_now.  The collision loop runs on the map of dftpav_set_grid_map every check_dt
 * seconds with outline points every vertex_res m, and always (the reference returns before it when the near / target rule
 * fires, :381-383: `replan` is the same, `collision` is additionally known).  exe_traj_index_ is derived from t_now, so
 * the call keeps no state; the table is not written.  The desired state is read at t_now + budget (Budget = 0.5 s in
 * the reference) from the segment the pidx walk of :445-457 stops at, and filtered against the slot's stored previous
 * desired state where it has one.  end_states [slots][4]: the goals (end_pt_) to test the local target against, NULL = the
 * stored ones.  ego_states [slots][6] (x, y, angle, velocity, steer, acceleration) or NULL: an empty slot with an ego state
 * wants a plan (executing_traj_ == nullptr, :361, :415-416), its desired state is the ego state with the stamp (curvature
 * 0).  ego_states has a row for every slot and no per-slot switch: with it given EVERY empty slot is flagged, and the tick
 * plans every one of them; a caller who wants some slots to stay idle passes NULL and fills those that should start with
 * dftpav_plan_queries + dftpav_planner_adopt.  DFTPAV_E_INVALID without a map or before the table was filled once. */
int dftpav_replan_check(dftpav_planner *p, double t_now, double budget, const double *end_states, const double *ego_states,
                        double check_dt, double vertex_res, const dftpav_replan_out *out);

/* One tick of PlanCycleCallback (traj_server_ros.cpp:130-192) for every slot: the check above (with pp's check_dt /
 * vertex_res), ONE small read-back of replan / start_state / start_ctrl -- the tick's one wait beyond those of
 * dftpav_plan_queries, which does its arrival test on the host anyway --, the flagged slots packed in rising slot order
 * into the queries of dftpav_plan_queries (that code, with t_now + budget as its t_now; query_slot[q] = the slot of query
 * q, n_queries their number; query_slot [slots]), and for every query that ends DFTPAV_PLAN_OK with a winner the adoption
 * of the winner into its slot with t_start = t_now + budget (:414, traj_manager.cpp:520), the desired state stored as
 * the slot's filter history (:461) and the goal stored.  A flagged slot whose planning fails keeps its executing plan
 * (next_traj_ stays null).  plan_out is indexed by query, as in a plain call.  check_out, query_slot, n_queries and plan_out
 * may be NULL.  With ego_states given, end_states must be given too (an empty slot has no stored goal).
 * Restarts stay keyed by (seed, query index in the call, restart): the restarts of a slot therefore depend on which other
 * slots replan in the same tick (restart 0, the searched hypothesis itself, does not).
 * With the conflict trigger on (dftpav_planner_set_conflict_trigger, below; off by default) a slot is also a query when the
 * trigger says it yields to another slot's executing plan: its kernels run behind the check, their yield row joins the one
 * read-back, and the replan row of check_out stays the check's own flag.  With the trigger on the call also refuses
 * (DFTPAV_E_INVALID, nothing changed) a t_now + budget that is not finite: it is the trigger's first clock. */
int dftpav_replan_tick(dftpav_planner *p, const dftpav_plan_params *pp, double t_now, double budget, const double *end_states,
                       const double *ego_states, const dftpav_replan_out *check_out, int *query_slot, int *n_queries,
                       const dftpav_plan_out *plan_out);
/* Device time in ms (the planner's HIP events) of the last check kernel, and of the last tick from the start of its check to
 * the end of its adoption (the host's read-back and grouping in between included).  Either pointer may be NULL. */
int dftpav_replan_last_ms(dftpav_planner *p, float *check_ms, float *tick_ms);

/* ---- the replan loop, its other half: the 100 Hz publisher of every executing plan's control state ----------
 * Replaces TrajPlannerServer::PublishData's trajectory feedback (traj_server_ros.cpp:240-289) for every slot of the table: the
 * walk of exe_traj_index_ (:248-252), Trajectory::GetState on that segment (:255, poly_traj_utils.hpp:378-406, 510-528),
 * FilterSingularityState against ctrl_state_hist_.back() (:257, :335-356) and the push_back of the filtered state (:258).  The
 * state published is what common::VehicleControlSignal(state) is built from (:261-264, :287).  The simulator drives the
 * vehicle open-loop from it, so it is also the ego state of the next tick.
 * Per slot the planner keeps, beside the table: exe_index (exe_traj_index_), the back of ctrl_state_hist_ as (time stamp,
 * angle), and whether there is one.
 *   dftpav_planner_install                         exe_index 0, no control history
 *   dftpav_planner_adopt, the tick's adoption      exe_index 0 (:177); the control history is kept if the slot had a plan (the
 *                                                  reference keeps ctrl_state_hist_ across replans)
 *   first plan into an empty slot by the tick      exe_index 0, the history seeded with (t_now + budget, the ego angle), as the
 *                                                  tick does for the desired-state history, in place of :438-439
 *   first plan into an empty slot by a plain adopt exe_index 0, no control history
 *   dftpav_planner_clear                           exe_index 0, the history dropped
 * NOT reproduced: the idle branch (:210-237), which holds the ego state still, with no plan read, when
 * nothing executes, when exe_index is past the last segment or when the segment lasts < 1e-5 s -- those ticks report
 * published = 0 and change nothing --; the 100-entry cap of ctrl_state_hist_ (:259: only its back is ever read); and
 * use_sim_state_ == false (:241).
 *
 * dftpav_planner_publish: K ticks with the clocks t [K], applied in order (they need not increase), for every slot, in ONE
 *   kernel launch (publish_kernel, replan.hip) on the handle's stream and one read-back at the end.  Per tick and slot, in the
 *   reference's statements and order: an empty slot, or exe_index past the last segment, publishes nothing; if
 *   end_time[exe_index] <= t the index advances by ONE (:248-250); past the last segment then, nothing is published, and the slot
 *   stays finished (:251-252); else the state is GetState(t - start_time[exe_index]) -- clamped to the segment's duration, a
 *   negative time evaluates piece 0 as it stands --, filtered against the history back where there is one, and becomes the
 *   history back.  states [K][slots][8]: time_stamp, x, y, angle, curvature, velocity, acceleration, steer (the fields and
 *   order of dftpav_replan_out.desired), zero where nothing is published.  published [K][slots]: 0 nothing, 1 published, 2
 *   published with the angle replaced by the filter.  Either may be NULL.  DFTPAV_E_INVALID before the table was filled
 *   once, for K < 1, K > DFTPAV_PUBLISH_MAX_TICKS, t NULL or a NaN clock; a refused call changes nothing.  The table is not
 *   written; dftpav_replan_check goes on deriving its index from its clock.
 * dftpav_planner_publisher_state: reads a slot's state back: exe_index [1], hist [2] (time stamp, angle), have_hist [1]; any may
 *   be NULL.  Before the table was filled once: zeros.
 * dftpav_planner_set_ctrl_history: the control history back of `slots` [n] (ctrl_state_hist_.back()): stamps and angles [n].  An
 *   empty slot is DFTPAV_E_INVALID, as for dftpav_planner_set_history.
 * dftpav_publish_last_ms: device time in ms (the planner's HIP events) of the last publish kernel; 0 before the first. */
#define DFTPAV_PUBLISH_CHUNK 256      /* ticks a workgroup of publish_kernel takes at a time */
#define DFTPAV_PUBLISH_MAX_TICKS 4096 /* the cap on K: 40 s at 100 Hz (the outputs are K * slots rows of device memory) */
int dftpav_planner_publish(dftpav_planner *p, int K, const double *t, double *states, int *published);
int dftpav_planner_publisher_state(dftpav_planner *p, int slot, int *exe_index, double *hist, int *have_hist);
int dftpav_planner_set_ctrl_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles);
int dftpav_publish_last_ms(dftpav_planner *p, float *ms);

/* ---- solved plans against the kinematic limits ------------------------------------------------------------------
 * The reference checks no plan against the vehicle's limits after the solve: velocity, longitudinal acceleration and curvature
 * enter OptimizeTrajectory as soft penalties only (wei_feas, traj_optimizer.cpp:422-779), the lateral-acceleration and
 * steering-rate penalties are switched off, and `success` means "status accepted and cost < fail_cost".  These calls evaluate,
 * on the device (limits.hip), what the reference can compute but never tests:
 *   Trajectory::getVel / getAcc / getLatAcc / getCurv / getSteer   plan_utils/poly_traj_utils.hpp:606-645
 *   Piece::getVel / getAcc / getLatAcc / getCurv / getSteer        poly_traj_utils.hpp:247-300, each with its |dsigma| < 1e-6 -> 0.0
 *                                                                  branch where the reference has one (getVel and getSteer have none)
 * over the samples CheckReplan walks (traj_server_ros.cpp:385-386: per gear segment t = 0.0; t < duration; t += check_dt), with
 * Trajectory::locatePieceIdx's subtraction walk for the local time (:510-528).  The sample times are the running sums of
 * dftpav_debug_validation_table, a sample's global index is the one `first_sample` of dftpav_batch_validate uses.  fp64 in the
 * reference's statements and order, dsigma.norm() as sqrt(x * x + y * y); pow(., 3) and std::atan are correctly rounded
 * (cr_trig.h) where the reference calls libm.  Held bit for bit by oracle_limits/limits_oracle.cpp in order 2.
 *
 * Per trajectory and quantity q (columns: velocity, longitudinal acceleration, lateral acceleration, curvature, steer):
 *   max_abs   the maximum of |q| over the samples.
 *   arg       the global sample index where that maximum is FIRST reached: ties go to the lowest index.
 *   violated  1 if |q| > limit, strictly, at any sample.  The limit of a sample is chosen by its segment's singul (> 0: the
 *             max_forward_* value, else max_backward_*) for velocity, acceleration and curvature; max_latacc and max_steer are one
 *             value each.
 *   NaN       a NaN sample violates its limit whatever the limit (+inf included) and is reported as the maximum, max_abs NaN, at
 *             the FIRST NaN sample of the trajectory.
 *   A trajectory without a sample reports max_abs 0, arg -1, nothing violated.  feasible: none of the five violated.
 * dftpav_default_limits: the parameters' values (config/minco_config.pb.txt:83-85 forward, :87-89 backward, :91 max_latacc);
 *   max_steer = +inf, the reference has no steer limit of its own.  Every limit must be > 0; +inf switches a test off.
 * dftpav_batch_check_limits: the B trajectories of a solved batch, from the coefficients dftpav_batch_coeffs produces (or those of
 *   dftpav_debug_batch_set_coeffs).  Rows [B].
 * dftpav_planner_check_limits: a row per slot of the executing table; empty slots (and every slot before the table was filled
 *   once) give zero rows, feasible included, with arg -1.  The table is not written.
 * dftpav_planner_set_limit_filter: l == NULL (the default): dftpav_plan_queries and dftpav_replan_tick do exactly what they do
 *   without this call -- the same launches, the same bits.  With limits: per layout group the limits kernel runs after the
 *   collision re-check and before the selection, and the selection passes over a restart that is not feasible, so the
 *   winner is the cheapest restart that succeeded, does not collide and respects every limit; a query whose every restart is
 *   rejected ends DFTPAV_PLAN_NO_VALID_RESTART (a tick then keeps the slot's old plan).  r_collision / r_first_sample of
 *   dftpav_plan_out stay the pure collision results.  The limits and check_dt are copied.
 * dftpav_planner_last_limits: the rows [Q][R] (query, restart) of the last dftpav_plan_queries call that ran with the filter on;
 *   zero rows with arg -1 for the queries no restart was solved for.  DFTPAV_E_INVALID when that call ran without the filter.
 * dftpav_limits_last_ms: device time in ms (the handle's HIP events) of the last limits kernel of one of the two check_limits calls.
 * Every pointer of dftpav_limits_out may be NULL.  A refused call changes nothing and returns DFTPAV_E_INVALID: no solved
 * coefficients (for the planner's filter: nothing), check_dt <= 0 or NaN, a check_dt that is not finite (its table of sample
 * times is not one validate's kernel can continue), a limit that is <= 0 or NaN, l or out NULL. */
typedef struct dftpav_limits {           /* every limit > 0; +inf switches a test off */
  double max_forward_vel, max_backward_vel, max_forward_acc, max_backward_acc,
         max_forward_cur, max_backward_cur, max_latacc, max_steer;
} dftpav_limits;
void dftpav_default_limits(const dftpav_params *p, dftpav_limits *l);
typedef struct dftpav_limits_out {        /* caller-allocated, any pointer may be NULL */
  double *max_abs;   /* [n][5] vel, acc, latacc, cur, steer */
  int *arg;          /* [n][5] */
  int *violated;     /* [n][5] */
  int *feasible;     /* [n]   none of the five violated */
} dftpav_limits_out;
int dftpav_batch_check_limits(dftpav_batch *b, double check_dt, const dftpav_limits *l, const dftpav_limits_out *out);
int dftpav_planner_check_limits(dftpav_planner *p, double check_dt, const dftpav_limits *l, const dftpav_limits_out *out);
int dftpav_planner_set_limit_filter(dftpav_planner *p, const dftpav_limits *l, double check_dt);
int dftpav_planner_last_limits(dftpav_planner *p, const dftpav_limits_out *out);
int dftpav_limits_last_ms(dftpav_handle *h, float *ms);

/* ---- the residual penalties of solved plans, and a selection filter on them -------------------------------------
 * `success` means "status accepted and cost < fail_cost": the cheapest collision-free restart may still lean on an active
 * corridor or moving-obstacle penalty.  The three penalty sums of dftpav_batch_cost_terms say how far, in the reference's own
 * arithmetic; no other criterion is judged.
 * dftpav_planner_set_penalty_filter: caps == NULL (the default): dftpav_plan_queries and dftpav_replan_tick do exactly what
 *   they do without this call -- the same launches, the same bits.  With caps: per layout group, after the collision re-check
 *   (and the limits kernel, when that filter is set), the terms launch runs on the group's solutions and penalty_gate_kernel
 *   (plan.hip) rejects a restart unless  corridor <= caps.corridor && surround <= caps.surround && feasibility <=
 *   caps.feasibility  (a NaN term is rejected; a cap of +inf never rejects a finite term; a cap of 0.0 is legal: no residual
 *   penalty at all).  The selection passes over a restart that collides, is not feasible or is rejected here (one reject flag
 *   per restart, set by whichever filter rejects it; the order of the filters does not show); a query whose every restart is rejected ends
 *   DFTPAV_PLAN_NO_VALID_RESTART (a tick then keeps the slot's old plan).  r_collision / r_first_sample of dftpav_plan_out stay
 *   the pure collision results.  The caps are copied.  A negative or NaN cap is DFTPAV_E_INVALID, and nothing changes.
 * dftpav_planner_last_cost_terms: r_terms [Q][R][5] and r_rejected [Q][R] (query, restart) of the last dftpav_plan_queries call
 *   that ran with the filter on; zero rows for the queries no restart was solved for.  Either may be NULL (both: DFTPAV_E_INVALID).
 *   DFTPAV_E_INVALID when that call ran without the filter.
 * dftpav_debug_penalty_gate: test hook, the gate on caller-supplied terms [n][5] and flags_in [n]: rejected [n] by the rule above,
 *   flags_out [n] = (flags_in != 0) | rejected.  rejected may be NULL. */
typedef struct dftpav_penalty_caps { double corridor, surround, feasibility; } dftpav_penalty_caps; /* +inf: not judged */
int dftpav_planner_set_penalty_filter(dftpav_planner *p, const dftpav_penalty_caps *caps);
int dftpav_planner_last_cost_terms(dftpav_planner *p, double *r_terms, int *r_rejected);
int dftpav_debug_penalty_gate(dftpav_handle *h, int n, const double *terms, const dftpav_penalty_caps *caps, const int *flags_in,
                              int *flags_out, int *rejected);

/* ---- the distance field of the grid map, the clearance of solved plans, and a selection filter on it -------------------
 * The collision re-check answers yes or no; these calls say how close a plan comes to the map's occupied cells.
 *
 * The field.  For the map of dftpav_set_grid_map, cell (ix, iy) gets
 *   d2[ix + size_x * iy] = min over cells (jx, jy) with cells[jx + size_x * jy] == 80 of (ix - jx)^2 + (iy - jy)^2,
 * int32 in cell units, exact (an exact Euclidean distance transform, distfield.hip); DFTPAV_DIST_FAR everywhere on a map without
 * an occupied cell.  It belongs to the handle and is built lazily, on the handle's stream, by the first call of this section that
 * needs it after a dftpav_set_grid_map; that call itself launches nothing new and only marks the field stale, and a handle that
 * never asks for clearance never allocates or launches any of this.  A map with a side above 16384 cells is refused by every
 * call here with DFTPAV_E_UNSUPPORTED (every sum then fits in 32 bits).
 * dftpav_grid_distance_field: builds the field if the map changed and copies it to d2 [size_y][size_x]; d2 == NULL: build only.
 *
 * The clearance of a plan.  Samples: exactly those of dftpav_batch_validate and dftpav_batch_check_limits -- per gear segment
 * t = 0.0; t < duration; t += check_dt, from the tabulated running sum of dftpav_debug_validation_table, with the global sample
 * indices of `first_sample`; the pose as the re-check forms it (yaw from the correctly rounded atan2, then sincos).  Probe points:
 * exactly those of the re-check's CheckCollisionUsingPosAndYaw -- the dense vertices of the four edges of the outline at the
 * reference's own spacing 0.1 (shapes.h:200-201), then its four corners.  A point's value is d2 at round((p - origin) / resolution);
 * a point outside the grid is SKIPPED, consistent with "out of range counts as free".  Per trajectory:
 *   min_d2     the minimum over all probe points of all samples; DFTPAV_DIST_FAR if there is no sample, every probe is out of
 *              range, or the map has no occupied cell
 *   arg        the lowest global sample index at which min_d2 is reached; -1 when min_d2 is DFTPAV_DIST_FAR
 *   clearance  resolution * sqrt((double)min_d2), +inf for DFTPAV_DIST_FAR
 * The meaning is grid-quantised: distances are between CELL CENTRES -- the cell a probe point rounds to and the nearest occupied
 * cell -- so the real distance from the outline to occupied area differs from `clearance` by at most one cell diagonal
 * (resolution * sqrt(2)); and only the outline is probed, not the footprint's interior (the reference's check has no interior
 * probes either).  min_d2 == 0 holds exactly when the re-check with vertex_res 0.1 and the same check_dt reports a collision, and
 * arg is then its first_sample.
 * dftpav_batch_check_clearance: the B trajectories of a solved batch (or the coefficients of dftpav_debug_batch_set_coeffs).  Rows [B].
 * dftpav_planner_check_clearance: a row per slot of the executing table; empty slots (and every slot before the table was filled
 *   once) give DFTPAV_DIST_FAR, -1, +inf.  The table is not written.
 * dftpav_planner_set_clearance_filter: min_clearance < 0 (the default): dftpav_plan_queries and dftpav_replan_tick do exactly what
 *   they do without this call -- the same launches, the same bits.  Otherwise: per layout group the clearance kernel runs after
 *   the collision re-check (and after the limits kernel, when that filter is set) and before the terms launch / penalty gate; a
 *   restart is rejected unless clearance >= min_clearance, and the selection passes over a restart that collides or that any
 *   filter rejected.  A query whose every restart is rejected ends DFTPAV_PLAN_NO_VALID_RESTART (a tick then keeps the slot's old
 *   plan).  r_collision / r_first_sample of dftpav_plan_out stay the pure collision results.  min_clearance = 0.0 is legal and
 *   rejects nothing that does not already collide at the spacing 0.1.  The device buffers of the rows are allocated by this call.
 * dftpav_planner_last_clearance: the rows [Q][R] (query, restart) of the last dftpav_plan_queries call that ran with the filter
 *   on; DFTPAV_DIST_FAR, -1, +inf for the queries no restart was solved for.  DFTPAV_E_INVALID when that call ran without it.
 * dftpav_clearance_last_ms: device time in ms (the handle's HIP events) of the last field build (both passes) and of the last
 *   clearance kernel of one of the two check_clearance calls; 0.0 for what has not run.  Either pointer may be NULL.
 * Every pointer of dftpav_clearance_out may be NULL.  A refused call changes nothing and returns DFTPAV_E_INVALID: no grid map
 * installed, no solved coefficients, check_dt <= 0, NaN or infinite, out NULL, a min_clearance that is NaN or +inf. */
#define DFTPAV_DIST_FAR 2147483647
int dftpav_grid_distance_field(dftpav_handle *h, int *d2 /*[size_y][size_x] or NULL: build only*/);
typedef struct dftpav_clearance_out { int *min_d2; int *arg; double *clearance; } dftpav_clearance_out; /* [n], any may be NULL */
int dftpav_batch_check_clearance(dftpav_batch *b, double check_dt, const dftpav_clearance_out *out);
int dftpav_planner_check_clearance(dftpav_planner *p, double check_dt, const dftpav_clearance_out *out);
int dftpav_planner_set_clearance_filter(dftpav_planner *p, double min_clearance, double check_dt); /* min_clearance < 0: off (default) */
int dftpav_planner_last_clearance(dftpav_planner *p, const dftpav_clearance_out *out);            /* rows [Q][R] */
int dftpav_clearance_last_ms(dftpav_handle *h, float *field_ms, float *check_ms);

/* ---- the goal field of the grid map, and the obstacle-aware heuristic of the hybrid A* search -------------------------
 * The search steers by getHeu (kino_astar.h:221-226), tie_breaker * |p - goal|: the straight line, whatever stands in it.  The
 * reference carries the other term as a commented-out line, kino_astar.cpp:247,
 *   tmp_f_score = tmp_g_score + lambda_heu_ * getObsHeu(pro_state.head(2));
 * and no getObsHeu anywhere.  These calls supply it: the cost-to-go around the obstacles on the grid, as a maximum with getHeu.
 *
 * The field.  For a goal at (x, y), whose cell c* is round((p - origin) / resolution) as everywhere here, F[c] is the cost of
 * the cheapest 8-connected path between c and c* -- an axial step 5, a diagonal step 7 -- int32, integer arithmetic, exact
 * (goalfield.hip).  A cell is BLOCKED iff d2[c] <= T, d2 the distance field above and T = (int)floor(r * r / (resolution *
 * resolution)) for the inflation radius r >= 0 in metres (r = 0: exactly the occupied cells; a map without one: nothing).  The
 * field spreads from c*: a step enters a cell inside the grid that is not blocked, and a diagonal step needs both cells it passes
 * between not blocked as well (no corner cutting).  c* holds 0 whether it is blocked or not; a goal outside the grid seeds
 * nothing; a cell never reached holds DFTPAV_FIELD_UNREACHED.  The distance field is built lazily as by the clearance calls, and
 * a side above 16384 cells is refused likewise (7 * 16384^2 < 2^31).
 * dftpav_grid_goal_field: the fields of n goals (x, y) into field [n][size_y][size_x] and the number of cells with a value into
 *   n_reached [n]; either may be NULL.  Goals that share a cell share one build.
 *
 * The heuristic.  dftpav_set_search_heuristic keeps its state on the handle.  Off (the default; gp == NULL or enabled == 0):
 * dftpav_kino_search, dftpav_plan_queries and dftpav_replan_tick launch what they launch without this call and return the same
 * bits.  On: each of them builds, on the handle's stream in front of its search launches, one field per distinct goal cell of the
 * call (blocked by inflate_radius), into a workspace the handle owns -- 2 GiB of fields at most, more goals than that are built
 * and searched in turns -- and the search forms, for the start node and for every expanded input at (x, y),
 *   h = lambda_heu * fmax(tie_breaker * |p - goal|, (double)F[cell of (x, y)] * unit),   unit = scale * resolution / 5.0,
 * a point outside the grid or an unreached cell counting as F = 0.  The 3D search and its 2D retry use the same field;
 * stage_ms[0] of dftpav_planner_info then includes the builds.  The default scale 1 / sqrt(1.16): a 5 / 7 path in the direction
 * theta costs 5 (cos theta + 0.4 sin theta) per cell of Euclidean length, at most 5 sqrt(1.16), so with this scale the field's
 * term never exceeds the straight-line distance where nothing is in the way.  Nothing more is claimed about admissibility: the
 * detour round an obstacle is an 8-connected one, inflation blocks cells the vehicle may cross, and outside the grid the search
 * treats space as free while the field knows nothing of it.
 * dftpav_goal_field_last_ms: device time in ms of the field builds (the fills and the kernel) of the last call that built any.
 * DFTPAV_E_INVALID, and nothing changed: no grid map, a radius that is negative or not finite, a scale that is negative or not
 * finite, n < 0, goals_xy NULL with n > 0; dftpav_goal_field_last_ms before any build.  dftpav_set_grid_map invalidates nothing
 * here: the fields are built per call. */
#define DFTPAV_FIELD_UNREACHED 0x7fffffff
typedef struct dftpav_goal_field_params { int enabled; double inflate_radius; double scale; } dftpav_goal_field_params;
void dftpav_default_goal_field_params(dftpav_goal_field_params *gp); /* 0, 0.0, 1 / sqrt(1.16) */
int dftpav_set_search_heuristic(dftpav_handle *h, const dftpav_goal_field_params *gp); /* NULL or enabled == 0: off (default) */
int dftpav_grid_goal_field(dftpav_handle *h, const double *goals_xy /*[n][2]*/, int n, double inflate_radius,
                           int *field /*[n][size_y][size_x] or NULL*/, int *n_reached /*[n] or NULL*/);
int dftpav_goal_field_last_ms(dftpav_handle *h, float *ms);

/* ---- goal fields limited to a window round start and goal --------------------------------------------------------------
 * A whole-map field costs what the map costs, however short the query: on an arena of 1500 x 1500 cells one field is 9 MB and
 * tens of milliseconds.  These calls build the field of the part of the map a query can use, and the search reads that.
 *
 * The window rule.  dftpav_goal_window is pure host code and the only place a window is computed; of the map it reads the sizes,
 * the resolution and the origin (cells may be NULL).  In cells: the goal cell (gx, gy) = round((p - origin) / resolution), as
 * above; a goal outside the grid has no window and no field (returns 0, win = 0, 0, 0, 0).  The start cell (sx, sy) by the same
 * rounding, each coordinate then clamped into the grid (a start may lie outside it).  m = (int)ceil(margin / resolution);
 *   x0 = max(0, min(sx, gx) - m),  x1 = min(size_x - 1, max(sx, gx) + m),  y0 and y1 likewise;
 * the box is then snapped outwards to the field's tiles of 64 x 32 cells:
 *   X0 = x0 / 64 * 64,  X1 = min(size_x, (x1 / 64 + 1) * 64),  WX = X1 - X0;  Y0, Y1, WY likewise with 32,
 * so a window is a rectangle of the whole-map field's own tiles, and queries near each other share windows.  A margin that
 * covers the grid gives (0, 0, size_x, size_y).  Returns 1 with win = (X0, Y0, WX, WY); DFTPAV_E_INVALID for a NULL pointer,
 * a side < 1, a resolution that is not positive and finite, an origin that is not finite, a margin that is negative or not finite.
 *
 * The windowed field is the field above of the CROPPED map, stored [WY][WX]: inside the window every rule is unchanged -- the
 * seed, the step costs 5 and 7, no corner cutting -- and a cell outside the window is what a cell outside the grid is: never
 * entered, never written.  Blocked is still d2[c] <= T with d2 the distance field of the WHOLE map at the cell's grid
 * coordinates, so an obstacle just outside the window inflates into it.  A cell whose only way to the goal leaves the window
 * holds DFTPAV_FIELD_UNREACHED; every other value is >= the whole-map field's, the cost of a path that also exists there.
 * dftpav_grid_goal_field_windowed: the windowed fields of n (start, goal) pairs, margin >= 0.  windows [n][4] and offsets [n]
 *   (either may be NULL) are written first: query q's rows [WY][WX] start at field + offsets[q], the queries packed in order
 *   (offsets[q + 1] = offsets[q] + WX * WY of q); with field == NULL and n_reached == NULL nothing is built, so a first call
 *   sizes the buffer.  A goal outside the grid has window (0, 0, 0, 0), no rows, and n_reached 0.  Pairs that share goal cell
 *   and window share one build.
 *
 * The heuristic.  dftpav_set_search_heuristic_window keeps a margin on the handle, beside and independent of
 * dftpav_set_search_heuristic's state: margin < 0 is off (the default), and then -- or while that heuristic is off -- every call
 * launches what it launched without this one and returns the same bits.  With both on, dftpav_kino_search, dftpav_plan_queries
 * and dftpav_replan_tick build one field per distinct (goal cell, window) of a turn, the window of each query's own start and
 * goal; the turns are sized by the call's largest window, not by the map (the 2 GiB cap stays); and the field's term of h at
 * (x, y) is read at (cx - X0) + WX * (cy - Y0), a point outside the window counting as F = 0 like a point outside the grid.
 * Not claimed: the window can cut off the only detour -- then the start's cell is unreached, the term is 0 there and the search
 * is the plain one; inside the window the field is an upper bound of the whole-map field; and still nothing about admissibility.
 * DFTPAV_E_INVALID, and nothing changed: a NULL handle, no grid map, a margin that is NaN or +inf (dftpav_grid_goal_field_windowed:
 * negative or not finite), a radius that is negative or not finite, n < 0, starts_xy or goals_xy NULL with n > 0. */
int dftpav_goal_window(const dftpav_grid_map *map_geometry, const double *start_xy /*[2]*/, const double *goal_xy /*[2]*/, double margin,
                       int *win /*[4]: X0, Y0, WX, WY*/); /* 1: a window; 0: the goal is outside the grid (no field); < 0: error */
int dftpav_set_search_heuristic_window(dftpav_handle *h, double margin); /* margin < 0: off (default), whole-map fields as before */
int dftpav_grid_goal_field_windowed(dftpav_handle *h, const double *starts_xy /*[n][2]*/, const double *goals_xy /*[n][2]*/, int n,
                                    double inflate_radius, double margin, int *windows /*[n][4] or NULL*/,
                                    long long *offsets /*[n] or NULL*/, int *field /*packed, or NULL*/, int *n_reached /*[n] or NULL*/);

/* ---- the Reeds-Shepp cost-to-go table, and the non-holonomic term of the hybrid A* heuristic ----------------------------
 * getHeu and the goal field above know positions only: neither knows that the vehicle cannot turn on the spot, nor that the goal
 * has a heading.  This is the other half of the usual pair (Dolgov et al.): the length of the shortest Reeds-Shepp path to the
 * goal, without obstacles, from a table.  It depends on the turning radius and the table's geometry only -- not on the map, not
 * on the goal's position -- so a handle builds it once and the search reads one double per heuristic.
 *
 * The table.  rho = 1 / max_frontend_cur of the search parameters in force (the rho of the shot); half = (int)ceil(extent /
 * cell), n = 2 half + 1, dth = 2 pi / (double)n_yaw.  T is double [n_yaw][n][n]:
 *   T[k][j][i] = rho * (normalised length of the shortest Reeds-Shepp path from ((i - half) cell, (j - half) cell, k dth) to
 *   (0, 0, 0)),
 * the expression the search forms for the length of its shot, by the same solver (rs_math.h; rstable.hip), fp64.  The handle owns
 * it, keyed by (rho, n_yaw, extent, cell): built on the handle's stream in front of the first search launch that needs it (or by
 * dftpav_rs_table), kept, and rebuilt only when a call asks for another key.  A handle holds one table.
 *
 * The heuristic.  dftpav_set_search_rs_heuristic keeps its state on the handle, beside and independent of
 * dftpav_set_search_heuristic; it needs no map.  Off (the default; gp == NULL or enabled == 0): dftpav_kino_search,
 * dftpav_plan_queries and dftpav_replan_tick launch what they launch without this call and return the same bits.  On: with c =
 * cos(goal yaw), s = sin(goal yaw) (correctly rounded), a state (x, y, yaw) has, in the goal's frame,
 *   lx = c (x - gx) + s (y - gy),  ly = c (y - gy) - s (x - gx),  fi = round(lx / cell) + half,  fj = round(ly / cell) + half,
 *   k = (int)round((yaw - goal yaw) / dth) reduced into [0, n_yaw) by integer remainder,
 * the term is scale * T[k][fj][fi] where 0 <= fi < n and 0 <= fj < n, and 0 elsewhere, and the search forms, for the start node
 * and for every expanded input,
 *   h = lambda_heu * fmax(fmax(tie_breaker * |p - goal|, the goal field's term if that heuristic is on), the table's term).
 * The 3D search and its 2D retry read the same table.  Not claimed: the table is obstacle-free; it is read at the nearest cell
 * and heading, so it is not a lower bound of the state's own Reeds-Shepp distance and no admissibility is claimed; beyond the
 * extent the term is 0.
 * dftpav_rs_table: builds (if the handle does not hold it) and reads out the table of rho = 1 / max_cur and gp's geometry,
 *   whether or not the heuristic is on (gp->enabled is not read); dims = (n_yaw, n, n); out == NULL: dims only, nothing built.
 * dftpav_rs_table_last_ms: device time in ms of the handle's last table build, and (n_builds, may be NULL) how many tables the
 *   handle has built in its life.
 * DFTPAV_E_INVALID, and nothing changed: a NULL handle (or gp, for dftpav_rs_table), n_yaw < 1, cell <= 0, extent < 0, scale < 0,
 * any of them not finite, max_cur not positive and finite; dftpav_rs_table_last_ms before any build.  DFTPAV_E_UNSUPPORTED, and
 * nothing changed: a table above 256 MiB (n_yaw * n * n * 8 bytes). */
typedef struct dftpav_rs_heuristic_params { int enabled; int n_yaw; double extent; double cell; double scale; } dftpav_rs_heuristic_params;
void dftpav_default_rs_heuristic_params(dftpav_rs_heuristic_params *gp); /* 0, 72, 15.0 (kino_astar.cpp:91), 0.25, 1.0 */
int dftpav_set_search_rs_heuristic(dftpav_handle *h, const dftpav_rs_heuristic_params *gp); /* NULL or enabled == 0: off (default) */
int dftpav_rs_table(dftpav_handle *h, double max_cur, const dftpav_rs_heuristic_params *gp, double *out /*[n_yaw][n][n] or NULL*/,
                    int *dims /*[3] or NULL*/);
int dftpav_rs_table_last_ms(dftpav_handle *h, float *ms, int *n_builds /* or NULL */);

/* ---- footprint conflicts between the executing plans, slot against slot ------------------------------------------------
 * Every other check of the executing table looks at one slot at a time.  This one relates two: do the vehicles of two slots come
 * within `margin` of one another at the same clock, when first, and who with.  A read-out beside limits and clearance (conflict.hip);
 * nothing of it feeds the solve.  What the tick does about two plans that meet is the conflict trigger's (below).  No grid map is
 * needed.
 *
 * The clocks.  t_k = t0 + (double)k * dt, k = 0 .. K - 1: absolute, on the clock of the table's start_time / end_time.
 *
 * The pose of an occupied slot at clock t: the vehicle as the publisher would drive it, held still outside its plan.
 *   segment e   the first i in [0, n_seg) with !(end_time[i] <= t), else n_seg - 1 (exe_traj_index_ derived from the clock as
 *               dftpav_replan_check derives it, traj_server_ros.cpp:248-252)
 *   local time  tt = t - start_time[e]; tt < 0 becomes 0; tt > duration[e] becomes duration[e]
 *   position    Trajectory::getPos(tt) of segment e (locatePieceIdx's subtraction walk, Piece::getPos)
 *   heading     Trajectory::getAngle(tt) = atan2(singul * sigma'_y, singul * sigma'_x), correctly rounded; cs, sn its cosine and sine
 *   footprint   the oriented box of the collision re-check (semantic_map_manager.cc:645-646, shapes.cc:110-149): centre
 *               c = pos + veh_d_cr * (cs, sn) and the four corners c +- 0.5 veh_length (cs, sn) +- 0.5 veh_width (sn, -cs), in the
 *               re-check's expressions and corner order; veh_width, veh_length, veh_d_cr are the handle's parameters.
 *
 * The separation of two occupied slots i != j at sample k, fp64 without contraction:
 *   1. broad phase: dx = cx_i - cx_j, dy = cy_i - cy_j, d2 = dx * dx + dy * dy; R = range + 2.0 * rad with rad = sqrt(0.25 * L * L +
 *      0.25 * W * W), L = veh_length, W = veh_width.  The pair-sample contributes NOTHING when !(d2 <= R * R).  This is part of
 *      the definition, not an optimisation: a pair further apart than that is not reported even to a slot with no nearer
 *      partner, and a pose that is not finite contributes nothing.
 *   2. overlap: the separating-axis test on the four axes, (cs, sn) and (-sn, cs) of both boxes.  For the axis owner A the other
 *      box's four corners p are taken into A's frame, lx = cs * (px - cx) + sn * (py - cy), ly = cs * (py - cy) - sn * (px - cx);
 *      A's x axis separates when all four lx > L / 2 or all four lx < -L / 2, its y axis likewise with ly and W / 2.  No axis
 *      separates: sep = 0.0.
 *   3. otherwise sep = sqrt(m), m the minimum of the 32 squared point-to-segment distances, each box's four corners p against the
 *      other's four edges a -> b (corner 1 -> 2 -> 3 -> 4 -> 1): u = ((p - a) . (b - a)) / ((b - a) . (b - a)), clamped to [0, 1]
 *      (!(u > 0) gives 0), q = a + u * (b - a), e = p - q, and the distance is ex * ex + ey * ey.
 *   4. sep(i, j, k) and sep(j, i, k) are the SAME BITS: dx and dy are only squared, and steps 2 and 3 are conjunctions and minima
 *      over one set of values whichever box is named first.
 *
 * Per slot i, each a lexicographic minimum, so no order of reduction shows:
 *   min_sep, sep_sample, sep_partner     the minimum of (sep, k, j) over all contributing pair-samples
 *   conflict_sample, conflict_partner    the minimum of (k, j) over the pair-samples with sep <= margin (an overlap always
 *                                        conflicts; margin = 0 is legal)
 * An empty slot, a slot with nothing inside the broad phase, and every slot before the table was filled once give +inf, -1, -1,
 * -1, -1.  Neither the table nor the publisher's state is written.
 *
 * dftpav_planner_check_conflicts(p, t0, dt, K, margin, range, out): the five rows [max_queries]; any pointer of out may be NULL.
 * dftpav_planner_sample_poses(p, t0, dt, K, poses): the pose half alone, poses [K][max_queries][4] = cx, cy, cs, sn; NaN rows for
 *   empty slots (and for every slot before the table was filled once).
 * dftpav_conflicts_last_ms: device time in ms (the handle's HIP events) of the pose kernel and of the pair and reduce kernels
 *   together, of the last of the two calls above; 0.0 for what has not run.  Either pointer may be NULL.
 * DFTPAV_E_INVALID, and nothing changed: p, out or poses NULL; K < 1 or K > DFTPAV_CONFLICT_MAX_SAMPLES; dt <= 0 or not finite;
 * t0 not finite; margin < 0 or NaN; range < margin or not finite (so a margin of +inf is refused with every range).
 *
 * Not claimed.  The heading is getAngle's: a plan sampled exactly at rest has the heading atan2(0, 0) = 0, as in the collision
 * re-check.  Between samples nothing is tested: choose dt against margin and the speed limit (two vehicles closing at 2 v_max move
 * 2 v_max dt between clocks).  Every slot is the handle's one vehicle size.  The moving obstacles of dftpav_set_surround take no
 * part. */
#define DFTPAV_CONFLICT_MAX_SAMPLES 4096 /* the cap on K, as the publisher's (the poses are 32 K * slots bytes of device memory) */
typedef struct dftpav_conflict_out {
  double *min_sep;                                                      /* [max_queries] */
  int *sep_sample, *sep_partner, *conflict_sample, *conflict_partner;   /* [max_queries] */
} dftpav_conflict_out; /* any may be NULL */
int dftpav_planner_check_conflicts(dftpav_planner *p, double t0, double dt, int K, double margin, double range, const dftpav_conflict_out *out);
int dftpav_planner_sample_poses(dftpav_planner *p, double t0, double dt, int K, double *poses /*[K][max_queries][4]*/);
int dftpav_conflicts_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms);

/* ---- footprint conflicts of candidate plans against the executing table, and the conflict filter ---------------------------
 * The check above relates the plans that execute.  This one relates plans that do not execute yet -- the trajectories of a batch --
 * to those that do, and as a selection filter of dftpav_plan_queries it feeds back: a restart that would drive through the vehicle
 * of another slot cannot win (cand_conflict.hip).  No grid map is needed by the read-outs.
 *
 * A candidate is trajectory c of a batch b: the batch's layout, its piece coefficients and piece durations as dftpav_batch_coeffs
 * returns them, and an absolute start clock t_start.
 *
 * The clocks.  t_k = t0 + (double)k * dt, k < K <= DFTPAV_CONFLICT_MAX_SAMPLES, as above.
 *
 * The pose of a candidate at clock t is the pose its slot would have after dftpav_planner_adopt(..., t_start): the segment times
 * are chained as the adoption chains them -- world = t_start; for every segment d = its piece duration summed piece by piece
 * (Trajectory::getTotalDuration), start_time = world, end_time = world + d, and the next segment starts at that end -- and segment,
 * local time, clamping, position, heading and box centre follow the statements of the pose above.  The candidate is held still before
 * t_start and after its last end_time.  The pose of a slot is the pose above, unchanged.
 *
 * The separation of candidate c and occupied slot j != own[c] at sample k is steps 1 to 3 above in the same expressions: the broad
 * phase on the centres with R = range + 2.0 * rad, the separating-axis test, the 32 corner-to-edge distances.  own[c] is the slot
 * the candidate would replace, or -1 if it replaces none: that slot takes no part.  An empty slot contributes nothing; so does a
 * pose that is not finite on either side.
 *
 * Per candidate, the lexicographic rules above:
 *   min_sep, sep_sample, sep_partner     the minimum of (sep, k, j)
 *   conflict_sample, conflict_partner    the minimum of (k, j) over sep <= margin (a negative margin: never)
 * A candidate that nothing contributed to, a candidate no kernel visits, and every candidate before the table was filled once give
 * +inf, -1, -1, -1, -1.  Nothing of the table, the publisher's state or the batch is written.
 *
 * dftpav_batch_check_conflicts(b, p, t_start, t0, dt, K, margin, range, own, out): the five rows [B] of the batch's B trajectories,
 *   on a solved batch (or the coefficients of dftpav_debug_batch_set_coeffs); own [B] or NULL for none; any pointer of out may be NULL.
 * dftpav_batch_sample_poses(b, t_start, t0, dt, K, poses): the candidates' poses alone, poses [K][B][4] = cx, cy, cs, sn.
 * dftpav_batch_conflicts_last_ms: device time in ms (the handle's HIP events) of the last of the two calls above: the pose kernel (of
 *   the table for the check, of the candidates for the poses) and the pair kernel; 0.0 for what has not run.
 *
 * The filter.  dftpav_planner_set_conflict_filter(p, margin, range, dt, K): margin < 0 is off (the default).  On, every restart of
 * a dftpav_plan_queries call is a candidate with t_start = t0 = the call's t_now (in dftpav_replan_tick: t_now + budget, the
 * adoption clock), tested per layout group after the collision re-check against the table's poses, which are evaluated once per
 * call; a restart with conflict_sample >= 0 is rejected beside the other filters' rejections, and a query whose every restart is
 * rejected ends DFTPAV_PLAN_NO_VALID_RESTART, so a tick keeps the old plan.  With a table never filled, or all empty, nothing is
 * rejected.  Off, a call allocates, clears and launches nothing of it and returns the same bits as before.
 * dftpav_planner_set_own_slots(p, own, Q): the own slots [Q] (-1: none) of the queries of the NEXT dftpav_plan_queries call only,
 *   which must bring Q queries (else DFTPAV_E_INVALID); that call consumes them, and the default is none.  dftpav_replan_tick sets
 *   them itself to its query_slot: a slot that replans is not in conflict with the plan it replaces.
 * dftpav_planner_last_conflicts(p, out): the rows [Q][n_restarts] of the last dftpav_plan_queries call, if it ran with the filter;
 *   otherwise DFTPAV_E_INVALID.
 *
 * DFTPAV_E_INVALID, and nothing changed, decided before the handle is touched: a NULL b, p, out or poses; b and p on different
 * handles; batch coefficients not available (nothing solved or set); K < 1 or K > DFTPAV_CONFLICT_MAX_SAMPLES; dt <= 0 or not finite;
 * t0 or t_start not finite; margin NaN; range < margin or not finite; an own entry outside [-1, max_queries).
 *
 * Not claimed.  Candidates of the same call are not tested against each other unless joint selection is on (below).  A slot that
 * replans in the same tick is tested as its old plan.  Between samples nothing is tested.  There is one vehicle size.  The moving
 * obstacles of dftpav_set_surround take no part.  What starts a replanning when two executing plans meet is the conflict trigger of
 * dftpav_replan_tick (below): the filter only rejects, and the search and the corridor of the slot that yields do not see the other
 * vehicle. */
int dftpav_batch_check_conflicts(dftpav_batch *b, dftpav_planner *p, double t_start, double t0, double dt, int K, double margin,
                                 double range, const int *own /*[B] or NULL = none*/, const dftpav_conflict_out *out /*rows [B]*/);
int dftpav_batch_sample_poses(dftpav_batch *b, double t_start, double t0, double dt, int K, double *poses /*[K][B][4]*/);
int dftpav_batch_conflicts_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms);
int dftpav_planner_set_conflict_filter(dftpav_planner *p, double margin, double range, double dt, int K); /* margin < 0: off (default) */
int dftpav_planner_set_own_slots(dftpav_planner *p, const int *own /*[Q]*/, int Q);
int dftpav_planner_last_conflicts(dftpav_planner *p, const dftpav_conflict_out *out /*rows [Q][n_restarts]*/);

/* ---- joint selection: the candidate plans of one call tested against each other ------------------------------------------
 * The conflict filter tests a candidate against the plans that execute.  When two queries of one call replan, each new plan is
 * tested against the other's OLD plan only, and both winners may cross at the same clock.  Joint selection closes that hole: it
 * is an option of the conflict filter (joint_select.hip) and uses the filter's margin, range, dt, K, its clocks
 * t_k = t_call + (double)k * dt, and its candidate pose: the pose after an adoption at t_start = t_call, held still before and
 * after.  Take a call of Q queries with R restarts each.
 *
 *   priority        the call's query order: query q' has priority over q when q' < q.  In dftpav_replan_tick this is the order of
 *                   the tick's query list.
 *   eligible(q, r)  the selection's test: succeeded, not colliding, no reject flag from the limit / clearance / penalty / conflict
 *                   filters, and a cost that is not NaN.  A query outside every layout group (no path, arrived, an unsupported
 *                   layout) has no eligible restart; neither has a query with a restart below mini_T (no plan is reported for it,
 *                   so it blocks nobody).
 *   conf(a, b)      for two candidates a = (q, r), b = (q', r') with q != q': there is a k < K with sep_k(a, b) <= margin.  sep_k is
 *                   steps 1 to 3 of the conflict check in the same expressions: the broad phase on the centres against
 *                   range + 2.0 * rad, the separating-axis test, the 32 corner-to-edge distances.  A pair outside the broad phase
 *                   contributes nothing; so does a pose that is not finite on either side.
 *   for q = 0, 1, ..., Q - 1 in turn:
 *     blocked(q, r) holds when a q' < q with a winner w(q') >= 0 exists and conf((q, r), (q', w(q'))).
 *     w(q)          the cheapest restart that is eligible and not blocked; ties go to the lowest r; -1 if there is none.
 *     Only WINNERS block: a rejected or dearer restart of q' blocks nobody.
 *   rows            per candidate (q, r), by the lexicographic rules above; the partners are the winners (q', w(q')) with q' < q and
 *                   the partner index is the QUERY index q':
 *                     min_sep, sep_sample, sep_partner     the minimum of (sep, k, q')
 *                     conflict_sample, conflict_partner    the minimum of (k, q') over sep <= margin
 *                   +inf, -1, -1, -1, -1 where nothing contributed.  blocked(q, r) == (conflict_sample >= 0), and both are reported.
 *   effect          a blocked restart gets the call's reject flag; the selection then runs unchanged and arrives at w(q).  With
 *                   joint selection on, the per-group selections run behind the joint stage, which runs once after the last
 *                   group.  A query with every restart blocked ends DFTPAV_PLAN_NO_VALID_RESTART, so a tick keeps its old plan.
 *   The table test stays as it is: a candidate is still tested against the old plan of every other occupied slot, replanning or
 *   not.  This is conservative: the other slot may fail to replan and keep that plan.
 *
 * Off by default.  Off, or with the conflict filter off, a call allocates, clears and launches nothing of it; the order of launches
 * and every returned bit are those of a planner without it.
 *
 * dftpav_planner_set_joint_selection(p, on): on is 0 or 1 (else DFTPAV_E_INVALID).  It makes its one allocation here (poses,
 *   conflict bits, rows), sized by max_queries * n_restarts and the filter's K, and reallocates when the filter is configured with a
 *   larger K.  Two design bounds: max_queries * n_restarts <= DFTPAV_JOINT_MAX_CANDIDATES (the conflict bits are then 8 MiB), and
 *   candidates x K <= 2^22 (128 MiB of poses).  Beyond either it refuses with DFTPAV_E_UNSUPPORTED and changes nothing; so does
 *   dftpav_planner_set_conflict_filter when, with joint selection on, its K would pass the second bound.
 * dftpav_planner_last_joint(p, out, blocked): the rows [Q][n_restarts] and blocked [Q][n_restarts] (or NULL) of the last
 *   dftpav_plan_queries call, if it ran with joint selection (and so with the conflict filter); otherwise DFTPAV_E_INVALID.
 * dftpav_joint_last_ms(h, pose_ms, pair_ms, select_ms): device time in ms (the handle's HIP events) of the pose kernels, of the pair
 *   kernel, and of the greedy and row kernels, of the last such call or dftpav_debug_joint_select (which runs no pose kernel); 0.0
 *   for what has not run.  Any pointer may be NULL.
 * dftpav_debug_joint_select (test hook): the pair, greedy and row kernels on caller-given poses [K][Q * R][4] = cx, cy, cs, sn, cost
 *   [Q * R] and eligible [Q * R] (0 / not 0), with the handle's vehicle size.  winner [Q], blocked [Q * R], out (rows [Q * R]) and
 *   every pointer of out may be NULL.  DFTPAV_E_INVALID, and nothing written: h, poses, cost or eligible NULL; Q < 1 or R < 1; K < 1
 *   or K > DFTPAV_CONFLICT_MAX_SAMPLES; margin NaN; range < margin or not finite.  DFTPAV_E_UNSUPPORTED, and nothing written, beyond
 *   the two design bounds.
 *
 * Not claimed.  Priorities other than call order.  No excusing of a replanning slot's old plan.  Nothing between samples.  One
 * vehicle size.  Greedy, not jointly optimal: a lower-priority query can end without a plan where a different choice for a higher
 * one would have served both. */
#define DFTPAV_JOINT_MAX_CANDIDATES 8192 /* the cap on max_queries * n_restarts of joint selection */
int dftpav_planner_set_joint_selection(dftpav_planner *p, int on); /* off by default */
int dftpav_planner_last_joint(dftpav_planner *p, const dftpav_conflict_out *out /*rows [Q][n_restarts]*/,
                              int *blocked /*[Q][n_restarts] or NULL*/);
int dftpav_joint_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms, float *select_ms);
int dftpav_debug_joint_select(dftpav_handle *h, int Q, int R, int K, const double *poses /*[K][Q*R][4]*/, const double *cost /*[Q*R]*/,
                              const int *eligible /*[Q*R]*/, double margin, double range, int *winner /*[Q]*/, int *blocked /*[Q*R]*/,
                              const dftpav_conflict_out *out /*rows [Q*R]*/);

/* ---- the conflict trigger: two executing plans that meet, and the slot without precedence replans ------------------------
 * The conflict check relates two executing plans, the conflict filter keeps a new plan away from those that execute, joint selection
 * keeps the new plans of one call apart.  None of them starts anything: dftpav_replan_tick flags a slot for the near / target rule,
 * a collision with the map, or an empty slot with an ego state.  With the trigger on the tick itself finds the pairs of executing
 * plans that conflict at the adoption clock, decides by a fixed precedence which slot gives way, and replans that slot in the same
 * call (conflict_trigger.hip).  Off, which is the default, nothing changes.
 *
 * Everything not named here is the definition of the conflict check above, in the same expressions: the clocks
 * t_k = t0 + (double)k * dt, k < K <= DFTPAV_CONFLICT_MAX_SAMPLES; the pose of an occupied slot, held still outside its plan; steps 1 to
 * 3 of the separation (the broad phase on the centres against range + 2.0 * rad, the separating-axis test, the 32 corner-to-edge
 * distances); a pair outside the broad phase, or with a pose that is not finite, contributes nothing.
 *
 *   can_yield(s)     the slot holds a plan and !(t_now > end_time[n_seg - 1]): the completion test of dftpav_replan_check
 *                    (traj_server_ros.cpp:150), read from the table's row.  A completed slot stands where its plan ended and the tick
 *                    plans nothing for it.  It cannot give way, so whoever meets it must.
 *   precedes(j, i)   for occupied i != j: !can_yield(j) || j < i.  A lower slot index is a higher priority: the order of the tick's
 *                    query list, and therefore the priority joint selection uses.
 *   per occupied i   yield_sample, yield_partner: the lexicographic minimum of (k, j) over the pair-samples with
 *                    sep(i, j, k) <= margin and precedes(j, i); -1, -1 when there is none.
 *                    yield = can_yield(i) && yield_sample >= 0.
 *   Empty slots, and every slot before the table was filled once, give 0, -1, -1.
 * The rows are existential and lexicographic, so no order of reduction shows; every output is an integer.  With every slot able to
 * yield, slot 0 never yields and the highest slot of a conflicting set always does.  When every conflicting partner of a slot
 * precedes it, its (yield_sample, yield_partner) are the (conflict_sample, conflict_partner) of dftpav_planner_check_conflicts at the
 * same arguments.
 *
 * dftpav_planner_check_yield(p, t_now, t0, dt, K, margin, range, out): a read-out: the three rows [max_queries]; any pointer of out
 *   may be NULL.  Nothing of the table, of the publisher's state or of the check's buffers is written.  No grid map is needed.
 * dftpav_planner_set_conflict_trigger(p, margin, range, dt, K): margin < 0 is off (the default).  The trigger makes its one
 *   allocation here (the table's poses 4 x [K][slots rounded up to 64], the partial rows, the rows); a tick allocates nothing.  The
 *   parameters are the trigger's own, not the filter's: a trigger margin ABOVE the filter's margin makes a plan that has just passed
 *   the filter trigger again on the next tick, so keep the trigger's margin at or below the filter's.
 * In dftpav_replan_tick, with the trigger on: behind the check and on the same stream the poses of the table are taken at
 *   t0 = t_now + budget -- the adoption clock and the clock of the filter's candidates; nothing before it can still be changed -- and
 *   the trigger's kernels follow with the tick's t_now.  yield [slots] joins the tick's read-back in front of its one wait; no second
 *   wait is added.  A slot becomes a query when replan || yield, in rising slot order.  A yielding slot has a start state (the check
 *   writes start_state and start_ctrl for every occupied, uncompleted slot whether or not it flagged it); its goal is end_states' row,
 *   or the stored one.  The replan row of check_out stays the check's own flag: the caller tells a yield from query_slot and
 *   dftpav_planner_last_trigger.  Own slots, planning, adoption, history and "a failed replanning keeps the old plan" are the
 *   tick's, unchanged.  With the trigger off the tick enqueues, copies and returns exactly what it did without this section.
 * dftpav_planner_last_trigger(p, out): the rows of the last dftpav_replan_tick, if it ran with the trigger; otherwise
 *   DFTPAV_E_INVALID.
 * dftpav_trigger_last_ms(h, pose_ms, pair_ms): device time in ms (the handle's HIP events) of the pose kernel and of the pair and
 *   reduce kernels together, of the last read-out, tick with the trigger, or dftpav_debug_conflict_trigger (which runs no pose kernel:
 *   0.0); 0.0 for what has not run.  Either pointer may be NULL.
 * dftpav_debug_conflict_trigger (test hook): the pair and reduce kernels on caller-given poses [K][S][4] = cx, cy, cs, sn and
 *   can_yield [S] (0 / not 0), with the handle's vehicle size; no pose kernel, no planner.  A slot whose row at k = 0 has a component
 *   that is not finite is an empty slot (it cannot yield, whatever its flag); a later row of an occupied slot that is not finite
 *   contributes nothing.  out and every pointer of it may be NULL.
 * DFTPAV_E_INVALID, and nothing changed, decided before the handle is touched: p, h, out, poses or can_yield NULL; S < 1; K < 1 or
 * K > DFTPAV_CONFLICT_MAX_SAMPLES; dt <= 0 or not finite; t0 or t_now not finite; margin < 0 or NaN (dftpav_planner_set_conflict_trigger:
 * NaN; < 0 is off); range < margin or not finite.
 *
 * Not claimed.  Between samples nothing is tested.  There is one vehicle size.  The moving obstacles of dftpav_set_surround take no
 * part.  Precedence is by slot index only.  The search and the corridor of the slot that yields do not see the other vehicle: only
 * the conflict filter rejects, so a yielder may end DFTPAV_PLAN_NO_VALID_RESTART every tick and keep its plan (with the filter off
 * it may adopt a plan that conflicts again).  dftpav_planner_stamp_slots (below) remains the way to make parked vehicles visible to
 * the search. */
typedef struct dftpav_yield_out {
  int *yield, *yield_sample, *yield_partner; /* [max_queries] */
} dftpav_yield_out; /* any may be NULL */
int dftpav_planner_check_yield(dftpav_planner *p, double t_now, double t0, double dt, int K, double margin, double range,
                               const dftpav_yield_out *out);
int dftpav_planner_set_conflict_trigger(dftpav_planner *p, double margin, double range, double dt, int K); /* margin < 0: off (default) */
int dftpav_planner_last_trigger(dftpav_planner *p, const dftpav_yield_out *out);
int dftpav_trigger_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms);
int dftpav_debug_conflict_trigger(dftpav_handle *h, int S, int K, const double *poses /*[K][S][4]*/, const int *can_yield /*[S]*/,
                                  double margin, double range, const dftpav_yield_out *out /*rows [S]*/);

/* ---- the stamps: vehicle footprints written into the grid map on the device -------------------------------------------
 * Every stage that plans or checks a plan (search, goal field, rectangle corridor, collision re-check, replan check, distance
 * field, clearance) looks at the occupancy grid of dftpav_set_grid_map alone.  A stamp makes cells of that grid occupied where a
 * vehicle is or will be, so that a plan made afterwards goes round it: stamp what has right of way, plan the rest, clear.  Off until
 * called: a handle that never stamped launches, allocates and computes what it did without this section (stamp.hip).
 *
 * A box is (cx, cy, cs, sn): the centre, cosine and sine of a row of dftpav_planner_sample_poses.  L, W are the handle's veh_length,
 * veh_width.  All arithmetic is fp64 without contraction.
 *   cell (ix, iy) has the centre   X = origin_x + (double)ix * resolution, Y = origin_y + (double)iy * resolution
 *   dx = X - cx, dy = Y - cy
 *   lx = cs * dx + sn * dy, ly = cs * dy - sn * dx          (the frame of the conflict check's step 2)
 *   hl = 0.5 * L + inflate, hw = 0.5 * W + inflate
 *   the box COVERS the cell iff fabs(lx) <= hl && fabs(ly) <= hw
 *   a box with a member that is not finite covers nothing
 *   a covered cell of the working map becomes 80
 * This is defined over all cells of the grid; what range of cells the device walks does not show.  inflate >= 0, finite.  With
 * inflate >= resolution / sqrt(2) every cell that the collision re-check can name for a point of the uninflated box (coord =
 * round((p - origin) / resolution): at most half a cell from p on either axis) is covered.
 *
 * State.  The map every call reads is the WORKING map.  The first stamp after a dftpav_set_grid_map keeps a BASE copy of the map as
 * uploaded; stamps accumulate in the working map until dftpav_grid_clear_stamps puts the base back (stamping a box twice changes
 * nothing).  Maps of up to 327 680 cells have a bit map beside the bytes (the rectangle corridor reads it): a stamp sets the same
 * bits, a clear makes them again from the bytes.  Every stamp and every clear marks the distance field stale, so the next call that
 * needs it builds it again.  dftpav_set_grid_map drops base and stamps.  Nothing else of a handle keeps state derived from the map
 * from one call to the next.
 *
 * dftpav_grid_stamp_poses(h, poses, n, inflate): n boxes from the host; n == 0 does nothing.
 * dftpav_planner_stamp_slots(p, select, t0, dt, K, inflate): the swept footprint of the selected slots of p's executing table, the
 *   boxes being the poses of dftpav_planner_sample_poses(p, t0, dt, K) on the device: t_k = t0 + (double)k * dt, held still outside
 *   the plan.  select [max_queries], 0: the slot stamps nothing; NULL: every occupied slot.  Empty slots stamp nothing.  K = 1 is
 *   "the vehicle where it stands at t0".  Neither the table nor the publisher's state is written.
 * dftpav_grid_clear_stamps(h): the working map is the base again, bytes other than 0 and 80 included; OK where nothing was stamped.
 * dftpav_grid_read_cells(h, cells, n_stamped): the working map [size_y][size_x], and the number of cells that are 80 in it and not
 *   80 in the base (0 where nothing was stamped); either pointer may be NULL.
 * dftpav_stamp_last_ms(h, pose_ms, stamp_ms): device time in ms (the handle's HIP events) of the pose kernel and of the box kernel
 *   of the last stamp call; pose_ms is 0.0 after dftpav_grid_stamp_poses, both before the first stamp.  Either pointer may be NULL.
 * All work goes on the handle's stream.  dftpav_planner_stamp_slots and dftpav_grid_clear_stamps return without a wait for it;
 * dftpav_grid_stamp_poses (its boxes come from the host) and dftpav_grid_read_cells end with one.
 * DFTPAV_E_INVALID, and nothing changed: h, p or poses NULL; no map; n < 0; K < 1 or K > DFTPAV_CONFLICT_MAX_SAMPLES; dt <= 0 or not
 * finite; t0 not finite; inflate < 0 or not finite; a planner whose table was never filled.
 *
 * Not claimed.  Between clocks nothing is stamped: choose dt against the speed and the inflation.  A slot stamped into the map is an
 * obstacle to every later check, the replan check of that slot itself included; select the slots that have right of way.  Every
 * box is the handle's one vehicle size. */
int dftpav_grid_stamp_poses(dftpav_handle *h, const double *poses /*[n][4] cx, cy, cs, sn*/, int n, double inflate);
int dftpav_planner_stamp_slots(dftpav_planner *p, const unsigned char *select /*[max_queries] or NULL: every occupied slot*/, double t0,
                               double dt, int K, double inflate);
int dftpav_grid_clear_stamps(dftpav_handle *h);
int dftpav_grid_read_cells(dftpav_handle *h, unsigned char *cells /*[size_y][size_x] or NULL*/, int *n_stamped /*or NULL*/);
int dftpav_stamp_last_ms(dftpav_handle *h, float *pose_ms, float *stamp_ms);

/* ---- the rendered map: the grid map made on the device from the arena's obstacle set -----------------------------------
 * The reference's world model makes the grid again every cycle (DataRenderer::GetObstacleMap and FakeMapper,
 * data_renderer.cc:146-259): the origin follows the ego vehicle, the grid is wiped to a background byte, the obstacle circles and
 * polygons of /arena_info_static are filled in, the remembered obstacle points are set.  dftpav_grid_render does the same from a few
 * kilobytes of vertices, so that a cycle is "render, stamp, plan, clear" and no map crosses the bus.  Off until called: a handle
 * that never renders launches, allocates and computes what it did without this section (render.hip).
 *
 * The definition.  A grid (size_x, size_y, resolution, origin_x, origin_y), a background byte and an obstacle set.  Every cell
 * starts as `background`; a covered cell becomes 80; every writer writes 80, so order and overlap do not show.  All arithmetic is
 * fp64 without contraction.
 *   Snapping: a world coordinate p becomes the cell coordinate rint((p - origin) / resolution), halves to even (numpy's rint).
 *   Polygon p has the vertices poly_xy[poly_off[p] .. poly_off[p + 1]), snapped to integers (X_v, Y_v); edge e runs from vertex e
 *   to vertex e + 1, cyclic.  A polygon whose snapped bounding box misses the grid covers nothing.
 *     interior, for each row y in [max(minY, 0), min(maxY, size_y - 1)]:
 *       edge e crosses row y iff (Y0 <= y && Y1 > y) || (Y1 <= y && Y0 > y)
 *       its abscissa is t = (double)(y - Y0) / (double)(Y1 - Y0), x = (double)X0 + t * (double)(X1 - X0)
 *       the abscissae of the row are sorted ascending (equal values are interchangeable); each pair (a, b) at the positions
 *       (2k, 2k + 1) covers ix in [max(ceil(a), 0), min(floor(b), size_x - 1)]
 *     outline, for each edge: n = max(|X1 - X0|, |Y1 - Y0|) + 1 steps; step k is the cell
 *       (rint((double)k * sx + (double)X0), rint((double)k * sy + (double)Y0)) with sx = (double)(X1 - X0) / (double)(n - 1) and
 *       sy likewise; the last step is exactly (X1, Y1); n == 1 is the single cell (X0, Y0); steps outside the grid are dropped
 *     A polygon of 0, 1 or 2 vertices is legal: the rule gives it no interior beyond its outline (0 vertices: nothing).
 *   Circle (cx, cy, radius): the centre snapped as above, r = (int)(radius / resolution), truncated (data_renderer.cc:178); the
 *   cells with integer dx * dx + dy * dy <= r * r round the centre, clipped to the grid.
 *   Point (x, y): its snapped cell becomes 80 if it lies inside the grid (SetValueUsingGlobalPosition, data_renderer.cc:253).
 * The polygon rule is, operation by operation, the one that made this project's default arena map (tests/golden/default_map.npz).
 *
 * State.  After dftpav_grid_render the handle is as dftpav_set_grid_map leaves it, given the rendered bytes: the rendered map is
 * the working map and the base of later stamps; stamps and the base copy of the map before are dropped; the distance field is
 * stale; the table of line sample offsets is that of `resolution`; maps of up to 327 680 cells have the corridor's bit map, made
 * from the bytes on the device.  A map of as many cells as the one before keeps its device allocations.
 *
 * dftpav_grid_render: all work goes on the handle's stream; the call waits for that stream before it changes the map (as
 *   dftpav_set_grid_map does) and ENDS WITH A WAIT for it: the obstacle set comes from the caller's memory.  obs NULL is the empty
 *   set, which renders the background alone.
 * dftpav_grid_origin_centred: host only.  out = (round(ego_x - extent_x / 2), round(ego_y - extent_y / 2)), C's round
 *   (data_renderer.cc:156-160): the origin that follows the ego vehicle, extent = cells * resolution.
 * dftpav_render_last_ms: device time in ms (the handle's HIP events) of the kernels of the last render, the bit map's included,
 *   without the copies of the obstacle set.
 * DFTPAV_E_INVALID, and nothing changed: h NULL; a count < 0; a count > 0 with its array NULL; size_x or size_y <= 0; resolution
 * not > 0 or not finite; origin, a coordinate or a radius not finite; radius < 0; a snapped coordinate, or a radius in cells, beyond
 * +-2^30; poly_off not non-decreasing from 0; a polygon of more than DFTPAV_RENDER_MAX_VERTS vertices (a wave holds an edge per
 * lane); dftpav_grid_origin_centred with out NULL or an argument not finite; dftpav_render_last_ms before any render.
 *
 * Not claimed.  OpenCV's choice of outline and rim cells: a cell on the outline of a polygon or on the rim of a disc may differ
 * from cv::fillPoly's / cv::circle's by one cell (OpenCV is not part of this project; the rules above are its documented ones).
 * The FOV ray casting of RayCastingOnObstacleMap (data_renderer.cc:264-): it marks scanned cells and remembers points, and adds
 * nothing to the cells equal to 80 that the planner reads; pass the remembered points as `points`.  Obstacles are not drawn into
 * an existing map: a render makes the whole map (boxes into an existing map: the stamps above). */
#define DFTPAV_RENDER_MAX_VERTS 64
typedef struct dftpav_obstacle_set {
  int n_poly;
  const int *poly_off;    /* [n_poly + 1], from 0, non-decreasing */
  const double *poly_xy;  /* [poly_off[n_poly]][2] world x, y */
  int n_circle;
  const double *circles;  /* [n_circle][3] cx, cy, radius */
  int n_point;
  const double *points;   /* [n_point][2] x, y */
} dftpav_obstacle_set;
int dftpav_grid_render(dftpav_handle *h, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                       unsigned char background, const dftpav_obstacle_set *obs);
int dftpav_grid_origin_centred(double ego_x, double ego_y, double extent_x, double extent_y, double out[2]);
int dftpav_render_last_ms(dftpav_handle *h, float *ms);

/* One-shot convenience == OptimizeTrajectory for B trajectories. */
int dftpav_solve_batch(dftpav_handle *h, const dftpav_layout *layout, int B,
                       const dftpav_batch_data *d, double *x, double *final_cost,
                       int *status, int *success, int *iters, int *evals);

/* The HIP stream of the handle as an opaque pointer (for callers that want to
 * order their own work after a solve). */
void *dftpav_stream(dftpav_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* DFTPAV_HIP_H */
