// capi.cpp — host half of the C-ABI declared in include/dftpav_hip.h.
//
// Holds what PolyTrajOptimizer::OptimizeTrajectory does before and after the
// L-BFGS call (traj_optimizer.cpp:7-134, 176-201): validation, corridor normal
// normalisation, boundary clamping, decision-vector packing, status mapping.
// Everything between (the solve itself) is the kernel in solver.hip.
// There is deliberately no CPU fallback: without a usable HIP device every
// entry point that needs one fails with DFTPAV_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <atomic>
#include <mutex>

#include <climits>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "e4_plan.h"
#include "traj_math.h"
#include "cr_trig.h"
#include "rs_math.h"
#include "search_args.h"
#include "plan_args.h"

namespace dftpav {
hipError_t launch_solver(const DevBatch &D, const DevBatch *d_dev, int mode, int threads, int grid, SchedArgs sched,
                         hipStream_t stream);
hipError_t launch_corridor(const unsigned char *cells, const unsigned *bits, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                           const double *states, int n, double veh_width, double veh_length, double veh_dcr, const double *dl,
                           int n_dl, double *hpoly, double *batch_cor, int Npts, int NptsPad, int replicate, hipStream_t stream);
hipError_t launch_frontend(const dftpav_frontend_params &fp, const double *paths, const int *path_len, int max_path,
                           const double *start_states, const double *end_states, const double *start_ctrl, int n_hyp,
                           const dftpav_frontend_out &out, hipStream_t stream);
hipError_t launch_restarts(const double *inner, const double *durs, int n_hyp, int n_restarts, int n_inner, int M, double sigma,
                           double lo, double hi, unsigned long long seed, double *out_inner, double *out_durs, hipStream_t stream);
hipError_t launch_fit(const double *states, int S, int n_states, const double *opM, double *dur, double *coef, double *total,
                      double *start, hipStream_t stream);
hipError_t launch_validate(const unsigned char *cells, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                           const double *coeffs, const double *piece_dt, const DevLayout &L, int B, double veh_width,
                           double veh_length, double veh_dcr, const double *t_tab, int n_t, double sample_dt, const double *v_tab,
                           int n_v, int *collision, int *first_sample, hipStream_t stream);
hipError_t launch_states(const double *coeffs, const double *piece_dt, const DevLayout &L, int B, double wheel_base, double t0,
                         double sample_dt, int n_samples, int filter, double *states, int *n_valid, hipStream_t stream);
hipError_t launch_shots(const double *from, const double *to, int n, double rho, double checkl, int max_samples,
                        const unsigned char *cells, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                        double veh_width, double veh_length, double veh_dcr, const double *v_tab, int n_v, double *length, int *type,
                        double *seg, double *samples, int *n_samples, int *collides, hipStream_t stream);
hipError_t launch_search(const SearchArgs &A, int blocks, hipStream_t stream);
// plan.hip: the kernels between the stages of dftpav_plan_queries
hipError_t launch_plan_paths(const int *status, const int *path_len, const int *skip, int n, int max_path, double *paths, int *fe_len,
                             hipStream_t stream);
hipError_t launch_plan_pack(const PlanPackArgs &A, hipStream_t stream);
hipError_t launch_plan_select(const PlanSelectArgs &A, hipStream_t stream);
hipError_t launch_replan_check(const ReplanArgs &A, hipStream_t stream);
hipError_t launch_exec_adopt(const ExecAdoptArgs &A, hipStream_t stream);
hipError_t launch_publish(const PublishArgs &A, hipStream_t stream);
hipError_t launch_pub_reset(const PubResetArgs &A, hipStream_t stream);
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
hipError_t launch_solver_quad(const DevBatch &D, const DevBatch *d_dev, int mode, const double *tabs, const double *cor_t, bool rect, double *scratch,
                              const RefPlan &pl, int scheduled, bool alone, hipStream_t stream);
// the QUAD shapes' copy of the corridor (solver_ref4.hip: one gear segment, solver_ref4m.hip: several)
size_t reference_order_quad_corridor_doubles(const DevLayout &L, int B);
hipError_t launch_quad_corridor(const DevBatch &D, double *cor_t, bool rect, hipStream_t stream);
hipError_t launch_quad_rect_check(const double *corridor, int B, int Npts, int NptsPad, int *d_flag, hipStream_t stream);
hipError_t launch_quadm_corridor(const DevBatch &D, double *cor_t, hipStream_t stream);
}
using namespace dftpav;

// An RCCL communicator and the number of handles that hold it (its creator and the handles it was shared with, each on its own
// host thread at most): the communicator is destroyed by whichever of them lets go last, in whatever order they do.  An RCCL
// communicator does not take concurrent enqueues: `mu` is held around every call on it (the holders' threads serialise there;
// the ORDER of the collectives across ranks stays the host's business -- same order on every rank).  Taking and dropping a
// reference (share / destroy / create) happens under g_comm_mu, so a handle never reads another's comm_ref while that one
// lets go of it.
struct CommShared {
  void *comm;
  std::atomic<int> holders;
  std::mutex mu;
};
static std::mutex g_comm_mu;

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
  hipEvent_t cev0 = nullptr, cev1 = nullptr; // around the last corridor kernel
  hipEvent_t mark[2] = {nullptr, nullptr};   // dftpav_mark
  bool ctimed = false;
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
    double *d_poses = nullptr, *d_t = nullptr, *d_v = nullptr, *d_rd = nullptr;
    int *d_col = nullptr, *d_first = nullptr, *d_valid = nullptr;
    size_t n_poses = 0, n_t = 0, n_v = 0, n_rd = 0;
    std::vector<double> poses, tt, vv; // host sources of the asynchronous copies
    int n_samples = 0;
    bool in_flight = false;
  } pc;
  int trace_b = -1, trace_cap = 0, trace_n = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;  // a solve was enqueued: ev0 / ev1 are recorded
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

extern "C" int dftpav_comm_destroy(dftpav_handle *h);

// ------------------------------------------------------------------ params
extern "C" void dftpav_default_params(dftpav_params *p) {
  std::memset(p, 0, sizeof(*p));
  // config/minco_config.pb.txt:65-100
  p->traj_resolution = 16;
  p->des_traj_resolution = 32;
  p->wei_obs = 1000.0;
  p->wei_surround = 5000.0;
  p->wei_feas = 2500.0;
  p->wei_sqrvar = 500.0;
  p->wei_time = 500.0;
  p->surround_clearance = 0.4;
  p->half_margin = 0.15;
  p->max_forward_vel = 5.0;
  p->max_forward_acc = 8.0;
  p->max_forward_cur = 1.0;
  p->max_backward_vel = 2.0;
  p->max_backward_acc = 4.0;
  p->max_backward_cur = 1.0;
  p->max_latacc = 5.0;
  p->max_phidot = 10000.0;
  p->gear_opt = 1;
  p->non_sinv = 0.24; // traj_optimizer.h:68
  p->mini_T = 0.1;
  p->fail_cost = 50000.0; // traj_optimizer.cpp:197
  // common/basics/semantics.h:66-76
  p->veh_width = 1.90;
  p->veh_length = 4.88;
  p->veh_wheel_base = 2.85;
  p->veh_d_cr = 1.015;
  // traj_optimizer.cpp:127-134 over lbfgs.hpp:15-129
  p->lbfgs_mem_size = 256;
  p->lbfgs_past = 3;
  p->lbfgs_delta = 1.0e-4;
  p->lbfgs_g_epsilon = 1.0e-16;
  p->lbfgs_max_iterations = 12000;
  p->lbfgs_max_linesearch = 64;
  p->lbfgs_min_step = 1.0e-32;
  p->lbfgs_max_step = 1.0e+20;
  p->lbfgs_f_dec_coeff = 1.0e-4;
  p->lbfgs_s_curv_coeff = 0.9;
  p->lbfgs_cautious_factor = 1.0e-6;
  p->lbfgs_machine_prec = 1.0e-16;
}

extern "C" int dftpav_num_vars(const dftpav_layout *l) { // traj_optimizer.cpp:80-86
  if (!l || l->M < 1) return DFTPAV_E_INVALID;
  int n = 0;
  for (int i = 0; i < l->M; i++) n += 2 * (l->piece_nums[i] - 1);
  n += l->M;
  n += 2 * (l->M - 1);
  n += 1 * (l->M - 1);
  return n;
}

extern "C" int dftpav_num_points(const dftpav_params *p, const dftpav_layout *l) { // traj_optimizer.cpp:44
  if (!p || !l || l->M < 1) return DFTPAV_E_INVALID;
  int s = 0;
  for (int i = 0; i < l->M; i++)
    s += (l->piece_nums[i] - 2) * (p->traj_resolution + 1) + 2 * (p->des_traj_resolution + 1);
  return s;
}

// sizeof probes so the Python mirror of the PODs can be checked against the compiled layout
extern "C" int dftpav_abi_sizeof_params(void) { return (int)sizeof(dftpav_params); }
extern "C" int dftpav_abi_sizeof_layout(void) { return (int)sizeof(dftpav_layout); }
extern "C" int dftpav_abi_sizeof_batch_data(void) { return (int)sizeof(dftpav_batch_data); }
extern "C" int dftpav_abi_sizeof_surround(void) { return (int)sizeof(dftpav_surround); }

// ------------------------------------------------------------------ handle
extern "C" int dftpav_create(const dftpav_params *params, int device, dftpav_handle **out) {
  if (!params || !out) return DFTPAV_E_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return DFTPAV_E_NO_DEVICE;
  if (params->lbfgs_past > 8 || params->lbfgs_past < 0) return DFTPAV_E_UNSUPPORTED;
  if (params->lbfgs_mem_size <= 0 || params->lbfgs_mem_size > 1024) return DFTPAV_E_UNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return DFTPAV_E_NO_DEVICE;
  auto *h = new dftpav_handle();
  h->params = *params;
  h->device = device;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return DFTPAV_E_NO_DEVICE;
  }
  *out = h;
  return DFTPAV_OK;
}

static int finish_pending(dftpav_batch *b);
// The obstacle set is captured by every batch's launch descriptor: suspended stragglers of a chained solve must finish
// against the obstacles they started with, so they are finished before the set changes.
static int finish_batches_of(dftpav_handle *h) {
  for (dftpav_batch *b : h->batches)
    if (int rc = finish_pending(b)) return rc;
  return DFTPAV_OK;
}

// DevSurround::theta: for piece k of an obstacle the largest double t with f_k(t) <= duration_k, where f_k is the
// reference's walk t -= d_0, ..., t -= d_{k-1} (poly_traj_utils.hpp:515-521) in fp64.  f_k is non-decreasing in t, so the
// boundary is found by bisection over the bit patterns of the non-negative doubles with that same arithmetic.  Returns
// false (no table: the kernels walk) if a duration is not positive and finite or the thresholds do not increase.
static bool build_theta(const std::vector<int> &off, const std::vector<double> &dur, std::vector<double> &theta) {
  theta.assign(dur.size(), 0.0);
  for (size_t u = 0; u + 1 < off.size(); u++) {
    const double *d = dur.data() + off[u];
    const int np = off[u + 1] - off[u];
    double prev = -1.0;
    for (int k = 0; k < np; k++) {
      if (!(d[k] > 0.0) || !std::isfinite(d[k])) return false;
      auto stops = [&](double t) {
        for (int i = 0; i < k; i++) t -= d[i];
        return !(t > d[k]);
      };
      unsigned long long lo = 0, hi; // bit patterns: stops(lo) holds, stops(hi) does not
      const double big = 1.0e300;
      std::memcpy(&hi, &big, 8);
      while (hi - lo > 1) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        double t;
        std::memcpy(&t, &mid, 8);
        if (stops(t)) lo = mid;
        else hi = mid;
      }
      double th;
      std::memcpy(&th, &lo, 8);
      if (!(th >= prev)) return false;
      prev = th;
      theta[off[u] + k] = th;
    }
  }
  return true;
}
// DevSurround::bbox: per piece a box that contains the obstacle's position for every local time in [0, duration].  With
// t = duration * s the piece is a quintic in s on [0, 1]; its Bernstein coefficients B_i = sum_{k<=i} C(i,k)/C(5,k) a_k
// duration^k span a hull the curve cannot leave, so their minimum and maximum per axis bound it.  The box is widened by
// 1e-6 m (+ 1e-9 relative): orders of magnitude above the rounding of this computation, of the kernels' evaluation of the
// position and of a local time that leaves [0, duration] by an ulp.
static void build_piece_boxes(const std::vector<double> &dur, const std::vector<double> &coef, std::vector<double> &box) {
  static const double binom5[6] = {1, 5, 10, 10, 5, 1};
  const size_t np = dur.size();
  box.assign(4 * np, 0.0);
  for (size_t k = 0; k < np; k++) {
    const double *cm = coef.data() + 12 * k; // 2x6 col-major, col 0 multiplies t^5
    for (int d = 0; d < 2; d++) {
      double b[6], pw = 1.0;
      for (int q = 0; q < 6; q++) {
        b[q] = cm[2 * (5 - q) + d] * pw; // a_q duration^q
        pw *= dur[k];
      }
      double lo = 0, hi = 0, mag = 0;
      for (int i = 0; i < 6; i++) {
        double B = 0.0, cik = 1.0; // C(i, q), built up with q
        for (int q = 0; q <= i; q++) {
          B += cik / binom5[q] * b[q];
          cik = cik * (i - q) / (q + 1);
        }
        if (i == 0 || B < lo) lo = B;
        if (i == 0 || B > hi) hi = B;
        mag = std::fmax(mag, std::fabs(B));
      }
      const double m = 1e-6 + 1e-9 * mag;
      box[4 * k + 2 * d] = lo - m;
      box[4 * k + 2 * d + 1] = hi + m;
    }
  }
}
// test hook (host only, no device): the tables the host derives from a set of moving obstacles -- theta [np] (zeros and
// return value 0 if the walk has no threshold table) and the piece boxes [np][4]
extern "C" int dftpav_debug_surround_tables(int S, const int *piece_offsets, const double *durations, const double *coeffs, double *theta,
                                            double *boxes) {
  if (S <= 0 || !piece_offsets || !durations || !coeffs) return DFTPAV_E_INVALID;
  const int np = piece_offsets[S];
  std::vector<int> off(piece_offsets, piece_offsets + S + 1);
  std::vector<double> dur(durations, durations + np), coef(coeffs, coeffs + 12 * (size_t)np), th, box;
  const bool ok = build_theta(off, dur, th);
  build_piece_boxes(dur, coef, box);
  if (theta) std::memcpy(theta, th.data(), sizeof(double) * np);
  if (boxes) std::memcpy(boxes, box.data(), sizeof(double) * 4 * (size_t)np);
  return ok ? 1 : 0;
}
// test hook (host only, no device): the distance gate of traj_optimizer.cpp:1393 for `npts` ego positions `sigma` [npts][2] at
// local times `t` [npts] against obstacle u, decided twice by the code the kernels run -- with the host's tables (threshold
// search + piece boxes) and without them (the reference's walk).  out_with / out_without [npts]: 1 = the pair passes the gate.
extern "C" int dftpav_debug_gate(int S, const int *piece_offsets, const double *durations, const double *coeffs, const double *total,
                                 const double *start, int u, double t_now, double trajtime, double veh_length_infl, int npts,
                                 const double *sigma, const double *t, int *out_with, int *out_without) {
  if (S <= 0 || u < 0 || u >= S || !piece_offsets || !durations || !coeffs || !total || !start) return DFTPAV_E_INVALID;
  const int np = piece_offsets[S];
  std::vector<int> off(piece_offsets, piece_offsets + S + 1);
  std::vector<double> dur(durations, durations + np), coef(coeffs, coeffs + 12 * (size_t)np), th, box;
  if (!build_theta(off, dur, th)) return 0;
  build_piece_boxes(dur, coef, box);
  dftpav::DevParams P{};
  P.veh_length_infl = veh_length_infl;
  dftpav::DevSurround A{S, piece_offsets, durations, coeffs, total, start, th.data(), box.data()};
  dftpav::DevSurround W{S, piece_offsets, durations, coeffs, total, start, nullptr, nullptr};
  for (int i = 0; i < npts; i++) {
    dftpav::DynObs ob;
    out_with[i] = dftpav::dyn_obstacle_near(P, A, u, t_now, t[i], trajtime, sigma + 2 * i, ob) ? 1 : 0;
    out_without[i] = dftpav::dyn_obstacle_near(P, W, u, t_now, t[i], trajtime, sigma + 2 * i, ob) ? 1 : 0;
  }
  return 1;
}
static int upload_boxes(dftpav_handle *h, const std::vector<double> &dur, const std::vector<double> &coef) {
  for (double v : coef)
    if (!std::isfinite(v)) return DFTPAV_OK; // no table: nothing is skipped
  std::vector<double> box;
  build_piece_boxes(dur, coef, box);
  if (box.empty()) return DFTPAV_OK;
  HIPCHK(h, hipMalloc(&h->d_sur_bbox, sizeof(double) * box.size()));
  HIPCHK(h, hipMemcpy(h->d_sur_bbox, box.data(), sizeof(double) * box.size(), hipMemcpyHostToDevice));
  return DFTPAV_OK;
}
static int upload_theta(dftpav_handle *h, const std::vector<int> &off, const std::vector<double> &dur) {
  std::vector<double> theta;
  if (!build_theta(off, dur, theta) || theta.empty()) return DFTPAV_OK; // d_sur_theta stays null: the kernels walk
  HIPCHK(h, hipMalloc(&h->d_sur_theta, sizeof(double) * theta.size()));
  HIPCHK(h, hipMemcpy(h->d_sur_theta, theta.data(), sizeof(double) * theta.size(), hipMemcpyHostToDevice));
  return DFTPAV_OK;
}

static void free_surround(dftpav_handle *h) {
  if (h->d_sur_off) (void)hipFree(h->d_sur_off);
  if (h->d_sur_dur) (void)hipFree(h->d_sur_dur);
  if (h->d_sur_theta) (void)hipFree(h->d_sur_theta);
  if (h->d_sur_bbox) (void)hipFree(h->d_sur_bbox);
  if (h->d_sur_coef) (void)hipFree(h->d_sur_coef);
  if (h->d_sur_total) (void)hipFree(h->d_sur_total);
  if (h->d_sur_start) (void)hipFree(h->d_sur_start);
  h->d_sur_off = nullptr;
  h->d_sur_dur = h->d_sur_coef = h->d_sur_total = h->d_sur_start = h->d_sur_theta = h->d_sur_bbox = nullptr;
  h->S = 0;
  h->sur_pieces = 0;
}

extern "C" void dftpav_destroy(dftpav_handle *h) {
  if (!h) return;
  (void)dftpav_comm_destroy(h);
  (void)hipSetDevice(h->device);
  free_surround(h);
  if (h->d_cells) (void)hipFree(h->d_cells);
  if (h->d_bits) (void)hipFree(h->d_bits);
  if (h->d_dl) (void)hipFree(h->d_dl);
  if (h->d_search_ws) (void)hipFree(h->d_search_ws);
  for (hipEvent_t &e : h->mark)
    if (e) (void)hipEventDestroy(e);
  if (h->cev0) (void)hipEventDestroy(h->cev0);
  if (h->cev1) (void)hipEventDestroy(h->cev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" const char *dftpav_last_error(const dftpav_handle *h) { return h ? h->err.c_str() : "null handle"; }
extern "C" void *dftpav_stream(dftpav_handle *h) { return h ? (void *)h->stream : nullptr; }

static void minco_operator(int N, std::vector<double> &Mop, std::vector<double> &MopT);

extern "C" int dftpav_sample_restarts(dftpav_handle *h, const double *inner_pts, const double *durations, int n_hyp, int n_restarts,
                                      int n_inner, int M, double sigma, double dur_lo, double dur_hi, unsigned long long seed,
                                      double *out_inner_pts, double *out_durations) {
  if (!h || !inner_pts || !durations || !out_inner_pts || !out_durations || n_hyp < 0 || n_restarts < 1 || n_inner < 0 ||
      (n_inner & 1) || M < 1 || !(sigma >= 0.0) || !(dur_lo > 0.0) || !(dur_hi >= dur_lo))
    return DFTPAV_E_INVALID;
  if (n_hyp == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t B = (size_t)n_hyp * n_restarts;
  double *d_in = nullptr, *d_du = nullptr, *d_oi = nullptr, *d_od = nullptr;
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  chk(hipMalloc(&d_in, sizeof(double) * std::max<size_t>(1, (size_t)n_hyp * n_inner)));
  chk(hipMalloc(&d_du, sizeof(double) * (size_t)n_hyp * M));
  chk(hipMalloc(&d_oi, sizeof(double) * std::max<size_t>(1, B * n_inner)));
  chk(hipMalloc(&d_od, sizeof(double) * B * M));
  if (rc == DFTPAV_OK) {
    chk(hipMemcpyAsync(d_in, inner_pts, sizeof(double) * (size_t)n_hyp * n_inner, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_du, durations, sizeof(double) * (size_t)n_hyp * M, hipMemcpyHostToDevice, h->stream));
    chk(launch_restarts(d_in, d_du, n_hyp, n_restarts, n_inner, M, sigma, dur_lo, dur_hi, seed, d_oi, d_od, h->stream));
    chk(hipMemcpyAsync(out_inner_pts, d_oi, sizeof(double) * B * n_inner, hipMemcpyDeviceToHost, h->stream));
    chk(hipMemcpyAsync(out_durations, d_od, sizeof(double) * B * M, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
  }
  for (double *p : {d_in, d_du, d_oi, d_od})
    if (p) (void)hipFree(p);
  return rc;
}

extern "C" int dftpav_frontend_resample(dftpav_handle *h, const dftpav_frontend_params *fp, const double *paths, const int *path_len,
                                        int max_path, const double *start_states, const double *end_states,
                                        const double *start_ctrl, int n_hyp, const dftpav_frontend_out *out) {
  if (!h || !fp || !paths || !path_len || !start_states || !end_states || !start_ctrl || !out || n_hyp < 0 || max_path < 2)
    return DFTPAV_E_INVALID;
  if (out->max_seg < 1 || out->max_seg > 16 || out->max_pieces < 2 || out->max_states < 1) return DFTPAV_E_UNSUPPORTED;
  if (fp->traj_res < 1 || fp->dense_traj_res < 1 || !(fp->piece_duration > 0.0)) return DFTPAV_E_INVALID;
  for (int i = 0; i < n_hyp; i++)
    if (path_len[i] < 2 || path_len[i] > max_path) return DFTPAV_E_INVALID;
  if (n_hyp == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nh = (size_t)n_hyp, MS = (size_t)out->max_seg, MP = (size_t)out->max_pieces, MST = (size_t)out->max_states;
  struct Buf {
    void **dev;
    const void *src; // host input (nullptr for outputs)
    void *dst;       // host output
    size_t bytes;
  };
  double *d_paths = nullptr, *d_ss = nullptr, *d_es = nullptr, *d_sc = nullptr;
  int *d_len = nullptr;
  dftpav_frontend_out D = *out; // device pointers below
  D.n_seg = nullptr; D.singul = nullptr; D.piece_nums = nullptr; D.piece_dt = nullptr; D.ini_states = nullptr;
  D.fin_states = nullptr; D.inner_pts = nullptr; D.n_states = nullptr; D.states = nullptr;
  Buf bufs[] = {
      {(void **)&d_paths, paths, nullptr, sizeof(double) * nh * max_path * 3},
      {(void **)&d_len, path_len, nullptr, sizeof(int) * nh},
      {(void **)&d_ss, start_states, nullptr, sizeof(double) * nh * 4},
      {(void **)&d_es, end_states, nullptr, sizeof(double) * nh * 4},
      {(void **)&d_sc, start_ctrl, nullptr, sizeof(double) * nh * 2},
      {(void **)&D.n_seg, nullptr, out->n_seg, sizeof(int) * nh},
      {(void **)&D.singul, nullptr, out->singul, sizeof(int) * nh * MS},
      {(void **)&D.piece_nums, nullptr, out->piece_nums, sizeof(int) * nh * MS},
      {(void **)&D.piece_dt, nullptr, out->piece_dt, sizeof(double) * nh * MS},
      {(void **)&D.ini_states, nullptr, out->ini_states, sizeof(double) * nh * MS * 6},
      {(void **)&D.fin_states, nullptr, out->fin_states, sizeof(double) * nh * MS * 6},
      {(void **)&D.inner_pts, nullptr, out->inner_pts, sizeof(double) * nh * MS * (MP - 1) * 2},
      {(void **)&D.n_states, nullptr, out->n_states, sizeof(int) * nh * MS},
      {(void **)&D.states, nullptr, out->states, sizeof(double) * nh * MS * MST * 3},
  };
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  for (Buf &b : bufs) {
    if (!b.src && !b.dst) {
      rc = DFTPAV_E_INVALID;
      break;
    }
    chk(hipMalloc(b.dev, b.bytes));
    if (rc != DFTPAV_OK) break;
    if (b.src) chk(hipMemcpyAsync(*b.dev, b.src, b.bytes, hipMemcpyHostToDevice, h->stream));
    else chk(hipMemsetAsync(*b.dev, 0, b.bytes, h->stream));
  }
  if (rc == DFTPAV_OK) chk(launch_frontend(*fp, d_paths, d_len, max_path, d_ss, d_es, d_sc, n_hyp, D, h->stream));
  if (rc == DFTPAV_OK)
    for (Buf &b : bufs)
      if (b.dst) chk(hipMemcpyAsync(b.dst, *b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
  chk(hipStreamSynchronize(h->stream));
  for (Buf &b : bufs)
    if (*b.dev) (void)hipFree(*b.dev);
  return rc;
}

// The solver numbers (constraint point, obstacle) pairs with 16 bits and keeps a 16-bit mask of obstacles per point; its
// tables of the obstacles' pieces live in LDS.  A set beyond that is refused where it is installed, not at the first solve.
static int check_surround_limits(dftpav_handle *h, int S, long long pieces) {
  if (S > DFTPAV_MAX_SURROUND || pieces > DFTPAV_MAX_SURROUND_PIECES) {
    h->err = "too many moving obstacles (at most DFTPAV_MAX_SURROUND = 16 with DFTPAV_MAX_SURROUND_PIECES = 512 pieces in all)";
    return DFTPAV_E_UNSUPPORTED;
  }
  return DFTPAV_OK;
}
extern "C" int dftpav_fit_surround(dftpav_handle *h, const double *states, int S, int n_states) {
  if (!h || (S > 0 && !states) || S < 0 || (S > 0 && n_states < 3)) return DFTPAV_E_INVALID;
  // (no limit here: the fit is also a service of its own, its result read back with dftpav_get_surround; a fitted set beyond
  // the solver's limits makes solve / eval / validate of a batch return DFTPAV_E_UNSUPPORTED, as the header says)
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_batches_of(h)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_surround(h);
  h->sur_version++;
  if (S == 0) return DFTPAV_OK; // ConverSurroundTrajFromPoints returns without obstacles, traj_manager.cpp:750-752
  const int N = n_states - 1, np = S * N;
  std::vector<int> off(S + 1);
  for (int i = 0; i <= S; i++) off[i] = i * N;
  std::vector<double> Mop, MopT;
  minco_operator(N, Mop, MopT);
  double *d_states = nullptr, *d_op = nullptr;
  HIPCHK(h, hipMalloc(&h->d_sur_off, sizeof(int) * (S + 1)));
  HIPCHK(h, hipMalloc(&h->d_sur_dur, sizeof(double) * np));
  HIPCHK(h, hipMalloc(&h->d_sur_coef, sizeof(double) * 12 * np));
  HIPCHK(h, hipMalloc(&h->d_sur_total, sizeof(double) * S));
  HIPCHK(h, hipMalloc(&h->d_sur_start, sizeof(double) * S));
  HIPCHK(h, hipMalloc(&d_states, sizeof(double) * 7 * (size_t)S * n_states));
  if (hipMalloc(&d_op, sizeof(double) * Mop.size()) != hipSuccess) {
    (void)hipFree(d_states);
    h->err = "hipMalloc";
    return DFTPAV_E_HIP;
  }
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  chk(hipMemcpyAsync(h->d_sur_off, off.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, h->stream));
  chk(hipMemcpyAsync(d_states, states, sizeof(double) * 7 * (size_t)S * n_states, hipMemcpyHostToDevice, h->stream));
  chk(hipMemcpyAsync(d_op, Mop.data(), sizeof(double) * Mop.size(), hipMemcpyHostToDevice, h->stream));
  if (rc == DFTPAV_OK)
    chk(launch_fit(d_states, S, n_states, d_op, h->d_sur_dur, h->d_sur_coef, h->d_sur_total, h->d_sur_start, h->stream));
  chk(hipStreamSynchronize(h->stream)); // off / Mop live on this stack frame
  (void)hipFree(d_states);
  (void)hipFree(d_op);
  if (rc == DFTPAV_OK) {
    std::vector<double> dur(np);
    if (hipMemcpy(dur.data(), h->d_sur_dur, sizeof(double) * np, hipMemcpyDeviceToHost) != hipSuccess) rc = DFTPAV_E_HIP;
    if (rc == DFTPAV_OK) rc = upload_theta(h, off, dur);
    if (rc == DFTPAV_OK && h->d_sur_theta) {
      std::vector<double> coef(12 * (size_t)np);
      if (hipMemcpy(coef.data(), h->d_sur_coef, sizeof(double) * coef.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = DFTPAV_E_HIP;
      if (rc == DFTPAV_OK) rc = upload_boxes(h, dur, coef);
    }
  }
  if (rc == DFTPAV_OK) {
    h->S = S;
    h->sur_pieces = np;
  } else {
    free_surround(h);
  }
  return rc;
}

extern "C" int dftpav_get_surround(dftpav_handle *h, int *S, int *n_pieces, int *piece_offsets, double *durations, double *coeffs,
                                   double *total_duration, double *start_time) {
  if (!h) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (S) *S = h->S;
  if (n_pieces) *n_pieces = h->sur_pieces;
  if (h->S == 0) return DFTPAV_OK;
  if (piece_offsets) HIPCHK(h, hipMemcpy(piece_offsets, h->d_sur_off, sizeof(int) * (h->S + 1), hipMemcpyDeviceToHost));
  if (durations) HIPCHK(h, hipMemcpy(durations, h->d_sur_dur, sizeof(double) * h->sur_pieces, hipMemcpyDeviceToHost));
  if (coeffs) HIPCHK(h, hipMemcpy(coeffs, h->d_sur_coef, sizeof(double) * 12 * h->sur_pieces, hipMemcpyDeviceToHost));
  if (total_duration) HIPCHK(h, hipMemcpy(total_duration, h->d_sur_total, sizeof(double) * h->S, hipMemcpyDeviceToHost));
  if (start_time) HIPCHK(h, hipMemcpy(start_time, h->d_sur_start, sizeof(double) * h->S, hipMemcpyDeviceToHost));
  return DFTPAV_OK;
}

// ------------------------------------------------- Reeds-Shepp shots
extern "C" int dftpav_reeds_shepp_shots(dftpav_handle *h, const double *from, const double *to, int n, double max_cur,
                                        double checkl, int max_samples, double vertex_res, double *length, int *type, double *seg,
                                        double *samples, int *n_samples, int *collides) {
  if (!h || n < 0 || !(max_cur > 0.0) || !(checkl > 0.0) || max_samples < 1 || max_samples > 4096) return DFTPAV_E_INVALID;
  if (n == 0) return DFTPAV_OK;
  if (!from || !to) return DFTPAV_E_INVALID;
  if (collides && (!h->d_cells || !(vertex_res > 0.0))) return DFTPAV_E_INVALID; // a collision check needs the map
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->cev0) HIPCHK(h, hipEventCreate(&h->cev0));
  if (!h->cev1) HIPCHK(h, hipEventCreate(&h->cev1));
  std::vector<double> vv; // spacing of the outline points as the reference's running sum (shapes.cc:128)
  if (collides) {
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = vertex_res; dl < longest; dl += vertex_res) vv.push_back(dl);
  }
  if (vv.empty()) vv.push_back(1.0);
  double *d_from = nullptr, *d_to = nullptr, *d_len = nullptr, *d_seg = nullptr, *d_smp = nullptr, *d_v = nullptr;
  int *d_type = nullptr, *d_ns = nullptr, *d_col = nullptr;
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  const size_t nsmp = (size_t)n * max_samples * 3;
  chk(hipMalloc(&d_from, sizeof(double) * 3 * (size_t)n));
  chk(hipMalloc(&d_to, sizeof(double) * 3 * (size_t)n));
  chk(hipMalloc(&d_len, sizeof(double) * (size_t)n));
  chk(hipMalloc(&d_seg, sizeof(double) * 5 * (size_t)n));
  chk(hipMalloc(&d_smp, sizeof(double) * nsmp));
  chk(hipMalloc(&d_v, sizeof(double) * vv.size()));
  chk(hipMalloc(&d_type, sizeof(int) * (size_t)n));
  chk(hipMalloc(&d_ns, sizeof(int) * (size_t)n));
  chk(hipMalloc(&d_col, sizeof(int) * (size_t)n));
  if (rc == DFTPAV_OK) {
    chk(hipMemcpyAsync(d_from, from, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_to, to, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_v, vv.data(), sizeof(double) * vv.size(), hipMemcpyHostToDevice, h->stream));
    chk(hipEventRecord(h->cev0, h->stream));
    chk(launch_shots(d_from, d_to, n, 1.0 / max_cur, checkl, max_samples, collides ? h->d_cells : nullptr, h->map.size_x,
                     h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, h->params.veh_width, h->params.veh_length,
                     h->params.veh_d_cr, d_v, (int)vv.size(), d_len, d_type, d_seg, d_smp, d_ns, d_col, h->stream));
    chk(hipEventRecord(h->cev1, h->stream));
    if (length) chk(hipMemcpyAsync(length, d_len, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (type) chk(hipMemcpyAsync(type, d_type, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (seg) chk(hipMemcpyAsync(seg, d_seg, sizeof(double) * 5 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (samples) chk(hipMemcpyAsync(samples, d_smp, sizeof(double) * nsmp, hipMemcpyDeviceToHost, h->stream));
    if (n_samples) chk(hipMemcpyAsync(n_samples, d_ns, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (collides) chk(hipMemcpyAsync(collides, d_col, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
    h->ctimed = rc == DFTPAV_OK;
  }
  for (void *p : {(void *)d_from, (void *)d_to, (void *)d_len, (void *)d_seg, (void *)d_smp, (void *)d_v, (void *)d_type, (void *)d_ns,
                  (void *)d_col})
    if (p) (void)hipFree(p);
  return rc;
}

// ------------------------------------------------- hybrid A* front-end search (search.hip)
extern "C" void dftpav_default_search_params(dftpav_search_params *sp) {
  std::memset(sp, 0, sizeof(*sp));
  // config/minco_config.pb.txt:13-59 (map_cfg), :81 (max_frontend_cur); kino_astar.h:167; kino_astar.cpp:426-427
  sp->map_size_x = 1000.0;
  sp->map_size_y = 1000.0;
  sp->map_resl = 0.3;
  sp->phi_grid_resolution = 0.3;
  sp->lambda_heu = 5.0;
  sp->tie_breaker = 1.0 + 1.0 / 10000;
  sp->allocate_num = 100000;
  sp->check_num = 5;
  sp->step_arc = 0.9;
  sp->max_frontend_cur = 1.0;
  sp->checkl = 0.2;
  sp->traj_forward_penalty = 1.0;
  sp->traj_back_penalty = 2.5;
  sp->traj_gear_switch_penalty = 15.0;
  sp->traj_steer_penalty = 0.5;
  sp->traj_steer_change_penalty = 0.0;
  sp->veh_width = 1.90 + 0.2;
  sp->veh_length = 4.88 + 0.2;
  sp->veh_d_cr = 1.015;
  sp->wheel_base = 2.85;
  sp->vertex_res = 0.1;
  sp->max_iters = 20000;
  sp->use3d = 1;
  sp->retry_2d = 1;
}

// the inputs of one expansion as the reference's loops build them (kino_astar.cpp:143-171): running sums, tabulated here
static int search_inputs(const dftpav_search_params &sp, double max_steer, int which, double *tab) {
  const double res = 0.5;
  int n = 0;
  auto steers = [&](double arc) {
    for (double steer = -max_steer; steer <= max_steer + 1e-3; steer += res * max_steer * 1.0) {
      if (n < kSearchMaxIn) {
        tab[2 * n] = steer;
        tab[2 * n + 1] = arc;
      }
      if (++n > 4 * kSearchMaxIn) return;
    }
  };
  if (which == 0) {
    for (double arc = sp.map_resl; arc <= 2 * sp.map_resl + 1e-3 && n <= kSearchMaxIn; arc += sp.map_resl) steers(arc);
  } else if (which == 1) {
    for (double arc = -sp.map_resl; arc >= -2 * sp.map_resl - 1e-3 && n <= kSearchMaxIn; arc -= sp.map_resl) steers(arc);
  } else {
    for (double arc = -sp.step_arc; arc <= sp.step_arc + 1e-3 && n <= kSearchMaxIn; arc += 0.5 * sp.step_arc) {
      if (std::fabs(arc) < 1.0e-2) continue;
      steers(arc);
    }
  }
  return n;
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

// The workspace of a search of n queries: per query in flight a node pool, the heap (node, key, position), the path list and the
// hash table (the power of two >= 2 allocate_num); `slots` queries in flight, n or as many as 6 GiB hold -- the queries beyond run
// in further launches over the same slots.  Each array holds every slot's part and starts on a 256-byte boundary: off[] in the
// order pool, h_node, h_pos, path_idx, h_key, table, and `bytes` for all of them.
struct SearchWorkspace {
  int hcap = 0, slots = 0;
  size_t per = 0, off[6] = {}, bytes = 0;
};
static SearchWorkspace search_workspace(const dftpav_search_params &P, int n) {
  SearchWorkspace W;
  W.hcap = 1;
  while (W.hcap < 2 * P.allocate_num) W.hcap <<= 1;
  const size_t A = (size_t)P.allocate_num;
  W.per = A * sizeof(SearchNode) + A * (3 * sizeof(int) + sizeof(double)) + (size_t)W.hcap * sizeof(int) + 256;
  const size_t budget = ((size_t)6 << 30) - 6 * 256; // 6 GiB at most, the arrays' alignment included
  W.slots = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / W.per));
  const size_t S = (size_t)W.slots;
  const size_t sizes[6] = {A * S * sizeof(SearchNode), A * S * sizeof(int), A * S * sizeof(int), A * S * sizeof(int),
                           A * S * sizeof(double), (size_t)W.hcap * S * sizeof(int)};
  for (int k = 0; k < 6; k++) {
    W.off[k] = W.bytes;
    W.bytes += (sizes[k] + 255) / 256 * 256;
  }
  return W;
}
extern "C" int dftpav_debug_search_slots(const dftpav_search_params *sp, int n, int *slots, size_t *bytes_per_query) {
  if (!sp || n < 1 || sp->allocate_num < 2) return DFTPAV_E_INVALID;
  const SearchWorkspace W = search_workspace(*sp, n);
  if (slots) *slots = W.slots;
  if (bytes_per_query) *bytes_per_query = W.per;
  return DFTPAV_OK;
}

static int search_setup(dftpav_handle *h, const dftpav_search_params *sp, int n, SearchSetup &U) {
  const dftpav_search_params &P = *sp;
  if (P.allocate_num < 2 || P.check_num < 1 || P.max_iters < 0 || !(P.map_resl > 0.0) || !(P.phi_grid_resolution > 0.0) ||
      !(P.step_arc > 0.0) || !(P.max_frontend_cur > 0.0) || !(P.checkl > 0.0) || !(P.vertex_res > 0.0) || !(P.wheel_base > 0.0))
    return DFTPAV_E_INVALID;
  // the tables of the running sums: inputs, outline point spacing, shot sample offsets
  const double max_steer = crt::atan(P.wheel_base * P.max_frontend_cur); // kino_astar.cpp:419 (correctly rounded)
  std::vector<double> in_tab(3 * kSearchMaxIn * 2, 0.0);
  int n_in[3];
  for (int w = 0; w < 3; w++) {
    n_in[w] = search_inputs(P, max_steer, w, in_tab.data() + (size_t)w * kSearchMaxIn * 2);
    if (n_in[w] > kSearchMaxIn || n_in[w] * P.check_num > kSearchThreads) return DFTPAV_E_UNSUPPORTED;
  }
  if (P.check_num > kSearchMaxCheck) return DFTPAV_E_UNSUPPORTED;
  std::vector<double> vv;
  const double longest = std::max(P.veh_length, P.veh_width) + 1.0;
  for (double dl = P.vertex_res; dl < longest; dl += P.vertex_res) vv.push_back(dl);
  if (vv.empty()) vv.push_back(longest);
  // a shot is tried within 15 m of the goal (kino_astar.cpp:90); an LSL path, which always exists, is no longer than
  // d + 2 r + 4 pi r, and the shortest path is no longer than it.  getKinoNode's second shot starts from a pose of the
  // terminal node's last arc: one step_arc more.  The table holds every offset up to that bound and a margin.
  const double rho = 1.0 / P.max_frontend_cur;
  const double bound = 15.0 + std::max(P.step_arc, 2 * P.map_resl) + (2.0 + 4.0 * rs::kPi) * rho;
  const double n_l_need = bound / P.checkl + 8.0;
  if (!(n_l_need < (double)kSearchMaxShot)) return DFTPAV_E_UNSUPPORTED;
  std::vector<double> ll;
  for (double l = 0.0; (int)ll.size() < (int)n_l_need; l += P.checkl) ll.push_back(l); // kino_astar.cpp:338, 594
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->cev0) HIPCHK(h, hipEventCreate(&h->cev0));
  if (!h->cev1) HIPCHK(h, hipEventCreate(&h->cev1));
  const SearchWorkspace W = search_workspace(P, n);
  const int hcap = W.hcap, slots = W.slots;
  const size_t ws = W.bytes;
  if (h->search_ws_bytes < ws) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->d_search_ws) (void)hipFree(h->d_search_ws);
    h->d_search_ws = nullptr;
    h->search_ws_bytes = 0;
    const hipError_t e = hipMalloc(&h->d_search_ws, ws);
    if (e != hipSuccess) { // the handle stays usable: no workspace, and no error left for the next launch's hipGetLastError
      (void)hipGetLastError();
      h->d_search_ws = nullptr;
      h->err = std::string("hipMalloc of the search workspace: ") + hipGetErrorString(e);
      return DFTPAV_E_HIP;
    }
    h->search_ws_bytes = ws;
  }
  unsigned char *w = (unsigned char *)h->d_search_ws;
  SearchArgs &S = U.S;
  S = SearchArgs{};
  S.pool = (SearchNode *)(w + W.off[0]);
  S.h_node = (int *)(w + W.off[1]);
  S.h_pos = (int *)(w + W.off[2]);
  S.path_idx = (int *)(w + W.off[3]);
  S.h_key = (double *)(w + W.off[4]);
  S.table = (int *)(w + W.off[5]);
  S.hcap = hcap;
  S.sp = P;
  S.cells = h->d_cells;
  S.size_x = h->map.size_x;
  S.size_y = h->map.size_y;
  S.resolution = h->map.resolution;
  S.origin_x = h->map.origin_x;
  S.origin_y = h->map.origin_y;
  S.inv_yaw_res = 1.0 / P.phi_grid_resolution; // kino_astar.cpp:421
  S.origin_sx = -0.5 * P.map_size_x;
  S.origin_sy = -0.5 * P.map_size_y;
  S.half_size_x = P.map_size_x * 0.5;
  S.half_size_y = P.map_size_y * 0.5;
  S.rho = rho;
  for (int k = 0; k < 3; k++) S.n_in[k] = n_in[k];
  S.n = n;
  S.n_v = (int)vv.size();
  S.n_l = (int)ll.size();
  U.tabs = in_tab;
  U.tabs.insert(U.tabs.end(), vv.begin(), vv.end());
  U.tabs.insert(U.tabs.end(), ll.begin(), ll.end());
  U.n_in_tab = in_tab.size();
  U.n_vv = vv.size();
  U.n_ll = ll.size();
  U.slots = slots;
  return DFTPAV_OK;
}

extern "C" int dftpav_kino_search(dftpav_handle *h, const dftpav_search_params *sp, const double *start_states,
                                  const double *start_ctrl, const double *end_states, int n, const dftpav_search_out *out) {
  (void)start_ctrl; // kept by search (kino_astar.cpp:54) for getKinoNode's flat states: dftpav_frontend_resample takes it
  if (!h || !sp || !out || n < 0 || out->max_nodes < 0 || out->max_path < 0) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (n == 0) return DFTPAV_OK;
  if (!start_states || !end_states || !out->status || !out->shot_success || !out->used_3d || !out->budget_hit || !out->iters ||
      !out->nodes_used || !out->n_nodes || !out->path_len || (out->max_nodes > 0 && !out->nodes) || (out->max_path > 0 && !out->paths))
    return DFTPAV_E_INVALID;
  SearchSetup U;
  if (int rc0 = search_setup(h, sp, n, U)) return rc0;
  SearchArgs &S = U.S;
  const std::vector<double> &tabs = U.tabs;
  const int slots = U.slots;
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  const size_t nn = (size_t)n;
  double *d_tabs = nullptr, *d_st = nullptr, *d_en = nullptr, *d_nodes = nullptr, *d_paths = nullptr;
  int *d_ints = nullptr;
  const size_t ntab = tabs.size();
  chk(hipMalloc(&d_tabs, sizeof(double) * ntab));
  chk(hipMalloc(&d_st, sizeof(double) * 4 * nn));
  chk(hipMalloc(&d_en, sizeof(double) * 4 * nn));
  chk(hipMalloc(&d_ints, sizeof(int) * 9 * nn));
  if (out->max_nodes > 0) chk(hipMalloc(&d_nodes, sizeof(double) * 6 * nn * out->max_nodes));
  if (out->max_path > 0) chk(hipMalloc(&d_paths, sizeof(double) * 3 * nn * out->max_path));
  if (rc == DFTPAV_OK) {
    chk(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(double) * ntab, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_st, start_states, sizeof(double) * 4 * nn, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_en, end_states, sizeof(double) * 4 * nn, hipMemcpyHostToDevice, h->stream));
    // rows past n_nodes / path_len read back as zeros
    if (d_nodes) chk(hipMemsetAsync(d_nodes, 0, sizeof(double) * 6 * nn * out->max_nodes, h->stream));
    if (d_paths) chk(hipMemsetAsync(d_paths, 0, sizeof(double) * 3 * nn * out->max_path, h->stream));
    S.in_tab = d_tabs;
    S.v_tab = d_tabs + U.n_in_tab;
    S.l_tab = d_tabs + U.n_in_tab + U.n_vv;
    S.start = d_st;
    S.end = d_en;
    int *const fields[9] = {out->status, out->shot_success, out->used_3d, out->budget_hit, out->iters, out->nodes_used,
                            out->n_nodes, out->path_len, nullptr};
    dftpav_search_out &O = S.out;
    O.max_nodes = out->max_nodes;
    O.max_path = out->max_path;
    O.status = d_ints;
    O.shot_success = d_ints + nn;
    O.used_3d = d_ints + 2 * nn;
    O.budget_hit = d_ints + 3 * nn;
    O.iters = d_ints + 4 * nn;
    O.nodes_used = d_ints + 5 * nn;
    O.n_nodes = d_ints + 6 * nn;
    O.path_len = d_ints + 7 * nn;
    O.nodes = d_nodes;
    O.paths = d_paths;
    chk(hipEventRecord(h->cev0, h->stream));
    for (int q0 = 0; q0 < n && rc == DFTPAV_OK; q0 += slots) {
      S.q0 = q0;
      chk(launch_search(S, std::min(slots, n - q0), h->stream));
    }
    chk(hipEventRecord(h->cev1, h->stream));
    for (int f = 0; f < 8; f++) chk(hipMemcpyAsync(fields[f], d_ints + f * nn, sizeof(int) * nn, hipMemcpyDeviceToHost, h->stream));
    if (d_nodes) chk(hipMemcpyAsync(out->nodes, d_nodes, sizeof(double) * 6 * nn * out->max_nodes, hipMemcpyDeviceToHost, h->stream));
    if (d_paths) chk(hipMemcpyAsync(out->paths, d_paths, sizeof(double) * 3 * nn * out->max_path, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
    h->ctimed = rc == DFTPAV_OK;
  }
  for (void *p : {(void *)d_tabs, (void *)d_st, (void *)d_en, (void *)d_ints, (void *)d_nodes, (void *)d_paths})
    if (p) (void)hipFree(p);
  if (rc == DFTPAV_OK)
    for (int q = 0; q < n; q++)
      if (out->status[q] == 0) return DFTPAV_E_UNSUPPORTED; // a shot beyond the sample table (not reached: see the bound)
  return rc;
}

extern "C" int dftpav_set_grid_map(dftpav_handle *h, const dftpav_grid_map *map) {
  if (!h || !map || !map->cells || map->size_x <= 0 || map->size_y <= 0 || !(map->resolution > 0.0)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->d_cells) (void)hipFree(h->d_cells);
  if (h->d_bits) (void)hipFree(h->d_bits);
  if (h->d_dl) (void)hipFree(h->d_dl);
  h->d_cells = nullptr;
  h->d_bits = nullptr;
  h->d_dl = nullptr;
  const size_t ncell = (size_t)map->size_x * map->size_y;
  HIPCHK(h, hipMalloc(&h->d_cells, ncell));
  HIPCHK(h, hipMemcpy(h->d_cells, map->cells, ncell, hipMemcpyHostToDevice));
  h->map = *map;
  h->map.cells = nullptr;
  if (ncell <= (size_t)8 * 40 * 1024) { // <= 40 KB of bits per workgroup: four workgroups per CU
    std::vector<unsigned> bits((ncell + 31) / 32, 0u);
    for (size_t i = 0; i < ncell; i++)
      if (map->cells[i] == 80) bits[i >> 5] |= 1u << (i & 31);
    HIPCHK(h, hipMalloc(&h->d_bits, sizeof(unsigned) * bits.size()));
    HIPCHK(h, hipMemcpy(h->d_bits, bits.data(), sizeof(unsigned) * bits.size(), hipMemcpyHostToDevice));
  }
  // sample offsets of CheckIfCollisionUsingLine (map_adapter.cpp:119): dl = 0, then dl += checkl; the longest
  // segment is the far edge of a fully grown rectangle
  const double checkl = map->resolution / 2.0;
  const double longest = std::max(h->params.veh_length, h->params.veh_width) + 2.0 * (10.0 + map->resolution) + 1.0;
  std::vector<double> dl;
  for (double v = 0.0; v < longest; v += checkl) dl.push_back(v);
  h->n_dl = (int)dl.size();
  HIPCHK(h, hipMalloc(&h->d_dl, sizeof(double) * dl.size()));
  HIPCHK(h, hipMemcpy(h->d_dl, dl.data(), sizeof(double) * dl.size(), hipMemcpyHostToDevice));
  if (!h->cev0) HIPCHK(h, hipEventCreate(&h->cev0));
  if (!h->cev1) HIPCHK(h, hipEventCreate(&h->cev1));
  return DFTPAV_OK;
}

// uploads the states and runs the corridor kernel into `hpoly` (device, [n][16]) or into a batch's corridor
static int run_corridor(dftpav_handle *h, const double *states, int n_states, double *d_hpoly, double *batch_cor, int Npts,
                        int NptsPad, int replicate) {
  double *d_states = nullptr;
  HIPCHK(h, hipMalloc(&d_states, sizeof(double) * 3 * (size_t)n_states));
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  chk(hipMemcpyAsync(d_states, states, sizeof(double) * 3 * (size_t)n_states, hipMemcpyHostToDevice, h->stream));
  chk(hipEventRecord(h->cev0, h->stream));
  if (rc == DFTPAV_OK)
    chk(launch_corridor(h->d_cells, h->d_bits, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, d_states,
                        n_states, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, h->d_dl, h->n_dl, d_hpoly,
                        batch_cor, Npts, NptsPad, replicate, h->stream));
  chk(hipEventRecord(h->cev1, h->stream));
  chk(hipStreamSynchronize(h->stream));
  h->ctimed = rc == DFTPAV_OK;
  (void)hipFree(d_states);
  return rc;
}

extern "C" int dftpav_corridor_last_ms(dftpav_handle *h, float *ms) {
  if (!h || !ms || !h->ctimed) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventElapsedTime(ms, h->cev0, h->cev1));
  return DFTPAV_OK;
}

extern "C" int dftpav_corridor_rectangles(dftpav_handle *h, const double *states, int n_states, double *hpoly) {
  if (!h || !states || !hpoly || n_states < 0) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (n_states == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  double *d_hpoly = nullptr;
  HIPCHK(h, hipMalloc(&d_hpoly, sizeof(double) * 16 * (size_t)n_states));
  int rc = run_corridor(h, states, n_states, d_hpoly, nullptr, 1, 1, 1);
  if (rc == DFTPAV_OK && hipMemcpy(hpoly, d_hpoly, sizeof(double) * 16 * (size_t)n_states, hipMemcpyDeviceToHost) != hipSuccess) {
    h->err = "hipMemcpy";
    rc = DFTPAV_E_HIP;
  }
  (void)hipFree(d_hpoly);
  return rc;
}

extern "C" int dftpav_set_surround(dftpav_handle *h, const dftpav_surround *s) {
  if (!h) return DFTPAV_E_INVALID;
  if (s && s->S > 0) {
    if (!s->piece_offsets) return DFTPAV_E_INVALID;
    if (int rc = check_surround_limits(h, s->S, s->piece_offsets[s->S])) return rc; // the installed set stays as it is
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_batches_of(h)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_surround(h);
  h->sur_version++;
  if (!s || s->S <= 0) return DFTPAV_OK;
  int S = s->S, np = s->piece_offsets[S];
  if (np <= 0 || s->piece_offsets[0] != 0) return DFTPAV_E_INVALID;
  for (int u = 0; u < S; u++) // every obstacle is a trajectory of at least one piece (Trajectory::locatePieceIdx has no empty case)
    if (s->piece_offsets[u + 1] <= s->piece_offsets[u]) return DFTPAV_E_INVALID;
  HIPCHK(h, hipMalloc(&h->d_sur_off, sizeof(int) * (S + 1)));
  HIPCHK(h, hipMalloc(&h->d_sur_dur, sizeof(double) * np));
  HIPCHK(h, hipMalloc(&h->d_sur_coef, sizeof(double) * 12 * np));
  HIPCHK(h, hipMalloc(&h->d_sur_total, sizeof(double) * S));
  HIPCHK(h, hipMalloc(&h->d_sur_start, sizeof(double) * S));
  HIPCHK(h, hipMemcpy(h->d_sur_off, s->piece_offsets, sizeof(int) * (S + 1), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_sur_dur, s->durations, sizeof(double) * np, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_sur_coef, s->coeffs, sizeof(double) * 12 * np, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_sur_total, s->total_duration, sizeof(double) * S, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_sur_start, s->start_time, sizeof(double) * S, hipMemcpyHostToDevice));
  if (int rc = upload_theta(h, std::vector<int>(s->piece_offsets, s->piece_offsets + S + 1), std::vector<double>(s->durations, s->durations + np)))
    return rc;
  if (h->d_sur_theta)
    if (int rc = upload_boxes(h, std::vector<double>(s->durations, s->durations + np), std::vector<double>(s->coeffs, s->coeffs + 12 * (size_t)np)))
      return rc;
  h->sur_pieces = np;
  h->S = S;
  return DFTPAV_OK;
}

// ------------------------------------------------- constant MINCO operator
// Columns of A_N^{-1} for the N+5 RHS rows that can be non-zero
// (poly_traj_utils.hpp:968-977): the reference's own banded LU
// (poly_traj_utils.hpp:776-826, restated in traj_math.h) applied to unit
// vectors, once per distinct N at batch creation.  fp64, fixed operation order:
// the operator's bits are part of the reproducible program (tests compare them
// with the oracle's).
static void minco_operator(int N, std::vector<double> &Mop, std::vector<double> &MopT) {
  const int n6 = 6 * N, nc = N + 5;
  std::vector<double> band((size_t)n6 * 13, 0.0);
  BandedLU A{n6, 6, 6, band.data()};
  minco_fill(A, N);
  banded_factorize(A);
  Mop.assign((size_t)n6 * nc, 0.0);
  MopT.assign((size_t)n6 * nc, 0.0);
  std::vector<double> col(n6);
  for (int c = 0; c < nc; c++) {
    int row = c < 3 ? c : (c < N + 2 ? 6 * (c - 3) + 5 : n6 - 3 + (c - (N + 2)));
    std::fill(col.begin(), col.end(), 0.0);
    col[row] = 1.0;
    banded_solve1(A, col.data());
    for (int r = 0; r < n6; r++) {
      Mop[(size_t)r * nc + c] = col[r];
      MopT[(size_t)c * n6 + r] = col[r];
    }
  }
}

// debug/test hook: the operator the kernels use for a segment of N pieces, [6N][N+5] row-major
extern "C" int dftpav_debug_minco_operator(int N, double *out) {
  if (N < 2 || !out) return DFTPAV_E_INVALID;
  std::vector<double> M, MT;
  minco_operator(N, M, MT);
  std::memcpy(out, M.data(), sizeof(double) * M.size());
  return DFTPAV_OK;
}

// -------------------------------------------------------------------- batch
static void fill_dev_params(const dftpav_params &p, DevParams &P) {
  P.wei_obs = p.wei_obs;
  P.wei_surround = p.wei_surround;
  P.wei_feas = p.wei_feas;
  P.wei_time = p.wei_time;
  P.surround_clearance = p.surround_clearance;
  P.max_vel[0] = p.max_forward_vel; P.max_vel[1] = p.max_backward_vel;
  P.max_acc[0] = p.max_forward_acc; P.max_acc[1] = p.max_backward_acc;
  P.max_cur[0] = p.max_forward_cur; P.max_cur[1] = p.max_backward_cur;
  P.non_sinv = p.non_sinv;
  P.mini_T = p.mini_T;
  P.fail_cost = p.fail_cost;
  // footprint, traj_optimizer.cpp:1749-1775
  double W = p.veh_width + 2 * p.half_margin, Lh = p.veh_length + 2 * p.half_margin, dcr = p.veh_d_cr;
  P.veh_length_infl = Lh;
  double le[4][2] = {{dcr + Lh / 2.0, W / 2.0}, {dcr + Lh / 2.0, -W / 2.0}, {dcr - Lh / 2.0, -W / 2.0},
                     {dcr - Lh / 2.0, W / 2.0}};
  for (int k = 0; k < 4; k++) { P.vec_le[k][0] = le[k][0]; P.vec_le[k][1] = le[k][1]; }
  P.vec_le[4][0] = le[0][0]; P.vec_le[4][1] = le[0][1];
  fill_footprint_edges(P);
  P.gear_opt = p.gear_opt;
  P.mem_size = p.lbfgs_mem_size;
  P.past = p.lbfgs_past;
  P.max_iterations = p.lbfgs_max_iterations;
  P.max_linesearch = p.lbfgs_max_linesearch;
  P.delta = p.lbfgs_delta;
  P.g_epsilon = p.lbfgs_g_epsilon;
  P.min_step = p.lbfgs_min_step;
  P.max_step = p.lbfgs_max_step;
  P.f_dec_coeff = p.lbfgs_f_dec_coeff;
  P.s_curv_coeff = p.lbfgs_s_curv_coeff;
  P.cautious_factor = p.lbfgs_cautious_factor;
  P.machine_prec = p.lbfgs_machine_prec;
}

extern "C" void dftpav_batch_destroy(dftpav_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->h->device);
  (void)hipStreamSynchronize(b->h->stream);
  void *ptrs[] = {b->d_x0, b->d_iniS, b->d_finS, b->d_corridor, b->d_pt_piece, b->d_pt_j, b->d_histS, b->d_histU, b->d_histV, b->d_histR, b->d_histM,
                  b->d_x_in, b->d_x_out, b->d_f, b->d_g, b->d_status, b->d_success, b->d_iters, b->d_evals,
                  b->d_hist, b->d_ticks, b->d_prof, b->d_dev, b->d_coef, b->d_dt, b->d_records,
                  b->d_queue, b->d_stragglers, b->d_stragglers2, b->d_sflag, b->d_iota, b->d_qctl, b->d_state, b->d_dev2,
                  b->d_f_eval, b->d_trace, b->d_cor_raw, b->d_ref_tab, b->d_ref_scratch, b->d_cor_t, b->d_rect_flag, b->pc.d_poses, b->pc.d_t, b->pc.d_v, b->pc.d_rd, b->pc.d_col, b->pc.d_first,
                  b->pc.d_valid};
  {
    auto &v = b->h->batches;
    v.erase(std::remove(v.begin(), v.end(), b), v.end());
  }
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (b->h_records) (void)hipHostFree(b->h_records);
  for (int w = 0; w < 2; w++)
    for (int t = 0; t < 5; t++)
      if (b->d_e4[w][t]) (void)hipFree(b->d_e4[w][t]);
  for (int i = 0; i < kMaxSeg; i++) {
    if (b->d_opM[i]) (void)hipFree(b->d_opM[i]);
    if (b->d_opMT[i]) (void)hipFree(b->d_opMT[i]);
  }
  if (b->h_stage) (void)hipHostFree(b->h_stage);
  if (b->stage_ev) (void)hipEventDestroy(b->stage_ev);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  delete b;
}

// the kernels' view of a layout: offsets of the segments' pieces, waypoints, right-hand-side rows and constraint points, and of
// tau | gear xy | gear angle inside x (traj_optimizer.cpp:96-115)
static void fill_dev_layout(const dftpav_layout &layout, int K, int Kd, DevLayout &L) {
  L = DevLayout{};
  L.M = layout.M;
  L.H = layout.H;
  L.K = K;
  L.Kd = Kd;
  L.Kmax = L.K > L.Kd ? L.K : L.Kd;
  int xoff = 0, poff = 0, roff = 0, ptoff = 0;
  for (int i = 0; i < L.M; i++) {
    int N = layout.piece_nums[i];
    L.piece_nums[i] = N;
    L.singuls[i] = layout.singuls[i];
    L.seg_piece0[i] = poff;
    L.seg_x0[i] = xoff;
    L.seg_rhs0[i] = roff;
    L.seg_pt0[i] = ptoff;
    poff += N;
    xoff += 2 * (N - 1);
    roff += N + 5;
    ptoff += (N - 2) * (L.K + 1) + 2 * (L.Kd + 1);
  }
  L.seg_piece0[L.M] = poff;
  L.seg_rhs0[L.M] = roff;
  L.seg_pt0[L.M] = ptoff;
  L.Ntot = poff;
  L.rhs_tot = roff;
  L.Npts = ptoff;
  L.x_tau0 = xoff;
  L.x_gear0 = xoff + L.M;
  L.x_ang0 = L.x_gear0 + 2 * (L.M - 1);
  L.n = L.x_ang0 + (L.M - 1);
  L.npad = ((L.n + 63) / 64) * 64;
}
// The reference order's developer options (device_types.h: RefOptions), read where a plan is chosen and nowhere else.
static RefOptions ref_options_from_env() {
  auto num = [](const char *name, int unset, int lo) { // the variable's number, at least lo; `unset` where it is not set
    const char *e = std::getenv(name);
    return e ? std::max(lo, std::atoi(e)) : unset;
  };
  RefOptions o{};
  const char *shape = std::getenv("DFTPAV_REF_SHAPE");
  o.shape = shape ? (unsigned char)shape[0] : -1;
  o.waves = num("DFTPAV_REF_WAVES", 0, 0);
  o.threads = num("DFTPAV_REF_THREADS", 0, 0);
  o.quad_waves = num("DFTPAV_REF_QUAD_WAVES", 0, 0);
  o.quad_hand = num("DFTPAV_REF_QUAD_HANDOVER", -1, 0);
  o.slice = num("DFTPAV_REF_SLICE", -1, 0);
  o.slots = num("DFTPAV_REF_SLOTS", 0, 1);
  o.exact_div = num("DFTPAV_REF_EXACT_DIV", 0, INT_MIN) != 0;
  o.verbose = std::getenv("DFTPAV_VERBOSE") != nullptr;
  return o;
}
// test hook (host only): is the reference order available for this layout with S moving obstacles, and which launch shape would
// a batch of B trajectories take on a device of n_cu CUs?  out = {supported, shape (RefKind), threads, workgroups per CU, persistent
// workgroups, slice, LDS bytes per workgroup, width of the sequential sums}
extern "C" int dftpav_debug_reference_plan(const dftpav_layout *layout, const dftpav_params *p, int S, int B, int n_cu, long long *out) {
  if (!layout || !p || !out || layout->M < 1 || layout->M > kMaxSeg || B < 1 || n_cu < 1) return DFTPAV_E_INVALID;
  DevLayout L;
  fill_dev_layout(*layout, p->traj_resolution, p->des_traj_resolution, L);
  DevParams P;
  fill_dev_params(*p, P);
  out[0] = reference_order_supported(L, P, S) ? 1 : 0;
  const RefPlan pl = reference_order_plan(L, P, S, B, n_cu, false, ref_options_from_env());
  out[1] = pl.kind; // 0: TEAM, 1: WAVE, 3: QUAD, 5: QUAD, several segments
  out[2] = pl.threads;
  out[3] = pl.wg_per_cu;
  out[4] = pl.slots;
  out[5] = pl.slice;
  out[6] = (long long)pl.lds;
  out[7] = L.n <= 16 ? 16 : (L.n <= 32 ? 32 : (L.n <= 40 ? 40 : (L.n <= 48 ? 48 : 64)));
  return DFTPAV_OK;
}

static int batch_create_impl(dftpav_handle *h, const dftpav_layout *layout, int B, int residency, dftpav_batch **out);
extern "C" int dftpav_batch_create(dftpav_handle *h, const dftpav_layout *layout, int B, dftpav_batch **out) {
  return batch_create_impl(h, layout, B, -1, out);
}
// residency: -1 = by the batch size (dftpav_batch_create); 0 = one workgroup per CU (lowest latency of a solve), 1 = two,
// 2 = four per CU (highest throughput): for callers that keep several small batches in flight on several handles
extern "C" int dftpav_batch_create_shaped(dftpav_handle *h, const dftpav_layout *layout, int B, int residency, dftpav_batch **out) {
  if (residency < -1 || residency > 2) return DFTPAV_E_INVALID;
  return batch_create_impl(h, layout, B, residency, out);
}
static int batch_create_impl(dftpav_handle *h, const dftpav_layout *layout, int B, int residency, dftpav_batch **out) {
  if (!h || !layout || !out || B < 1) return DFTPAV_E_INVALID;
  *out = nullptr;
  if (layout->M < 1 || layout->M > kMaxSeg || layout->H < 1) return DFTPAV_E_UNSUPPORTED;
  for (int i = 0; i < layout->M; i++) {
    if (layout->piece_nums[i] < 2) return DFTPAV_E_ONE_PIECE; // "There is only a piece?", traj_optimizer.cpp:38-41
  }
  const dftpav_params &p = h->params;
  if (p.traj_resolution < 1 || p.des_traj_resolution < 1) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  auto *b = new dftpav_batch();
  b->h = h;
  b->B = B;
  b->residency = residency;
  DevLayout &L = b->L;
  fill_dev_layout(*layout, p.traj_resolution, p.des_traj_resolution, L);
  if (L.n > 256 || L.Ntot > 1024 || L.Npts > 32767) {
    delete b;
    return DFTPAV_E_UNSUPPORTED;
  }
  fill_dev_params(p, b->P);
  // Residency plan.  Few trajectories (<= one per CU): latency shape, operators and the corridor
  // staged in LDS.  Many: throughput shape, LDS kept small so that two workgroups share a CU.
  {
    int n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
    int shape = B <= n_cu ? 0 : (B <= 2 * n_cu ? 1 : 2);
    if (residency >= 0) shape = residency;
    if (const char *e = std::getenv("DFTPAV_MODE")) shape = std::atoi(e); // 0 latency, 1 two per CU, 2 four per CU
    b->threads = solver_threads(L, shape);
    int per_cu = shape == 0 ? 1 : (shape == 1 ? 2 : 8);
    if (shape == 2) {
      // one wave per trajectory and eight per CU when a workgroup's LDS fits an eighth of the CU; layouts with more state
      // (many pieces or points: BASELINE configs[4]) take two waves per trajectory and as many workgroups as their LDS allows
      const size_t l64 = solver_lds_bytes(L, b->P, kWave, false, false, 0) + 64;
      if (l64 > 20 * 1024 || L.Npts > 1024) {
        // Two or four waves per trajectory, whichever keeps more waves resident on a CU with the obstacle set installed on
        // the handle right now (its tables are part of a workgroup's LDS): BASELINE configs[4] holds 3 workgroups of 128
        // threads (6 waves) or 2 of 256 (8 waves) per CU -- 415 against 355 ms per 1024.  Without obstacles both give 8
        // waves and the narrower workgroup wastes less in the serial phases.
        const int np = h->S > 0 ? h->sur_pieces : 0;
        size_t best_waves = 0;
        for (int waves = 2; waves <= 4; waves += 2) {
          const int T = waves * kWave;
          const size_t cap = 8 / (size_t)waves; // 256 VGPRs: two waves per SIMD
          auto resident = [&](bool coef) {
            return std::min<size_t>(cap, (160 * 1024) / (solver_lds_bytes(L, b->P, T, false, false, np, coef) + 64));
          };
          const size_t wg = std::max<size_t>(1, np > 0 && np <= kSurCoefLds && resident(true) == resident(false) ? resident(true) : resident(false));
          if (wg * waves > best_waves) {
            best_waves = wg * waves;
            b->threads = T;
            per_cu = (int)wg;
          }
        }
      } else if (residency < 0 && B < 2 * n_cu * per_cu) {
        // Fewer trajectories than two per one-wave slot: an isolated batch of this size ends with most of the device idle
        // behind its longest solves.  Two waves per trajectory on half as many slots finish each solve sooner and keep the
        // time-sliced queue busy: 14.7 k against 13.5 k solves/s at B = 1024, 17.2 k against 12.8 k at 1536, 17.6 k against
        // 15.0 k at 2048, 21.3 k against 19.8 k at 3072; equal at 4096, where the one-wave shape is 12 % ahead as soon as
        // batches follow one another on two streams (the bench).  A caller that streams smaller batches asks for the
        // one-wave shape with dftpav_batch_create_shaped(..., 2, ...).
        b->threads = 2 * kWave;
        const size_t l128 = solver_lds_bytes(L, b->P, b->threads, false, false, 0) + 64;
        per_cu = (int)std::min<size_t>(4, std::max<size_t>(1, (160 * 1024) / l128));
      }
    }
    if (const char *e = std::getenv("DFTPAV_THREADS")) b->threads = std::atoi(e);
    // LDS budget per workgroup: the whole CU, half of it, its share in the throughput shape
    const size_t budget = shape == 0 ? 158 * 1024 : (shape == 1 ? 78 * 1024 : (size_t)(160 * 1024) / per_cu - 512);
    b->op_in_lds = solver_lds_bytes(L, b->P, b->threads, true, false, 512) + 64 <= budget;
    b->cor_in_lds = solver_lds_bytes(L, b->P, b->threads, b->op_in_lds, true, 512) + 64 <= budget;
    if (const char *e = std::getenv("DFTPAV_LDS")) { // bit 0 operators, bit 1 corridor
      int v = std::atoi(e);
      b->op_in_lds = (v & 1) != 0;
      b->cor_in_lds = (v & 2) != 0;
    }
    // More trajectories than resident workgroups: solve lengths differ several-fold, and a launch of one
    // workgroup per trajectory ends with a long tail of half-empty CUs.  Instead `slots` persistent
    // workgroups take trajectories from a queue, run them `slice` iterations at a time and put the
    // unfinished ones back, so all trajectories advance together; when no more than `hand_over` are left
    // they are finished by a second launch in the latency shape (one wide workgroup per CU).
    b->slots = n_cu * per_cu;
    // iterations per slice: long slices cost fewer suspensions, short ones balance the end of a solve better; layouts with
    // many constraint points (costly iterations, few trajectories per slot) take the short ones (measured)
    b->slice = L.Npts > 1024 ? (b->threads >= 4 * kWave ? 32 : 48) : 128;
    b->hand_over = n_cu;
    if (const char *e = std::getenv("DFTPAV_SLOTS")) b->slots = std::atoi(e);
    if (const char *e = std::getenv("DFTPAV_SLICE")) b->slice = std::atoi(e);
    if (const char *e = std::getenv("DFTPAV_HANDOVER")) b->hand_over = std::atoi(e);
    b->sched = B >= b->slots && b->slots > 0 && b->slice > 0;
    if (const char *e = std::getenv("DFTPAV_SCHED")) b->sched = std::atoi(e) != 0 && b->slots > 0 && b->slice > 0;
    if (b->hand_over > B) b->hand_over = B;
    b->threads2 = solver_threads(L, 0);
    b->op_in_lds2 = solver_lds_bytes(L, b->P, b->threads2, true, false, 512) + 64 <= 158 * 1024;
    b->cor_in_lds2 = solver_lds_bytes(L, b->P, b->threads2, b->op_in_lds2, true, 512) + 64 <= 158 * 1024;
  }
  size_t lds = solver_lds_bytes(L, b->P, b->threads, b->op_in_lds, b->cor_in_lds, 512) + 64;
  if (lds > 160 * 1024 || b->threads < 64 || b->threads > 512 || b->threads % 64) {
    delete b;
    return DFTPAV_E_UNSUPPORTED;
  }
  b->NptsPad = ((L.Npts + 63) / 64) * 64;
  const int n = L.n, M = L.M;
  int rc = DFTPAV_OK;
  auto fail = [&](int code) {
    dftpav_batch_destroy(b);
    return code;
  };
#define BCHK(call)                                                             \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);              \
      return fail(DFTPAV_E_HIP);                                               \
    }                                                                          \
  } while (0)
  BCHK(hipMalloc(&b->d_x0, sizeof(double) * (size_t)B * n));
  BCHK(hipMalloc(&b->d_iniS, sizeof(double) * (size_t)B * M * 6));
  BCHK(hipMalloc(&b->d_finS, sizeof(double) * (size_t)B * M * 6));
  BCHK(hipMalloc(&b->d_corridor, sizeof(double) * (size_t)B * L.H * 4 * b->NptsPad));
  BCHK(hipMemset(b->d_corridor, 0, sizeof(double) * (size_t)B * L.H * 4 * b->NptsPad));
  BCHK(hipMalloc(&b->d_pt_piece, sizeof(int16_t) * L.Npts));
  BCHK(hipMalloc(&b->d_pt_j, sizeof(int16_t) * L.Npts));
  // s and y of a stored pair are interleaved element by element: one 16-byte load fetches both (solver.hip, load_block)
  BCHK(hipMalloc(&b->d_histS, sizeof(double) * 2 * (size_t)B * b->P.mem_size * L.npad));
  b->d_histY = b->d_histS + 1; // alias into the same allocation, never freed on its own
  // never-written slots are read (and discarded) by the unconditional prefetch loads: keep them finite
  BCHK(hipMemset(b->d_histS, 0, sizeof(double) * 2 * (size_t)B * b->P.mem_size * L.npad));
  BCHK(hipMalloc(&b->d_histU, sizeof(double) * (size_t)B * b->P.mem_size * 8));
  BCHK(hipMalloc(&b->d_histV, sizeof(double) * (size_t)B * b->P.mem_size * 8));
  BCHK(hipMemset(b->d_histU, 0, sizeof(double) * (size_t)B * b->P.mem_size * 8));
  BCHK(hipMemset(b->d_histV, 0, sizeof(double) * (size_t)B * b->P.mem_size * 8));
  BCHK(hipMalloc(&b->d_histR, sizeof(double) * (size_t)B * b->P.mem_size * 2));
  BCHK(hipMemset(b->d_histR, 0, sizeof(double) * (size_t)B * b->P.mem_size * 2));
  BCHK(hipMalloc(&b->d_x_in, sizeof(double) * (size_t)B * n));
  BCHK(hipMalloc(&b->d_x_out, sizeof(double) * (size_t)B * n));
  BCHK(hipMalloc(&b->d_f, sizeof(double) * (size_t)B));
  BCHK(hipMalloc(&b->d_f_eval, sizeof(double) * (size_t)B));
  BCHK(hipMalloc(&b->d_g, sizeof(double) * (size_t)B * n));
  BCHK(hipMalloc(&b->d_status, sizeof(int) * (size_t)B));
  BCHK(hipMalloc(&b->d_success, sizeof(int) * (size_t)B));
  BCHK(hipMalloc(&b->d_iters, sizeof(int) * (size_t)B));
  BCHK(hipMalloc(&b->d_evals, sizeof(int) * (size_t)B));
  BCHK(hipMalloc(&b->d_hist, sizeof(long long) * (size_t)B));
  BCHK(hipMalloc(&b->d_ticks, sizeof(long long) * (size_t)B));
  BCHK(hipMalloc(&b->d_prof, sizeof(long long) * (size_t)B * 12));
  BCHK(hipMalloc(&b->d_records, (size_t)16 * (B + 1)));
  BCHK(hipMemset(b->d_records, 0, (size_t)16 * (B + 1)));
  // (pinned host memory the kernels can write; without it dftpav_batch_records copies from the device)
  if (std::getenv("DFTPAV_RECORDS_ON_HOST_OFF") == nullptr && hipHostMalloc(reinterpret_cast<void **>(&b->h_records), (size_t)16 * B, hipHostMallocDefault) == hipSuccess) {
    std::memset(b->h_records, 0, (size_t)16 * B);
  } else {
    (void)hipGetLastError();
    b->h_records = nullptr;
  }
  BCHK(hipMalloc(&b->d_dev, sizeof(DevBatch)));
  BCHK(hipMalloc(&b->d_dev2, sizeof(DevBatch)));
  if (b->sched) {
    const size_t stride = (size_t)solver_state_doubles(L, b->P);
    b->qcap = 2 * B; // own trajectories + the stragglers adopted from a previous batch of the same size
    BCHK(hipMalloc(&b->d_queue, sizeof(int) * (size_t)b->qcap));
    BCHK(hipMalloc(&b->d_stragglers, sizeof(int) * (size_t)B));
    BCHK(hipMalloc(&b->d_stragglers2, sizeof(int) * (size_t)B));
    BCHK(hipMalloc(&b->d_sflag, sizeof(int) * (size_t)B));
    BCHK(hipMalloc(&b->d_iota, sizeof(int) * (size_t)B));
    BCHK(hipMalloc(&b->d_qctl, sizeof(unsigned) * 16)); // [0..7] live counters, [8..15] their initial values
    {
      // queue = all trajectories: {head 0, published B, reserved B, unfinished B, stragglers 0}
      const unsigned ctl0[8] = {0u, (unsigned)B, (unsigned)B, (unsigned)B, 0u, 0u, 0u, 0u};
      BCHK(hipMemcpy(b->d_qctl + 8, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
    }
    BCHK(hipMalloc(&b->d_state, sizeof(double) * stride * (size_t)B));
    std::vector<int> iota(B);
    for (int i = 0; i < B; i++) iota[i] = i;
    BCHK(hipMemcpy(b->d_iota, iota.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice));
  }
  BCHK(hipMalloc(&b->d_coef, sizeof(double) * (size_t)B * 12 * L.Ntot));
  BCHK(hipMalloc(&b->d_dt, sizeof(double) * (size_t)B * M));
  BCHK(hipEventCreate(&b->ev0));
  BCHK(hipEventCreate(&b->ev1));
  // constraint point -> (piece, j) tables, the pointid order of traj_optimizer.cpp:486-514
  {
    std::vector<int16_t> pp(L.Npts), pj(L.Npts);
    int pt = 0;
    for (int sg = 0; sg < M; sg++)
      for (int lp = 0; lp < L.piece_nums[sg]; lp++) {
        int K = (lp == 0 || lp == L.piece_nums[sg] - 1) ? L.Kd : L.K;
        for (int j = 0; j <= K; j++, pt++) {
          pp[pt] = (int16_t)(L.seg_piece0[sg] + lp);
          pj[pt] = (int16_t)j;
        }
      }
    BCHK(hipMemcpy(b->d_pt_piece, pp.data(), sizeof(int16_t) * L.Npts, hipMemcpyHostToDevice));
    BCHK(hipMemcpy(b->d_pt_j, pj.data(), sizeof(int16_t) * L.Npts, hipMemcpyHostToDevice));
  }
  // E4 lane plans of the two launch shapes
  for (int which = 0; which < 2; which++) {
    const E4Plan pl = build_e4_plan(L, which == 0 ? b->threads : b->threads2);
    (which == 0 ? b->e4 : b->e4b) = E4Sizes{pl.rounds, pl.groups, pl.left, pl.lcap};
    const std::vector<int> *tabs[5] = {&pl.gtab, &pl.ltab, &pl.wave, &pl.round, &pl.piece};
    for (int t = 0; t < 5; t++) {
      BCHK(hipMalloc(&b->d_e4[which][t], sizeof(int) * tabs[t]->size()));
      BCHK(hipMemcpy(b->d_e4[which][t], tabs[t]->data(), sizeof(int) * tabs[t]->size(), hipMemcpyHostToDevice));
    }
  }
  for (int sg = 0; sg < M; sg++) {
    int N = L.piece_nums[sg];
    std::vector<double> Mop, MopT;
    minco_operator(N, Mop, MopT);
    BCHK(hipMalloc(&b->d_opM[sg], sizeof(double) * Mop.size()));
    BCHK(hipMalloc(&b->d_opMT[sg], sizeof(double) * MopT.size()));
    BCHK(hipMemcpy(b->d_opM[sg], Mop.data(), sizeof(double) * Mop.size(), hipMemcpyHostToDevice));
    BCHK(hipMemcpy(b->d_opMT[sg], MopT.data(), sizeof(double) * MopT.size(), hipMemcpyHostToDevice));
  }
#undef BCHK
  (void)rc;
  h->batches.push_back(b);
  *out = b;
  return DFTPAV_OK;
}

// RealT2VirtualT, traj_optimizer.cpp:360-369
static double real_to_virtual(double rt, double mini_T) {
  return rt > 1.0 + mini_T ? (std::sqrt(2.0 * rt - 1.0 - 2 * mini_T) - 1.0)
                           : (1.0 - std::sqrt(2.0 / (rt - mini_T) - 1.0));
}

static void clamp_col(double *col, double lim) { // traj_optimizer.cpp:65-76
  double nrm = std::sqrt(col[0] * col[0] + col[1] * col[1]);
  if (nrm >= lim) {
    double nx = col[0] / nrm, ny = col[1] / nrm;
    col[0] = nx * (lim - 1.0e-2);
    col[1] = ny * (lim - 1.0e-2);
  }
}

extern "C" int dftpav_batch_upload(dftpav_batch *b, const dftpav_batch_data *d) {
  if (!b || !d || !d->ini_states || !d->fin_states || !d->inner_pts || !d->init_Ts) return DFTPAV_E_INVALID;
  b->pending = false; // new inputs: whatever a chained solve of the old ones left suspended is moot
  dftpav_handle *h = b->h;
  const dftpav_params &p = h->params;
  const DevLayout &L = b->L;
  const int B = b->B, M = L.M, n = L.n;
  const int ninner = L.x_tau0;
  // initTs.minCoeff() < mini_T, traj_optimizer.cpp:30-33
  for (size_t i = 0; i < (size_t)B * M; i++)
    if (d->init_Ts[i] < p.mini_T) return DFTPAV_E_MINI_T;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<double> ini(d->ini_states, d->ini_states + (size_t)B * M * 6);
  std::vector<double> fin(d->fin_states, d->fin_states + (size_t)B * M * 6);
  for (int t = 0; t < B; t++)
    for (int i = 0; i < M; i++) {
      double mv = L.singuls[i] > 0 ? p.max_forward_vel : p.max_backward_vel;
      double ma = L.singuls[i] > 0 ? p.max_forward_acc : p.max_backward_acc;
      double *I = ini.data() + ((size_t)t * M + i) * 6, *F = fin.data() + ((size_t)t * M + i) * 6;
      clamp_col(I + 2, mv);
      clamp_col(F + 2, mv);
      clamp_col(I + 4, ma);
      clamp_col(F + 4, ma);
    }
  // x0 packing, traj_optimizer.cpp:96-115
  b->x0_host.assign((size_t)B * n, 0.0);
  for (int t = 0; t < B; t++) {
    double *x = b->x0_host.data() + (size_t)t * n;
    std::memcpy(x, d->inner_pts + (size_t)t * ninner, sizeof(double) * ninner);
    for (int i = 0; i < M; i++) x[L.x_tau0 + i] = real_to_virtual(d->init_Ts[(size_t)t * M + i], p.mini_T);
    for (int i = 0; i < M - 1; i++) {
      const double *F = fin.data() + ((size_t)t * M + i) * 6;
      x[L.x_gear0 + 2 * i + 0] = F[0];
      x[L.x_gear0 + 2 * i + 1] = F[1];
      x[L.x_ang0 + i] = std::atan2(F[3], F[2]);
    }
  }
  // corridor: the private normalised copy of traj_optimizer.cpp:15,49-52 is made on the device (corridor_layout_kernel):
  // the caller's columns go up as they are, one copy, and are normalised and transposed there
  HIPCHK(h, hipMemcpy(b->d_x0, b->x0_host.data(), sizeof(double) * (size_t)B * n, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(b->d_iniS, ini.data(), sizeof(double) * ini.size(), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(b->d_finS, fin.data(), sizeof(double) * fin.size(), hipMemcpyHostToDevice));
  // a new upload without half-planes does not inherit the previous cycle's: they must follow from
  // dftpav_batch_corridor_from_states / _from_hypotheses before the next solve
  b->have_corridor = false;
  b->cor_rect = false;
  if (d->corridor) {
    const size_t nraw = (size_t)B * L.Npts * L.H * 4;
    if (!b->d_cor_raw) HIPCHK(h, hipMalloc(&b->d_cor_raw, sizeof(double) * nraw));
    HIPCHK(h, hipMemcpyAsync(b->d_cor_raw, d->corridor, sizeof(double) * nraw, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_corridor_layout(b->d_cor_raw, b->d_corridor, B, L.Npts, L.H, b->NptsPad, h->stream));
    // whether they are all rectangles is asked here, in front of the wait this call ends with anyway.  DFTPAV_RECT_CORRIDOR=0: not
    // asked -- the batch keeps the sixteen-double layout (A/B runs, tests); read here, where the layout is decided, not per launch
    int not_rect = 1;
    const char *knob = std::getenv("DFTPAV_RECT_CORRIDOR");
    if (L.H == 4 && L.M == 1 && !(knob && std::strcmp(knob, "0") == 0)) {
      if (!b->d_rect_flag) HIPCHK(h, hipMalloc(&b->d_rect_flag, sizeof(int)));
      HIPCHK(h, launch_quad_rect_check(b->d_corridor, B, L.Npts, b->NptsPad, b->d_rect_flag, h->stream));
      HIPCHK(h, hipMemcpyAsync(&not_rect, b->d_rect_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream)); // the caller's buffer is free again when this returns
    b->cor_rect = not_rect == 0;
    b->have_corridor = true;
    b->cor_t_dirty = true;
  }
  b->t_now = d->t_now;
  b->epis = d->help_eps;
  b->uploaded = true;
  b->solved = false;
  b->coef_override = false;
  b->dev_version = -1; // t_now / help_eps live in the device copy of the launch descriptor: refresh it
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_corridor_from_hypotheses(dftpav_batch *b, const double *states, int n_restarts) {
  if (!b || !states || n_restarts < 1 || b->B % n_restarts) return DFTPAV_E_INVALID;
  b->pending = false; // as dftpav_batch_upload
  dftpav_handle *h = b->h;
  if (!h->d_cells) return DFTPAV_E_INVALID;       // no map
  if (b->L.H != 4) return DFTPAV_E_UNSUPPORTED;   // rectangles
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rc = run_corridor(h, states, (b->B / n_restarts) * b->L.Npts, nullptr, b->d_corridor, b->L.Npts, b->NptsPad, n_restarts);
  if (rc == DFTPAV_OK) {
    b->have_corridor = true;
    b->cor_t_dirty = true;
    b->cor_rect = false; // (not asked: see dftpav_batch::cor_rect)
  }
  return rc;
}
extern "C" int dftpav_batch_corridor_from_states(dftpav_batch *b, const double *states) {
  return dftpav_batch_corridor_from_hypotheses(b, states, 1);
}

extern "C" int dftpav_batch_get_x0(dftpav_batch *b, double *x0) {
  if (!b || !x0 || !b->uploaded) return DFTPAV_E_INVALID;
  std::memcpy(x0, b->x0_host.data(), sizeof(double) * b->x0_host.size());
  return DFTPAV_OK;
}

// Whether the obstacles' coefficient blocks (96 B per piece) are staged in LDS for a launch shape: only if that does not
// cost a resident workgroup -- BASELINE configs[4] at 128 threads holds 3 workgroups per CU without them and 2 with them,
// and one more workgroup hides far more latency than the LDS copy saves.
static int sur_coef_in_lds(const dftpav_batch *b, int threads, bool op, bool cor) {
  const dftpav_handle *h = b->h;
  if (h->S <= 0 || h->sur_pieces > kSurCoefLds) return 0;
  const size_t by_waves = std::max<size_t>(1, 512 / (size_t)threads);
  auto resident = [&](bool coef) {
    const size_t lds = solver_lds_bytes(b->L, b->P, threads, op, cor, h->sur_pieces, coef) + 64;
    return std::min<size_t>(by_waves, (160 * 1024) / lds);
  };
  return resident(true) == resident(false) ? 1 : 0;
}

static DevBatch make_dev(dftpav_batch *b) {
  DevBatch D{};
  D.L = b->L;
  D.P = b->P;
  D.B = b->n_active > 0 ? b->n_active : b->B;
  D.x0 = b->d_x0;
  D.iniS = b->d_iniS;
  D.finS = b->d_finS;
  D.corridor = b->d_corridor;
  D.NptsPad = b->NptsPad;
  D.pt_piece = b->d_pt_piece;
  D.pt_j = b->d_pt_j;
  D.op_in_lds = b->op_in_lds ? 1 : 0;
  D.cor_in_lds = b->cor_in_lds ? 1 : 0;
  D.e4_rounds = b->e4.rounds;
  D.e4_groups = b->e4.groups;
  D.e4_left = b->e4.left;
  D.e4_lcap = b->e4.lcap;
  D.e4_gtab = b->d_e4[0][0];
  D.e4_ltab = b->d_e4[0][1];
  D.e4_wave = b->d_e4[0][2];
  D.e4_round = b->d_e4[0][3];
  D.e4_piece = b->d_e4[0][4];
  int off = 0;
  for (int i = 0; i < kMaxSeg; i++) {
    D.opM[i] = b->d_opM[i];
    D.opMT[i] = b->d_opMT[i];
    D.op_off[i] = off;
    if (i < b->L.M) off += 6 * b->L.piece_nums[i] * (b->L.piece_nums[i] + 5);
  }
  dftpav_handle *h = b->h;
  D.sur.S = h->S;
  D.sur_np = h->sur_pieces;
  D.sur_coef_lds = sur_coef_in_lds(b, b->threads, b->op_in_lds, b->cor_in_lds);
  D.sur.piece_off = h->d_sur_off;
  D.sur.durations = h->d_sur_dur;
  D.sur.theta = h->d_sur_theta;
  D.sur.bbox = h->d_sur_bbox;
  D.sur.coeffs = h->d_sur_coef;
  D.sur.total = h->d_sur_total;
  D.sur.start = h->d_sur_start;
  D.t_now = b->t_now;
  D.epis = b->epis;
  D.histS = b->d_histS;
  D.histY = b->d_histY;
  D.histU = b->d_histU;
  D.histV = b->d_histV;
  D.histR = b->d_histR;
  D.histM = b->d_histM;
  D.queue = b->d_queue;
  D.qctl = b->d_qctl;
  D.stragglers = b->d_stragglers;
  D.stragglers2 = b->d_stragglers2;
  D.qcap = b->qcap;
  D.state = b->d_state;
  D.sflag = b->d_sflag;
  D.state_stride = solver_state_doubles(b->L, b->P);
  D.x_in = b->d_x_in;
  D.x_out = b->d_x_out;
  D.f_out = b->d_f;
  D.g_out = b->d_g;
  D.f_eval = b->d_f_eval;
  D.status = b->d_status;
  D.success = b->d_success;
  D.iters = b->d_iters;
  D.evals = b->d_evals;
  D.hist_sum = b->d_hist;
  D.ticks = b->d_ticks;
  D.records = b->d_records;
  D.records_host = b->h_records;
  D.prof = b->prof_on ? b->d_prof : nullptr;
  D.coef_out = b->d_coef;
  D.dt_out = b->d_dt;
  D.trace = b->d_trace;
  D.trace_b = b->trace_b;
  D.trace_cap = b->trace_cap;
  D.trace_n = b->trace_n;
  return D;
}

// refreshes the device copy of the launch descriptor when something it captures changed
static int sync_dev(dftpav_batch *b, DevBatch &D) {
  dftpav_handle *h = b->h;
  // the kernel numbers (constraint point, obstacle) pairs with 16 bits and keeps a 16-bit mask of obstacles per point
  if (h->S > 16 || (long long)b->L.Npts * h->S > 65535 || h->sur_pieces > 512) {
    h->err = "too many moving obstacles for this layout (S <= 16, Npts * S <= 65535, <= 512 pieces in all)";
    return DFTPAV_E_UNSUPPORTED;
  }
  if (b->order == DFTPAV_ORDER_REFERENCE && h->S != b->ref_S) { // the obstacle set changed after the order was chosen
    h->err = "reference order: the number of moving obstacles changed -- choose the order again (dftpav_batch_set_order)";
    return DFTPAV_E_UNSUPPORTED;
  }
  D = make_dev(b);
  int version = h->sur_version * 4 + (b->prof_on ? 1 : 0) + (b->uploaded ? 2 : 0);
  if (version != b->dev_version) {
    if (!b->h_stage) HIPCHK(h, hipHostMalloc(reinterpret_cast<void **>(&b->h_stage), 2 * sizeof(DevBatch), hipHostMallocDefault));
    if (!b->stage_ev) HIPCHK(h, hipEventCreateWithFlags(&b->stage_ev, hipEventDisableTiming));
    if (b->stage_busy) HIPCHK(h, hipEventSynchronize(b->stage_ev)); // the previous copies out of the staging area (long done)
    b->h_stage[0] = D;
    DevBatch &D2 = b->h_stage[1];
    D2 = D; // the same batch in the latency shape (follow-up launch of a scheduled solve)
    D2.op_in_lds = b->op_in_lds2 ? 1 : 0;
    D2.cor_in_lds = b->cor_in_lds2 ? 1 : 0;
    D2.sur_coef_lds = sur_coef_in_lds(b, b->threads2, b->op_in_lds2, b->cor_in_lds2);
    D2.e4_rounds = b->e4b.rounds;
    D2.e4_groups = b->e4b.groups;
    D2.e4_left = b->e4b.left;
    D2.e4_lcap = b->e4b.lcap;
    D2.e4_gtab = b->d_e4[1][0];
    D2.e4_ltab = b->d_e4[1][1];
    D2.e4_wave = b->d_e4[1][2];
    D2.e4_round = b->d_e4[1][3];
    D2.e4_piece = b->d_e4[1][4];
    HIPCHK(h, hipMemcpyAsync(b->d_dev, &b->h_stage[0], sizeof(DevBatch), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(b->d_dev2, &b->h_stage[1], sizeof(DevBatch), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(b->stage_ev, h->stream));
    b->stage_busy = true;
    b->dev_version = version;
  }
  return DFTPAV_OK;
}

// debug/test hook: switch the in-kernel phase profiler on/off and read it back ([B][12] shader clocks)
extern "C" int dftpav_debug_profile(dftpav_batch *b, int enable, long long *out) {
  if (!b) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (out) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, b->d_prof, sizeof(long long) * (size_t)b->B * 12, hipMemcpyDeviceToHost));
  }
  b->prof_on = enable != 0;
  return DFTPAV_OK;
}

// Records every evaluation of one trajectory during the following solves (what lbfgs_optimize shows its progress callback,
// lbfgs.hpp:242-249,617-624, but per evaluation): used by the lockstep parity test against the reference's line search.
extern "C" int dftpav_batch_trace_range(dftpav_batch *b, int first, int count, int max_evals) {
  if (!b || max_evals < 0 || (max_evals > 0 && (first < 0 || count < 1 || first + count > b->B))) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (max_evals > 0 && b->order == DFTPAV_ORDER_REFERENCE) { // solver_ref.hip records nothing: say so instead of returning empty traces
    h->err = "dftpav_batch_trace: not available in the reference order (the lockstep replay is a check of the device order)";
    return DFTPAV_E_UNSUPPORTED;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b->d_trace) {
    HIPCHK(h, hipFree(b->d_trace));
    b->d_trace = nullptr;
  }
  b->trace_b = -1;
  b->trace_cap = 0;
  b->trace_n = 0;
  if (max_evals > 0) {
    const size_t nd = (size_t)count * (8 + (size_t)max_evals * (3 * (size_t)b->L.npad + 8));
    HIPCHK(h, hipMalloc(&b->d_trace, sizeof(double) * nd));
    HIPCHK(h, hipMemset(b->d_trace, 0, sizeof(double) * nd));
    b->trace_b = first;
    b->trace_n = count;
    b->trace_cap = max_evals;
  }
  b->dev_version = -1;
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_trace(dftpav_batch *b, int traj, int max_evals) { return dftpav_batch_trace_range(b, traj, 1, max_evals); }

extern "C" int dftpav_batch_get_trace_of(dftpav_batch *b, int traj, double *out, int *n_evals) {
  if (!b || !n_evals || !b->d_trace || traj < b->trace_b || traj >= b->trace_b + b->trace_n) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int n = b->L.n, npad = b->L.npad;
  const size_t stride = 3 * (size_t)npad + 8;
  const size_t block = 8 + (size_t)b->trace_cap * stride;
  std::vector<double> raw(block);
  HIPCHK(h, hipMemcpy(raw.data(), b->d_trace + (size_t)(traj - b->trace_b) * block, sizeof(double) * block, hipMemcpyDeviceToHost));
  int cnt = (int)raw[0];
  if (cnt > b->trace_cap) cnt = b->trace_cap;
  *n_evals = cnt;
  if (out)
    for (int i = 0; i < cnt; i++) {
      const double *r = raw.data() + 8 + (size_t)i * stride;
      double *o = out + (size_t)i * (3 * n + 4);
      std::memcpy(o, r, sizeof(double) * n);
      std::memcpy(o + n, r + npad, sizeof(double) * n);
      std::memcpy(o + 2 * n, r + 2 * npad, sizeof(double) * n);
      std::memcpy(o + 3 * n, r + 3 * npad, sizeof(double) * 4);
    }
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_get_trace(dftpav_batch *b, double *out, int *n_evals) {
  if (!b) return DFTPAV_E_INVALID;
  return dftpav_batch_get_trace_of(b, b->trace_b, out, n_evals);
}

// every launch of the solve kernel for a batch goes through here: the reference-order kernel when the batch asks for it
static hipError_t launch_ref(dftpav_batch *b, const DevBatch &D, int mode, int scheduled) {
  const RefPlan &pl = b->ref_plan;
  if (pl.kind < kRefQuad || mode == kModeCoeffs)
    return launch_solver_ref(D, b->d_dev, mode, b->d_ref_tab, b->d_ref_scratch, pl, scheduled, b->h->stream);
  // the QUAD shapes read their own layout of the corridor; the one-segment kernel's fast instance (H = 4, help_eps == 0.0) reads a
  // batch of rectangles as 10 doubles per point (solver_ref4.hip: RECT)
  const bool rect = b->cor_rect && pl.kind == kRefQuad && pl.fast && D.epis == 0.0;
  if (b->cor_t_dirty || rect != b->cor_t_rect) {
    const hipError_t e = pl.kind == kRefQuadSeg ? launch_quadm_corridor(D, b->d_cor_t, b->h->stream) : launch_quad_corridor(D, b->d_cor_t, rect, b->h->stream);
    if (e != hipSuccess) return e;
    b->cor_t_dirty = false;
    b->cor_t_rect = rect;
  }
  // A batch that has the device to itself (the default; dftpav_batch_set_hand_over(b, 0) says that other batches follow on other
  // streams) takes every wave slot and hands its last trajectories to the WAVE shape.  In a stream of batches the launch is half as
  // wide as the batch (solver_ref.hip: quad_shape).
  const bool alone = b->hand_over != 0 && scheduled && mode == kModeSolve;
  return launch_solver_quad(D, b->d_dev, mode, b->d_ref_tab, b->d_cor_t, rect, b->d_ref_scratch, pl, scheduled, alone, b->h->stream);
}
// test hook: the layout of the QUAD shapes' corridor copy the last reference-order launch of this batch read -- 1: rectangles (10
// doubles per point), 0: sixteen doubles per point, -1: no current copy (another shape, or the corridor changed since)
extern "C" int dftpav_debug_batch_corridor_layout(const dftpav_batch *b) {
  if (!b || b->order != DFTPAV_ORDER_REFERENCE || b->ref_plan.kind < kRefQuad || b->cor_t_dirty) return -1;
  return b->cor_t_rect ? 1 : 0;
}
static hipError_t launch_for(dftpav_batch *b, const DevBatch &D, int mode) {
  if (b->order == DFTPAV_ORDER_REFERENCE) return launch_ref(b, D, mode, 0);
  return launch_solver(D, b->d_dev, mode, b->threads, b->B, SchedArgs{0, 0, 0, nullptr}, b->h->stream);
}

// The coefficient tables of the four substitution sweeps of BandedSystem::solve / solveAdj (poly_traj_utils.hpp:805-852) for
// a segment of N pieces, row-oriented: row i of a sweep takes tab[i][0..5] against its six predecessors in the order the
// reference's column loops reach it (solver_ref.hip, sweep).  From the reference's own LU (banded_factorize, traj_math.h).
//   [0] solve, forward:     L(i, i-6+k)      [1] solve, backward:    U(i, i+6-k), then / U(i,i)
//   [2] solveAdj, forward:  U(i-6+k, i), then / U(i,i)               [3] solveAdj, backward: L(i+6-k, i)
//   each row 8 doubles: the six coefficients, U(i,i), 1 / U(i,i).
// Returns false if a row of a middle block (rows 6 .. 6N-7) has another non-zero pattern than the kernel assumes there.
static bool reference_order_tables(int N, std::vector<double> &out) {
  const int n6 = 6 * N;
  std::vector<double> band((size_t)n6 * 13, 0.0);
  BandedLU A{n6, 6, 6, band.data()};
  minco_fill(A, N);
  banded_factorize(A);
  out.assign((size_t)(4 * 48) * N, 0.0); // the full form [4][6N][8]; reference_order_pack_tables makes the kernel's
  double *t[4];
  for (int q = 0; q < 4; q++) t[q] = out.data() + (size_t)q * 8 * n6;
  bool ok = true;
  for (int i = 0; i < n6; i++) {
    for (int k = 0; k < 6; k++) {
      const int jl = i - 6 + k, jh = i + 6 - k;
      if (jl >= 0) {
        t[0][8 * i + k] = A.at(i, jl);
        t[2][8 * i + k] = A.at(jl, i);
      }
      if (jh <= n6 - 1) {
        t[1][8 * i + k] = A.at(i, jh);
        t[3][8 * i + k] = A.at(jh, i);
      }
    }
    for (int q = 0; q < 4; q++) {
      int m = 0;
      for (int k = 0; k < 6; k++)
        if (t[q][8 * i + k] != 0.0) m |= 1 << k;
      if (i >= 6 && i < n6 - 6 && m != reference_order_interior_mask(q, i % 6)) ok = false;
      t[q][8 * i + 6] = A.at(i, i);
      { // the kernel divides by the diagonal through its reciprocal (solver_ref.hip: div_by_rcp): the bits of the division as long
        // as the diagonal is an ordinary number -- O(1) for every MINCO system; anything else is refused here
        const double dg = std::fabs(A.at(i, i));
        if (!(dg >= 0x1p-500 && dg <= 0x1p500)) ok = false;
        t[q][8 * i + 7] = 1.0 / A.at(i, i);
      }
    }
  }
  return ok;
}
// test hook (host only): the correctly rounded sin / cos the reference-order kernel uses for the junction angles (cr_trig.h),
// run on the host for n arguments
extern "C" int dftpav_debug_cr_sincos(int n, const double *x, double *s, double *c) {
  if (n < 0 || !x || !s || !c) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++) dftpav::crt::sincos(x[i], s[i], c[i]);
  return DFTPAV_OK;
}
// test hook (host only): which = 0 exp, 1 log, 2 x^3 -- the correctly rounded functions of cr_trig.h for n arguments; 3 / 4: exp / log
// by their accurate phase alone (what the quick phase with its rounding test stands in front of)
extern "C" int dftpav_debug_cr_fn(int which, int n, const double *x, double *y) {
  if (n < 0 || !x || !y || which < 0 || which > 6) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++) {
    switch (which) {
      case 0: y[i] = dftpav::crt::exp_cr(x[i]); break;
      case 1: y[i] = dftpav::crt::log_cr(x[i]); break;
      case 2: y[i] = dftpav::crt::cube_cr(x[i]); break;
      case 3: y[i] = dftpav::crt::exp_cr_impl<false>(x[i]); break;
      case 4: y[i] = dftpav::crt::log_cr_impl<false>(x[i]); break;
      case 5: y[i] = dftpav::crt::atan(x[i]); break;   // (the step kernels' reference order: validate / states / frontend)
      default: y[i] = dftpav::crt::tan(x[i]); break;
    }
  }
  return DFTPAV_OK;
}
extern "C" int dftpav_debug_cr_atan2(int n, const double *y, const double *x, double *out) {
  if (n < 0 || !x || !y || !out) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++) out[i] = dftpav::crt::atan2(y[i], x[i]);
  return DFTPAV_OK;
}
// test hook (host only): the sweep tables of a segment of N pieces, [4][6N][8]; returns 1 if the middle blocks have the assumed pattern
extern "C" int dftpav_debug_reference_tables(int N, double *out) {
  if (N < 2) return DFTPAV_E_INVALID;
  std::vector<double> tab;
  const bool ok = reference_order_tables(N, tab);
  if (out) std::memcpy(out, tab.data(), sizeof(double) * tab.size());
  return ok ? 1 : 0;
}

// test hook (host only): the same tables in the layout the kernel reads (solver_ref.hip: "The table of one sweep"): blocks in
// traversal order, whole rows at the two ends, only the coefficients of the interior pattern in between; *n_doubles = their size
extern "C" int dftpav_debug_reference_tables_packed(int N, double *out, int *n_doubles) {
  if (N < 2 || !n_doubles) return DFTPAV_E_INVALID;
  *n_doubles = (int)reference_order_table_doubles(N);
  if (!out) return DFTPAV_OK;
  std::vector<double> full;
  const bool ok = reference_order_tables(N, full);
  reference_order_pack_tables(N, full.data(), out);
  return ok ? 1 : 0;
}

// the ring, the flags and the state records of a scheduled solve, for a batch whose device-order plan did not need them
static hipError_t ensure_ring_buffers(dftpav_batch *b) {
  if (b->d_queue && b->d_sflag && b->d_iota && b->d_qctl && b->d_state) return hipSuccess;
  const int B = b->B;
  const size_t stride = (size_t)solver_state_doubles(b->L, b->P);
  int *q = nullptr, *fl = nullptr, *io = nullptr;
  unsigned *ctl = nullptr;
  double *st = nullptr;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t r) {
    if (e == hipSuccess && r != hipSuccess) e = r;
  };
  const int qcap = 2 * B;
  chk(hipMalloc(&q, sizeof(int) * (size_t)qcap));
  chk(hipMalloc(&fl, sizeof(int) * (size_t)B));
  chk(hipMalloc(&io, sizeof(int) * (size_t)B));
  chk(hipMalloc(&ctl, sizeof(unsigned) * 16));
  chk(hipMalloc(&st, sizeof(double) * stride * (size_t)B));
  if (e == hipSuccess) {
    const unsigned ctl0[8] = {0u, (unsigned)B, (unsigned)B, (unsigned)B, 0u, 0u, 0u, 0u};
    chk(hipMemcpy(ctl + 8, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
    std::vector<int> iota(B);
    for (int i = 0; i < B; i++) iota[i] = i;
    chk(hipMemcpy(io, iota.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice));
  }
  if (e != hipSuccess) {
    for (void *p : {(void *)q, (void *)fl, (void *)io, (void *)ctl, (void *)st})
      if (p) (void)hipFree(p);
    (void)hipGetLastError();
    return e;
  }
  // (a batch either has all of them -- its device-order plan is scheduled -- or none)
  b->d_queue = q;
  b->d_sflag = fl;
  b->d_iota = io;
  b->d_qctl = ctl;
  b->d_state = st;
  b->qcap = qcap;
  b->dev_version = -1; // the device descriptor carries these pointers
  return hipSuccess;
}

extern "C" int dftpav_batch_set_order(dftpav_batch *b, int order) {
  if (!b || (order != DFTPAV_ORDER_DEVICE && order != DFTPAV_ORDER_REFERENCE)) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (order == b->order && (order == DFTPAV_ORDER_DEVICE || b->ref_S == h->S)) return DFTPAV_OK;
  if (order == DFTPAV_ORDER_REFERENCE && b->d_trace) { // the reference-order kernel does not record evaluations
    h->err = "reference order: dftpav_batch_trace is a device-order facility -- switch the trace off first";
    return DFTPAV_E_UNSUPPORTED;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (order == DFTPAV_ORDER_REFERENCE) {
    if (!reference_order_supported(b->L, b->P, h->S)) {
      h->err = "reference order: n <= 256 variables, H <= 12 half-planes, 5 H + S + 4 <= 64 terms per point, every gear segment >= 2 pieces, 159 KB of LDS";
      return DFTPAV_E_UNSUPPORTED;
    }
    int n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
    const RefPlan pl = reference_order_plan(b->L, b->P, h->S, b->B, n_cu, b->residency == 2, ref_options_from_env());
    if (pl.kind != kRefTeam && ensure_ring_buffers(b) != hipSuccess) {
      h->err = "reference order: no device memory for the ring of this batch";
      return DFTPAV_E_HIP;
    }
    // Everything else is built on the side and committed to the batch together: a failure leaves the batch as it was (the
    // order, its plan, the corridor copy, the tables and the term records) and frees what this call allocated.
    const bool new_tab = !b->d_ref_tab || !b->d_ref_scratch || b->ref_S != h->S;
    std::vector<double> tab; // the tables of the segments, one after the other
    for (int sg = 0; new_tab && sg < b->L.M; sg++) {
      std::vector<double> one;
      if (!reference_order_tables(b->L.piece_nums[sg], one)) {
        h->err = "reference order: the LU factors of this band system do not have the pattern the kernel assumes";
        return DFTPAV_E_UNSUPPORTED;
      }
      std::vector<double> packed(reference_order_table_doubles(b->L.piece_nums[sg]));
      reference_order_pack_tables(b->L.piece_nums[sg], one.data(), packed.data());
      tab.insert(tab.end(), packed.begin(), packed.end());
    }
    double *cor_t = b->d_cor_t, *d_tab = nullptr, *d_scr = nullptr; // (the corridor copy's size does not change: a batch keeps its first)
    double *hist_m = b->d_histM;                                    // (nor does the history mirror's)
    auto undo = [&](const char *msg) {
      if (cor_t != b->d_cor_t) (void)hipFree(cor_t);
      if (hist_m != b->d_histM) (void)hipFree(hist_m);
      if (d_tab) (void)hipFree(d_tab);
      if (d_scr) (void)hipFree(d_scr);
      (void)hipGetLastError();
      h->err = msg;
      return DFTPAV_E_HIP; // the order stays as it was, the batch usable
    };
    if (pl.kind >= kRefQuad && !cor_t && hipMalloc(&cor_t, sizeof(double) * reference_order_quad_corridor_doubles(b->L, b->B)) != hipSuccess)
      return undo("reference order: no device memory for the QUAD shape's copy of the corridor");
    // cleared as histS is: the elements of a row that are no variables must read +0.0 (solver_ref4.hip: q4_rec_sum)
    if (pl.kind == kRefQuad && !hist_m &&
        (hipMalloc(&hist_m, sizeof(double) * quad_mirror_doubles(b->L, b->B)) != hipSuccess ||
         hipMemset(hist_m, 0, sizeof(double) * quad_mirror_doubles(b->L, b->B)) != hipSuccess))
      return undo("reference order: no device memory for the QUAD shape's mirror of the history ends");
    if (new_tab && (hipMalloc(&d_tab, sizeof(double) * tab.size()) != hipSuccess ||
                    hipMalloc(&d_scr, sizeof(double) * reference_order_scratch_doubles(b->L, b->B, h->S)) != hipSuccess ||
                    hipMemcpy(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) != hipSuccess))
      return undo("reference order: no device memory for the term records of this batch");
    if (new_tab) {
      if (b->d_ref_tab) (void)hipFree(b->d_ref_tab);
      if (b->d_ref_scratch) (void)hipFree(b->d_ref_scratch);
      b->d_ref_tab = d_tab;
      b->d_ref_scratch = d_scr;
      b->ref_S = h->S;
    }
    if (pl.kind >= kRefQuad) b->cor_t_dirty = true;
    b->d_cor_t = cor_t;
    b->d_histM = hist_m;
    b->dev_version = -1; // (the device descriptor carries the mirror's pointer)
    b->ref_plan = pl;
  }
  b->order = order;
  b->solved = false;
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_get_order(const dftpav_batch *b) { return b ? b->order : DFTPAV_E_INVALID; }

extern "C" int dftpav_batch_eval(dftpav_batch *b, const double *x, double *f, double *g) {
  if (!b || !x || !b->uploaded || !b->have_corridor) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  const size_t nb = (size_t)b->B * b->L.n;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(b->d_x_in, x, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, launch_for(b, D, kModeEval));
  if (f) HIPCHK(h, hipMemcpyAsync(f, b->d_f_eval, sizeof(double) * b->B, hipMemcpyDeviceToHost, h->stream));
  if (g) HIPCHK(h, hipMemcpyAsync(g, b->d_g, sizeof(double) * nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// the follow-up launch of a scheduled solve: the stragglers in the latency shape
static int launch_stragglers(dftpav_batch *b, const DevBatch &D, int source) {
  dftpav_handle *h = b->h;
  DevBatch D2 = D;
  D2.op_in_lds = b->op_in_lds2 ? 1 : 0;
  D2.cor_in_lds = b->cor_in_lds2 ? 1 : 0;
  D2.sur_coef_lds = sur_coef_in_lds(b, b->threads2, b->op_in_lds2, b->cor_in_lds2);
  D2.e4_rounds = b->e4b.rounds;
  D2.e4_groups = b->e4b.groups;
  D2.e4_left = b->e4b.left;
  D2.e4_lcap = b->e4b.lcap;
  D2.e4_gtab = b->d_e4[1][0];
  D2.e4_ltab = b->d_e4[1][1];
  D2.e4_wave = b->d_e4[1][2];
  D2.e4_round = b->d_e4[1][3];
  D2.e4_piece = b->d_e4[1][4];
  HIPCHK(h, launch_solver(D2, b->d_dev2, kModeSolve, b->threads2, b->hand_over, SchedArgs{source, 0, 0, nullptr}, h->stream));
  return DFTPAV_OK;
}

// a chained solve left the stragglers of `b` suspended: finish them now (no-op otherwise)
static int finish_pending(dftpav_batch *b) {
  if (!b->pending) return DFTPAV_OK;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  if (b->hand_over > 0)
    if (int rc = launch_stragglers(b, D, 2)) return rc;
  HIPCHK(h, hipEventRecord(b->ev1, h->stream));
  b->pending = false;
  return DFTPAV_OK;
}

static bool chain_compatible(const dftpav_batch *a, const dftpav_batch *b) {
  return a->h == b->h && a->sched && b->sched && a->B == b->B && a->threads == b->threads &&
         a->op_in_lds == b->op_in_lds && a->cor_in_lds == b->cor_in_lds && a->threads2 == b->threads2 &&
         a->hand_over == b->hand_over && a->hand_over > 0 && a->NptsPad == b->NptsPad && a->prof_on == b->prof_on &&
         std::memcmp(&a->L, &b->L, sizeof(DevLayout)) == 0 && std::memcmp(&a->P, &b->P, sizeof(DevParams)) == 0 &&
         a->t_now == b->t_now && a->epis == b->epis;
}

static int solve_impl(dftpav_batch *b, dftpav_batch *prev, bool chained) {
  if (!b || !b->uploaded || !b->have_corridor || prev == b) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  b->pending = false; // a new solve of this batch supersedes whatever it had suspended
  if (prev && prev->pending && !(chained && chain_compatible(b, prev)))
    if (int rc = finish_pending(prev)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, hipEventRecord(b->ev0, h->stream));
  if (b->order == DFTPAV_ORDER_REFERENCE) {
    if (b->ref_plan.ring) {
      // more trajectories than resident waves: persistent workgroups whose waves pop trajectories from the ring and run them a
      // slice of iterations at a time (solver_ref.hip); queue = all trajectories, flags cleared, counters reset on the stream
      HIPCHK(h, launch_ring_reset(D, h->stream));
      HIPCHK(h, launch_ref(b, D, kModeSolve, 1));
    } else {
      HIPCHK(h, launch_for(b, D, kModeSolve)); // every trajectory has its team from the start
    }
  } else if (!b->sched) {
    HIPCHK(h, launch_solver(D, b->d_dev, kModeSolve, b->threads, b->B, SchedArgs{0, 0, 0, nullptr}, h->stream));
  } else {
    // queue = all trajectories, flags cleared, counters reset: device-to-device, nothing waits on the host
    HIPCHK(h, hipMemcpyAsync(b->d_queue, b->d_iota, sizeof(int) * (size_t)b->B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(b->d_sflag, 0, sizeof(int) * (size_t)b->B, h->stream));
    HIPCHK(h, hipMemcpyAsync(b->d_qctl, b->d_qctl + 8, sizeof(unsigned) * 8, hipMemcpyDeviceToDevice, h->stream));
    const int grid = b->slots < b->B ? b->slots : b->B;
    const bool adopt = chained && prev && prev->pending;
    if (adopt) {
      DevBatch Dprev;
      if (int rc = sync_dev(prev, Dprev)) return rc;
      HIPCHK(h, launch_adopt(D, Dprev, h->stream));
      HIPCHK(h, launch_solver(D, b->d_dev, kModeSolve, b->threads, grid, SchedArgs{1, b->slice, b->hand_over, prev->d_dev}, h->stream));
      // whatever of the adopted trajectories met this batch's end game: finished in the latency shape (normally none:
      // the workgroups of this launch leave at once)
      if (int rc = launch_stragglers(prev, Dprev, 3)) return rc;
      HIPCHK(h, hipEventRecord(prev->ev1, h->stream));
      prev->pending = false;
    } else {
      HIPCHK(h, launch_solver(D, b->d_dev, kModeSolve, b->threads, grid, SchedArgs{1, b->slice, b->hand_over, nullptr}, h->stream));
    }
    if (chained && b->hand_over > 0) {
      b->pending = true;
    } else if (b->hand_over > 0) {
      if (int rc = launch_stragglers(b, D, 2)) return rc;
    }
  }
  HIPCHK(h, hipEventRecord(b->ev1, h->stream));
  b->timed = true;
  b->solved = true;
  b->coef_override = false;
  return DFTPAV_OK;
}

extern "C" int dftpav_mark(dftpav_handle *h, int slot) {
  if (!h || slot < 0 || slot > 1) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->mark[slot]) HIPCHK(h, hipEventCreate(&h->mark[slot]));
  HIPCHK(h, hipEventRecord(h->mark[slot], h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_marks_elapsed_ms(dftpav_handle *from, int from_slot, dftpav_handle *to, int to_slot, float *ms) {
  if (!from || !to || !ms || from_slot < 0 || from_slot > 1 || to_slot < 0 || to_slot > 1 || !from->mark[from_slot] ||
      !to->mark[to_slot] || from->device != to->device)
    return DFTPAV_E_INVALID;
  HIPCHK(to, hipSetDevice(to->device));
  HIPCHK(to, hipEventSynchronize(to->mark[to_slot]));
  HIPCHK(to, hipEventElapsedTime(ms, from->mark[from_slot], to->mark[to_slot]));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_set_hand_over(dftpav_batch *b, int hand_over) {
  if (!b) return DFTPAV_E_INVALID;
  if (int rc = finish_pending(b)) return rc;
  if (hand_over < 0) { // back to the plan's default: one trajectory per CU
    int n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, b->h->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
    hand_over = n_cu;
  }
  b->hand_over = hand_over < b->B ? hand_over : b->B;
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_solve_async(dftpav_batch *b) { return solve_impl(b, nullptr, false); }

extern "C" int dftpav_batch_solve_chained(dftpav_batch *b, dftpav_batch *prev) { return solve_impl(b, prev, true); }

extern "C" int dftpav_batch_finish(dftpav_batch *b) {
  if (!b) return DFTPAV_E_INVALID;
  return finish_pending(b);
}

extern "C" int dftpav_batch_sync(dftpav_batch *b) {
  if (!b) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_last_solve_ms(dftpav_batch *b, float *ms) {
  if (!b || !ms || !b->timed) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventSynchronize(b->ev1));
  HIPCHK(h, hipEventElapsedTime(ms, b->ev0, b->ev1));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_results(dftpav_batch *b, double *x, double *final_cost, int *status, int *success,
                                    int *iters, int *evals, long long *hist_sum, double *latency_us) {
  if (!b || !b->solved) return DFTPAV_E_INVALID; // nothing solved since the last upload
  dftpav_handle *h = b->h;
  const int B = b->B;
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (x) HIPCHK(h, hipMemcpy(x, b->d_x_out, sizeof(double) * (size_t)B * b->L.n, hipMemcpyDeviceToHost));
  if (final_cost) HIPCHK(h, hipMemcpy(final_cost, b->d_f, sizeof(double) * B, hipMemcpyDeviceToHost));
  if (status) HIPCHK(h, hipMemcpy(status, b->d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (success) HIPCHK(h, hipMemcpy(success, b->d_success, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(h, hipMemcpy(iters, b->d_iters, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (evals) HIPCHK(h, hipMemcpy(evals, b->d_evals, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (hist_sum) HIPCHK(h, hipMemcpy(hist_sum, b->d_hist, sizeof(long long) * B, hipMemcpyDeviceToHost));
  if (latency_us) {
    std::vector<long long> t(B);
    HIPCHK(h, hipMemcpy(t.data(), b->d_ticks, sizeof(long long) * B, hipMemcpyDeviceToHost));
    for (int i = 0; i < B; i++) latency_us[i] = (double)t[i] * 0.01; // wall_clock64: 100 MHz
  }
  return DFTPAV_OK;
}

// ------------------------------------------------------------------ RCCL behind the C-ABI
// The one collective of the path: an all-gather of 16-byte result records over xGMI.  RCCL is loaded at the first use
// (dlopen by its soname: inside a process that already holds an RCCL -- PyTorch ships one -- this is that same copy, so a
// process never runs two), which keeps the library loadable where no RCCL is installed: only these entry points fail there.
namespace {
struct RcclUniqueId {
  char internal[DFTPAV_UNIQUE_ID_BYTES];
};
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(RcclUniqueId *) = nullptr;
  int (*CommInitRank)(void **, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  bool ok = false;
};
RcclApi &rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (!api.lib) return;
    api.GetUniqueId = reinterpret_cast<int (*)(RcclUniqueId *)>(dlsym(api.lib, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<int (*)(void **, int, RcclUniqueId, int)>(dlsym(api.lib, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(api.lib, "ncclCommDestroy"));
    api.AllGather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, hipStream_t)>(dlsym(api.lib, "ncclAllGather"));
    api.GetErrorString = reinterpret_cast<const char *(*)(int)>(dlsym(api.lib, "ncclGetErrorString"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather;
  });
  return api;
}
constexpr int kNcclUint8 = 1; // ncclUint8 == ncclChar + 1 (rccl.h)
} // namespace
#define RCCLCHK(h, call)                                                                                        \
  do {                                                                                                          \
    int e_ = (call);                                                                                            \
    if (e_ != 0) {                                                                                              \
      (h)->err = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e_) : "rccl error"); \
      return DFTPAV_E_COMM;                                                                                     \
    }                                                                                                           \
  } while (0)

extern "C" int dftpav_comm_unique_id(void *id) {
  if (!id) return DFTPAV_E_INVALID;
  if (!rccl().ok) return DFTPAV_E_COMM;
  RcclUniqueId u;
  if (rccl().GetUniqueId(&u) != 0) return DFTPAV_E_COMM;
  std::memcpy(id, u.internal, DFTPAV_UNIQUE_ID_BYTES);
  return DFTPAV_OK;
}
// Is RCCL loadable here?  (dlopen + dlsym only: no bootstrap root is started, unlike dftpav_comm_unique_id.)
extern "C" int dftpav_comm_available(void) { return rccl().ok ? 1 : 0; }
// lets go of h's reference to its communicator; g_comm_mu is held by the caller, h's stream is drained
static void comm_release_locked(dftpav_handle *h) {
  if (h->comm_ref && h->comm_ref->holders.fetch_sub(1) == 1) { // the last holder (every holder has drained its own stream)
    {
      std::lock_guard<std::mutex> lk(h->comm_ref->mu);
      (void)rccl().CommDestroy(h->comm_ref->comm);
    }
    delete h->comm_ref;
  }
  h->comm = nullptr;
  h->comm_ref = nullptr;
}
extern "C" int dftpav_comm_destroy(dftpav_handle *h) {
  if (!h) return DFTPAV_E_INVALID;
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    std::lock_guard<std::mutex> reg(g_comm_mu);
    comm_release_locked(h);
  }
  if (h->d_comm_send) (void)hipFree(h->d_comm_send);
  h->d_comm_send = nullptr;
  h->comm_send_bytes = 0;
  h->comm_ranks = 0;
  return DFTPAV_OK;
}
extern "C" int dftpav_comm_create(dftpav_handle *h, int nranks, int rank, const void *unique_id) {
  if (!h || nranks < 1 || rank < 0 || rank >= nranks || !unique_id) return DFTPAV_E_INVALID;
  if (!rccl().ok) {
    h->err = "RCCL (librccl.so.1) is not loadable";
    return DFTPAV_E_COMM;
  }
  if (int rc = dftpav_comm_destroy(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  RcclUniqueId u;
  std::memcpy(u.internal, unique_id, DFTPAV_UNIQUE_ID_BYTES);
  RCCLCHK(h, rccl().CommInitRank(&h->comm, nranks, u, rank));
  {
    std::lock_guard<std::mutex> reg(g_comm_mu);
    h->comm_ref = new CommShared;
    h->comm_ref->comm = h->comm;
    h->comm_ref->holders.store(1);
  }
  h->comm_ranks = nranks;
  h->comm_rank = rank;
  return DFTPAV_OK;
}
// Several handles (= HIP streams) of one process on one communicator: a host that keeps k batches in flight on k handles sets
// ONE communicator up per rank instead of k (k ncclCommInitRank rendezvous and k sets of RCCL buffers per rank otherwise).
// RCCL orders successive operations of a communicator among the streams they are enqueued on; what the host owes it is the
// same order of collectives on every rank -- which a round-robin over the handles is.
extern "C" int dftpav_comm_share(dftpav_handle *h, dftpav_handle *owner) {
  if (!h || !owner || h == owner) return DFTPAV_E_INVALID;
  // h's stream is drained BEFORE the registry lock is taken (its collectives may still be in flight on the communicator it gives up)
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
  }
  std::lock_guard<std::mutex> reg(g_comm_mu);
  if (owner->comm && owner->comm_ref && owner->comm_ref == h->comm_ref) return DFTPAV_OK; // already the same communicator
  // the owner is checked and the new reference taken FIRST: a share that fails leaves h as it was (round 5 released h's own
  // communicator before the check -- a failed share could then destroy it on this rank alone and hang the other ranks)
  if (!owner->comm || !owner->comm_ref || owner->device != h->device) { // read under the lock: the owner may be letting go
    h->err = "dftpav_comm_share: the other handle needs a communicator (dftpav_comm_create, or shared itself) on the same device";
    return DFTPAV_E_INVALID;
  }
  owner->comm_ref->holders.fetch_add(1);
  if (h->comm) comm_release_locked(h); // ... only then the old one goes
  if (h->d_comm_send) (void)hipFree(h->d_comm_send); // (sized for the communicator it belonged to)
  h->d_comm_send = nullptr;
  h->comm_send_bytes = 0;
  h->comm = owner->comm;
  h->comm_ref = owner->comm_ref;
  h->comm_ranks = owner->comm_ranks;
  h->comm_rank = owner->comm_rank;
  return DFTPAV_OK;
}
extern "C" int dftpav_comm_layout(int global_B, int nranks, int rank, int *first, int *count, int *block) {
  if (global_B < 1 || nranks < 1 || rank < 0 || rank >= nranks) return DFTPAV_E_INVALID;
  const long long lo = (long long)global_B * rank / nranks, hi = (long long)global_B * (rank + 1) / nranks;
  if (first) *first = (int)lo;
  if (count) *count = (int)(hi - lo);
  if (block) *block = (global_B + nranks - 1) / nranks; // the largest shard: every rank's block in the gathered buffer
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_allgather_results(dftpav_batch *b, int global_B, void *all_records) {
  if (!b || !all_records || !b->uploaded || !b->solved) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (!h->comm) {
    h->err = "dftpav_comm_create first";
    return DFTPAV_E_INVALID;
  }
  int first = 0, count = 0, block = 0;
  if (int rc = dftpav_comm_layout(global_B, h->comm_ranks, h->comm_rank, &first, &count, &block)) return rc;
  if (count != b->B) {
    h->err = "this batch is not the shard dftpav_comm_layout assigns to the rank";
    return DFTPAV_E_INVALID;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  const size_t bytes = (size_t)block * 16;
  if (block <= b->B + 1) {
    // the send buffer IS the batch's record array (its epilogue-written records, one zero record of padding behind them for
    // the ranks whose shard is one short of the block): nothing of ours runs between the solve and the collective
    std::lock_guard<std::mutex> lk(h->comm_ref->mu);
    RCCLCHK(h, rccl().AllGather(b->d_records, all_records, bytes, kNcclUint8, h->comm, h->stream));
    return DFTPAV_OK;
  }
  if (h->comm_send_bytes < bytes) {
    if (h->d_comm_send) (void)hipFree(h->d_comm_send);
    h->d_comm_send = nullptr;
    HIPCHK(h, hipMalloc(&h->d_comm_send, bytes));
    h->comm_send_bytes = bytes;
  }
  HIPCHK(h, hipMemsetAsync(h->d_comm_send, 0, bytes, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_comm_send, b->d_records, (size_t)16 * count, hipMemcpyDeviceToDevice, h->stream));
  std::lock_guard<std::mutex> lk(h->comm_ref->mu);
  RCCLCHK(h, rccl().AllGather(h->d_comm_send, all_records, bytes, kNcclUint8, h->comm, h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_pack_results(dftpav_batch *b, void *device_dst) {
  if (!b || !device_dst || !b->solved) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  // the records are written by the solver's epilogue as trajectories finish: a copy on the stream, no kernel of ours
  HIPCHK(h, hipMemcpyAsync(device_dst, b->d_records, (size_t)16 * b->B, hipMemcpyDeviceToDevice, h->stream));
  return DFTPAV_OK;
}

// The 16-byte records of the last solve on the host: waits for the solve; no work on the device behind it
extern "C" int dftpav_batch_records(dftpav_batch *b, void *host_dst) {
  if (!b || !host_dst || !b->solved) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (int rc = finish_pending(b)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  // The epilogues wrote every record a second time into pinned host memory of the batch (DevBatch::records_host): when the stream has
  // drained they are there.  (A copy from the device -- to pageable or to pinned memory -- is a blit KERNEL of the runtime,
  // __amd_rocclr_copyBuffer in a kernel trace; in a stream of batches it queued for a CU behind the other streams' persistent waves and was
  // seen to take 240-300 ms per delivery on configs[1], the host's loop with it: round 6.)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b->h_records) {
    std::memcpy(host_dst, b->h_records, (size_t)16 * b->B);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipMemcpyAsync(host_dst, b->d_records, (size_t)16 * b->B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// test hook: the steps after the solve (dftpav_batch_validate, dftpav_batch_sample_states) on GIVEN coefficients [B][Ntot][6][2] and piece
// durations [B][M] instead of a solution's -- so that the kernels can be held against committed vectors of arbitrary trajectories
// (tests/golden/steps.npz).  Cleared by the next upload or solve.
extern "C" int dftpav_debug_batch_set_coeffs(dftpav_batch *b, const double *coeffs, const double *piece_dt) {
  if (!b || !coeffs || !piece_dt) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(b->d_coef, coeffs, sizeof(double) * (size_t)b->B * 12 * b->L.Ntot, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(b->d_dt, piece_dt, sizeof(double) * (size_t)b->B * b->L.M, hipMemcpyHostToDevice));
  b->coef_override = true;
  b->uploaded = true;
  b->solved = true;
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_coeffs(dftpav_batch *b, double *coeffs, double *piece_dt) {
  if (!b || !b->uploaded || !b->solved) return DFTPAV_E_INVALID; // the coefficients are those of the solution x
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, launch_for(b, D, kModeCoeffs));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (coeffs)
    HIPCHK(h, hipMemcpy(coeffs, b->d_coef, sizeof(double) * (size_t)b->B * 12 * b->L.Ntot, hipMemcpyDeviceToHost));
  if (piece_dt) HIPCHK(h, hipMemcpy(piece_dt, b->d_dt, sizeof(double) * (size_t)b->B * b->L.M, hipMemcpyDeviceToHost));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_validate(dftpav_batch *b, double sample_dt, double vertex_res, int *collision, int *first_sample) {
  if (!b || !b->uploaded || !b->solved || !(sample_dt > 0.0) || !(vertex_res > 0.0)) return DFTPAV_E_INVALID; // nothing solved yet
  dftpav_handle *h = b->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  HIPCHK(h, hipSetDevice(h->device));
  // coefficients and piece durations of the solutions, regenerated on the device from x (as dftpav_batch_coeffs)
  if (int rc = finish_pending(b)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  if (!b->coef_override) HIPCHK(h, launch_for(b, D, kModeCoeffs));
  // the two running sums of the reference, tabulated: sample times (traj_server_ros.cpp:387) and the spacing of the
  // outline points (shapes.cc:128)
  std::vector<double> tt, vv;
  {
    double t = 0.0;
    for (int k = 0; k < 4096; k++, t += sample_dt) tt.push_back(t);
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = vertex_res; dl < longest; dl += vertex_res) vv.push_back(dl);
    if (vv.empty()) vv.push_back(vertex_res);
  }
  double *d_t = nullptr, *d_v = nullptr;
  int *d_col = nullptr, *d_first = nullptr;
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  chk(hipMalloc(&d_t, sizeof(double) * tt.size()));
  chk(hipMalloc(&d_v, sizeof(double) * vv.size()));
  chk(hipMalloc(&d_col, sizeof(int) * (size_t)b->B));
  chk(hipMalloc(&d_first, sizeof(int) * (size_t)b->B));
  if (rc == DFTPAV_OK) {
    chk(hipMemcpyAsync(d_t, tt.data(), sizeof(double) * tt.size(), hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_v, vv.data(), sizeof(double) * vv.size(), hipMemcpyHostToDevice, h->stream));
    chk(hipEventRecord(h->cev0, h->stream));
    chk(launch_validate(h->d_cells, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, b->d_coef,
                        b->d_dt, b->L, b->B, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, d_t, (int)tt.size(),
                        sample_dt, d_v, (int)vv.size(), d_col, d_first, h->stream));
    chk(hipEventRecord(h->cev1, h->stream));
    if (collision) chk(hipMemcpyAsync(collision, d_col, sizeof(int) * (size_t)b->B, hipMemcpyDeviceToHost, h->stream));
    if (first_sample) chk(hipMemcpyAsync(first_sample, d_first, sizeof(int) * (size_t)b->B, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
    h->ctimed = rc == DFTPAV_OK;
  }
  for (void *p : {(void *)d_t, (void *)d_v, (void *)d_col, (void *)d_first})
    if (p) (void)hipFree(p);
  return rc;
}

extern "C" int dftpav_batch_sample_states(dftpav_batch *b, double t0, double sample_dt, int n_samples, int filter_singularity,
                                          double *states, int *n_valid) {
  if (!b || !b->uploaded || !b->solved || !(sample_dt > 0.0) || n_samples <= 0 || !states) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  if (!b->coef_override) HIPCHK(h, launch_for(b, D, kModeCoeffs));
  double *d_states = nullptr;
  int *d_valid = nullptr;
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  if (!h->cev0) chk(hipEventCreate(&h->cev0));
  if (!h->cev1) chk(hipEventCreate(&h->cev1));
  const size_t nst = (size_t)b->B * (size_t)n_samples * 8;
  chk(hipMalloc(&d_states, sizeof(double) * nst));
  chk(hipMalloc(&d_valid, sizeof(int) * (size_t)b->B));
  if (rc == DFTPAV_OK) {
    chk(hipEventRecord(h->cev0, h->stream));
    chk(launch_states(b->d_coef, b->d_dt, b->L, b->B, h->params.veh_wheel_base, t0, sample_dt, n_samples, filter_singularity != 0,
                      d_states, d_valid, h->stream));
    chk(hipEventRecord(h->cev1, h->stream));
    chk(hipMemcpyAsync(states, d_states, sizeof(double) * nst, hipMemcpyDeviceToHost, h->stream));
    if (n_valid) chk(hipMemcpyAsync(n_valid, d_valid, sizeof(int) * (size_t)b->B, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
    h->ctimed = rc == DFTPAV_OK;
  }
  if (d_states) (void)hipFree(d_states);
  if (d_valid) (void)hipFree(d_valid);
  return rc;
}

// ------------------------------------------------- one planning cycle, stream-ordered
// TrajPlanner::RunMINCOParking from getRectangleConst on (traj_manager.cpp:551-626) and the consumers of its result
// (CheckReplan's collision re-check, traj_server_ros.cpp:385-397; the state playback, :244-259,335-356) as ONE enqueue:
// upload of the boundary states / waypoints / durations, then on the handle's stream and without the host in between
//   constraint-point poses -> rectangles of every hypothesis (corridor.hip) -> solve (solver.hip) -> coefficients of the
//   solutions -> collision re-check (validate.hip) -> state read-out (states.hip).
// dftpav_plan_cycle returns when everything is enqueued; dftpav_plan_cycle_fetch waits and copies the results out.
static int grow(dftpav_handle *h, void **p, size_t *have, size_t want, size_t elem) {
  if (*have >= want && *p) return DFTPAV_OK;
  if (*p) HIPCHK(h, hipFree(*p));
  *p = nullptr;
  HIPCHK(h, hipMalloc(p, elem * want));
  *have = want;
  return DFTPAV_OK;
}

extern "C" int dftpav_plan_cycle(dftpav_batch *b, const dftpav_batch_data *d, const double *states, int n_restarts, double check_dt,
                                 double vertex_res, double t0, double state_dt, int n_samples, int filter_singularity) {
  if (!b || !d || !states || n_restarts < 1 || b->B % n_restarts || !(check_dt > 0.0) || !(vertex_res > 0.0) || !(state_dt > 0.0) ||
      n_samples < 1)
    return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (!h->d_cells) return DFTPAV_E_INVALID;     // no map
  if (b->L.H != 4) return DFTPAV_E_UNSUPPORTED; // rectangles
  dftpav_batch_data dd = *d;
  dd.corridor = nullptr; // the half-planes come from the map
  if (int rc = dftpav_batch_upload(b, &dd)) return rc; // waits for the previous cycle of this handle, then copies the small inputs
  HIPCHK(h, hipSetDevice(h->device));
  auto &pc = b->pc;
  const int B = b->B, n_hyp = B / n_restarts;
  const size_t n_poses = (size_t)n_hyp * b->L.Npts;
  pc.poses.assign(states, states + 3 * n_poses);
  {
    void *p = pc.d_poses;
    if (int rc = grow(h, &p, &pc.n_poses, 3 * n_poses, sizeof(double))) return rc;
    pc.d_poses = (double *)p;
  }
  if (!h->cev0) HIPCHK(h, hipEventCreate(&h->cev0));
  if (!h->cev1) HIPCHK(h, hipEventCreate(&h->cev1));
  HIPCHK(h, hipMemcpyAsync(pc.d_poses, pc.poses.data(), sizeof(double) * 3 * n_poses, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_corridor(h->d_cells, h->d_bits, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y,
                            pc.d_poses, (int)n_poses, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, h->d_dl, h->n_dl,
                            nullptr, b->d_corridor, b->L.Npts, b->NptsPad, n_restarts, h->stream));
  b->have_corridor = true;
  b->cor_t_dirty = true;
  b->cor_rect = false; // (nothing here waits for the device: the sixteen-double layout)
  if (int rc = solve_impl(b, nullptr, false)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, launch_for(b, D, kModeCoeffs));
  // the two running sums of the reference, tabulated (as dftpav_batch_validate)
  pc.tt.clear();
  pc.vv.clear();
  {
    double t = 0.0;
    for (int k = 0; k < 4096; k++, t += check_dt) pc.tt.push_back(t);
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = vertex_res; dl < longest; dl += vertex_res) pc.vv.push_back(dl);
    if (pc.vv.empty()) pc.vv.push_back(vertex_res);
  }
  {
    void *p = pc.d_t;
    if (int rc = grow(h, &p, &pc.n_t, pc.tt.size(), sizeof(double))) return rc;
    pc.d_t = (double *)p;
    p = pc.d_v;
    if (int rc = grow(h, &p, &pc.n_v, pc.vv.size(), sizeof(double))) return rc;
    pc.d_v = (double *)p;
    size_t nb = pc.d_col ? (size_t)B : 0;
    p = pc.d_col;
    if (int rc = grow(h, &p, &nb, (size_t)B, sizeof(int))) return rc;
    pc.d_col = (int *)p;
    nb = pc.d_first ? (size_t)B : 0;
    p = pc.d_first;
    if (int rc = grow(h, &p, &nb, (size_t)B, sizeof(int))) return rc;
    pc.d_first = (int *)p;
    nb = pc.d_valid ? (size_t)B : 0;
    p = pc.d_valid;
    if (int rc = grow(h, &p, &nb, (size_t)B, sizeof(int))) return rc;
    pc.d_valid = (int *)p;
    p = pc.d_rd;
    if (int rc = grow(h, &p, &pc.n_rd, (size_t)B * n_samples * 8, sizeof(double))) return rc;
    pc.d_rd = (double *)p;
  }
  HIPCHK(h, hipMemcpyAsync(pc.d_t, pc.tt.data(), sizeof(double) * pc.tt.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(pc.d_v, pc.vv.data(), sizeof(double) * pc.vv.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_validate(h->d_cells, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, b->d_coef, b->d_dt,
                            b->L, b->B, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, pc.d_t, (int)pc.tt.size(), check_dt,
                            pc.d_v, (int)pc.vv.size(), pc.d_col, pc.d_first, h->stream));
  HIPCHK(h, launch_states(b->d_coef, b->d_dt, b->L, b->B, h->params.veh_wheel_base, t0, state_dt, n_samples, filter_singularity != 0,
                          pc.d_rd, pc.d_valid, h->stream));
  pc.n_samples = n_samples;
  pc.in_flight = true;
  return DFTPAV_OK;
}

extern "C" int dftpav_plan_cycle_fetch(dftpav_batch *b, double *x, double *final_cost, int *status, int *success, int *iters, int *collision,
                                       int *first_sample, double *states, int *n_valid) {
  if (!b || !b->pc.in_flight) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (int rc = dftpav_batch_results(b, x, final_cost, status, success, iters, nullptr, nullptr, nullptr)) return rc; // waits for the stream
  const size_t B = (size_t)b->B;
  if (collision) HIPCHK(h, hipMemcpy(collision, b->pc.d_col, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (first_sample) HIPCHK(h, hipMemcpy(first_sample, b->pc.d_first, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (states) HIPCHK(h, hipMemcpy(states, b->pc.d_rd, sizeof(double) * B * b->pc.n_samples * 8, hipMemcpyDeviceToHost));
  if (n_valid) HIPCHK(h, hipMemcpy(n_valid, b->pc.d_valid, sizeof(int) * B, hipMemcpyDeviceToHost));
  b->pc.in_flight = false;
  return DFTPAV_OK;
}

// ------------------------------------------------- serialised trajectories (include/dftpav_hip.h, "DPTJ" v1)
namespace {
constexpr size_t kWireHeader = 32, kWireSegment = 24, kWirePiece = 104;
template <class T> inline void put(unsigned char *&p, T v) {
  std::memcpy(p, &v, sizeof(T));
  p += sizeof(T);
}
template <class T> inline T get(const unsigned char *&p) {
  T v;
  std::memcpy(&v, p, sizeof(T));
  p += sizeof(T);
  return v;
}
} // namespace

extern "C" size_t dftpav_wire_size(int n_segments, const int *piece_nums) {
  if (n_segments <= 0 || n_segments > kMaxSeg || !piece_nums) return 0;
  size_t n = kWireHeader;
  for (int i = 0; i < n_segments; i++) {
    if (piece_nums[i] <= 0) return 0;
    n += kWireSegment + kWirePiece * (size_t)piece_nums[i];
  }
  return n;
}

extern "C" int dftpav_wire_pack(const dftpav_layout *layout, const double *coeffs, const double *piece_dt, int drone_id,
                                int traj_id, double start_time, void *buf, size_t capacity, size_t *written) {
  if (!layout || !coeffs || !piece_dt || !buf) return DFTPAV_E_INVALID;
  const size_t need = dftpav_wire_size(layout->M, layout->piece_nums);
  if (need == 0 || capacity < need) return DFTPAV_E_INVALID;
  unsigned char *p = (unsigned char *)buf;
  std::memcpy(p, "DPTJ", 4);
  p += 4;
  put<unsigned short>(p, 1);
  put<unsigned char>(p, 5);
  put<unsigned char>(p, 2);
  put<int>(p, drone_id);
  put<int>(p, traj_id);
  put<int>(p, layout->M);
  put<int>(p, 0);
  put<double>(p, start_time);
  double world = start_time; // addSingulTraj: each segment starts where the previous one ended
  int piece = 0;
  for (int i = 0; i < layout->M; i++) {
    const int N = layout->piece_nums[i];
    double dur = 0.0; // getTotalDuration: piece durations summed in order
    for (int q = 0; q < N; q++) dur += piece_dt[i];
    put<int>(p, layout->singuls ? layout->singuls[i] : 1);
    put<int>(p, N);
    put<double>(p, world);
    put<double>(p, dur);
    world = world + dur;
    for (int q = 0; q < N; q++, piece++) {
      put<double>(p, piece_dt[i]);
      const double *c = coeffs + (size_t)piece * 12; // [k][d], k = power
      for (int k = 5; k >= 0; k--) {                   // column 0 of CoefficientMat multiplies t^5
        put<double>(p, c[2 * k]);
        put<double>(p, c[2 * k + 1]);
      }
    }
  }
  if (written) *written = need;
  return DFTPAV_OK;
}

extern "C" int dftpav_wire_info(const void *buf, size_t size, int *drone_id, int *traj_id, double *start_time, int *n_segments,
                                int *n_pieces) {
  if (!buf || size < kWireHeader) return DFTPAV_E_INVALID;
  const unsigned char *p = (const unsigned char *)buf;
  if (std::memcmp(p, "DPTJ", 4) != 0) return DFTPAV_E_INVALID;
  p += 4;
  if (get<unsigned short>(p) != 1 || get<unsigned char>(p) != 5 || get<unsigned char>(p) != 2) return DFTPAV_E_INVALID;
  const int did = get<int>(p), tid = get<int>(p), M = get<int>(p);
  (void)get<int>(p);
  const double st = get<double>(p);
  if (M <= 0 || M > kMaxSeg) return DFTPAV_E_INVALID;
  size_t off = kWireHeader;
  int pieces = 0;
  for (int i = 0; i < M; i++) {
    if (size < off + kWireSegment) return DFTPAV_E_INVALID;
    const unsigned char *q = (const unsigned char *)buf + off;
    const int sg = get<int>(q), N = get<int>(q);
    if ((sg != 1 && sg != -1) || N <= 0 || N > 4096) return DFTPAV_E_INVALID;
    off += kWireSegment + kWirePiece * (size_t)N;
    pieces += N;
  }
  if (size < off) return DFTPAV_E_INVALID;
  if (drone_id) *drone_id = did;
  if (traj_id) *traj_id = tid;
  if (start_time) *start_time = st;
  if (n_segments) *n_segments = M;
  if (n_pieces) *n_pieces = pieces;
  return DFTPAV_OK;
}

extern "C" int dftpav_wire_unpack(const void *buf, size_t size, int *singuls, int *piece_nums, double *seg_start,
                                  double *seg_duration, double *durations, double *coeffs) {
  int M = 0;
  if (int rc = dftpav_wire_info(buf, size, nullptr, nullptr, nullptr, &M, nullptr)) return rc;
  const unsigned char *p = (const unsigned char *)buf + kWireHeader;
  int piece = 0;
  for (int i = 0; i < M; i++) {
    const int sg = get<int>(p), N = get<int>(p);
    const double st = get<double>(p), du = get<double>(p);
    if (singuls) singuls[i] = sg;
    if (piece_nums) piece_nums[i] = N;
    if (seg_start) seg_start[i] = st;
    if (seg_duration) seg_duration[i] = du;
    for (int q = 0; q < N; q++, piece++) {
      const double d = get<double>(p);
      if (durations) durations[piece] = d;
      for (int k = 0; k < 12; k++) {
        const double c = get<double>(p);
        if (coeffs) coeffs[(size_t)piece * 12 + k] = c;
      }
    }
  }
  return DFTPAV_OK;
}

extern "C" int dftpav_set_surround_wire(dftpav_handle *h, const void *const *bufs, const size_t *sizes, int S) {
  if (!h) return DFTPAV_E_INVALID;
  if (S <= 0) return dftpav_set_surround(h, nullptr);
  if (!bufs || !sizes) return DFTPAV_E_INVALID;
  std::vector<int> off(1, 0);
  std::vector<double> dur, coef, total, start;
  for (int s = 0; s < S; s++) {
    int M = 0, np = 0;
    double st = 0.0;
    if (int rc = dftpav_wire_info(bufs[s], sizes[s], nullptr, nullptr, &st, &M, &np)) return rc;
    std::vector<int> sg(M), pn(M);
    const size_t at = dur.size();
    dur.resize(at + np);
    coef.resize((at + np) * 12);
    if (int rc = dftpav_wire_unpack(bufs[s], sizes[s], sg.data(), pn.data(), nullptr, nullptr, dur.data() + at, coef.data() + at * 12))
      return rc;
    for (int i = 0; i < M; i++)
      if (sg[i] != 1) return DFTPAV_E_INVALID; // the obstacle model is forward-only (traj_manager.cpp:726,775)
    double tot = 0.0; // LocalTrajData::duration = Trajectory::getTotalDuration of the joined pieces
    for (int q = 0; q < np; q++) tot += dur[at + q];
    off.push_back((int)(at + np));
    total.push_back(tot);
    start.push_back(st);
  }
  dftpav_surround sur{S, off.data(), dur.data(), coef.data(), total.data(), start.data()};
  return dftpav_set_surround(h, &sur);
}

extern "C" int dftpav_solve_batch(dftpav_handle *h, const dftpav_layout *layout, int B, const dftpav_batch_data *d,
                                  double *x, double *final_cost, int *status, int *success, int *iters, int *evals) {
  dftpav_batch *b = nullptr;
  int rc = dftpav_batch_create(h, layout, B, &b);
  if (rc != DFTPAV_OK) return rc;
  rc = dftpav_batch_upload(b, d);
  if (rc == DFTPAV_OK) rc = dftpav_batch_solve_async(b);
  if (rc == DFTPAV_OK) rc = dftpav_batch_results(b, x, final_cost, status, success, iters, evals, nullptr, nullptr);
  dftpav_batch_destroy(b);
  return rc;
}

// ------------------------------------------------- a batch of queries to their plans (plan.hip)
// TrajPlanner::RunOnceParking from the arrival test on (traj_manager.cpp:194-217) for Q queries: search -> resampling on the device,
// one read-back of the tables that decide the layouts, then per layout group pack -> rectangles -> reference-order solve ->
// coefficients -> collision re-check -> selection, all enqueued on the handle's stream with no wait between stages or groups.
extern "C" void dftpav_default_plan_params(dftpav_plan_params *pp) {
  std::memset(pp, 0, sizeof(*pp));
  dftpav_default_search_params(&pp->search);
  // minco_config.pb.txt:66-67, 76-80; kino_astar.h:207; semantics.h:68 (the defaults of dftpav_frontend_resample's callers)
  pp->frontend.max_forward_vel = 5.0;
  pp->frontend.max_forward_acc = 8.0;
  pp->frontend.max_backward_vel = 2.0;
  pp->frontend.max_backward_acc = 4.0;
  pp->frontend.non_siguav = 0.2;
  pp->frontend.wheel_base = 2.85;
  pp->frontend.piece_duration = 1.0;
  pp->frontend.traj_res = 16;
  pp->frontend.dense_traj_res = 32;
  pp->sigma = 0.3;
  pp->dur_lo = 0.8;
  pp->dur_hi = 1.25;
  pp->seed = 0;
  pp->check_dt = 0.05;  // traj_server_ros.cpp:387
  pp->vertex_res = 0.1; // shapes.h:201
  pp->max_seg = 8;
  pp->max_pieces = 64;
  pp->max_path = 4096;
}
extern "C" int dftpav_abi_sizeof_plan_params(void) { return (int)sizeof(dftpav_plan_params); }
extern "C" int dftpav_abi_sizeof_plan_out(void) { return (int)sizeof(dftpav_plan_out); }

extern "C" int dftpav_plan_group_layouts(int Q, int max_seg, const int *search_status, const int *n_seg, const int *singul,
                                         const int *piece_nums, int *group, int *group_first, int *n_groups, int *plan_status) {
  if (Q < 0 || max_seg < 1 || !n_groups || (Q > 0 && (!search_status || !n_seg || !singul || !piece_nums || !group || !group_first)))
    return DFTPAV_E_INVALID;
  int ng = 0;
  for (int q = 0; q < Q; q++) {
    group[q] = -1;
    if (search_status[q] != DFTPAV_SEARCH_REACH_END) {
      if (plan_status) plan_status[q] = DFTPAV_PLAN_NO_PATH;
      continue;
    }
    const int M = n_seg[q];
    if (M < 1 || M > max_seg) {
      if (plan_status) plan_status[q] = DFTPAV_PLAN_TOO_MANY_SEGMENTS;
      continue;
    }
    const int *sg = singul + (size_t)q * max_seg, *pn = piece_nums + (size_t)q * max_seg;
    int g = 0;
    for (; g < ng; g++) {
      const int f = group_first[g];
      if (n_seg[f] == M && std::memcmp(singul + (size_t)f * max_seg, sg, sizeof(int) * M) == 0 &&
          std::memcmp(piece_nums + (size_t)f * max_seg, pn, sizeof(int) * M) == 0)
        break;
    }
    if (g == ng) group_first[ng++] = q;
    group[q] = g;
    if (plan_status) plan_status[q] = DFTPAV_PLAN_OK;
  }
  *n_groups = ng;
  return DFTPAV_OK;
}

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
  dftpav_frontend_out fe{}; // device pointers
  double *d_poses = nullptr;
  size_t fe_zero_bytes = 0; // the front-end outputs are one stretch of the arena, zeroed per call (as dftpav_frontend_resample does)
  unsigned char *d_fe0 = nullptr;
  // compact outputs (zeroed per call): one stretch too
  unsigned char *d_out0 = nullptr;
  size_t out_zero_bytes = 0;
  int *d_winner = nullptr, *d_witers = nullptr, *d_rint[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double *d_wcost = nullptr, *d_wx = nullptr, *d_wcoef = nullptr, *d_wdt = nullptr, *d_rcost = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed = false;
  std::vector<int> group_sizes;
  // host staging of the tables that decide the grouping
  std::vector<int> h_sints, h_nseg, h_singul, h_pn, h_nstates, h_skip, h_members, h_minit;
  std::vector<double> h_dt, h_vt;
  // ---- the replan loop (dftpav_planner_install ... dftpav_replan_tick)
  // what the last dftpav_plan_queries call left behind for dftpav_planner_adopt: its size and paddings, per query the final
  // plan_status and winner, and the goals
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
  hipEvent_t rev[4] = {nullptr, nullptr, nullptr, nullptr}; // check start / end, tick start / end
  bool check_timed = false, tick_timed = false;
  // ---- the publisher (dftpav_planner_publish): its state per slot lives in d_exec beside the table; clocks and outputs grow on demand
  PubTable P{};
  int *d_pub_mode = nullptr; // [slots] of d_rc: what an adoption does to the control history of each adopted pair
  unsigned char *d_pub = nullptr;
  size_t pub_ticks = 0; // d_pub holds the clocks and outputs of this many ticks
  double *d_pub_t = nullptr, *d_pub_states = nullptr;
  int *d_pub_code = nullptr;
  hipEvent_t pev[2] = {nullptr, nullptr};
  bool pub_timed = false;
};

extern "C" int dftpav_planner_create(dftpav_handle *h, int max_queries, int n_restarts, dftpav_planner **out) {
  if (out) *out = nullptr;
  if (!h || !out) return DFTPAV_E_INVALID;
  if (max_queries < 1 || n_restarts < 1 || n_restarts > 65535 || (long long)max_queries * n_restarts > (1 << 24)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  auto *p = new dftpav_planner();
  p->h = h;
  p->max_queries = max_queries;
  p->R = n_restarts;
  for (auto &e : p->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      h->err = "dftpav_planner_create: hipEventCreate";
      for (auto &f : p->ev)
        if (f) (void)hipEventDestroy(f);
      delete p;
      return DFTPAV_E_HIP;
    }
  for (auto &e : p->rev)
    if (hipEventCreate(&e) != hipSuccess) {
      h->err = "dftpav_planner_create: hipEventCreate";
      for (auto &f : p->ev) (void)hipEventDestroy(f);
      for (auto &f : p->rev)
        if (f) (void)hipEventDestroy(f);
      delete p;
      return DFTPAV_E_HIP;
    }
  *out = p;
  return DFTPAV_OK;
}
extern "C" void dftpav_planner_destroy(dftpav_planner *p) {
  if (!p) return;
  (void)hipSetDevice(p->h->device);
  (void)hipStreamSynchronize(p->h->stream);
  for (auto &e : p->cache) dftpav_batch_destroy(e.b);
  if (p->d_arena) (void)hipFree(p->d_arena);
  if (p->d_exec) (void)hipFree(p->d_exec);
  if (p->d_rc) (void)hipFree(p->d_rc);
  if (p->d_pub) (void)hipFree(p->d_pub);
  for (auto &e : p->pev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : p->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : p->rev)
    if (e) (void)hipEventDestroy(e);
  delete p;
}

extern "C" int dftpav_planner_info(dftpav_planner *p, int *n_batches, int *n_groups, int *group_sizes, float *stage_ms) {
  if (!p) return DFTPAV_E_INVALID;
  if (n_batches) *n_batches = (int)p->cache.size();
  if (n_groups) *n_groups = (int)p->group_sizes.size();
  if (group_sizes)
    for (size_t g = 0; g < p->group_sizes.size(); g++) group_sizes[g] = p->group_sizes[g];
  if (stage_ms) {
    dftpav_handle *h = p->h;
    for (int k = 0; k < 4; k++) stage_ms[k] = 0.0f;
    if (p->timed) {
      HIPCHK(h, hipSetDevice(h->device));
      HIPCHK(h, hipEventSynchronize(p->ev[3]));
      HIPCHK(h, hipEventElapsedTime(&stage_ms[0], p->ev[0], p->ev[1]));
      HIPCHK(h, hipEventElapsedTime(&stage_ms[1], p->ev[1], p->ev[2]));
      HIPCHK(h, hipEventElapsedTime(&stage_ms[2], p->ev[2], p->ev[3]));
      HIPCHK(h, hipEventElapsedTime(&stage_ms[3], p->ev[0], p->ev[3]));
    }
  }
  return DFTPAV_OK;
}

// carves the planner's arena for these paddings (a no-op while they are those of the previous call)
static int planner_buffers(dftpav_planner *p, const dftpav_plan_params &pp, int max_states, size_t n_tabs, size_t n_vt) {
  dftpav_handle *h = p->h;
  const long long sig[6] = {pp.max_seg, pp.max_pieces, pp.max_path, max_states, (long long)n_tabs, (long long)n_vt};
  if (p->d_arena && std::memcmp(sig, p->sig, sizeof(sig)) == 0) return DFTPAV_OK;
  const size_t Q = (size_t)p->max_queries, R = (size_t)p->R, MS = (size_t)pp.max_seg, MP = (size_t)pp.max_pieces, MST = (size_t)max_states;
  for (int pass = 0; pass < 2; pass++) { // measure, then carve
    unsigned char *w = p->d_arena;
    size_t used = 0;
    auto take = [&](size_t bytes) {
      void *r = pass ? (void *)(w + used) : nullptr;
      used += (bytes + 255) / 256 * 256;
      return r;
    };
    p->d_st = (double *)take(sizeof(double) * 4 * Q);
    p->d_en = (double *)take(sizeof(double) * 4 * Q);
    p->d_ct = (double *)take(sizeof(double) * 2 * Q);
    p->d_tabs = (double *)take(sizeof(double) * n_tabs);
    p->d_vt = (double *)take(sizeof(double) * n_vt);
    p->d_paths = (double *)take(sizeof(double) * 3 * Q * (size_t)pp.max_path);
    p->d_skip = (int *)take(sizeof(int) * Q);
    p->d_sints = (int *)take(sizeof(int) * 9 * Q);
    p->d_fe_len = (int *)take(sizeof(int) * Q);
    p->d_members = (int *)take(sizeof(int) * Q);
    p->d_col = (int *)take(sizeof(int) * Q * R);
    p->d_first = (int *)take(sizeof(int) * Q * R);
    p->d_poses = (double *)take(sizeof(double) * 3 * Q * MS * MST);
    const size_t fe0 = used;
    p->d_fe0 = (unsigned char *)take(0);
    p->fe.max_seg = pp.max_seg;
    p->fe.max_pieces = pp.max_pieces;
    p->fe.max_states = max_states;
    p->fe.n_seg = (int *)take(sizeof(int) * Q);
    p->fe.singul = (int *)take(sizeof(int) * Q * MS);
    p->fe.piece_nums = (int *)take(sizeof(int) * Q * MS);
    p->fe.piece_dt = (double *)take(sizeof(double) * Q * MS);
    p->fe.ini_states = (double *)take(sizeof(double) * Q * MS * 6);
    p->fe.fin_states = (double *)take(sizeof(double) * Q * MS * 6);
    p->fe.inner_pts = (double *)take(sizeof(double) * Q * MS * (MP - 1) * 2);
    p->fe.n_states = (int *)take(sizeof(int) * Q * MS);
    p->fe.states = (double *)take(sizeof(double) * Q * MS * MST * 3);
    p->fe_zero_bytes = used - fe0;
    const size_t out0 = used;
    p->d_out0 = (unsigned char *)take(0);
    p->d_minit = (int *)take(sizeof(int) * Q);
    p->d_winner = (int *)take(sizeof(int) * Q);
    p->d_witers = (int *)take(sizeof(int) * Q);
    p->d_wcost = (double *)take(sizeof(double) * Q);
    p->d_wx = (double *)take(sizeof(double) * Q * DFTPAV_PLAN_MAX_VARS);
    p->d_wcoef = (double *)take(sizeof(double) * Q * MS * MP * 12);
    p->d_wdt = (double *)take(sizeof(double) * Q * MS);
    p->d_rcost = (double *)take(sizeof(double) * Q * R);
    for (int k = 0; k < 6; k++) p->d_rint[k] = (int *)take(sizeof(int) * Q * R);
    p->out_zero_bytes = used - out0;
    if (pass == 0) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (p->d_arena && p->arena_bytes < used) {
        (void)hipFree(p->d_arena);
        p->d_arena = nullptr;
        p->arena_bytes = 0;
      }
      if (!p->d_arena) {
        HIPCHK(h, hipMalloc(&p->d_arena, used));
        p->arena_bytes = used;
      }
    }
  }
  std::memcpy(p->sig, sig, sizeof(sig));
  return DFTPAV_OK;
}

// the batch of a layout: from the cache, or created with room for max_queries * n_restarts trajectories in the reference order.
// *out == nullptr with DFTPAV_OK: the layout is outside the reference order's limits.
static int planner_batch(dftpav_planner *p, const dftpav_layout &lay, dftpav_batch **out) {
  dftpav_handle *h = p->h;
  *out = nullptr;
  std::vector<int> key;
  key.push_back(lay.M);
  key.insert(key.end(), lay.singuls, lay.singuls + lay.M);
  key.insert(key.end(), lay.piece_nums, lay.piece_nums + lay.M);
  dftpav_batch *b = nullptr;
  for (auto &e : p->cache)
    if (e.key == key) b = e.b;
  if (lay.M > kMaxSeg) return DFTPAV_OK;
  for (int i = 0; i < lay.M; i++)
    if (lay.piece_nums[i] < 2) return DFTPAV_OK;
  DevLayout L;
  fill_dev_layout(lay, h->params.traj_resolution, h->params.des_traj_resolution, L);
  DevParams P;
  fill_dev_params(h->params, P);
  if (L.n > DFTPAV_PLAN_MAX_VARS || L.Ntot > 1024 || L.Npts > 32767 || (long long)L.Npts * h->S > 65535 || !reference_order_supported(L, P, h->S))
    return DFTPAV_OK;
  const bool fresh = b == nullptr;
  if (fresh) {
    const int rc = dftpav_batch_create(h, &lay, p->max_queries * p->R, &b);
    if (rc == DFTPAV_E_UNSUPPORTED) return DFTPAV_OK;
    if (rc) return rc;
  }
  const int rc = dftpav_batch_set_order(b, DFTPAV_ORDER_REFERENCE); // (nothing to do for a cached batch unless the obstacles changed)
  if (rc) {
    if (fresh) dftpav_batch_destroy(b);
    return rc == DFTPAV_E_UNSUPPORTED ? DFTPAV_OK : rc;
  }
  if (fresh) p->cache.push_back({key, b});
  *out = b;
  return DFTPAV_OK;
}

extern "C" int dftpav_plan_queries(dftpav_planner *p, const dftpav_plan_params *pp, const double *start_states, const double *start_ctrl,
                                   const double *end_states, int Q, double t_now, const dftpav_plan_out *out) {
  if (!p || !pp || !out || Q < 0 || Q > p->max_queries) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  const dftpav_frontend_params &fp = pp->frontend;
  if (pp->max_seg < 1 || pp->max_seg > kMaxSeg || pp->max_pieces < 2 || pp->max_pieces > 1024 || pp->max_path < 2 || pp->max_path > (1 << 20) ||
      !(pp->sigma >= 0.0) || !(pp->dur_lo > 0.0) || !(pp->dur_hi >= pp->dur_lo) || !(pp->check_dt > 0.0) || !(pp->vertex_res > 0.0) ||
      fp.traj_res != h->params.traj_resolution || fp.dense_traj_res != h->params.des_traj_resolution || fp.traj_res < 1 || fp.dense_traj_res < 1 ||
      !(fp.piece_duration > 0.0) || !(fp.max_forward_vel > 0.0) || !(fp.max_forward_acc > 0.0) || !(fp.max_backward_vel > 0.0) ||
      !(fp.max_backward_acc > 0.0))
    return DFTPAV_E_INVALID;
  p->group_sizes.clear();
  p->timed = false;
  p->last_Q = 0; // nothing to adopt until this call has ended well
  if (Q == 0) return DFTPAV_OK;
  if (!start_states || !start_ctrl || !end_states) return DFTPAV_E_INVALID;
  SearchSetup U;
  if (int rc = search_setup(h, &pp->search, Q, U)) return rc;
  const int R = p->R, MS = pp->max_seg, MP = pp->max_pieces;
  const int MST = (MP - 2) * (fp.traj_res + 1) + 2 * (fp.dense_traj_res + 1); // poses of a segment of max_pieces pieces
  // the two running sums of the collision re-check, tabulated (as dftpav_batch_validate): sample times | outline point spacing
  std::vector<double> &vt = p->h_vt;
  vt.clear();
  {
    double t = 0.0;
    for (int k = 0; k < 4096; k++, t += pp->check_dt) vt.push_back(t);
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = pp->vertex_res; dl < longest; dl += pp->vertex_res) vt.push_back(dl);
    if (vt.size() == 4096) vt.push_back(pp->vertex_res);
  }
  const int n_t = 4096, n_v = (int)vt.size() - 4096;
  if (int rc = planner_buffers(p, *pp, MST, U.tabs.size(), vt.size())) return rc;
  const size_t nq = (size_t)Q;
  // ---- arrival test (traj_manager.cpp:196), uploads, search, resampling
  p->h_skip.assign(Q, 0);
  for (int q = 0; q < Q; q++) {
    const double dx = end_states[4 * q] - start_states[4 * q], dy = end_states[4 * q + 1] - start_states[4 * q + 1];
    if (std::sqrt(dx * dx + dy * dy) < 1.0) p->h_skip[q] = 1;
  }
  HIPCHK(h, hipMemcpyAsync(p->d_st, start_states, sizeof(double) * 4 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_en, end_states, sizeof(double) * 4 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_ct, start_ctrl, sizeof(double) * 2 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_skip, p->h_skip.data(), sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_tabs, U.tabs.data(), sizeof(double) * U.tabs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_vt, vt.data(), sizeof(double) * vt.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_paths, 0, sizeof(double) * 3 * nq * pp->max_path, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_fe0, 0, p->fe_zero_bytes, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_out0, 0, p->out_zero_bytes, h->stream));
  SearchArgs &S = U.S;
  S.in_tab = p->d_tabs;
  S.v_tab = p->d_tabs + U.n_in_tab;
  S.l_tab = p->d_tabs + U.n_in_tab + U.n_vv;
  S.start = p->d_st;
  S.end = p->d_en;
  {
    dftpav_search_out &O = S.out;
    int *d = p->d_sints;
    O.max_nodes = 0;
    O.max_path = pp->max_path;
    O.status = d;
    O.shot_success = d + nq;
    O.used_3d = d + 2 * nq;
    O.budget_hit = d + 3 * nq;
    O.iters = d + 4 * nq;
    O.nodes_used = d + 5 * nq;
    O.n_nodes = d + 6 * nq;
    O.path_len = d + 7 * nq;
    O.nodes = nullptr;
    O.paths = p->d_paths;
  }
  HIPCHK(h, hipEventRecord(p->ev[0], h->stream));
  for (int q0 = 0; q0 < Q; q0 += U.slots) {
    S.q0 = q0;
    HIPCHK(h, launch_search(S, std::min(U.slots, Q - q0), h->stream));
  }
  HIPCHK(h, hipEventRecord(p->ev[1], h->stream));
  HIPCHK(h, launch_plan_paths(S.out.status, S.out.path_len, p->d_skip, Q, pp->max_path, p->d_paths, p->d_fe_len, h->stream));
  HIPCHK(h, launch_frontend(fp, p->d_paths, p->d_fe_len, pp->max_path, p->d_st, p->d_en, p->d_ct, Q, p->fe, h->stream));
  HIPCHK(h, hipEventRecord(p->ev[2], h->stream));
  // ---- the one read-back before the end: the tables that decide the grouping
  p->h_sints.assign(8 * nq, 0);
  p->h_nseg.assign(nq, 0);
  p->h_singul.assign(nq * MS, 0);
  p->h_pn.assign(nq * MS, 0);
  p->h_nstates.assign(nq * MS, 0);
  p->h_dt.assign(nq * MS, 0.0);
  for (int f = 0; f < 8; f++)
    HIPCHK(h, hipMemcpyAsync(p->h_sints.data() + f * nq, p->d_sints + f * nq, sizeof(int) * nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_nseg.data(), p->fe.n_seg, sizeof(int) * nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_singul.data(), p->fe.singul, sizeof(int) * nq * MS, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_pn.data(), p->fe.piece_nums, sizeof(int) * nq * MS, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_nstates.data(), p->fe.n_states, sizeof(int) * nq * MS, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->h_dt.data(), p->fe.piece_dt, sizeof(double) * nq * MS, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int *s_status = p->h_sints.data(), *s_iters = p->h_sints.data() + 4 * nq, *s_len = p->h_sints.data() + 7 * nq;
  for (int q = 0; q < Q; q++)
    if (s_status[q] == 0) return DFTPAV_E_UNSUPPORTED; // a shot beyond the sample table (as dftpav_kino_search)
  // ---- grouping.  Queries that were not resampled (arrived, a path beyond its padding) are kept out of it, as those without a path are
  std::vector<int> gate(nq), group(nq), first(nq), status(nq);
  for (int q = 0; q < Q; q++) {
    const bool usable = s_status[q] == DFTPAV_SEARCH_REACH_END && s_len[q] >= 2 && s_len[q] <= pp->max_path && !p->h_skip[q];
    gate[q] = usable ? DFTPAV_SEARCH_REACH_END : DFTPAV_SEARCH_NO_PATH;
    if (!usable) {
      p->h_nseg[q] = 0;
      for (int i = 0; i < MS; i++) p->h_singul[(size_t)q * MS + i] = p->h_pn[(size_t)q * MS + i] = p->h_nstates[(size_t)q * MS + i] = 0, p->h_dt[(size_t)q * MS + i] = 0.0;
    } else if (p->h_nseg[q] >= 1 && p->h_nseg[q] <= MS) {
      for (int i = 0; i < p->h_nseg[q]; i++) // a segment of more pieces than the padding: its waypoints and poses were cut
        if (p->h_pn[(size_t)q * MS + i] > MP || p->h_nstates[(size_t)q * MS + i] > MST) gate[q] = -1;
    }
  }
  int ng = 0;
  if (int rc = dftpav_plan_group_layouts(Q, MS, gate.data(), p->h_nseg.data(), p->h_singul.data(), p->h_pn.data(), group.data(), first.data(), &ng,
                                         status.data()))
    return rc;
  for (int q = 0; q < Q; q++) {
    if (p->h_skip[q]) status[q] = DFTPAV_PLAN_ARRIVED;
    else if (gate[q] == -1 || (s_status[q] == DFTPAV_SEARCH_REACH_END && s_len[q] > pp->max_path)) status[q] = DFTPAV_PLAN_TOO_MANY_SEGMENTS;
  }
  // ---- the groups' batches (created on first use), the members in group order
  std::vector<dftpav_batch *> batch(ng, nullptr);
  std::vector<int> g_off(ng + 1, 0);
  p->h_members.clear();
  for (int g = 0; g < ng; g++) {
    const int f = first[g];
    dftpav_layout lay{p->h_nseg[f], p->h_pn.data() + (size_t)f * MS, p->h_singul.data() + (size_t)f * MS, 4};
    if (int rc = planner_batch(p, lay, &batch[g])) return rc;
    g_off[g] = (int)p->h_members.size();
    for (int q = 0; q < Q; q++)
      if (group[q] == g) {
        if (batch[g]) p->h_members.push_back(q);
        else status[q] = DFTPAV_PLAN_LAYOUT_UNSUPPORTED;
      }
    g_off[g + 1] = (int)p->h_members.size();
    p->group_sizes.push_back(g_off[g + 1] - g_off[g]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (!p->h_members.empty())
    HIPCHK(h, hipMemcpyAsync(p->d_members, p->h_members.data(), sizeof(int) * p->h_members.size(), hipMemcpyHostToDevice, h->stream));
  // ---- per group: pack -> rectangles -> solve -> coefficients -> collision re-check -> selection; nothing waits in between
  size_t pose_off = 0;
  for (int g = 0; g < ng; g++) {
    dftpav_batch *b = batch[g];
    const int nm = g_off[g + 1] - g_off[g];
    if (!b || nm == 0) continue;
    const DevLayout &L = b->L;
    b->pending = false;
    b->n_active = nm * R;
    b->t_now = t_now;
    b->epis = 0.0; // help_eps of the live call, traj_manager.cpp:610
    b->uploaded = true;
    b->solved = false;
    b->coef_override = false;
    b->dev_version = -1; // n_active / t_now live in the device copy of the launch descriptor
    PlanPackArgs A{};
    A.L = L;
    A.fe = p->fe;
    A.members = p->d_members + g_off[g];
    A.n_members = nm;
    A.n_restarts = R;
    A.sigma = pp->sigma;
    A.lo = pp->dur_lo;
    A.hi = pp->dur_hi;
    A.seed = pp->seed;
    A.mini_T = h->params.mini_T;
    A.max_vel[0] = h->params.max_forward_vel;
    A.max_vel[1] = h->params.max_backward_vel;
    A.max_acc[0] = h->params.max_forward_acc;
    A.max_acc[1] = h->params.max_backward_acc;
    A.x0 = b->d_x0;
    A.iniS = b->d_iniS;
    A.finS = b->d_finS;
    A.poses = p->d_poses + 3 * pose_off;
    A.mini_t_flag = p->d_minit;
    HIPCHK(h, launch_plan_pack(A, h->stream));
    HIPCHK(h, launch_corridor(h->d_cells, h->d_bits, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, A.poses,
                              nm * L.Npts, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, h->d_dl, h->n_dl, nullptr, b->d_corridor,
                              L.Npts, b->NptsPad, R, h->stream));
    pose_off += (size_t)nm * L.Npts;
    b->have_corridor = true;
    b->cor_t_dirty = true;
    b->cor_rect = false; // (nothing here waits for the device: the sixteen-double layout)
    if (int rc = solve_impl(b, nullptr, false)) return rc;
    DevBatch D;
    if (int rc = sync_dev(b, D)) return rc;
    HIPCHK(h, launch_for(b, D, kModeCoeffs));
    int *col = p->d_col + (size_t)g_off[g] * R, *fst = p->d_first + (size_t)g_off[g] * R;
    HIPCHK(h, launch_validate(h->d_cells, h->map.size_x, h->map.size_y, h->map.resolution, h->map.origin_x, h->map.origin_y, b->d_coef, b->d_dt, L,
                              nm * R, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr, p->d_vt, n_t, pp->check_dt, p->d_vt + n_t, n_v,
                              col, fst, h->stream));
    PlanSelectArgs Z{};
    Z.cost = b->d_f;
    Z.success = b->d_success;
    Z.collision = col;
    Z.status = b->d_status;
    Z.iters = b->d_iters;
    Z.evals = b->d_evals;
    Z.first_sample = fst;
    Z.x = b->d_x_out;
    Z.coef = b->d_coef;
    Z.dt = b->d_dt;
    Z.n = L.n;
    Z.n_coef = 12 * L.Ntot;
    Z.M = L.M;
    Z.members = A.members;
    Z.n_members = nm;
    Z.R = R;
    Z.winner = p->d_winner;
    Z.w_cost = p->d_wcost;
    Z.w_iters = p->d_witers;
    Z.w_x = p->d_wx;
    Z.w_coef = p->d_wcoef;
    Z.w_dt = p->d_wdt;
    Z.x_stride = DFTPAV_PLAN_MAX_VARS;
    Z.coef_stride = MS * MP * 12;
    Z.dt_stride = MS;
    Z.r_cost = p->d_rcost;
    Z.r_status = p->d_rint[0];
    Z.r_success = p->d_rint[1];
    Z.r_iters = p->d_rint[2];
    Z.r_evals = p->d_rint[3];
    Z.r_collision = p->d_rint[4];
    Z.r_first_sample = p->d_rint[5];
    HIPCHK(h, launch_plan_select(Z, h->stream));
  }
  HIPCHK(h, hipEventRecord(p->ev[3], h->stream));
  p->timed = true;
  // ---- the compact results
  std::vector<int> winner(nq, -1);
  p->h_minit.assign(nq, 0);
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  HIPCHK(h, fetch(winner.data(), p->d_winner, sizeof(int) * nq));
  HIPCHK(h, fetch(p->h_minit.data(), p->d_minit, sizeof(int) * nq));
  HIPCHK(h, fetch(out->final_cost, p->d_wcost, sizeof(double) * nq));
  HIPCHK(h, fetch(out->iters, p->d_witers, sizeof(int) * nq));
  HIPCHK(h, fetch(out->x, p->d_wx, sizeof(double) * nq * DFTPAV_PLAN_MAX_VARS));
  HIPCHK(h, fetch(out->coeffs, p->d_wcoef, sizeof(double) * nq * MS * MP * 12));
  HIPCHK(h, fetch(out->coeff_dt, p->d_wdt, sizeof(double) * nq * MS));
  HIPCHK(h, fetch(out->r_final_cost, p->d_rcost, sizeof(double) * nq * R));
  int *const r_out[6] = {out->r_status, out->r_success, out->r_iters, out->r_evals, out->r_collision, out->r_first_sample};
  for (int k = 0; k < 6; k++) HIPCHK(h, fetch(r_out[k], p->d_rint[k], sizeof(int) * nq * R));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int q = 0; q < Q; q++) {
    if (status[q] != DFTPAV_PLAN_OK) {
      winner[q] = -1;
      continue;
    }
    if (p->h_minit[q]) { // a restart below mini_T: OptimizeTrajectory refuses the call (see the header); no plan is reported
      winner[q] = -1;
      if (out->final_cost) out->final_cost[q] = 0.0;
      if (out->iters) out->iters[q] = 0;
      if (out->x) std::memset(out->x + (size_t)q * DFTPAV_PLAN_MAX_VARS, 0, sizeof(double) * DFTPAV_PLAN_MAX_VARS);
      if (out->coeffs) std::memset(out->coeffs + (size_t)q * MS * MP * 12, 0, sizeof(double) * MS * MP * 12);
      if (out->coeff_dt) std::memset(out->coeff_dt + (size_t)q * MS, 0, sizeof(double) * MS);
    }
    if (winner[q] < 0) status[q] = DFTPAV_PLAN_NO_VALID_RESTART;
  }
  if (out->plan_status) std::memcpy(out->plan_status, status.data(), sizeof(int) * nq);
  if (out->winner) std::memcpy(out->winner, winner.data(), sizeof(int) * nq);
  if (out->n_seg) std::memcpy(out->n_seg, p->h_nseg.data(), sizeof(int) * nq);
  if (out->singul) std::memcpy(out->singul, p->h_singul.data(), sizeof(int) * nq * MS);
  if (out->piece_nums) std::memcpy(out->piece_nums, p->h_pn.data(), sizeof(int) * nq * MS);
  if (out->piece_dt) std::memcpy(out->piece_dt, p->h_dt.data(), sizeof(double) * nq * MS);
  if (out->search_status) std::memcpy(out->search_status, s_status, sizeof(int) * nq);
  if (out->search_iters) std::memcpy(out->search_iters, s_iters, sizeof(int) * nq);
  if (out->search_path_len) std::memcpy(out->search_path_len, s_len, sizeof(int) * nq);
  // what dftpav_planner_adopt needs of this call (the winners' pieces stay where they are, in the arena)
  p->last_status = status;
  p->last_winner = winner;
  p->last_goal.assign(end_states, end_states + 4 * nq);
  p->last_MS = MS;
  p->last_MP = MP;
  p->last_Q = Q;
  return DFTPAV_OK;
}

extern "C" int dftpav_debug_plan_select(dftpav_handle *h, int n_query, int n_restarts, const double *cost, const int *success,
                                        const int *collision, int *winner_out) {
  if (!h || n_query < 0 || n_restarts < 1 || (n_query > 0 && (!cost || !success || !collision || !winner_out))) return DFTPAV_E_INVALID;
  if (n_query == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nt = (size_t)n_query * n_restarts;
  double *d_cost = nullptr;
  int *d_int = nullptr; // success | collision | winner
  int rc = DFTPAV_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFTPAV_OK) {
      h->err = hipGetErrorString(e);
      rc = DFTPAV_E_HIP;
    }
  };
  chk(hipMalloc(&d_cost, sizeof(double) * nt));
  chk(hipMalloc(&d_int, sizeof(int) * (2 * nt + n_query)));
  if (rc == DFTPAV_OK) {
    chk(hipMemcpyAsync(d_cost, cost, sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_int, success, sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
    chk(hipMemcpyAsync(d_int + nt, collision, sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
    PlanSelectArgs Z{};
    Z.cost = d_cost;
    Z.success = d_int;
    Z.collision = d_int + nt;
    Z.n_members = n_query;
    Z.R = n_restarts;
    Z.winner = d_int + 2 * nt;
    chk(launch_plan_select(Z, h->stream));
    chk(hipMemcpyAsync(winner_out, d_int + 2 * nt, sizeof(int) * n_query, hipMemcpyDeviceToHost, h->stream));
    chk(hipStreamSynchronize(h->stream));
  }
  if (d_cost) (void)hipFree(d_cost);
  if (d_int) (void)hipFree(d_int);
  return rc;
}

// ------------------------------------------------- the replan loop: the executing table, its check and the tick (replan.hip)
// TrajPlannerServer's 20 Hz loop (traj_server_ros.cpp:130-192, 359-501) for every slot of a planner at once.  The table lives in
// device memory; the host mirrors what it needs to pack queries without a read-back: which slots are occupied, and their goals.
extern "C" int dftpav_abi_sizeof_replan_out(void) { return (int)sizeof(dftpav_replan_out); }

// the table, allocated (and zeroed: every slot empty) by the first call that fills it; later calls must bring the same padding
static int exec_table(dftpav_planner *p, int MS, int MP) {
  dftpav_handle *h = p->h;
  if (MS < 1 || MS > kMaxSeg || MP < 1 || MP > 1024) return DFTPAV_E_INVALID;
  if (p->d_exec) return (p->T.max_seg == MS && p->T.max_pieces == MP) ? DFTPAV_OK : DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = (size_t)p->max_queries, ms = (size_t)MS, mp = (size_t)MP;
  ExecTable T{};
  PubTable P{};
  T.n_slots = p->max_queries;
  T.max_seg = MS;
  T.max_pieces = MP;
  unsigned char *base = nullptr;
  size_t used = 0;
  for (int pass = 0; pass < 2; pass++) { // measure, then carve
    used = 0;
    auto take = [&](size_t bytes) {
      void *r = pass ? (void *)(base + used) : nullptr;
      used += (bytes + 255) / 256 * 256;
      return r;
    };
    T.coeffs = (double *)take(sizeof(double) * S * ms * mp * 12);
    T.coeff_dt = (double *)take(sizeof(double) * S * ms);
    T.duration = (double *)take(sizeof(double) * S * ms);
    T.start_time = (double *)take(sizeof(double) * S * ms);
    T.end_time = (double *)take(sizeof(double) * S * ms);
    T.end_state = (double *)take(sizeof(double) * S * 4);
    T.hist = (double *)take(sizeof(double) * S * 2);
    T.n_seg = (int *)take(sizeof(int) * S);
    T.singul = (int *)take(sizeof(int) * S * ms);
    T.piece_nums = (int *)take(sizeof(int) * S * ms);
    T.have_hist = (int *)take(sizeof(int) * S);
    P.hist = (double *)take(sizeof(double) * S * 2);
    P.exe_index = (int *)take(sizeof(int) * S);
    P.have = (int *)take(sizeof(int) * S);
    if (pass == 0) {
      HIPCHK(h, hipMalloc(&base, used));
      if (hipMemsetAsync(base, 0, used, h->stream) != hipSuccess) {
        (void)hipFree(base);
        h->err = "dftpav_planner: hipMemsetAsync of the executing table";
        return DFTPAV_E_HIP;
      }
    }
  }
  p->d_exec = base;
  p->T = T;
  p->P = P;
  p->h_occupied.assign(S, 0);
  p->h_goal.assign(4 * S, 0.0);
  return DFTPAV_OK;
}

// slots [n]: each inside the table, none twice
static bool slots_valid(const dftpav_planner *p, int n, const int *slots) {
  std::vector<char> seen((size_t)p->max_queries, 0);
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= p->max_queries || seen[slots[i]]) return false;
    seen[slots[i]] = 1;
  }
  return true;
}

extern "C" int dftpav_planner_install(dftpav_planner *p, int n, const int *slots, int max_seg, int max_pieces, const int *n_seg,
                                      const int *singul, const int *piece_nums, const double *coeff_dt, const double *coeffs,
                                      const double *end_states, double t_start) {
  if (!p || n < 0 || n > p->max_queries) return DFTPAV_E_INVALID;
  if (n > 0 && (!slots || !n_seg || !singul || !piece_nums || !coeff_dt || !coeffs || !end_states)) return DFTPAV_E_INVALID;
  if (max_seg < 1 || max_seg > kMaxSeg || max_pieces < 1 || max_pieces > 1024) return DFTPAV_E_INVALID;
  if (p->d_exec && (p->T.max_seg != max_seg || p->T.max_pieces != max_pieces)) return DFTPAV_E_INVALID;
  if (!slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  const size_t MS = (size_t)max_seg, MP = (size_t)max_pieces;
  for (int i = 0; i < n; i++) {
    if (n_seg[i] < 1 || n_seg[i] > max_seg) return DFTPAV_E_INVALID;
    for (int j = 0; j < n_seg[i]; j++) {
      const int N = piece_nums[(size_t)i * MS + j];
      if (N < 1 || N > max_pieces) return DFTPAV_E_INVALID; // so the pieces of a plan fit its row of max_seg * max_pieces
    }
  }
  if (int rc = exec_table(p, max_seg, max_pieces)) return rc;
  if (n == 0) return DFTPAV_OK;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const ExecTable &T = p->T;
  std::vector<int> sg(MS), pn(MS);
  std::vector<double> dtv(MS), dur(MS), st(MS), en(MS);
  for (int i = 0; i < n; i++) {
    const size_t s = (size_t)slots[i];
    const int M = n_seg[i];
    double world = t_start;
    for (size_t j = 0; j < MS; j++) {
      const bool used = (int)j < M;
      sg[j] = used ? singul[(size_t)i * MS + j] : 0;
      pn[j] = used ? piece_nums[(size_t)i * MS + j] : 0;
      dtv[j] = used ? coeff_dt[(size_t)i * MS + j] : 0.0;
      double d = 0.0; // Trajectory::getTotalDuration: the piece durations summed in order
      for (int k = 0; k < pn[j]; k++) d += dtv[j];
      dur[j] = used ? d : 0.0;
      st[j] = used ? world : 0.0;          // traj_container.hpp:58-73: start_time, then end_time = start_time + duration
      en[j] = used ? world + d : 0.0;
      if (used) world = world + d;         // traj_manager.cpp:618-625: the next segment starts at that end
    }
    const int zero = 0;
    const double hist0[2] = {0.0, 0.0};
    // (pageable host memory: each copy has left its source when the call returns)
    HIPCHK(h, hipMemcpyAsync(T.coeffs + s * MS * MP * 12, coeffs + (size_t)i * MS * MP * 12, sizeof(double) * MS * MP * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.coeff_dt + s * MS, dtv.data(), sizeof(double) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.duration + s * MS, dur.data(), sizeof(double) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.start_time + s * MS, st.data(), sizeof(double) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.end_time + s * MS, en.data(), sizeof(double) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.end_state + s * 4, end_states + 4 * (size_t)i, sizeof(double) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.hist + s * 2, hist0, sizeof(double) * 2, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.singul + s * MS, sg.data(), sizeof(int) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.piece_nums + s * MS, pn.data(), sizeof(int) * MS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.have_hist + s, &zero, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(T.n_seg + s, &M, sizeof(int), hipMemcpyHostToDevice, h->stream));
    // the publisher starts on segment 0 without control history
    HIPCHK(h, hipMemsetAsync(p->P.exe_index + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(p->P.have + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(p->P.hist + s * 2, 0, sizeof(double) * 2, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream)); // the staging vectors are reused by the next plan
    p->h_occupied[s] = M;
    std::memcpy(&p->h_goal[4 * s], end_states + 4 * (size_t)i, sizeof(double) * 4);
  }
  return DFTPAV_OK;
}

// the winners of the last call into their slots; d_desired: the slots' new filter history, or nullptr for none
static int adopt_impl(dftpav_planner *p, int n, const int *queries, const int *slots, double t_start, const double *d_desired, int *adopted) {
  dftpav_handle *h = p->h;
  if (p->last_Q <= 0) return DFTPAV_E_INVALID; // no call of dftpav_plan_queries to adopt from
  if (!slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++)
    if (queries[i] < 0 || queries[i] >= p->last_Q) return DFTPAV_E_INVALID;
  if (int rc = exec_table(p, p->last_MS, p->last_MP)) return rc;
  std::vector<int> pairs, mode;
  for (int i = 0; i < n; i++) {
    const int q = queries[i];
    const bool ok = p->last_status[q] == DFTPAV_PLAN_OK && p->last_winner[q] >= 0;
    if (adopted) adopted[i] = ok ? 1 : 0;
    if (!ok) continue;
    pairs.push_back(q);
    pairs.push_back(slots[i]);
    // ctrl_state_hist_ outlives a replan; a first plan starts it from the tick's desired state (the ego state), or without one
    mode.push_back(p->h_occupied[slots[i]] ? kPubKeep : (d_desired ? kPubSeed : kPubDrop));
  }
  const int na = (int)pairs.size() / 2;
  if (na == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(p->d_pairs, pairs.data(), sizeof(int) * pairs.size(), hipMemcpyHostToDevice, h->stream));
  ExecAdoptArgs A{};
  A.T = p->T;
  A.pairs = p->d_pairs;
  A.n = na;
  A.q_n_seg = p->fe.n_seg;
  A.q_singul = p->fe.singul;
  A.q_piece_nums = p->fe.piece_nums;
  A.q_dt = p->d_wdt;
  A.q_coeffs = p->d_wcoef;
  A.q_goal = p->d_en;
  A.desired = d_desired;
  A.t_start = t_start;
  HIPCHK(h, launch_exec_adopt(A, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_pub_mode, mode.data(), sizeof(int) * mode.size(), hipMemcpyHostToDevice, h->stream));
  PubResetArgs R{};
  R.P = p->P;
  R.pairs = p->d_pairs;
  R.mode = p->d_pub_mode;
  R.n = na;
  R.desired = d_desired;
  HIPCHK(h, launch_pub_reset(R, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream)); // `pairs` and `mode` have left the host; the table is current when the call returns
  for (int k = 0; k < na; k++) {
    const int q = pairs[2 * k], s = pairs[2 * k + 1];
    p->h_occupied[s] = p->h_nseg[q];
    std::memcpy(&p->h_goal[4 * (size_t)s], &p->last_goal[4 * (size_t)q], sizeof(double) * 4);
  }
  return DFTPAV_OK;
}

// the device buffers of the check: outputs, inputs and the (query, slot) pairs of an adoption
static int replan_buffers(dftpav_planner *p) {
  if (p->d_rc) return DFTPAV_OK;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = (size_t)p->max_queries;
  unsigned char *base = nullptr;
  size_t used = 0;
  for (int pass = 0; pass < 2; pass++) {
    used = 0;
    auto take = [&](size_t bytes) {
      void *r = pass ? (void *)(base + used) : nullptr;
      used += (bytes + 255) / 256 * 256;
      return r;
    };
    p->d_rc_des = (double *)take(sizeof(double) * 8 * S);
    p->d_rc_st = (double *)take(sizeof(double) * 4 * S);
    p->d_rc_ct = (double *)take(sizeof(double) * 2 * S);
    p->d_rc_goal = (double *)take(sizeof(double) * 4 * S);
    p->d_rc_ego = (double *)take(sizeof(double) * 6 * S);
    p->d_rc_tab = (double *)take(sizeof(double) * (4096 + 4096));
    p->d_rc_int = (int *)take(sizeof(int) * kRcInts * S);
    p->d_pairs = (int *)take(sizeof(int) * 2 * S);
    p->d_pub_mode = (int *)take(sizeof(int) * S);
    if (pass == 0) HIPCHK(h, hipMalloc(&base, used));
  }
  p->d_rc = base;
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_adopt(dftpav_planner *p, int n, const int *queries, const int *slots, double t_start, int *adopted) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && (!queries || !slots))) return DFTPAV_E_INVALID;
  if (p->d_exec && p->last_Q > 0 && (p->T.max_seg != p->last_MS || p->T.max_pieces != p->last_MP)) return DFTPAV_E_INVALID;
  if (int rc = replan_buffers(p)) return rc;
  return adopt_impl(p, n, queries, slots, t_start, nullptr, adopted);
}

extern "C" int dftpav_planner_set_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && (!slots || !stamps || !angles))) return DFTPAV_E_INVALID;
  if (!p->d_exec || !slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++)
    if (!p->h_occupied[slots[i]]) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const int one = 1;
  for (int i = 0; i < n; i++) {
    const double hv[2] = {stamps[i], angles[i]};
    HIPCHK(h, hipMemcpyAsync(p->T.hist + 2 * (size_t)slots[i], hv, sizeof(hv), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(p->T.have_hist + slots[i], &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_clear(dftpav_planner *p, int n, const int *slots) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && !slots)) return DFTPAV_E_INVALID;
  if (!slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  if (!p->d_exec) return DFTPAV_OK; // nothing was ever installed: every slot is empty
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const ExecTable &T = p->T;
  const size_t MS = (size_t)T.max_seg, MP = (size_t)T.max_pieces;
  for (int i = 0; i < n; i++) {
    const size_t s = (size_t)slots[i];
    HIPCHK(h, hipMemsetAsync(T.n_seg + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(T.have_hist + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(T.singul + s * MS, 0, sizeof(int) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.piece_nums + s * MS, 0, sizeof(int) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.coeff_dt + s * MS, 0, sizeof(double) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.duration + s * MS, 0, sizeof(double) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.start_time + s * MS, 0, sizeof(double) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.end_time + s * MS, 0, sizeof(double) * MS, h->stream));
    HIPCHK(h, hipMemsetAsync(T.end_state + s * 4, 0, sizeof(double) * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(T.hist + s * 2, 0, sizeof(double) * 2, h->stream));
    HIPCHK(h, hipMemsetAsync(T.coeffs + s * MS * MP * 12, 0, sizeof(double) * MS * MP * 12, h->stream));
    HIPCHK(h, hipMemsetAsync(p->P.exe_index + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(p->P.have + s, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(p->P.hist + s * 2, 0, sizeof(double) * 2, h->stream));
    p->h_occupied[s] = 0;
    for (int k = 0; k < 4; k++) p->h_goal[4 * s + k] = 0.0;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_executing(dftpav_planner *p, int slot, int *n_seg, int *singul, int *piece_nums, double *coeff_dt,
                                        double *coeffs, double *duration, double *start_time, double *end_time, double *end_state,
                                        double *hist, int *have_hist) {
  if (!p || slot < 0 || slot >= p->max_queries) return DFTPAV_E_INVALID;
  if (!p->d_exec) { // nothing was ever installed: the slot is empty, and no padding is known to size the arrays by
    if (n_seg) *n_seg = 0;
    if (have_hist) *have_hist = 0;
    return DFTPAV_OK;
  }
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const ExecTable &T = p->T;
  const size_t MS = (size_t)T.max_seg, MP = (size_t)T.max_pieces, s = (size_t)slot;
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  HIPCHK(h, fetch(n_seg, T.n_seg + s, sizeof(int)));
  HIPCHK(h, fetch(singul, T.singul + s * MS, sizeof(int) * MS));
  HIPCHK(h, fetch(piece_nums, T.piece_nums + s * MS, sizeof(int) * MS));
  HIPCHK(h, fetch(coeff_dt, T.coeff_dt + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch(coeffs, T.coeffs + s * MS * MP * 12, sizeof(double) * MS * MP * 12));
  HIPCHK(h, fetch(duration, T.duration + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch(start_time, T.start_time + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch(end_time, T.end_time + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch(end_state, T.end_state + s * 4, sizeof(double) * 4));
  HIPCHK(h, fetch(hist, T.hist + s * 2, sizeof(double) * 2));
  HIPCHK(h, fetch(have_hist, T.have_hist + s, sizeof(int)));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_padding(dftpav_planner *p, int *max_seg, int *max_pieces) {
  if (!p) return DFTPAV_E_INVALID;
  if (max_seg) *max_seg = p->d_exec ? p->T.max_seg : 0;
  if (max_pieces) *max_pieces = p->d_exec ? p->T.max_pieces : 0;
  return DFTPAV_OK;
}

// enqueues the check on the handle's stream (results stay in the planner's device buffers)
static int replan_check_enqueue(dftpav_planner *p, double t_now, double budget, const double *end_states, const double *ego_states,
                                double check_dt, double vertex_res) {
  dftpav_handle *h = p->h;
  if (!h->d_cells || !p->d_exec) return DFTPAV_E_INVALID; // no map; no table
  if (!(check_dt > 0.0) || !(vertex_res > 0.0) || !(t_now == t_now) || !(budget == budget)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = replan_buffers(p)) return rc;
  const size_t S = (size_t)p->max_queries;
  if (p->rc_dt != check_dt || p->rc_res != vertex_res) {
    // the two running sums of the reference, tabulated (as dftpav_batch_validate): sample times | outline point spacing
    std::vector<double> tab;
    double t = 0.0;
    for (int k = 0; k < 4096; k++, t += check_dt) tab.push_back(t);
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = vertex_res; dl < longest && tab.size() < 8192; dl += vertex_res) tab.push_back(dl);
    if (tab.size() == 4096) tab.push_back(vertex_res);
    if (tab.size() >= 8192) return DFTPAV_E_UNSUPPORTED; // an outline of 4096 points and more
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(p->d_rc_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    p->rc_n_t = 4096;
    p->rc_n_v = (int)tab.size() - 4096;
    p->rc_dt = check_dt;
    p->rc_res = vertex_res;
  }
  if (end_states) HIPCHK(h, hipMemcpyAsync(p->d_rc_goal, end_states, sizeof(double) * 4 * S, hipMemcpyHostToDevice, h->stream));
  if (ego_states) HIPCHK(h, hipMemcpyAsync(p->d_rc_ego, ego_states, sizeof(double) * 6 * S, hipMemcpyHostToDevice, h->stream));
  ReplanArgs A{};
  A.T = p->T;
  A.cells = h->d_cells;
  A.size_x = h->map.size_x;
  A.size_y = h->map.size_y;
  A.resolution = h->map.resolution;
  A.origin_x = h->map.origin_x;
  A.origin_y = h->map.origin_y;
  A.veh_width = h->params.veh_width;
  A.veh_length = h->params.veh_length;
  A.veh_dcr = h->params.veh_d_cr;
  A.wheel_base = h->params.veh_wheel_base;
  A.t_tab = p->d_rc_tab;
  A.n_t = p->rc_n_t;
  A.sample_dt = check_dt;
  A.v_tab = p->d_rc_tab + p->rc_n_t;
  A.n_v = p->rc_n_v;
  A.t_now = t_now;
  A.budget = budget;
  A.goals = end_states ? p->d_rc_goal : nullptr;
  A.ego = ego_states ? p->d_rc_ego : nullptr;
  A.o_int = p->d_rc_int;
  A.desired = p->d_rc_des;
  A.start_state = p->d_rc_st;
  A.start_ctrl = p->d_rc_ct;
  HIPCHK(h, hipEventRecord(p->rev[0], h->stream));
  HIPCHK(h, launch_replan_check(A, h->stream));
  HIPCHK(h, hipEventRecord(p->rev[1], h->stream));
  p->check_timed = true;
  return DFTPAV_OK;
}

// copies of the check's results for the caller (enqueued; the caller of this function waits for the stream)
static int replan_check_fetch(dftpav_planner *p, const dftpav_replan_out *out) {
  if (!out) return DFTPAV_OK;
  dftpav_handle *h = p->h;
  const size_t S = (size_t)p->max_queries;
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  int *const io[kRcInts] = {out->occupied, out->complete, out->exe_index, out->is_close_turnpoint, out->is_near, out->target_moved,
                            out->collision, out->first_sample, out->replan};
  for (int k = 0; k < kRcInts; k++) HIPCHK(h, fetch(io[k], p->d_rc_int + (size_t)k * S, sizeof(int) * S));
  HIPCHK(h, fetch(out->desired, p->d_rc_des, sizeof(double) * 8 * S));
  HIPCHK(h, fetch(out->start_state, p->d_rc_st, sizeof(double) * 4 * S));
  HIPCHK(h, fetch(out->start_ctrl, p->d_rc_ct, sizeof(double) * 2 * S));
  return DFTPAV_OK;
}

extern "C" int dftpav_replan_check(dftpav_planner *p, double t_now, double budget, const double *end_states, const double *ego_states,
                                   double check_dt, double vertex_res, const dftpav_replan_out *out) {
  if (!p) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (int rc = replan_check_enqueue(p, t_now, budget, end_states, ego_states, check_dt, vertex_res)) return rc;
  if (int rc = replan_check_fetch(p, out)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_replan_tick(dftpav_planner *p, const dftpav_plan_params *pp, double t_now, double budget, const double *end_states,
                                  const double *ego_states, const dftpav_replan_out *check_out, int *query_slot, int *n_queries,
                                  const dftpav_plan_out *plan_out) {
  if (n_queries) *n_queries = 0;
  if (!p || !pp) return DFTPAV_E_INVALID;
  if (ego_states && !end_states) return DFTPAV_E_INVALID; // an empty slot has no stored goal
  dftpav_handle *h = p->h;
  // the padding of the plans to come must be the table's: checked before anything runs
  if (p->d_exec && (p->T.max_seg != pp->max_seg || p->T.max_pieces != pp->max_pieces)) return DFTPAV_E_INVALID;
  if (!p->d_exec) { // an all-empty table is a valid start (every vehicle waits for its first plan)
    if (int rc = exec_table(p, pp->max_seg, pp->max_pieces)) return rc;
  }
  p->tick_timed = false;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(p->rev[2], h->stream));
  if (int rc = replan_check_enqueue(p, t_now, budget, end_states, ego_states, pp->check_dt, pp->vertex_res)) return rc;
  // ---- the tick's one extra wait: replan, start_state, start_ctrl (with whatever else of the check the caller asked for)
  const size_t S = (size_t)p->max_queries;
  std::vector<int> flag(S, 0);
  std::vector<double> st(4 * S), ct(2 * S);
  HIPCHK(h, hipMemcpyAsync(flag.data(), p->d_rc_int + (size_t)kRcReplan * S, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(st.data(), p->d_rc_st, sizeof(double) * 4 * S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ct.data(), p->d_rc_ct, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, h->stream));
  if (int rc = replan_check_fetch(p, check_out)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // ---- the flagged slots, in rising slot order, are the queries
  std::vector<int> slot_of;
  std::vector<double> qs, qc, qe;
  for (size_t s = 0; s < S; s++) {
    if (!flag[s]) continue;
    slot_of.push_back((int)s);
    qs.insert(qs.end(), st.begin() + 4 * s, st.begin() + 4 * s + 4);
    qc.insert(qc.end(), ct.begin() + 2 * s, ct.begin() + 2 * s + 2);
    const double *g = end_states ? end_states + 4 * s : &p->h_goal[4 * s];
    qe.insert(qe.end(), g, g + 4);
  }
  const int nq = (int)slot_of.size();
  if (n_queries) *n_queries = nq;
  if (query_slot)
    for (int q = 0; q < nq; q++) query_slot[q] = slot_of[q];
  if (nq > 0) {
    static const dftpav_plan_out none{};
    const double stamp = t_now + budget; // desired_state.time_stamp, traj_server_ros.cpp:414; `now` of the plan, traj_manager.cpp:520
    if (int rc = dftpav_plan_queries(p, pp, qs.data(), qc.data(), qe.data(), nq, stamp, plan_out ? plan_out : &none)) return rc;
    std::vector<int> qi(nq);
    for (int q = 0; q < nq; q++) qi[q] = q;
    if (int rc = adopt_impl(p, nq, qi.data(), slot_of.data(), stamp, p->d_rc_des, nullptr)) return rc;
  }
  HIPCHK(h, hipEventRecord(p->rev[3], h->stream));
  p->tick_timed = true;
  return DFTPAV_OK;
}

extern "C" int dftpav_replan_last_ms(dftpav_planner *p, float *check_ms, float *tick_ms) {
  if (!p) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (check_ms) *check_ms = 0.0f;
  if (tick_ms) *tick_ms = 0.0f;
  HIPCHK(h, hipSetDevice(h->device));
  if (check_ms && p->check_timed) {
    HIPCHK(h, hipEventSynchronize(p->rev[1]));
    HIPCHK(h, hipEventElapsedTime(check_ms, p->rev[0], p->rev[1]));
  }
  if (tick_ms && p->tick_timed) {
    HIPCHK(h, hipEventSynchronize(p->rev[3]));
    HIPCHK(h, hipEventElapsedTime(tick_ms, p->rev[2], p->rev[3]));
  }
  return DFTPAV_OK;
}

// ------------------------------------------------- the publisher: PublishData (traj_server_ros.cpp:195-318) for every slot (replan.hip)
extern "C" int dftpav_planner_publish(dftpav_planner *p, int K, const double *t, double *states, int *published) {
  if (!p || !p->d_exec || !t || K < 1 || K > DFTPAV_PUBLISH_MAX_TICKS) return DFTPAV_E_INVALID;
  for (int k = 0; k < K; k++)
    if (!(t[k] == t[k])) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = (size_t)p->max_queries;
  for (auto &e : p->pev)
    if (!e) HIPCHK(h, hipEventCreate(&e));
  if ((size_t)K > p->pub_ticks) { // the clocks and the outputs of K ticks: one allocation, grown to the largest K met
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (p->d_pub) (void)hipFree(p->d_pub);
    p->d_pub = nullptr;
    p->pub_ticks = 0;
    unsigned char *base = nullptr;
    size_t used = 0;
    for (int pass = 0; pass < 2; pass++) {
      used = 0;
      auto take = [&](size_t bytes) {
        void *r = pass ? (void *)(base + used) : nullptr;
        used += (bytes + 255) / 256 * 256;
        return r;
      };
      p->d_pub_states = (double *)take(sizeof(double) * 8 * S * (size_t)K);
      p->d_pub_t = (double *)take(sizeof(double) * (size_t)K);
      p->d_pub_code = (int *)take(sizeof(int) * S * (size_t)K);
      if (pass == 0) HIPCHK(h, hipMalloc(&base, used));
    }
    p->d_pub = base;
    p->pub_ticks = (size_t)K;
  }
  p->pub_timed = false;
  HIPCHK(h, hipMemcpyAsync(p->d_pub_t, t, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, h->stream));
  PublishArgs A{};
  A.T = p->T;
  A.P = p->P;
  A.K = K;
  A.t = p->d_pub_t;
  A.wheel_base = h->params.veh_wheel_base;
  A.states = states ? p->d_pub_states : nullptr;
  A.published = published ? p->d_pub_code : nullptr;
  HIPCHK(h, hipEventRecord(p->pev[0], h->stream));
  HIPCHK(h, launch_publish(A, h->stream));
  HIPCHK(h, hipEventRecord(p->pev[1], h->stream));
  p->pub_timed = true;
  if (states) HIPCHK(h, hipMemcpyAsync(states, p->d_pub_states, sizeof(double) * 8 * S * (size_t)K, hipMemcpyDeviceToHost, h->stream));
  if (published) HIPCHK(h, hipMemcpyAsync(published, p->d_pub_code, sizeof(int) * S * (size_t)K, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream)); // the one wait: `t` has left the host, the outputs have arrived
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_publisher_state(dftpav_planner *p, int slot, int *exe_index, double *hist, int *have_hist) {
  if (!p || slot < 0 || slot >= p->max_queries) return DFTPAV_E_INVALID;
  if (!p->d_exec) { // nothing was ever installed
    if (exe_index) *exe_index = 0;
    if (hist) hist[0] = hist[1] = 0.0;
    if (have_hist) *have_hist = 0;
    return DFTPAV_OK;
  }
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t s = (size_t)slot;
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess; };
  HIPCHK(h, fetch(exe_index, p->P.exe_index + s, sizeof(int)));
  HIPCHK(h, fetch(hist, p->P.hist + s * 2, sizeof(double) * 2));
  HIPCHK(h, fetch(have_hist, p->P.have + s, sizeof(int)));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_set_ctrl_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && (!slots || !stamps || !angles))) return DFTPAV_E_INVALID;
  if (!p->d_exec || !slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++)
    if (!p->h_occupied[slots[i]]) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const int one = 1;
  for (int i = 0; i < n; i++) {
    const double hv[2] = {stamps[i], angles[i]};
    HIPCHK(h, hipMemcpyAsync(p->P.hist + 2 * (size_t)slots[i], hv, sizeof(hv), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(p->P.have + slots[i], &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return DFTPAV_OK;
}

extern "C" int dftpav_publish_last_ms(dftpav_planner *p, float *ms) {
  if (!p || !ms) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  *ms = 0.0f;
  if (!p->pub_timed) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventSynchronize(p->pev[1]));
  HIPCHK(h, hipEventElapsedTime(ms, p->pev[0], p->pev[1]));
  return DFTPAV_OK;
}
