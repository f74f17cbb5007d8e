// capi.cpp — host half of the C-ABI declared in include/dftpav_hip.h: parameters, the handle and its moving obstacles, and a batch
// from its creation to its results.
//
// Holds what PolyTrajOptimizer::OptimizeTrajectory does before and after the
// L-BFGS call (traj_optimizer.cpp:7-134, 176-201): validation, corridor normal
// normalisation, boundary clamping, decision-vector packing, status mapping.
// Everything between (the solve itself) is the kernel in solver.hip.
// The other host units are listed in capi_internal.h.
#include "capi_internal.h"

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
  if (h->d_dist) (void)hipFree(h->d_dist);
  if (h->d_gf) (void)hipFree(h->d_gf);
  if (h->d_gf_meta) (void)hipFree(h->d_gf_meta);
  if (h->d_rs) (void)hipFree(h->d_rs);
  if (h->d_cells_base) (void)hipFree(h->d_cells_base);
  if (h->d_stamp_ws) (void)hipFree(h->d_stamp_ws);
  if (h->d_render_ws) (void)hipFree(h->d_render_ws);
  if (h->stamp_sel_ev) (void)hipEventDestroy(h->stamp_sel_ev);
  const hipStream_t stream = h->stream;
  delete h; // every EventMarks of the handle releases its events here: in front of their stream
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" const char *dftpav_last_error(const dftpav_handle *h) { return h ? h->err.c_str() : "null handle"; }
extern "C" void *dftpav_stream(dftpav_handle *h) { return h ? (void *)h->stream : nullptr; }

static void minco_operator(int N, std::vector<double> &Mop, std::vector<double> &MopT);

// The solver numbers (constraint point, obstacle) pairs with 16 bits and keeps a 16-bit mask of obstacles per point; its
// tables of the obstacles' pieces live in LDS.  A set beyond that is refused where it is installed, not at the first solve.
static int check_surround_limits(dftpav_handle *h, int S, long long pieces) {
  if (S > DFTPAV_MAX_SURROUND || pieces > DFTPAV_MAX_SURROUND_PIECES) {
    h->err = "too many moving obstacles (at most DFTPAV_MAX_SURROUND = 16 with DFTPAV_MAX_SURROUND_PIECES = 512 pieces in all)";
    return DFTPAV_E_UNSUPPORTED;
  }
  return DFTPAV_OK;
}
// the fit itself: the obstacles' pieces into the handle's (freshly freed) tables, then the host's tables from them
static int fit_surround_tables(dftpav_handle *h, const double *states, int S, int n_states) {
  const int N = n_states - 1, np = S * N;
  std::vector<int> off(S + 1);
  for (int i = 0; i <= S; i++) off[i] = i * N;
  std::vector<double> Mop, MopT;
  minco_operator(N, Mop, MopT);
  HIPCHK(h, hipMalloc(&h->d_sur_off, sizeof(int) * (S + 1)));
  HIPCHK(h, hipMalloc(&h->d_sur_dur, sizeof(double) * np));
  HIPCHK(h, hipMalloc(&h->d_sur_coef, sizeof(double) * 12 * np));
  HIPCHK(h, hipMalloc(&h->d_sur_total, sizeof(double) * S));
  HIPCHK(h, hipMalloc(&h->d_sur_start, sizeof(double) * S));
  {
    DevScratch tmp(h);
    double *d_states = nullptr, *d_op = nullptr;
    HIPCHK(h, tmp.alloc(d_states, 7 * (size_t)S * n_states));
    HIPCHK(h, tmp.alloc(d_op, Mop.size()));
    HIPCHK(h, hipMemcpyAsync(h->d_sur_off, off.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_states, states, sizeof(double) * 7 * (size_t)S * n_states, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_op, Mop.data(), sizeof(double) * Mop.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_fit(d_states, S, n_states, d_op, h->d_sur_dur, h->d_sur_coef, h->d_sur_total, h->d_sur_start, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream)); // off / Mop live on this stack frame
  }
  std::vector<double> dur(np);
  HIPCHK(h, hipMemcpy(dur.data(), h->d_sur_dur, sizeof(double) * np, hipMemcpyDeviceToHost));
  if (int rc = upload_theta(h, off, dur)) return rc;
  if (h->d_sur_theta) {
    std::vector<double> coef(12 * (size_t)np);
    HIPCHK(h, hipMemcpy(coef.data(), h->d_sur_coef, sizeof(double) * coef.size(), hipMemcpyDeviceToHost));
    if (int rc = upload_boxes(h, dur, coef)) return rc;
  }
  h->S = S;
  h->sur_pieces = np;
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
  const int rc = fit_surround_tables(h, states, S, n_states);
  if (rc) free_surround(h);
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
void dftpav::fill_dev_params(const dftpav_params &p, DevParams &P) {
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
                  b->d_f_eval, b->d_terms, b->d_trace, b->d_cor_raw, b->d_ref_tab, b->d_ref_scratch, b->d_cor_t, b->d_rect_flag, b->pc.d_poses, b->pc.d_tab, b->pc.d_rd, b->pc.d_col, b->pc.d_first,
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
  delete b; // (solve_ev's events with it)
}

// the kernels' view of a layout: offsets of the segments' pieces, waypoints, right-hand-side rows and constraint points, and of
// tau | gear xy | gear angle inside x (traj_optimizer.cpp:96-115)
void dftpav::fill_dev_layout(const dftpav_layout &layout, int K, int Kd, DevLayout &L) {
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
  BCHK(hipMalloc(&b->d_terms, sizeof(double) * (size_t)B * kCostTerms * (M + 1))); // terms [B][5] | seg_terms [B][M][5]
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
  D.terms_out = b->d_terms;
  D.seg_terms_out = b->d_terms + (size_t)b->B * kCostTerms;
  D.trace = b->d_trace;
  D.trace_b = b->trace_b;
  D.trace_cap = b->trace_cap;
  D.trace_n = b->trace_n;
  return D;
}

// refreshes the device copy of the launch descriptor when something it captures changed
int dftpav::sync_dev(dftpav_batch *b, DevBatch &D) {
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
  if (pl.kind < kRefQuad || mode == kModeCoeffs || mode >= kModeTerms) // (the read-outs: the TEAM / WAVE kernel for every plan)
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
hipError_t dftpav::launch_for(dftpav_batch *b, const DevBatch &D, int mode) {
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
static int ensure_ring_buffers(dftpav_batch *b) {
  if (b->d_queue && b->d_sflag && b->d_iota && b->d_qctl && b->d_state) return DFTPAV_OK;
  dftpav_handle *h = b->h;
  const int B = b->B;
  const size_t stride = (size_t)solver_state_doubles(b->L, b->P);
  int *q = nullptr, *fl = nullptr, *io = nullptr;
  unsigned *ctl = nullptr;
  double *st = nullptr;
  const int qcap = 2 * B;
  DevScratch tmp(h); // (a batch either has all of them -- its device-order plan is scheduled -- or none)
  HIPCHK(h, tmp.alloc(q, (size_t)qcap));
  HIPCHK(h, tmp.alloc(fl, (size_t)B));
  HIPCHK(h, tmp.alloc(io, (size_t)B));
  HIPCHK(h, tmp.alloc(ctl, 16));
  HIPCHK(h, tmp.alloc(st, stride * (size_t)B));
  const unsigned ctl0[8] = {0u, (unsigned)B, (unsigned)B, (unsigned)B, 0u, 0u, 0u, 0u};
  HIPCHK(h, hipMemcpy(ctl + 8, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
  std::vector<int> iota(B);
  for (int i = 0; i < B; i++) iota[i] = i;
  HIPCHK(h, hipMemcpy(io, iota.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice));
  tmp.keep();
  b->d_queue = q;
  b->d_sflag = fl;
  b->d_iota = io;
  b->d_qctl = ctl;
  b->d_state = st;
  b->qcap = qcap;
  b->dev_version = -1; // the device descriptor carries these pointers
  return DFTPAV_OK;
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
    if (pl.kind != kRefTeam && ensure_ring_buffers(b) != DFTPAV_OK) {
      (void)hipGetLastError();
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
    if (prepare_solver_quad(pl) != hipSuccess) return undo("reference order: the QUAD kernel does not take the plan's dynamic LDS");
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

static_assert(DFTPAV_COST_TERMS == kCostTerms && DFTPAV_TERM_SMOOTH == kTermSmooth && DFTPAV_TERM_TIME == kTermTime &&
                  DFTPAV_TERM_CORRIDOR == kTermCorridor && DFTPAV_TERM_SURROUND == kTermSurround && DFTPAV_TERM_FEAS == kTermFeas,
              "the kernels' order of the cost's terms is the C-ABI's");
// the terms launch of a reference-order batch on the handle's stream, nothing waits: d_x == nullptr: at the solution (x_out), else at
// d_x [B][n] in device memory.  The results are b->d_terms (terms [B][5], then seg_terms [B][M][5] from B * 5 doubles on, B the
// batch's capacity).
int dftpav::cost_terms_on_stream(dftpav_batch *b, const double *d_x) {
  dftpav_handle *h = b->h;
  if (b->order != DFTPAV_ORDER_REFERENCE) return DFTPAV_E_UNSUPPORTED;
  const int nb = b->n_active > 0 ? b->n_active : b->B;
  if (d_x && d_x != b->d_x_in)
    HIPCHK(h, hipMemcpyAsync(b->d_x_in, d_x, sizeof(double) * (size_t)nb * b->L.n, hipMemcpyDeviceToDevice, h->stream));
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, launch_for(b, D, d_x ? kModeTerms : kModeTermsSolved));
  return DFTPAV_OK;
}
extern "C" int dftpav_batch_cost_terms(dftpav_batch *b, const double *x, double *terms, double *seg_terms) {
  if (!b) return DFTPAV_E_INVALID;
  if (b->order != DFTPAV_ORDER_REFERENCE) return DFTPAV_E_UNSUPPORTED; // the device order does not keep the penalty classes apart
  if (!b->uploaded || !b->have_corridor || (!x && !b->solved)) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  const size_t nb = (size_t)(b->n_active > 0 ? b->n_active : b->B);
  HIPCHK(h, hipSetDevice(h->device));
  if (!x) {
    if (int rc = finish_pending(b)) return rc;
  } else {
    HIPCHK(h, hipMemcpyAsync(b->d_x_in, x, sizeof(double) * nb * b->L.n, hipMemcpyHostToDevice, h->stream));
  }
  if (int rc = cost_terms_on_stream(b, x ? b->d_x_in : nullptr)) return rc;
  HIPCHK(h, fetch_async(h, terms, b->d_terms, sizeof(double) * nb * kCostTerms));
  HIPCHK(h, fetch_async(h, seg_terms, b->d_terms + (size_t)b->B * kCostTerms, sizeof(double) * nb * b->L.M * kCostTerms));
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
int dftpav::finish_pending(dftpav_batch *b) {
  if (!b->pending) return DFTPAV_OK;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  if (b->hand_over > 0)
    if (int rc = launch_stragglers(b, D, 2)) return rc;
  HIPCHK(h, b->solve_ev.record(1, h->stream));
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

int dftpav::solve_impl(dftpav_batch *b, dftpav_batch *prev, bool chained) {
  if (!b || !b->uploaded || !b->have_corridor || prev == b) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  b->pending = false; // a new solve of this batch supersedes whatever it had suspended
  if (prev && prev->pending && !(chained && chain_compatible(b, prev)))
    if (int rc = finish_pending(prev)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, b->solve_ev.record(0, h->stream));
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
      HIPCHK(h, prev->solve_ev.record(1, h->stream));
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
  HIPCHK(h, b->solve_ev.record(1, h->stream));
  b->solve_ev.complete();
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
  if (!b || !ms || !b->solve_ev.reached()) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, b->solve_ev.elapsed(ms, 0, 1, true));
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
