// capi_conflicts.cpp — the footprint-conflict family: executing plans against each other (conflict.hip), candidate plans against the
// executing table and the conflict filter (cand_conflict.hip), joint selection (joint_select.hip), the conflict trigger of the tick
// (conflict_trigger.hip).  What the four repeat is stated once, in front of them.
#include "capi_internal.h"

// ------------------------------------------------- what the family shares
bool dftpav::conflict_clocks_ok(double t0, double dt, int K) {
  return K >= 1 && K <= DFTPAV_CONFLICT_MAX_SAMPLES && dt > 0.0 && std::isfinite(dt) && std::isfinite(t0);
}
// margin and range of the checks among executing plans (dftpav_planner_check_conflicts, dftpav_planner_check_yield,
// dftpav_debug_conflict_trigger, and the two set_* entries behind their "margin < 0: off"): a margin < 0 or NaN is refused, as the header says
static bool margin_range_ok(double margin, double range) { return margin >= 0.0 && std::isfinite(range) && !(range < margin); }
// of the candidates' read-outs (dftpav_batch_check_conflicts, dftpav_debug_joint_select): a margin < 0 is legal there -- "never
// conflicts", the rows of the separation alone -- and only NaN is refused.  (Either way +inf fails range < margin.)
static bool margin_range_not_nan(double margin, double range) { return margin == margin && std::isfinite(range) && !(range < margin); }

static size_t tile_pad(size_t n) { return (n + kConflictTile - 1) / kConflictTile * kConflictTile; } // up to whole tiles
int dftpav::conflict_s_pad(const dftpav_planner *p) { return (int)tile_pad((size_t)p->max_queries); }

// the vehicle and the two distances of a pair launch
static PairConsts pair_consts(const dftpav_handle *h, double margin, double range) {
  const double L = h->params.veh_length, W = h->params.veh_width;
  const double rad = std::sqrt(0.25 * L * L + 0.25 * W * W);
  const double R = range + 2.0 * rad;
  return PairConsts{0.5 * L, 0.5 * W, margin, R * R};
}

// cx | cy | cs | sn, each [K][pad], from one base
template <class Poses> static void pose_arrays(Poses &P, double *d_pose, size_t n) {
  P.cx = d_pose;
  P.cy = d_pose + n;
  P.cs = d_pose + 2 * n;
  P.sn = d_pose + 3 * n;
}
static ConflictPoses conflict_poses(double *d_pose, unsigned char *d_occupied, int K, size_t S_pad) {
  ConflictPoses P{};
  pose_arrays(P, d_pose, (size_t)K * S_pad);
  P.occupied = d_occupied;
  P.K = K;
  P.S_pad = (int)S_pad;
  return P;
}
static JointPoses joint_poses(double *d_pose, int K, size_t C_pad) {
  JointPoses P{};
  pose_arrays(P, d_pose, (size_t)K * C_pad);
  P.K = K;
  P.C_pad = (int)C_pad;
  return P;
}

// n rows of `rows` into the caller's arrays, each unless the caller did not ask for it (nothing waits); no out: nothing
static int fetch_conflict_rows(dftpav_handle *h, const dftpav_conflict_out *out, const ConflictRows &rows, size_t n) {
  if (!out) return DFTPAV_OK;
  HIPCHK(h, fetch_async(h, out->min_sep, rows.min_sep, sizeof(double) * n));
  HIPCHK(h, fetch_async(h, out->sep_sample, rows.sep_sample, sizeof(int) * n));
  HIPCHK(h, fetch_async(h, out->sep_partner, rows.sep_partner, sizeof(int) * n));
  HIPCHK(h, fetch_async(h, out->conflict_sample, rows.conflict_sample, sizeof(int) * n));
  HIPCHK(h, fetch_async(h, out->conflict_partner, rows.conflict_partner, sizeof(int) * n));
  return DFTPAV_OK;
}
// the rows of something that nothing comes near: +inf, -1.  On the host into the caller's arrays; on the device (+inf from h_inf)
static void fill_empty_conflict_rows(const dftpav_conflict_out *out, size_t n) {
  if (out->min_sep) std::fill(out->min_sep, out->min_sep + n, HUGE_VAL);
  for (int *row : {out->sep_sample, out->sep_partner, out->conflict_sample, out->conflict_partner})
    if (row) std::fill(row, row + n, -1);
}
static int clear_conflict_rows(dftpav_handle *h, const ConflictRows &r, const std::vector<double> &h_inf, size_t n) {
  HIPCHK(h, hipMemcpyAsync(r.min_sep, h_inf.data(), sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  for (int *row : {r.sep_sample, r.sep_partner, r.conflict_sample, r.conflict_partner})
    HIPCHK(h, hipMemsetAsync(row, 0xff, sizeof(int) * n, h->stream));
  return DFTPAV_OK;
}

// The caller's poses [K][n][4] of a debug hook as the kernels read them: cx | cy | cs | sn, each [K][n_pad], NaN behind the last item.
// A pose with a component that is not finite takes no part: NaN throughout; nor does any pose of an item whose byte in `part` is 0
// (nullptr: every item takes part)
static bool finite4(const double *ps) { return std::isfinite(ps[0]) && std::isfinite(ps[1]) && std::isfinite(ps[2]) && std::isfinite(ps[3]); }
static std::vector<double> pack_poses(const double *poses, size_t K, size_t n, size_t n_pad, const unsigned char *part) {
  const size_t N = K * n_pad;
  std::vector<double> soa(4 * N, std::nan(""));
  for (size_t k = 0; k < K; k++)
    for (size_t i = 0; i < n; i++) {
      const double *ps = poses + (k * n + i) * 4;
      if ((part && !part[i]) || !finite4(ps)) continue;
      for (size_t f = 0; f < 4; f++) soa[f * N + k * n_pad + i] = ps[f];
    }
  return soa;
}

// The read-out of a chain pose -> pairs over three marks.  `from`: the mark a chain must have reached for anything to be reported (1:
// a poses-only call reports its pose span; 2: only a whole chain counts); posed: the chain recorded mark 0.  (Every chain waited for the stream.)
static int pose_pair_ms(dftpav_handle *h, const EventMarks<3> &ev, int from, bool posed, float *pose_ms, float *pair_ms) {
  if (pose_ms) *pose_ms = 0.0f;
  if (pair_ms) *pair_ms = 0.0f;
  if (!ev.reached(from)) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (pose_ms && posed) HIPCHK(h, ev.elapsed(pose_ms, 0, 1, false));
  if (pair_ms && ev.reached(2)) HIPCHK(h, ev.elapsed(pair_ms, 1, 2, false));
  return DFTPAV_OK;
}

// ------------------------------------------------- footprint conflicts between the executing plans (conflict.hip)
int dftpav::conflict_poses_into(dftpav_planner *p, double *d_pose, unsigned char *d_occupied, EventMarks<3> *ev, double t0, double dt, int K,
                                ConflictPoses &P) {
  dftpav_handle *h = p->h;
  P = conflict_poses(d_pose, d_occupied, K, (size_t)conflict_s_pad(p));
  ConflictPoseArgs A{};
  A.T = p->T;
  A.P = P;
  A.t0 = t0;
  A.dt = dt;
  A.dcr = h->params.veh_d_cr;
  if (ev) {
    ev->reset(); // until the whole chain has run
    HIPCHK(h, ev->record(0, h->stream));
  }
  HIPCHK(h, launch_conflict_poses(A, h->stream));
  if (ev) HIPCHK(h, ev->record(1, h->stream));
  return DFTPAV_OK;
}
// the same into buffers of `tmp`
static int conflict_poses_on_stream(dftpav_planner *p, DevScratch &tmp, EventMarks<3> &ev, double t0, double dt, int K, ConflictPoses &P) {
  dftpav_handle *h = p->h;
  double *d_pose = nullptr;
  unsigned char *d_occupied = nullptr;
  HIPCHK(h, tmp.alloc(d_pose, 4 * (size_t)K * conflict_s_pad(p)));
  HIPCHK(h, tmp.alloc(d_occupied, (size_t)conflict_s_pad(p)));
  return conflict_poses_into(p, d_pose, d_occupied, &ev, t0, dt, K, P);
}

extern "C" int dftpav_planner_sample_poses(dftpav_planner *p, double t0, double dt, int K, double *poses) {
  if (!p || !poses || !conflict_clocks_ok(t0, dt, K)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  const size_t S = (size_t)p->max_queries;
  if (!p->d_exec) { // nothing was ever installed: every slot is empty
    std::fill(poses, poses + (size_t)K * S * 4, std::nan(""));
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)K * conflict_s_pad(p);
  std::vector<double> soa(4 * n); // cx | cy | cs | sn, each [K][S_pad]; declared in front of tmp, whose end waits for the stream
  DevScratch tmp(h);
  ConflictPoses P{};
  if (int rc = conflict_poses_on_stream(p, tmp, h->conf_ev, t0, dt, K, P)) return rc;
  HIPCHK(h, hipMemcpyAsync(soa.data(), P.cx, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < (size_t)K; k++)
    for (size_t s = 0; s < S; s++)
      for (size_t c = 0; c < 4; c++) poses[(k * S + s) * 4 + c] = soa[c * n + k * P.S_pad + s];
  h->conf_ev.complete(1); // the poses alone
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_check_conflicts(dftpav_planner *p, double t0, double dt, int K, double margin, double range,
                                              const dftpav_conflict_out *out) {
  if (!p || !out || !conflict_clocks_ok(t0, dt, K) || !margin_range_ok(margin, range)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  const size_t S = (size_t)p->max_queries;
  if (!p->d_exec) { // nothing was ever installed: every slot is empty
    fill_empty_conflict_rows(out, S);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  DevScratch tmp(h);
  ConflictPoses P{};
  if (int rc = conflict_poses_on_stream(p, tmp, h->conf_ev, t0, dt, K, P)) return rc;
  const size_t tiles = (size_t)P.S_pad / kConflictTile;
  const size_t rows = tiles * P.S_pad; // the partial rows [tiles][S_pad]; behind them the outputs [S]
  double *d_sep = nullptr;
  int *d_int = nullptr;
  HIPCHK(h, tmp.alloc(d_sep, rows + S));
  HIPCHK(h, tmp.alloc(d_int, 4 * (rows + S)));
  ConflictPairArgs A{};
  A.P = P;
  A.part = conflict_rows(d_sep, d_int, rows);
  A.V = pair_consts(h, margin, range);
  ConflictReduceArgs Rd{};
  Rd.part = A.part;
  Rd.out = conflict_rows(d_sep + rows, d_int + 4 * rows, S);
  Rd.n_slots = p->max_queries;
  Rd.S_pad = P.S_pad;
  Rd.tiles = (int)tiles;
  HIPCHK(h, launch_conflict_pairs(A, h->stream));
  HIPCHK(h, launch_conflict_reduce(Rd, h->stream));
  HIPCHK(h, h->conf_ev.record(2, h->stream));
  if (int rc = fetch_conflict_rows(h, out, Rd.out, S)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->conf_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_conflicts_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms) {
  return h ? pose_pair_ms(h, h->conf_ev, 1, true, pose_ms, pair_ms) : DFTPAV_E_INVALID;
}

// ------------------------------------------------- footprint conflicts of candidate plans against the executing table (cand_conflict.hip)
// the first n trajectories of a batch as candidates that start at t_start, at the clocks t0 + k dt
static CandBatch cand_batch(const dftpav_handle *h, const dftpav_batch *b, int n, double t_start, double t0, double dt) {
  CandBatch C{};
  C.coeffs = b->d_coef;
  C.piece_dt = b->d_dt;
  C.L = b->L;
  C.B = n;
  C.t_start = t_start;
  C.t0 = t0;
  C.dt = dt;
  C.dcr = h->params.veh_d_cr;
  return C;
}
static bool planner_has_plans(const dftpav_planner *p) {
  if (!p->d_exec) return false;
  for (int m : p->h_occupied)
    if (m) return true;
  return false;
}
static bool own_slots_ok(const dftpav_planner *p, const int *own, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (own[i] < -1 || own[i] >= p->max_queries) return false;
  return true;
}

extern "C" int dftpav_batch_sample_poses(dftpav_batch *b, double t_start, double t0, double dt, int K, double *poses) {
  if (!b || !poses || !b->uploaded || !b->solved || !conflict_clocks_ok(t0, dt, K) || !std::isfinite(t_start)) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  const size_t n = (size_t)K * b->B * 4;
  DevScratch tmp(h);
  CandPoseArgs A{};
  A.C = cand_batch(h, b, b->B, t_start, t0, dt);
  A.K = K;
  HIPCHK(h, tmp.alloc(A.poses, n));
  h->cand_ev.reset();
  HIPCHK(h, h->cand_ev.record(0, h->stream));
  HIPCHK(h, launch_cand_poses(A, h->stream));
  HIPCHK(h, h->cand_ev.record(1, h->stream));
  HIPCHK(h, hipMemcpyAsync(poses, A.poses, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cand_ev.complete(1); // the poses alone
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_check_conflicts(dftpav_batch *b, dftpav_planner *p, double t_start, double t0, double dt, int K, double margin,
                                            double range, const int *own, const dftpav_conflict_out *out) {
  if (!b || !p || !out || b->h != p->h || !b->uploaded || !b->solved) return DFTPAV_E_INVALID;
  if (!conflict_clocks_ok(t0, dt, K) || !std::isfinite(t_start) || !margin_range_not_nan(margin, range)) return DFTPAV_E_INVALID;
  const size_t B = (size_t)b->B;
  if (own && !own_slots_ok(p, own, B)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (!p->d_exec) { // nothing was ever installed: no slot to come near
    fill_empty_conflict_rows(out, B);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  DevScratch tmp(h);
  CandPairArgs A{};
  if (int rc = conflict_poses_on_stream(p, tmp, h->cand_ev, t0, dt, K, A.P)) return rc;
  double *d_sep = nullptr;
  int *d_int = nullptr, *d_own = nullptr;
  HIPCHK(h, tmp.alloc(d_sep, B));
  HIPCHK(h, tmp.alloc(d_int, 4 * B));
  if (own) {
    HIPCHK(h, tmp.alloc(d_own, B));
    HIPCHK(h, hipMemcpyAsync(d_own, own, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  }
  A.C = cand_batch(h, b, b->B, t_start, t0, dt);
  A.rows = conflict_rows(d_sep, d_int, B);
  A.members = nullptr;
  A.R = 1;
  A.own = d_own;
  A.reject = nullptr;
  A.V = pair_consts(h, margin, range);
  HIPCHK(h, launch_cand_pairs(A, h->stream));
  HIPCHK(h, h->cand_ev.record(2, h->stream));
  if (int rc = fetch_conflict_rows(h, out, A.rows, B)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cand_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_conflicts_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms) {
  return h ? pose_pair_ms(h, h->cand_ev, 1, true, pose_ms, pair_ms) : DFTPAV_E_INVALID;
}

// the conflict filter (ConflictFilter, capi_internal.h)
int ConflictFilter::configure(dftpav_planner *p, double margin_, double range_, double dt_, int K_) {
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (!d || cap_K < K_) { // the poses are sized by K: a larger K takes a new allocation
    const size_t rows_cap = (size_t)p->max_queries * p->R, S_pad = (size_t)conflict_s_pad(p);
    double *pose = nullptr, *sep = nullptr;
    unsigned char *occ = nullptr;
    int *own = nullptr, *ints = nullptr;
    if (int rc = regrow(h, d, [&](auto &take) {
          pose = (double *)take(sizeof(double) * 4 * (size_t)K_ * S_pad);
          sep = (double *)take(sizeof(double) * rows_cap);
          ints = (int *)take(sizeof(int) * 4 * rows_cap);
          own = (int *)take(sizeof(int) * (size_t)p->max_queries);
          occ = (unsigned char *)take(S_pad);
        }))
      return rc;
    d_pose = pose, d_sep = sep, d_int = ints, d_own = own, d_occupied = occ;
    cap = rows_cap;
    cap_K = K_;
    h_inf.assign(rows_cap, HUGE_VAL);
  }
  margin = margin_, range = range_, dt = dt_, K = K_;
  on = true;
  return DFTPAV_OK;
}
int ConflictFilter::clear(dftpav_planner *p, size_t n_rows, double t_now, const std::vector<int> &own) { // +inf, -1
  dftpav_handle *h = p->h;
  if (int rc = clear_conflict_rows(h, rows(), h_inf, n_rows)) return rc;
  t_call = t_now;
  have_table = planner_has_plans(p);
  if (!have_table) return DFTPAV_OK; // nothing to come near: the cleared rows are the result
  h_own.assign((size_t)p->max_queries, -1);
  std::copy(own.begin(), own.end(), h_own.begin());
  HIPCHK(h, hipMemcpyAsync(d_own, h_own.data(), sizeof(int) * h_own.size(), hipMemcpyHostToDevice, h->stream));
  return conflict_poses_into(p, d_pose, d_occupied, nullptr, t_now, dt, K, P);
}
int ConflictFilter::run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject) {
  if (!have_table) return DFTPAV_OK;
  CandPairArgs A{};
  A.C = cand_batch(h, b, nm * R, t_call, t_call, dt);
  A.P = P;
  A.rows = rows();
  A.members = members;
  A.R = R;
  A.own = d_own;
  A.reject = reject;
  A.V = pair_consts(h, margin, range);
  HIPCHK(h, launch_cand_pairs(A, h->stream));
  return DFTPAV_OK;
}
int ConflictFilter::fetch(dftpav_handle *h, const dftpav_conflict_out *out, size_t n_rows) { return fetch_conflict_rows(h, out, rows(), n_rows); }

extern "C" int dftpav_planner_set_conflict_filter(dftpav_planner *p, double margin, double range, double dt, int K) {
  if (!p || margin != margin) return DFTPAV_E_INVALID;
  if (margin < 0.0) { // off: the buffers stay, nothing reads them
    p->cnf.on = false;
    return DFTPAV_OK;
  }
  if (!conflict_clocks_ok(0.0, dt, K) || !margin_range_ok(margin, range)) return DFTPAV_E_INVALID;
  // joint selection holds poses at the filter's K: its bound is tested before anything changes; its allocation grows first and alone
  // (a larger one that the filter then does not use changes nothing a call can see), and the filter's parameters change last
  if (p->jnt.on && !JointSelect::fits((size_t)p->max_queries * p->R, K)) return DFTPAV_E_UNSUPPORTED;
  const bool was_on = p->cnf.on;
  const double m0 = p->cnf.margin, r0 = p->cnf.range, d0 = p->cnf.dt;
  const int K0 = p->cnf.K;
  if (int rc = p->cnf.configure(p, margin, range, dt, K)) return rc; // (a failed allocation leaves the filter as it was)
  if (p->jnt.on)
    if (int rc = p->jnt.configure(p, K)) { // the filter back to what it was: a refused call changes nothing
      p->cnf.on = was_on, p->cnf.margin = m0, p->cnf.range = r0, p->cnf.dt = d0, p->cnf.K = K0;
      return rc;
    }
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_set_own_slots(dftpav_planner *p, const int *own, int Q) {
  if (!p || Q < 0 || Q > p->max_queries || (Q > 0 && !own)) return DFTPAV_E_INVALID;
  if (!own_slots_ok(p, own, (size_t)Q)) return DFTPAV_E_INVALID;
  p->own_next.assign(own, own + Q);
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_last_conflicts(dftpav_planner *p, const dftpav_conflict_out *out) {
  if (!p || !out || !p->cnf.last || p->last_Q <= 0) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->cnf.fetch(h, out, (size_t)p->last_Q * p->R)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// ------------------------------------------------- joint selection: the candidates of one call against each other (joint_select.hip)
int JointSelect::configure(dftpav_planner *p, int K_) {
  dftpav_handle *h = p->h;
  const size_t C = (size_t)p->max_queries * p->R;
  if (!fits(C, K_)) return DFTPAV_E_UNSUPPORTED;
  const int K = K_ > 0 ? K_ : 1;
  HIPCHK(h, hipSetDevice(h->device));
  if (!d || cap_K < K) { // the poses are sized by K: a larger K takes a new allocation
    const size_t C_pad = tile_pad(C), Q = (size_t)p->max_queries;
    double *pose = nullptr, *cost = nullptr, *sep = nullptr;
    unsigned long long *bits = nullptr;
    int *elig = nullptr, *flag = nullptr, *blk = nullptr, *win = nullptr, *wc = nullptr, *ints = nullptr;
    if (int rc = regrow(h, d, [&](auto &take) {
          pose = (double *)take(sizeof(double) * 4 * (size_t)K * C_pad);
          bits = (unsigned long long *)take(sizeof(unsigned long long) * C_pad * (C_pad / kConflictTile));
          cost = (double *)take(sizeof(double) * C);
          sep = (double *)take(sizeof(double) * C);
          ints = (int *)take(sizeof(int) * 4 * C);
          elig = (int *)take(sizeof(int) * C);
          flag = (int *)take(sizeof(int) * C);
          blk = (int *)take(sizeof(int) * C);
          win = (int *)take(sizeof(int) * Q);
          wc = (int *)take(sizeof(int) * Q);
        }))
      return rc;
    d_pose = pose, d_bits = bits, d_cost = cost, d_sep = sep, d_int = ints, d_elig = elig, d_flag = flag, d_blocked = blk, d_winner = win, d_wcand = wc;
    cap = C;
    cap_pad = C_pad;
    cap_K = K;
    h_inf.assign(C, HUGE_VAL);
  }
  on = true;
  return DFTPAV_OK;
}
// the rows +inf, -1; nobody eligible, no flag, nobody blocked; NaN (all bits set) for every pose of the call
int JointSelect::clear(dftpav_planner *p, int Q, int K) {
  dftpav_handle *h = p->h;
  const size_t C = (size_t)Q * p->R, C_pad = tile_pad(C);
  if (C > cap || K > cap_K) return DFTPAV_E_INVALID; // (configure sized it for the planner and the filter)
  P = joint_poses(d_pose, K, C_pad);
  if (int rc = clear_conflict_rows(h, rows(), h_inf, C)) return rc;
  HIPCHK(h, hipMemsetAsync(d_flag, 0xff, sizeof(int) * C, h->stream));
  HIPCHK(h, hipMemsetAsync(d_elig, 0, sizeof(int) * C, h->stream));
  HIPCHK(h, hipMemsetAsync(d_blocked, 0, sizeof(int) * C, h->stream));
  HIPCHK(h, hipMemsetAsync(d_cost, 0, sizeof(double) * C, h->stream));
  HIPCHK(h, hipMemsetAsync(d_pose, 0xff, sizeof(double) * 4 * (size_t)K * C_pad, h->stream));
  return DFTPAV_OK;
}
int JointSelect::pose_group(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int flag0, const int *col,
                            const int *reject, double t_call, double dt) {
  JointPoseArgs A{};
  A.C = cand_batch(h, b, nm * R, t_call, t_call, dt);
  A.P = P;
  A.J = cands();
  A.members = members;
  A.R = R;
  A.flag0 = flag0;
  A.f = b->d_f;
  A.success = b->d_success;
  A.collision = col;
  A.reject = reject;
  HIPCHK(h, launch_joint_poses(A, h->stream));
  return DFTPAV_OK;
}
// the three stages behind the poses on the handle's stream: marks 2 and 3 of joint_ev (nothing waits)
static int joint_stages(dftpav_handle *h, const JointPoses &P, const JointCands &J, unsigned long long *bits, int Q, int R, double margin,
                        double range, const int *minit, int *reject, int *winner, int *wcand, int *blocked, const ConflictRows &rows) {
  JointPairArgs A{};
  A.P = P;
  A.bits = bits;
  A.C = Q * R;
  A.R = R;
  A.tiles = P.C_pad / kConflictTile;
  A.V = pair_consts(h, margin, range);
  HIPCHK(h, launch_joint_pairs(A, h->stream));
  HIPCHK(h, h->joint_ev.record(2, h->stream));
  JointGreedyArgs G{};
  G.bits = bits;
  G.J = J;
  G.minit = minit;
  G.Q = Q;
  G.R = R;
  G.tiles = A.tiles;
  G.winner = winner;
  G.wcand = wcand;
  G.blocked = blocked;
  G.reject = reject;
  HIPCHK(h, launch_joint_greedy(G, h->stream));
  JointRowsArgs W{};
  W.P = P;
  W.wcand = wcand;
  W.rows = rows;
  W.C = A.C;
  W.Q = Q;
  W.R = R;
  W.V = A.V;
  HIPCHK(h, launch_joint_rows(W, h->stream));
  HIPCHK(h, h->joint_ev.record(3, h->stream));
  return DFTPAV_OK;
}
int JointSelect::run(dftpav_planner *p, int Q, double margin, double range) {
  return joint_stages(p->h, P, cands(), d_bits, Q, p->R, margin, range, p->d_minit, p->d_reject, d_winner, d_wcand, d_blocked, rows());
}
int JointSelect::fetch(dftpav_handle *h, const dftpav_conflict_out *out, int *blocked, size_t n_rows) {
  if (int rc = fetch_conflict_rows(h, out, rows(), n_rows)) return rc;
  HIPCHK(h, fetch_async(h, blocked, d_blocked, sizeof(int) * n_rows));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_set_joint_selection(dftpav_planner *p, int on) {
  if (!p || (on != 0 && on != 1)) return DFTPAV_E_INVALID;
  if (!on) { // off: the buffers stay, nothing reads them
    p->jnt.on = false;
    return DFTPAV_OK;
  }
  return p->jnt.configure(p, p->cnf.K);
}

extern "C" int dftpav_planner_last_joint(dftpav_planner *p, const dftpav_conflict_out *out, int *blocked) {
  if (!p || !out || !p->jnt.last || p->last_Q <= 0) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->jnt.fetch(h, out, blocked, (size_t)p->last_Q * p->R)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_joint_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms, float *select_ms) {
  if (!h) return DFTPAV_E_INVALID;
  for (float *ms : {pose_ms, pair_ms, select_ms})
    if (ms) *ms = 0.0f;
  if (!h->joint_ev.reached(3)) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (pose_ms && h->joint_posed) HIPCHK(h, h->joint_ev.elapsed(pose_ms, 0, 1, false)); // (both chains waited for the stream)
  if (pair_ms) HIPCHK(h, h->joint_ev.elapsed(pair_ms, 1, 2, false));
  if (select_ms) HIPCHK(h, h->joint_ev.elapsed(select_ms, 2, 3, false));
  return DFTPAV_OK;
}

extern "C" int dftpav_debug_joint_select(dftpav_handle *h, int Q, int R, int K, const double *poses, const double *cost, const int *eligible,
                                         double margin, double range, int *winner, int *blocked, const dftpav_conflict_out *out) {
  if (!h || !poses || !cost || !eligible || Q < 1 || R < 1 || !conflict_clocks_ok(0.0, 1.0, K)) return DFTPAV_E_INVALID;
  if (!margin_range_not_nan(margin, range)) return DFTPAV_E_INVALID;
  if ((long long)Q * R > DFTPAV_JOINT_MAX_CANDIDATES || !JointSelect::fits((size_t)Q * R, K)) return DFTPAV_E_UNSUPPORTED;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t C = (size_t)Q * R, C_pad = tile_pad(C), n = (size_t)K * C_pad;
  const std::vector<double> soa = pack_poses(poses, (size_t)K, C, C_pad, nullptr); // declared in front of tmp, whose end waits for the stream
  std::vector<int> elig(C);
  for (size_t i = 0; i < C; i++) elig[i] = eligible[i] != 0 ? 1 : 0;
  DevScratch tmp(h);
  double *d_pose = nullptr, *d_dbl = nullptr; // d_dbl: cost | min_sep
  unsigned long long *d_bits = nullptr;
  int *d_int = nullptr; // eligible | blocked | four rows, each [C]; winner | wcand, each [Q]
  HIPCHK(h, tmp.alloc(d_pose, 4 * n));
  HIPCHK(h, tmp.alloc(d_dbl, 2 * C));
  HIPCHK(h, tmp.alloc(d_bits, C_pad * (C_pad / kConflictTile)));
  HIPCHK(h, tmp.alloc(d_int, 6 * C + 2 * (size_t)Q));
  HIPCHK(h, hipMemcpyAsync(d_pose, soa.data(), sizeof(double) * 4 * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_dbl, cost, sizeof(double) * C, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_int, elig.data(), sizeof(int) * C, hipMemcpyHostToDevice, h->stream));
  const JointCands J{d_dbl, d_int, nullptr};
  int *d_blocked = d_int + C, *d_winner = d_int + 6 * C, *d_wcand = d_winner + Q;
  const ConflictRows rows = conflict_rows(d_dbl + C, d_int + 2 * C, C);
  h->joint_ev.reset();
  h->joint_posed = false;
  HIPCHK(h, h->joint_ev.record(1, h->stream));
  if (int rc = joint_stages(h, joint_poses(d_pose, K, C_pad), J, d_bits, Q, R, margin, range, nullptr, nullptr, d_winner, d_wcand, d_blocked, rows))
    return rc;
  HIPCHK(h, fetch_async(h, winner, d_winner, sizeof(int) * (size_t)Q));
  HIPCHK(h, fetch_async(h, blocked, d_blocked, sizeof(int) * C));
  if (int rc = fetch_conflict_rows(h, out, rows, C)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->joint_ev.complete();
  return DFTPAV_OK;
}

// ------------------------------------------------- the conflict trigger: who yields to whom (conflict_trigger.hip)
// the pair and reduce kernels behind the poses on the handle's stream, up to mark 2 of trig_ev (nothing waits).  d_part: sample |
// partner, each [tiles][S_pad]; d_rows: yield | sample | partner, each [n_slots]
static int trigger_stages(dftpav_handle *h, const ConflictPoses &P, const TriggerYield &Y, int n_slots, double margin, double range,
                          int *d_part, int *d_rows) {
  const size_t tiles = (size_t)P.S_pad / kConflictTile, rows = tiles * P.S_pad;
  TriggerPairArgs A{};
  A.P = P;
  A.Y = Y;
  A.part = TriggerRows{d_part, d_part + rows};
  A.V = pair_consts(h, margin, range);
  TriggerReduceArgs Rd{};
  Rd.part = A.part;
  Rd.yield = d_rows;
  Rd.out = TriggerRows{d_rows + n_slots, d_rows + 2 * (size_t)n_slots};
  Rd.Y = Y;
  Rd.occupied = P.occupied;
  Rd.n_slots = n_slots;
  Rd.S_pad = P.S_pad;
  Rd.tiles = (int)tiles;
  HIPCHK(h, launch_trigger_pairs(A, h->stream));
  HIPCHK(h, launch_trigger_reduce(Rd, h->stream));
  HIPCHK(h, h->trig_ev.record(2, h->stream));
  return DFTPAV_OK;
}
static int fetch_yield(dftpav_handle *h, const dftpav_yield_out *out, const int *d_rows, size_t S) {
  if (!out) return DFTPAV_OK;
  HIPCHK(h, fetch_async(h, out->yield, d_rows, sizeof(int) * S));
  HIPCHK(h, fetch_async(h, out->yield_sample, d_rows + S, sizeof(int) * S));
  HIPCHK(h, fetch_async(h, out->yield_partner, d_rows + 2 * S, sizeof(int) * S));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_check_yield(dftpav_planner *p, double t_now, double t0, double dt, int K, double margin, double range,
                                          const dftpav_yield_out *out) {
  if (!p || !out || !conflict_clocks_ok(t0, dt, K) || !std::isfinite(t_now) || !margin_range_ok(margin, range)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  const size_t S = (size_t)p->max_queries;
  if (!p->d_exec) { // nothing was ever installed: every slot is empty
    if (out->yield) std::fill(out->yield, out->yield + S, 0);
    for (int *row : {out->yield_sample, out->yield_partner})
      if (row) std::fill(row, row + S, -1);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  DevScratch tmp(h);
  ConflictPoses P{};
  if (int rc = conflict_poses_on_stream(p, tmp, h->trig_ev, t0, dt, K, P)) return rc;
  h->trig_posed = true;
  int *d_part = nullptr, *d_rows = nullptr;
  HIPCHK(h, tmp.alloc(d_part, 2 * ((size_t)P.S_pad / kConflictTile) * P.S_pad));
  HIPCHK(h, tmp.alloc(d_rows, 3 * S));
  if (int rc = trigger_stages(h, P, TriggerYield{p->T, t_now, nullptr}, p->max_queries, margin, range, d_part, d_rows)) return rc;
  if (int rc = fetch_yield(h, out, d_rows, S)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->trig_ev.complete();
  return DFTPAV_OK;
}

int ConflictTrigger::configure(dftpav_planner *p, double margin_, double range_, double dt_, int K_) {
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (!d || cap_K < K_) { // the poses are sized by K: a larger K takes a new allocation
    const size_t S_pad = (size_t)conflict_s_pad(p), tiles = S_pad / kConflictTile;
    double *pose = nullptr;
    unsigned char *occ = nullptr;
    int *part = nullptr, *rows = nullptr;
    if (int rc = regrow(h, d, [&](auto &take) {
          pose = (double *)take(sizeof(double) * 4 * (size_t)K_ * S_pad);
          part = (int *)take(sizeof(int) * 2 * tiles * S_pad);
          rows = (int *)take(sizeof(int) * 3 * (size_t)p->max_queries);
          occ = (unsigned char *)take(S_pad);
        }))
      return rc;
    d_pose = pose, d_part = part, d_rows = rows, d_occupied = occ;
    cap_K = K_;
    last = false; // the rows of the last tick went with the old allocation
  }
  margin = margin_, range = range_, dt = dt_, K = K_;
  on = true;
  return DFTPAV_OK;
}
int ConflictTrigger::run(dftpav_planner *p, double t_now, double t0) {
  dftpav_handle *h = p->h;
  ConflictPoses P{};
  if (int rc = conflict_poses_into(p, d_pose, d_occupied, &h->trig_ev, t0, dt, K, P)) return rc;
  h->trig_posed = true;
  return trigger_stages(h, P, TriggerYield{p->T, t_now, nullptr}, p->max_queries, margin, range, d_part, d_rows);
}
int ConflictTrigger::fetch(dftpav_planner *p, const dftpav_yield_out *out) { return fetch_yield(p->h, out, d_rows, (size_t)p->max_queries); }

extern "C" int dftpav_planner_set_conflict_trigger(dftpav_planner *p, double margin, double range, double dt, int K) {
  if (!p || margin != margin) return DFTPAV_E_INVALID;
  if (margin < 0.0) { // off: the buffers stay, nothing reads them
    p->trg.on = false;
    return DFTPAV_OK;
  }
  if (!conflict_clocks_ok(0.0, dt, K) || !margin_range_ok(margin, range)) return DFTPAV_E_INVALID;
  return p->trg.configure(p, margin, range, dt, K); // (a failed allocation leaves the trigger as it was)
}

extern "C" int dftpav_planner_last_trigger(dftpav_planner *p, const dftpav_yield_out *out) {
  if (!p || !out || !p->trg.last) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->trg.fetch(p, out)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_trigger_last_ms(dftpav_handle *h, float *pose_ms, float *pair_ms) {
  return h ? pose_pair_ms(h, h->trig_ev, 2, h->trig_posed, pose_ms, pair_ms) : DFTPAV_E_INVALID;
}

extern "C" int dftpav_debug_conflict_trigger(dftpav_handle *h, int S, int K, const double *poses, const int *can_yield, double margin,
                                             double range, const dftpav_yield_out *out) {
  if (!h || !poses || !can_yield || S < 1 || !conflict_clocks_ok(0.0, 1.0, K) || !margin_range_ok(margin, range)) return DFTPAV_E_INVALID;
  const size_t S_pad = tile_pad((size_t)S), n = (size_t)K * S_pad;
  if (n > ((size_t)1 << 26)) return DFTPAV_E_UNSUPPORTED; // 2 GiB of poses
  HIPCHK(h, hipSetDevice(h->device));
  // occupied | can_yield, each [S_pad], and the packed poses; declared in front of tmp, whose end waits for the stream
  std::vector<unsigned char> bytes(2 * S_pad, 0);
  for (size_t s = 0; s < (size_t)S; s++) {
    bytes[s] = finite4(poses + s * 4) ? 1 : 0; // the row at k = 0 decides whether the slot holds a plan
    bytes[S_pad + s] = bytes[s] && can_yield[s] != 0 ? 1 : 0;
  }
  const std::vector<double> soa = pack_poses(poses, (size_t)K, (size_t)S, S_pad, bytes.data());
  DevScratch tmp(h);
  double *d_pose = nullptr;
  unsigned char *d_bytes = nullptr;
  int *d_part = nullptr, *d_rows = nullptr;
  HIPCHK(h, tmp.alloc(d_pose, 4 * n));
  HIPCHK(h, tmp.alloc(d_bytes, 2 * S_pad));
  HIPCHK(h, tmp.alloc(d_part, 2 * (S_pad / kConflictTile) * S_pad));
  HIPCHK(h, tmp.alloc(d_rows, 3 * (size_t)S));
  HIPCHK(h, hipMemcpyAsync(d_pose, soa.data(), sizeof(double) * 4 * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_bytes, bytes.data(), 2 * S_pad, hipMemcpyHostToDevice, h->stream));
  TriggerYield Y{};
  Y.flags = d_bytes + S_pad;
  h->trig_ev.reset();
  h->trig_posed = false;
  HIPCHK(h, h->trig_ev.record(1, h->stream));
  if (int rc = trigger_stages(h, conflict_poses(d_pose, d_bytes, K, S_pad), Y, S, margin, range, d_part, d_rows)) return rc;
  if (int rc = fetch_yield(h, out, d_rows, (size_t)S)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->trig_ev.complete();
  return DFTPAV_OK;
}
