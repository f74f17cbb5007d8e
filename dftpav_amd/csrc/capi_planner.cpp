// capi_planner.cpp — a planner: a batch of queries to their plans, the table of executing plans, its replan check and tick, and
// the publisher.
#include "capi_internal.h"

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

extern "C" int dftpav_planner_create(dftpav_handle *h, int max_queries, int n_restarts, dftpav_planner **out) {
  if (out) *out = nullptr;
  if (!h || !out) return DFTPAV_E_INVALID;
  if (max_queries < 1 || n_restarts < 1 || n_restarts > 65535 || (long long)max_queries * n_restarts > (1 << 24)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  auto *p = new dftpav_planner();
  p->h = h;
  p->max_queries = max_queries;
  p->R = n_restarts;
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
  p->lim.release();
  p->pen.release();
  p->clr.release();
  p->cnf.release();
  p->jnt.release();
  p->trg.release();
  delete p; // (its EventMarks' events with it)
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
    if (p->plan_ev.reached()) {
      HIPCHK(h, hipSetDevice(h->device));
      HIPCHK(h, p->plan_ev.elapsed(&stage_ms[3], 0, 3, true)); // (the one wait: mark 3 is the last)
      for (int k = 0; k < 3; k++) HIPCHK(h, p->plan_ev.elapsed(&stage_ms[k], k, k + 1, false));
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
  auto fields = [&](auto &take) {
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
    p->d_reject = (int *)take(sizeof(int) * Q * R);
    p->d_poses = (double *)take(sizeof(double) * 3 * Q * MS * MST);
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
  };
  const size_t used = carve(nullptr, fields);
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
  carve(p->d_arena, fields);
  // the two stretches zeroed per call: the front-end outputs (up to the compact outputs), the compact outputs (up to the end)
  p->fe_zero_bytes = (size_t)(p->d_out0 - p->d_fe0);
  p->out_zero_bytes = used - (size_t)(p->d_out0 - p->d_arena);
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

// One call of dftpav_plan_queries: what its stages (below, in the order the exported function runs them) hand to one another.
struct PlanCall {
  dftpav_planner *p;
  dftpav_handle *h;
  const dftpav_plan_params *pp;
  const double *start_states, *start_ctrl, *end_states;
  int Q;
  double t_now;
  const dftpav_plan_out *out;
  int R = 0, MS = 0, MP = 0, MST = 0; // restarts; the paddings: segments, pieces of a segment, poses of a segment of max_pieces pieces
  int n_t = 0, n_v = 0;               // the validation table (p->h_vt, p->d_vt): sample times | outline point spacings
  SearchSetup U;
  GoalFieldPlan G; // dftpav_set_search_heuristic; off: G.per_turn == 0 and nothing differs
  std::vector<int> gate, group, first, status; // per query: what the grouping saw, its group, per group its first query, plan_status
  std::vector<dftpav_batch *> batch;           // per group (nullptr: a layout outside the reference order's limits)
  std::vector<int> g_off;                      // group g's members are p->h_members [g_off[g], g_off[g + 1])
  size_t pose_off = 0;                         // poses of p->d_poses the groups so far have used
  std::vector<int> own;                        // dftpav_planner_set_own_slots: per query, or empty for none
};

static int plan_check_params(const dftpav_planner *p, const dftpav_plan_params *pp, const dftpav_plan_out *out, int Q) {
  if (!p || !pp || !out || Q < 0 || Q > p->max_queries) return DFTPAV_E_INVALID;
  const dftpav_handle *h = p->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  const dftpav_frontend_params &fp = pp->frontend;
  if (pp->max_seg < 1 || pp->max_seg > kMaxSeg || pp->max_pieces < 2 || pp->max_pieces > 1024 || pp->max_path < 2 || pp->max_path > (1 << 20) ||
      !(pp->sigma >= 0.0) || !(pp->dur_lo > 0.0) || !(pp->dur_hi >= pp->dur_lo) || !(pp->check_dt > 0.0) || !(pp->vertex_res > 0.0) ||
      fp.traj_res != h->params.traj_resolution || fp.dense_traj_res != h->params.des_traj_resolution || fp.traj_res < 1 || fp.dense_traj_res < 1 ||
      !(fp.piece_duration > 0.0) || !(fp.max_forward_vel > 0.0) || !(fp.max_forward_acc > 0.0) || !(fp.max_backward_vel > 0.0) ||
      !(fp.max_backward_acc > 0.0))
    return DFTPAV_E_INVALID;
  return DFTPAV_OK;
}

// arrival test (traj_manager.cpp:196), tables and buffers, uploads, search, resampling: marks 0 to 2
static int plan_search(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  const dftpav_plan_params *pp = c.pp;
  const int Q = c.Q;
  SearchSetup &U = c.U;
  if (int rc = search_setup(h, &pp->search, Q, U)) return rc;
  if (int rc = search_heuristic_plan(h, c.start_states, c.end_states, Q, U, c.G)) return rc;
  c.R = p->R, c.MS = pp->max_seg, c.MP = pp->max_pieces;
  c.MST = (c.MP - 2) * (pp->frontend.traj_res + 1) + 2 * (pp->frontend.dense_traj_res + 1);
  // the two running sums of the collision re-check, tabulated (as dftpav_batch_validate): sample times | outline point spacing
  std::vector<double> &vt = p->h_vt;
  if (int rc = validation_table(h->params, pp->check_dt, pp->vertex_res, 0, vt, &c.n_t, &c.n_v)) return rc;
  if (int rc = planner_buffers(p, *pp, c.MST, U.tabs.size(), vt.size())) return rc;
  const size_t nq = (size_t)Q;
  p->h_skip.assign(Q, 0);
  for (int q = 0; q < Q; q++) {
    const double dx = c.end_states[4 * q] - c.start_states[4 * q], dy = c.end_states[4 * q + 1] - c.start_states[4 * q + 1];
    if (std::sqrt(dx * dx + dy * dy) < 1.0) p->h_skip[q] = 1;
  }
  HIPCHK(h, hipMemcpyAsync(p->d_st, c.start_states, sizeof(double) * 4 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_en, c.end_states, sizeof(double) * 4 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_ct, c.start_ctrl, sizeof(double) * 2 * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_skip, p->h_skip.data(), sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_tabs, U.tabs.data(), sizeof(double) * U.tabs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(p->d_vt, vt.data(), sizeof(double) * vt.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_paths, 0, sizeof(double) * 3 * nq * pp->max_path, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_fe0, 0, p->fe_zero_bytes, h->stream));
  HIPCHK(h, hipMemsetAsync(p->d_out0, 0, p->out_zero_bytes, h->stream));
  SearchArgs &S = U.S;
  wire_search(U, p->d_tabs, p->d_st, p->d_en, p->d_sints, nq, 0, nullptr, pp->max_path, p->d_paths);
  HIPCHK(h, p->plan_ev.record(0, h->stream));
  for (int q0 = 0; q0 < Q; q0 += U.slots) {
    S.q0 = q0;
    if (c.G.per_turn)
      if (int rc = goal_field_turn(h, c.G, q0 / U.slots, &S, nullptr)) return rc;
    HIPCHK(h, launch_search(S, std::min(U.slots, Q - q0), h->stream));
  }
  HIPCHK(h, p->plan_ev.record(1, h->stream));
  HIPCHK(h, launch_plan_paths(S.out.status, S.out.path_len, p->d_skip, Q, pp->max_path, p->d_paths, p->d_fe_len, h->stream));
  HIPCHK(h, launch_frontend(pp->frontend, p->d_paths, p->d_fe_len, pp->max_path, p->d_st, p->d_en, p->d_ct, Q, p->fe, h->stream));
  HIPCHK(h, p->plan_ev.record(2, h->stream));
  return DFTPAV_OK;
}

// the one read-back before the end: the tables that decide the grouping
static int plan_read_layouts(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  const size_t nq = (size_t)c.Q, MS = (size_t)c.MS;
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
  for (int q = 0; q < c.Q; q++)
    if (p->h_sints[q] == 0) return DFTPAV_E_UNSUPPORTED; // a search status of 0: a shot beyond the sample table (as dftpav_kino_search)
  return DFTPAV_OK;
}

// The layout groups, their batches (created on first use) and their members in group order.  Queries that were not resampled
// (arrived, a path beyond its padding) are kept out of the grouping, as those without a path are.
static int plan_group(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  const int Q = c.Q, MS = c.MS;
  const size_t nq = (size_t)Q;
  const int *s_status = p->h_sints.data(), *s_len = p->h_sints.data() + 7 * nq;
  c.gate.resize(nq), c.group.resize(nq), c.first.resize(nq), c.status.resize(nq);
  for (int q = 0; q < Q; q++) {
    const bool usable = s_status[q] == DFTPAV_SEARCH_REACH_END && s_len[q] >= 2 && s_len[q] <= c.pp->max_path && !p->h_skip[q];
    c.gate[q] = usable ? DFTPAV_SEARCH_REACH_END : DFTPAV_SEARCH_NO_PATH;
    if (!usable) {
      p->h_nseg[q] = 0;
      for (int i = 0; i < MS; i++) p->h_singul[(size_t)q * MS + i] = p->h_pn[(size_t)q * MS + i] = p->h_nstates[(size_t)q * MS + i] = 0, p->h_dt[(size_t)q * MS + i] = 0.0;
    } else if (p->h_nseg[q] >= 1 && p->h_nseg[q] <= MS) {
      for (int i = 0; i < p->h_nseg[q]; i++) // a segment of more pieces than the padding: its waypoints and poses were cut
        if (p->h_pn[(size_t)q * MS + i] > c.MP || p->h_nstates[(size_t)q * MS + i] > c.MST) c.gate[q] = -1;
    }
  }
  int ng = 0;
  if (int rc = dftpav_plan_group_layouts(Q, MS, c.gate.data(), p->h_nseg.data(), p->h_singul.data(), p->h_pn.data(), c.group.data(),
                                         c.first.data(), &ng, c.status.data()))
    return rc;
  for (int q = 0; q < Q; q++) {
    if (p->h_skip[q]) c.status[q] = DFTPAV_PLAN_ARRIVED;
    else if (c.gate[q] == -1 || (s_status[q] == DFTPAV_SEARCH_REACH_END && s_len[q] > c.pp->max_path)) c.status[q] = DFTPAV_PLAN_TOO_MANY_SEGMENTS;
  }
  c.batch.assign(ng, nullptr);
  c.g_off.assign(ng + 1, 0);
  p->h_members.clear();
  for (int g = 0; g < ng; g++) {
    const int f = c.first[g];
    dftpav_layout lay{p->h_nseg[f], p->h_pn.data() + (size_t)f * MS, p->h_singul.data() + (size_t)f * MS, 4};
    if (int rc = planner_batch(p, lay, &c.batch[g])) return rc;
    c.g_off[g] = (int)p->h_members.size();
    for (int q = 0; q < Q; q++)
      if (c.group[q] == g) {
        if (c.batch[g]) p->h_members.push_back(q);
        else c.status[q] = DFTPAV_PLAN_LAYOUT_UNSUPPORTED;
      }
    c.g_off[g + 1] = (int)p->h_members.size();
    p->group_sizes.push_back(c.g_off[g + 1] - c.g_off[g]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (!p->h_members.empty())
    HIPCHK(h, hipMemcpyAsync(p->d_members, p->h_members.data(), sizeof(int) * p->h_members.size(), hipMemcpyHostToDevice, h->stream));
  return DFTPAV_OK;
}

// the filters' rows of the queries no restart is solved for, and the reject flags (trajectory order as d_col: the filters only set them)
static int plan_clear_filter_rows(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  const size_t rows = (size_t)c.Q * c.R;
  if (p->clr.on) { // the map's distance field if the map changed since its last build
    if (int rc = ensure_dist_field(h)) return rc;
    if (int rc = p->clr.clear(h, rows)) return rc;
  }
  if (p->lim.on)
    if (int rc = p->lim.clear(h, rows)) return rc;
  if (p->pen.on)
    if (int rc = p->pen.clear(h, rows)) return rc;
  if (p->cnf.on) // with the own slots of the call and the table's poses at its clocks
    if (int rc = p->cnf.clear(p, rows, c.t_now, c.own)) return rc;
  if (p->cnf.on && p->jnt.on) // the joint rows, and NaN for the poses of the queries no group holds
    if (int rc = p->jnt.clear(p, c.Q, p->cnf.K)) return rc;
  if (p->lim.on || p->clr.on || p->pen.on || p->cnf.on) HIPCHK(h, hipMemsetAsync(p->d_reject, 0, sizeof(int) * rows, h->stream));
  return DFTPAV_OK;
}

// a group's queries out of the front-end arrays into its batch, their restarts drawn; *poses: the group's constraint-point poses
static int plan_pack_group(PlanCall &c, int g, double **poses) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  dftpav_batch *b = c.batch[g];
  const int nm = c.g_off[g + 1] - c.g_off[g];
  b->pending = false;
  b->n_active = nm * c.R;
  b->t_now = c.t_now;
  b->epis = 0.0; // help_eps of the live call, traj_manager.cpp:610
  b->uploaded = true;
  b->solved = false;
  b->coef_override = false;
  b->dev_version = -1; // n_active / t_now live in the device copy of the launch descriptor
  PlanPackArgs A{};
  A.L = b->L;
  A.fe = p->fe;
  A.members = p->d_members + c.g_off[g];
  A.n_members = nm;
  A.n_restarts = c.R;
  A.sigma = c.pp->sigma;
  A.lo = c.pp->dur_lo;
  A.hi = c.pp->dur_hi;
  A.seed = c.pp->seed;
  A.mini_T = h->params.mini_T;
  A.max_vel[0] = h->params.max_forward_vel;
  A.max_vel[1] = h->params.max_backward_vel;
  A.max_acc[0] = h->params.max_forward_acc;
  A.max_acc[1] = h->params.max_backward_acc;
  A.x0 = b->d_x0;
  A.iniS = b->d_iniS;
  A.finS = b->d_finS;
  A.poses = *poses = p->d_poses + 3 * c.pose_off;
  A.mini_t_flag = p->d_minit;
  HIPCHK(h, launch_plan_pack(A, h->stream));
  c.pose_off += (size_t)nm * b->L.Npts;
  return DFTPAV_OK;
}

// per query of a group the cheapest restart that may win, its plan into the compact outputs, every restart's row
static int plan_select_group(PlanCall &c, int g, int *col, int *fst, int *rej) {
  dftpav_planner *p = c.p;
  const dftpav_batch *b = c.batch[g];
  PlanSelectArgs Z{};
  Z.cost = b->d_f;
  Z.success = b->d_success;
  Z.collision = col;
  Z.reject = rej;
  Z.status = b->d_status;
  Z.iters = b->d_iters;
  Z.evals = b->d_evals;
  Z.first_sample = fst;
  Z.x = b->d_x_out;
  Z.coef = b->d_coef;
  Z.dt = b->d_dt;
  Z.n = b->L.n;
  Z.n_coef = 12 * b->L.Ntot;
  Z.M = b->L.M;
  Z.members = p->d_members + c.g_off[g];
  Z.n_members = c.g_off[g + 1] - c.g_off[g];
  Z.R = c.R;
  Z.winner = p->d_winner;
  Z.w_cost = p->d_wcost;
  Z.w_iters = p->d_witers;
  Z.w_x = p->d_wx;
  Z.w_coef = p->d_wcoef;
  Z.w_dt = p->d_wdt;
  Z.x_stride = DFTPAV_PLAN_MAX_VARS;
  Z.coef_stride = c.MS * c.MP * 12;
  Z.dt_stride = c.MS;
  Z.r_cost = p->d_rcost;
  Z.r_status = p->d_rint[0];
  Z.r_success = p->d_rint[1];
  Z.r_iters = p->d_rint[2];
  Z.r_evals = p->d_rint[3];
  Z.r_collision = p->d_rint[4];
  Z.r_first_sample = p->d_rint[5];
  HIPCHK(c.h, launch_plan_select(Z, c.h->stream));
  return DFTPAV_OK;
}

// one group: pack -> rectangles -> solve -> coefficients -> collision re-check (-> limits) (-> clearance) (-> penalty gate) (-> conflicts) -> selection;
// nothing waits in between, or between groups.  With joint selection on the group ends behind its filters: its batch stays resident,
// and its candidates' poses and its selection follow the last group (plan_joint_stage)
static int plan_one_group(PlanCall &c, int g) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  dftpav_batch *b = c.batch[g];
  const int nm = c.g_off[g + 1] - c.g_off[g], R = c.R;
  if (!b || nm == 0) return DFTPAV_OK;
  double *poses = nullptr;
  if (int rc = plan_pack_group(c, g, &poses)) return rc;
  if (int rc = corridor_into_batch(b, poses, nm * b->L.Npts, R)) return rc;
  if (int rc = solve_impl(b, nullptr, false)) return rc;
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  const size_t row0 = (size_t)c.g_off[g] * R;
  const int *members = p->d_members + c.g_off[g];
  int *col = p->d_col + row0, *fst = p->d_first + row0;
  if (int rc = validate_on_stream(b, nm * R, p->d_vt, c.n_t, c.n_v, c.pp->check_dt, col, fst)) return rc;
  int *rej = p->lim.on || p->clr.on || p->pen.on || p->cnf.on ? p->d_reject + row0 : nullptr;
  if (p->lim.on) // rejects a trajectory that is not feasible
    if (int rc = p->lim.run(h, b, members, nm, R, rej)) return rc;
  if (p->clr.on) // rejects a trajectory unless clearance >= min_clearance
    if (int rc = p->clr.run(h, b, members, nm, R, rej)) return rc;
  if (p->pen.on) // rejects a trajectory with a penalty sum above its cap
    if (int rc = p->pen.run(h, b, members, nm, R, rej)) return rc;
  if (p->cnf.on) // rejects a trajectory that comes within the margin of an executing plan
    if (int rc = p->cnf.run(h, b, members, nm, R, rej)) return rc;
  if (p->cnf.on && p->jnt.on) return DFTPAV_OK; // the selection waits for the joint stage
  return plan_select_group(c, g, col, fst, rej);
}

// joint selection, behind the last group: the candidates of the call against each other, the blocked ones flagged, then the
// selection of every group as plan_one_group would have launched it
static int plan_joint_stage(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  h->joint_ev.reset(); // until the whole chain has run
  h->joint_posed = true;
  HIPCHK(h, h->joint_ev.record(0, h->stream));
  for (size_t g = 0; g < c.batch.size(); g++) { // every group's candidates in query order: poses, cost, eligibility, flag index
    const int nm = c.g_off[g + 1] - c.g_off[g];
    if (!c.batch[g] || nm == 0) continue;
    const size_t row0 = (size_t)c.g_off[g] * c.R;
    if (int rc = p->jnt.pose_group(h, c.batch[g], p->d_members + c.g_off[g], nm, c.R, (int)row0, p->d_col + row0, p->d_reject + row0, c.t_now, p->cnf.dt))
      return rc;
  }
  HIPCHK(h, h->joint_ev.record(1, h->stream));
  if (int rc = p->jnt.run(p, c.Q, p->cnf.margin, p->cnf.range)) return rc;
  for (size_t g = 0; g < c.batch.size(); g++) {
    if (!c.batch[g] || c.g_off[g + 1] == c.g_off[g]) continue;
    const size_t row0 = (size_t)c.g_off[g] * c.R;
    if (int rc = plan_select_group(c, (int)g, p->d_col + row0, p->d_first + row0, p->d_reject + row0)) return rc;
  }
  return DFTPAV_OK;
}

// the compact results, the final wait, the statuses that depend on them, and what dftpav_planner_adopt needs of this call
static int plan_results(PlanCall &c) {
  dftpav_planner *p = c.p;
  dftpav_handle *h = c.h;
  const dftpav_plan_out *out = c.out;
  const int Q = c.Q;
  const size_t nq = (size_t)Q, R = (size_t)c.R, MS = (size_t)c.MS, MP = (size_t)c.MP;
  std::vector<int> &winner = p->last_winner, &status = c.status;
  winner.assign(nq, -1);
  p->h_minit.assign(nq, 0);
  HIPCHK(h, fetch_async(h, winner.data(), p->d_winner, sizeof(int) * nq));
  HIPCHK(h, fetch_async(h, p->h_minit.data(), p->d_minit, sizeof(int) * nq));
  HIPCHK(h, fetch_async(h, out->final_cost, p->d_wcost, sizeof(double) * nq));
  HIPCHK(h, fetch_async(h, out->iters, p->d_witers, sizeof(int) * nq));
  HIPCHK(h, fetch_async(h, out->x, p->d_wx, sizeof(double) * nq * DFTPAV_PLAN_MAX_VARS));
  HIPCHK(h, fetch_async(h, out->coeffs, p->d_wcoef, sizeof(double) * nq * MS * MP * 12));
  HIPCHK(h, fetch_async(h, out->coeff_dt, p->d_wdt, sizeof(double) * nq * MS));
  HIPCHK(h, fetch_async(h, out->r_final_cost, p->d_rcost, sizeof(double) * nq * R));
  int *const r_out[6] = {out->r_status, out->r_success, out->r_iters, out->r_evals, out->r_collision, out->r_first_sample};
  for (int k = 0; k < 6; k++) HIPCHK(h, fetch_async(h, r_out[k], p->d_rint[k], sizeof(int) * nq * R));
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
  if (out->search_status) std::memcpy(out->search_status, p->h_sints.data(), sizeof(int) * nq);
  if (out->search_iters) std::memcpy(out->search_iters, p->h_sints.data() + 4 * nq, sizeof(int) * nq);
  if (out->search_path_len) std::memcpy(out->search_path_len, p->h_sints.data() + 7 * nq, sizeof(int) * nq);
  // what dftpav_planner_adopt needs of this call (the winners' pieces stay where they are, in the arena; last_winner: above)
  p->last_status = status;
  p->last_goal.assign(c.end_states, c.end_states + 4 * nq);
  p->last_MS = c.MS;
  p->last_MP = c.MP;
  p->last_Q = Q;
  p->lim.last = p->lim.on;
  p->pen.last = p->pen.on;
  p->clr.last = p->clr.on;
  p->cnf.last = p->cnf.on;
  p->jnt.last = p->cnf.on && p->jnt.on;
  if (p->jnt.last) h->joint_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_plan_queries(dftpav_planner *p, const dftpav_plan_params *pp, const double *start_states, const double *start_ctrl,
                                   const double *end_states, int Q, double t_now, const dftpav_plan_out *out) {
  if (int rc = plan_check_params(p, pp, out, Q)) return rc;
  p->group_sizes.clear();
  p->plan_ev.reset();
  p->last_Q = 0; // nothing to adopt, no filter rows to read, until this call has ended well
  p->lim.last = p->pen.last = p->clr.last = p->cnf.last = p->jnt.last = false;
  std::vector<int> own;
  own.swap(p->own_next); // consumed by this call, whatever becomes of it
  if (Q == 0) return DFTPAV_OK;
  if (!start_states || !start_ctrl || !end_states) return DFTPAV_E_INVALID;
  if (!own.empty() && (int)own.size() != Q) return DFTPAV_E_INVALID; // own slots set for another number of queries
  PlanCall c{p, p->h, pp, start_states, start_ctrl, end_states, Q, t_now, out};
  c.own.swap(own);
  if (int rc = plan_search(c)) return rc;            // marks 0, 1, 2
  if (int rc = plan_read_layouts(c)) return rc;      // the one wait before the end
  if (int rc = plan_group(c)) return rc;
  if (int rc = plan_clear_filter_rows(c)) return rc; // (nothing with every filter off)
  for (size_t g = 0; g < c.batch.size(); g++)
    if (int rc = plan_one_group(c, (int)g)) return rc;
  if (p->cnf.on && p->jnt.on)
    if (int rc = plan_joint_stage(c)) return rc;
  HIPCHK(c.h, p->plan_ev.record(3, c.h->stream));
  p->plan_ev.complete();
  return plan_results(c);
}

extern "C" int dftpav_debug_plan_select(dftpav_handle *h, int n_query, int n_restarts, const double *cost, const int *success,
                                        const int *collision, int *winner_out) {
  if (!h || n_query < 0 || n_restarts < 1 || (n_query > 0 && (!cost || !success || !collision || !winner_out))) return DFTPAV_E_INVALID;
  if (n_query == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nt = (size_t)n_query * n_restarts;
  double *d_cost = nullptr;
  int *d_int = nullptr; // success | collision | winner
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_cost, nt));
  HIPCHK(h, tmp.alloc(d_int, 2 * nt + n_query));
  HIPCHK(h, hipMemcpyAsync(d_cost, cost, sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_int, success, sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_int + nt, collision, sizeof(int) * nt, hipMemcpyHostToDevice, h->stream));
  PlanSelectArgs Z{};
  Z.cost = d_cost;
  Z.success = d_int;
  Z.collision = d_int + nt;
  Z.n_members = n_query;
  Z.R = n_restarts;
  Z.winner = d_int + 2 * nt;
  HIPCHK(h, launch_plan_select(Z, h->stream));
  HIPCHK(h, hipMemcpyAsync(winner_out, d_int + 2 * nt, sizeof(int) * n_query, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_debug_penalty_gate(dftpav_handle *h, int n, const double *terms, const dftpav_penalty_caps *caps, const int *flags_in,
                                         int *flags_out, int *rejected) {
  if (!h || !caps || n < 0 || (n > 0 && (!terms || !flags_in || !flags_out))) return DFTPAV_E_INVALID;
  if (!(caps->corridor >= 0.0) || !(caps->surround >= 0.0) || !(caps->feasibility >= 0.0)) return DFTPAV_E_INVALID;
  if (n == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  double *d_terms = nullptr;
  int *d_int = nullptr; // flags (flags_in != 0 going in, flags_out coming back) | rejected
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_terms, (size_t)n * kCostTerms));
  HIPCHK(h, tmp.alloc(d_int, 2 * (size_t)n));
  std::vector<int> flags((size_t)n);
  for (int t = 0; t < n; t++) flags[t] = flags_in[t] != 0 ? 1 : 0;
  HIPCHK(h, hipMemcpyAsync(d_terms, terms, sizeof(double) * (size_t)n * kCostTerms, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_int, flags.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  PenaltyGateArgs G{};
  G.terms = d_terms;
  G.n = n;
  G.R = 1;
  G.cap_corridor = caps->corridor;
  G.cap_surround = caps->surround;
  G.cap_feas = caps->feasibility;
  G.r_rejected = d_int + n;
  G.reject = d_int;
  HIPCHK(h, launch_penalty_gate(G, h->stream));
  HIPCHK(h, hipMemcpyAsync(flags_out, d_int, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, fetch_async(h, rejected, d_int + n, sizeof(int) * (size_t)n));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// ------------------------------------------------- the replan loop: the executing table, its check and the tick (replan.hip)
// TrajPlannerServer's 20 Hz loop (traj_server_ros.cpp:130-192, 359-501) for every slot of a planner at once.  The table lives in
// device memory; the host mirrors what it needs to pack queries without a read-back: which slots are occupied, and their goals.
extern "C" int dftpav_abi_sizeof_replan_out(void) { return (int)sizeof(dftpav_replan_out); }

// The rows of a slot -- the executing plan (ExecTable) and the publisher's state beside it (PubTable) -- named once: f(row, n) gets
// every device array and the elements it holds per slot.  The table is carved and a slot is cleared by this list.
template <class F> static void for_each_slot_row(ExecTable &T, PubTable &P, F &&f) {
  const size_t ms = (size_t)T.max_seg, mp = (size_t)T.max_pieces;
  f(T.coeffs, ms * mp * 12);
  f(T.coeff_dt, ms);
  f(T.duration, ms);
  f(T.start_time, ms);
  f(T.end_time, ms);
  f(T.end_state, (size_t)4);
  f(T.hist, (size_t)2);
  f(T.n_seg, (size_t)1);
  f(T.singul, ms);
  f(T.piece_nums, ms);
  f(T.have_hist, (size_t)1);
  f(P.hist, (size_t)2);
  f(P.exe_index, (size_t)1);
  f(P.have, (size_t)1);
}
struct SlotRow { // one of them as bytes: where the row starts, and the bytes of a slot
  unsigned char *base;
  size_t bytes;
};
static std::vector<SlotRow> slot_rows(ExecTable T, PubTable P) {
  std::vector<SlotRow> rows;
  for_each_slot_row(T, P, [&](auto *&row, size_t per_slot) { rows.push_back({(unsigned char *)row, sizeof(*row) * per_slot}); });
  return rows;
}

// the table, allocated (and zeroed: every slot empty) by the first call that fills it; later calls must bring the same padding
static int exec_table(dftpav_planner *p, int MS, int MP) {
  dftpav_handle *h = p->h;
  if (MS < 1 || MS > kMaxSeg || MP < 1 || MP > 1024) return DFTPAV_E_INVALID;
  if (p->d_exec) return (p->T.max_seg == MS && p->T.max_pieces == MP) ? DFTPAV_OK : DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t S = (size_t)p->max_queries;
  ExecTable T{};
  PubTable P{};
  T.n_slots = p->max_queries;
  T.max_seg = MS;
  T.max_pieces = MP;
  auto fields = [&](auto &take) {
    for_each_slot_row(T, P, [&](auto *&row, size_t per_slot) { row = static_cast<decltype(+row)>(take(sizeof(*row) * S * per_slot)); });
  };
  unsigned char *base = nullptr;
  const size_t used = carve(nullptr, fields);
  HIPCHK(h, hipMalloc(&base, used));
  if (hipMemsetAsync(base, 0, used, h->stream) != hipSuccess) {
    (void)hipFree(base);
    h->err = "dftpav_planner: hipMemsetAsync of the executing table";
    return DFTPAV_E_HIP;
  }
  carve(base, fields);
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
  auto fields = [&](auto &take) {
    p->d_rc_des = (double *)take(sizeof(double) * 8 * S);
    p->d_rc_st = (double *)take(sizeof(double) * 4 * S);
    p->d_rc_ct = (double *)take(sizeof(double) * 2 * S);
    p->d_rc_goal = (double *)take(sizeof(double) * 4 * S);
    p->d_rc_ego = (double *)take(sizeof(double) * 6 * S);
    p->d_rc_tab = (double *)take(sizeof(double) * (4096 + 4096));
    p->d_rc_int = (int *)take(sizeof(int) * kRcInts * S);
    p->d_pairs = (int *)take(sizeof(int) * 2 * S);
    p->d_pub_mode = (int *)take(sizeof(int) * S);
  };
  unsigned char *base = nullptr;
  HIPCHK(h, hipMalloc(&base, carve(nullptr, fields)));
  carve(base, fields);
  p->d_rc = base;
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_adopt(dftpav_planner *p, int n, const int *queries, const int *slots, double t_start, int *adopted) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && (!queries || !slots))) return DFTPAV_E_INVALID;
  if (p->d_exec && p->last_Q > 0 && (p->T.max_seg != p->last_MS || p->T.max_pieces != p->last_MP)) return DFTPAV_E_INVALID;
  if (int rc = replan_buffers(p)) return rc;
  return adopt_impl(p, n, queries, slots, t_start, nullptr, adopted);
}

// a (stamp, angle) pair per slot into a history row and its flag: the replan check's filter history, or the publisher's
static int set_history_rows(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles, double *d_hist, int *d_have) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && (!slots || !stamps || !angles))) return DFTPAV_E_INVALID;
  if (!p->d_exec || !slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  for (int i = 0; i < n; i++)
    if (!p->h_occupied[slots[i]]) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const int one = 1;
  for (int i = 0; i < n; i++) {
    const double hv[2] = {stamps[i], angles[i]};
    HIPCHK(h, hipMemcpyAsync(d_hist + 2 * (size_t)slots[i], hv, sizeof(hv), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_have + slots[i], &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return DFTPAV_OK;
}
extern "C" int dftpav_planner_set_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles) {
  return set_history_rows(p, n, slots, stamps, angles, p ? p->T.hist : nullptr, p ? p->T.have_hist : nullptr);
}
extern "C" int dftpav_planner_set_ctrl_history(dftpav_planner *p, int n, const int *slots, const double *stamps, const double *angles) {
  return set_history_rows(p, n, slots, stamps, angles, p ? p->P.hist : nullptr, p ? p->P.have : nullptr);
}

extern "C" int dftpav_planner_clear(dftpav_planner *p, int n, const int *slots) {
  if (!p || n < 0 || n > p->max_queries || (n > 0 && !slots)) return DFTPAV_E_INVALID;
  if (!slots_valid(p, n, slots)) return DFTPAV_E_INVALID;
  if (!p->d_exec) return DFTPAV_OK; // nothing was ever installed: every slot is empty
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  const std::vector<SlotRow> rows = slot_rows(p->T, p->P);
  for (int i = 0; i < n; i++) {
    const size_t s = (size_t)slots[i];
    for (const SlotRow &r : rows) HIPCHK(h, hipMemsetAsync(r.base + s * r.bytes, 0, r.bytes, h->stream));
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
  HIPCHK(h, fetch_async(h, n_seg, T.n_seg + s, sizeof(int)));
  HIPCHK(h, fetch_async(h, singul, T.singul + s * MS, sizeof(int) * MS));
  HIPCHK(h, fetch_async(h, piece_nums, T.piece_nums + s * MS, sizeof(int) * MS));
  HIPCHK(h, fetch_async(h, coeff_dt, T.coeff_dt + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch_async(h, coeffs, T.coeffs + s * MS * MP * 12, sizeof(double) * MS * MP * 12));
  HIPCHK(h, fetch_async(h, duration, T.duration + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch_async(h, start_time, T.start_time + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch_async(h, end_time, T.end_time + s * MS, sizeof(double) * MS));
  HIPCHK(h, fetch_async(h, end_state, T.end_state + s * 4, sizeof(double) * 4));
  HIPCHK(h, fetch_async(h, hist, T.hist + s * 2, sizeof(double) * 2));
  HIPCHK(h, fetch_async(h, have_hist, T.have_hist + s, sizeof(int)));
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
    std::vector<double> tab; // (d_rc_tab holds 4096 spacings at most: an outline of 4096 points and more is refused)
    int n_t = 0, n_v = 0;
    if (int rc = validation_table(h->params, check_dt, vertex_res, 4096, tab, &n_t, &n_v)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(p->d_rc_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    p->rc_n_t = n_t;
    p->rc_n_v = n_v;
    p->rc_dt = check_dt;
    p->rc_res = vertex_res;
  }
  if (end_states) HIPCHK(h, hipMemcpyAsync(p->d_rc_goal, end_states, sizeof(double) * 4 * S, hipMemcpyHostToDevice, h->stream));
  if (ego_states) HIPCHK(h, hipMemcpyAsync(p->d_rc_ego, ego_states, sizeof(double) * 6 * S, hipMemcpyHostToDevice, h->stream));
  ReplanArgs A{};
  A.T = p->T;
  A.grid = dev_grid(h);
  A.fp = dev_footprint(h, p->d_rc_tab + p->rc_n_t, p->rc_n_v);
  A.wheel_base = h->params.veh_wheel_base;
  A.tab = SampleTable{p->d_rc_tab, p->rc_n_t, check_dt};
  A.t_now = t_now;
  A.budget = budget;
  A.goals = end_states ? p->d_rc_goal : nullptr;
  A.ego = ego_states ? p->d_rc_ego : nullptr;
  A.o_int = p->d_rc_int;
  A.desired = p->d_rc_des;
  A.start_state = p->d_rc_st;
  A.start_ctrl = p->d_rc_ct;
  HIPCHK(h, p->check_ev.record(0, h->stream));
  HIPCHK(h, launch_replan_check(A, h->stream));
  HIPCHK(h, p->check_ev.record(1, h->stream));
  p->check_ev.complete(); // (never reset: a check that fails leaves the read-out answering)
  return DFTPAV_OK;
}

// copies of the check's results for the caller (enqueued; the caller of this function waits for the stream)
static int replan_check_fetch(dftpav_planner *p, const dftpav_replan_out *out) {
  if (!out) return DFTPAV_OK;
  dftpav_handle *h = p->h;
  const size_t S = (size_t)p->max_queries;
  int *const io[kRcInts] = {out->occupied, out->complete, out->exe_index, out->is_close_turnpoint, out->is_near, out->target_moved,
                            out->collision, out->first_sample, out->replan};
  for (int k = 0; k < kRcInts; k++) HIPCHK(h, fetch_async(h, io[k], p->d_rc_int + (size_t)k * S, sizeof(int) * S));
  HIPCHK(h, fetch_async(h, out->desired, p->d_rc_des, sizeof(double) * 8 * S));
  HIPCHK(h, fetch_async(h, out->start_state, p->d_rc_st, sizeof(double) * 4 * S));
  HIPCHK(h, fetch_async(h, out->start_ctrl, p->d_rc_ct, sizeof(double) * 2 * S));
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
  const bool trigger = p->trg.on;
  if (trigger && !std::isfinite(t_now + budget)) return DFTPAV_E_INVALID; // the trigger's first clock is the adoption clock
  p->trg.last = false;
  if (!p->d_exec) { // an all-empty table is a valid start (every vehicle waits for its first plan)
    if (int rc = exec_table(p, pp->max_seg, pp->max_pieces)) return rc;
  }
  p->tick_ev.reset();
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, p->tick_ev.record(0, h->stream));
  if (int rc = replan_check_enqueue(p, t_now, budget, end_states, ego_states, pp->check_dt, pp->vertex_res)) return rc;
  // ---- the conflict trigger, behind the check on the same stream: the table's poses from the adoption clock on, then who yields
  if (trigger)
    if (int rc = p->trg.run(p, t_now, t_now + budget)) return rc;
  // ---- the tick's one extra wait: replan, start_state, start_ctrl (with whatever else of the check the caller asked for)
  const size_t S = (size_t)p->max_queries;
  std::vector<int> &flag = p->h_rc_flag; // (the planner's: a failing fetch below returns with these copies enqueued)
  std::vector<double> &st = p->h_rc_st, &ct = p->h_rc_ct;
  flag.assign(S, 0);
  st.resize(4 * S);
  ct.resize(2 * S);
  HIPCHK(h, hipMemcpyAsync(flag.data(), p->d_rc_int + (size_t)kRcReplan * S, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(st.data(), p->d_rc_st, sizeof(double) * 4 * S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ct.data(), p->d_rc_ct, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, h->stream));
  if (int rc = replan_check_fetch(p, check_out)) return rc;
  if (trigger) { // yield joins the read-back in front of the one wait
    p->trg.h_yield.assign(S, 0);
    HIPCHK(h, hipMemcpyAsync(p->trg.h_yield.data(), p->trg.d_rows, sizeof(int) * S, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (trigger) {
    h->trig_ev.complete();
    p->trg.last = true;
  }
  // ---- the flagged slots (the check's flag, or the trigger's yield), in rising slot order, are the queries
  std::vector<int> slot_of;
  std::vector<double> qs, qc, qe;
  for (size_t s = 0; s < S; s++) {
    if (!flag[s] && !(trigger && p->trg.h_yield[s])) continue;
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
    p->own_next = slot_of; // a query is the replan of its slot: not in conflict with the plan it replaces
    const int rc_plan = dftpav_plan_queries(p, pp, qs.data(), qc.data(), qe.data(), nq, stamp, plan_out ? plan_out : &none);
    p->own_next.clear(); // (a call refused before it consumed them)
    if (rc_plan) return rc_plan;
    std::vector<int> qi(nq);
    for (int q = 0; q < nq; q++) qi[q] = q;
    if (int rc = adopt_impl(p, nq, qi.data(), slot_of.data(), stamp, p->d_rc_des, nullptr)) return rc;
  }
  HIPCHK(h, p->tick_ev.record(1, h->stream));
  p->tick_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_replan_last_ms(dftpav_planner *p, float *check_ms, float *tick_ms) {
  if (!p) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (check_ms) *check_ms = 0.0f;
  if (tick_ms) *tick_ms = 0.0f;
  HIPCHK(h, hipSetDevice(h->device));
  if (check_ms && p->check_ev.reached()) HIPCHK(h, p->check_ev.elapsed(check_ms, 0, 1, true));
  if (tick_ms && p->tick_ev.reached()) HIPCHK(h, p->tick_ev.elapsed(tick_ms, 0, 1, true));
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
  if ((size_t)K > p->pub_ticks) { // the clocks and the outputs of K ticks: one allocation, grown to the largest K met
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (p->d_pub) (void)hipFree(p->d_pub);
    p->d_pub = nullptr;
    p->pub_ticks = 0;
    auto fields = [&](auto &take) {
      p->d_pub_states = (double *)take(sizeof(double) * 8 * S * (size_t)K);
      p->d_pub_t = (double *)take(sizeof(double) * (size_t)K);
      p->d_pub_code = (int *)take(sizeof(int) * S * (size_t)K);
    };
    unsigned char *base = nullptr;
    HIPCHK(h, hipMalloc(&base, carve(nullptr, fields)));
    carve(base, fields);
    p->d_pub = base;
    p->pub_ticks = (size_t)K;
  }
  p->pub_ev.reset();
  HIPCHK(h, hipMemcpyAsync(p->d_pub_t, t, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, h->stream));
  PublishArgs A{};
  A.T = p->T;
  A.P = p->P;
  A.K = K;
  A.t = p->d_pub_t;
  A.wheel_base = h->params.veh_wheel_base;
  A.states = states ? p->d_pub_states : nullptr;
  A.published = published ? p->d_pub_code : nullptr;
  HIPCHK(h, p->pub_ev.record(0, h->stream));
  HIPCHK(h, launch_publish(A, h->stream));
  HIPCHK(h, p->pub_ev.record(1, h->stream));
  p->pub_ev.complete();
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
  HIPCHK(h, fetch_async(h, exe_index, p->P.exe_index + s, sizeof(int)));
  HIPCHK(h, fetch_async(h, hist, p->P.hist + s * 2, sizeof(double) * 2));
  HIPCHK(h, fetch_async(h, have_hist, p->P.have + s, sizeof(int)));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_publish_last_ms(dftpav_planner *p, float *ms) {
  if (!p || !ms) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  *ms = 0.0f;
  if (!p->pub_ev.reached()) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, p->pub_ev.elapsed(ms, 0, 1, true));
  return DFTPAV_OK;
}

// ------------------------------------------------- the sample table of a selection filter
// A validation_table for (check_dt, vertex_res) kept on the device.  It lies at the head of the filter's one allocation `base`, made by
// the first call (rows(take) names the filter's other arrays), and is uploaded again only when check_dt is not the one T holds.  A
// refusal changes nothing.
template <class F> static int cached_table(dftpav_handle *h, double check_dt, double vertex_res, unsigned char *&base, CachedTable &T, F &&rows) {
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> tab;
  int n_t = 0, n_v = 0;
  if (int rc = validation_table(h->params, check_dt, vertex_res, 0, tab, &n_t, &n_v)) return rc;
  if (!base) {
    if (int rc = regrow(h, base, [&](auto &take) {
          T.d = (double *)take(sizeof(double) * tab.size()); // (its size follows from the parameters alone)
          rows(take);
        }))
      return rc;
    T.dt = 0.0;
  }
  if (T.dt != check_dt) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(T.d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    T.dt = check_dt;
    T.n_t = n_t;
    T.n_v = n_v;
  }
  return DFTPAV_OK;
}

// ------------------------------------------------- solved plans against the kinematic limits (limits.hip)
extern "C" int dftpav_planner_check_limits(dftpav_planner *p, double check_dt, const dftpav_limits *l, const dftpav_limits_out *out) {
  if (!p || !l || !out || !(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  LimitsCommon C{};
  if (!limits_common(h->params, *l, C)) return DFTPAV_E_INVALID;
  const size_t S = (size_t)p->max_queries;
  if (!p->d_exec) { // nothing was ever installed: every slot is empty
    if (out->max_abs) std::fill(out->max_abs, out->max_abs + kLimQ * S, 0.0);
    if (out->arg) std::fill(out->arg, out->arg + kLimQ * S, -1);
    if (out->violated) std::fill(out->violated, out->violated + kLimQ * S, 0);
    if (out->feasible) std::fill(out->feasible, out->feasible + S, 0);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  return check_limits_rows(h, check_dt, S, out, C, [&](const LimitsCommon &done) {
    return launch_limits_table(LimitsTableArgs{done, p->T}, h->stream);
  });
}

// the limit filter (LimitFilter, capi_internal.h)
bool LimitFilter::common(const dftpav_handle *h, LimitsCommon &C) const {
  C = rows();
  C.tab = SampleTable{tab.d, tab.n_t, tab.dt};
  return limits_common(h->params, lim, C);
}
int LimitFilter::configure(dftpav_handle *h, size_t rows_cap, const dftpav_limits &l, double check_dt) {
  if (int rc = cached_table(h, check_dt, 1.0, d, tab, [&](auto &take) { // (the kernel reads the sample times only)
        d_max = (double *)take(sizeof(double) * kLimQ * rows_cap);
        d_int = (int *)take(sizeof(int) * (2 * kLimQ + 1) * rows_cap);
      }))
    return rc;
  cap = rows_cap;
  lim = l;
  on = true;
  return DFTPAV_OK;
}
int LimitFilter::clear(dftpav_handle *h, size_t rows) { // zero, arg -1
  const LimitsCommon C = this->rows();
  HIPCHK(h, hipMemsetAsync(C.max_abs, 0, sizeof(double) * kLimQ * rows, h->stream));
  HIPCHK(h, hipMemsetAsync(C.arg, 0xff, sizeof(int) * kLimQ * rows, h->stream));
  HIPCHK(h, hipMemsetAsync(C.violated, 0, sizeof(int) * kLimQ * rows, h->stream));
  HIPCHK(h, hipMemsetAsync(C.feasible, 0, sizeof(int) * rows, h->stream));
  return DFTPAV_OK;
}
int LimitFilter::run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject) {
  LimitsBatchArgs A{};
  if (!common(h, A.C)) return DFTPAV_E_INVALID; // (checked when the filter was set)
  A.coeffs = b->d_coef;
  A.piece_dt = b->d_dt;
  A.L = b->L;
  A.B = nm * R;
  A.members = members;
  A.R = R;
  A.reject = reject;
  HIPCHK(h, launch_limits_batch(A, h->stream));
  return DFTPAV_OK;
}
int LimitFilter::fetch(dftpav_handle *h, const dftpav_limits_out *out, size_t rows) { return fetch_limits(h, out, this->rows(), rows); }

extern "C" int dftpav_planner_set_limit_filter(dftpav_planner *p, const dftpav_limits *l, double check_dt) {
  if (!p) return DFTPAV_E_INVALID;
  if (!l) { // off: the buffers stay, nothing reads them
    p->lim.on = false;
    return DFTPAV_OK;
  }
  if (!(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID;
  LimitsCommon C{};
  if (!limits_common(p->h->params, *l, C)) return DFTPAV_E_INVALID;
  return p->lim.configure(p->h, (size_t)p->max_queries * p->R, *l, check_dt);
}

extern "C" int dftpav_planner_last_limits(dftpav_planner *p, const dftpav_limits_out *out) {
  if (!p || !out || !p->lim.last || p->last_Q <= 0) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->lim.fetch(h, out, (size_t)p->last_Q * p->R)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// ------------------------------------------------- the residual penalties of solved plans (solver_ref.hip: kModeTerms, plan.hip)
// the penalty filter (PenaltyFilter, capi_internal.h)
int PenaltyFilter::configure(dftpav_handle *h, size_t rows_cap, const dftpav_penalty_caps &c) {
  if (!d) {
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = regrow(h, d, [&](auto &take) {
          d_terms = (double *)take(sizeof(double) * kCostTerms * rows_cap);
          d_rej = (int *)take(sizeof(int) * rows_cap);
        }))
      return rc;
  }
  caps = c;
  on = true;
  return DFTPAV_OK;
}
int PenaltyFilter::clear(dftpav_handle *h, size_t rows) { // zero
  HIPCHK(h, hipMemsetAsync(d_terms, 0, sizeof(double) * kCostTerms * rows, h->stream));
  HIPCHK(h, hipMemsetAsync(d_rej, 0, sizeof(int) * rows, h->stream));
  return DFTPAV_OK;
}
int PenaltyFilter::run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject) {
  if (int rc = cost_terms_on_stream(b, nullptr)) return rc;
  PenaltyGateArgs G{};
  G.terms = b->d_terms;
  G.members = members;
  G.n = nm * R;
  G.R = R;
  G.cap_corridor = caps.corridor;
  G.cap_surround = caps.surround;
  G.cap_feas = caps.feasibility;
  G.r_terms = d_terms;
  G.r_rejected = d_rej;
  G.reject = reject;
  HIPCHK(h, launch_penalty_gate(G, h->stream));
  return DFTPAV_OK;
}
int PenaltyFilter::fetch(dftpav_handle *h, double *r_terms, int *r_rejected, size_t rows) {
  HIPCHK(h, fetch_async(h, r_terms, d_terms, sizeof(double) * kCostTerms * rows));
  HIPCHK(h, fetch_async(h, r_rejected, d_rej, sizeof(int) * rows));
  return DFTPAV_OK;
}

extern "C" int dftpav_planner_set_penalty_filter(dftpav_planner *p, const dftpav_penalty_caps *caps) {
  if (!p) return DFTPAV_E_INVALID;
  if (!caps) { // off: the buffers stay, nothing reads them
    p->pen.on = false;
    return DFTPAV_OK;
  }
  if (!(caps->corridor >= 0.0) || !(caps->surround >= 0.0) || !(caps->feasibility >= 0.0)) return DFTPAV_E_INVALID; // negative, NaN
  return p->pen.configure(p->h, (size_t)p->max_queries * p->R, *caps);
}

extern "C" int dftpav_planner_last_cost_terms(dftpav_planner *p, double *r_terms, int *r_rejected) {
  if (!p || (!r_terms && !r_rejected) || !p->pen.last || p->last_Q <= 0) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->pen.fetch(h, r_terms, r_rejected, (size_t)p->last_Q * p->R)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// ------------------------------------------------- the clearance of executing plans, and the clearance filter (clearance.hip)
extern "C" int dftpav_planner_check_clearance(dftpav_planner *p, double check_dt, const dftpav_clearance_out *out) {
  if (!p || !out || !(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  const size_t S = (size_t)p->max_queries;
  if (!p->d_exec) { // nothing was ever installed: every slot is empty
    if (out->min_d2) std::fill(out->min_d2, out->min_d2 + S, DFTPAV_DIST_FAR);
    if (out->arg) std::fill(out->arg, out->arg + S, -1);
    if (out->clearance) std::fill(out->clearance, out->clearance + S, HUGE_VAL);
    return DFTPAV_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  return check_clearance_rows(h, check_dt, S, out, [&](const ClearanceCommon &C) {
    return launch_clearance_table(ClearanceTableArgs{C, p->T}, h->stream);
  });
}

// the clearance filter (ClearanceFilter, capi_internal.h)
int ClearanceFilter::configure(dftpav_handle *h, size_t rows_cap, double min_clearance, double check_dt) {
  if (int rc = cached_table(h, check_dt, kClearanceVertexRes, d, tab, [&](auto &take) {
        d_m = (double *)take(sizeof(double) * rows_cap);
        d_d2 = (int *)take(sizeof(int) * rows_cap);
        d_arg = (int *)take(sizeof(int) * rows_cap);
      }))
    return rc;
  if (h_inf.empty()) h_inf.assign(rows_cap, HUGE_VAL);
  min = min_clearance;
  on = true;
  return DFTPAV_OK;
}
int ClearanceFilter::clear(dftpav_handle *h, size_t rows) { // FAR, -1, +inf
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)d_d2, DFTPAV_DIST_FAR, rows, h->stream));
  HIPCHK(h, hipMemsetAsync(d_arg, 0xff, sizeof(int) * rows, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_m, h_inf.data(), sizeof(double) * rows, hipMemcpyHostToDevice, h->stream));
  return DFTPAV_OK;
}
int ClearanceFilter::run(dftpav_handle *h, dftpav_batch *b, const int *members, int nm, int R, int *reject) {
  ClearanceBatchArgs A{};
  A.C = clearance_common(h, tab.d, tab.n_t, tab.n_v, tab.dt);
  A.C.min_d2 = d_d2;
  A.C.arg = d_arg;
  A.C.clearance = d_m;
  A.coeffs = b->d_coef;
  A.piece_dt = b->d_dt;
  A.L = b->L;
  A.B = nm * R;
  A.members = members;
  A.R = R;
  A.reject = reject;
  A.min_clearance = min;
  HIPCHK(h, launch_clearance_batch(A, h->stream));
  return DFTPAV_OK;
}
int ClearanceFilter::fetch(dftpav_handle *h, const dftpav_clearance_out *out, size_t rows) { return fetch_clearance(h, out, d_d2, d_arg, d_m, rows); }

extern "C" int dftpav_planner_set_clearance_filter(dftpav_planner *p, double min_clearance, double check_dt) {
  if (!p) return DFTPAV_E_INVALID;
  if (min_clearance < 0.0) { // off: the buffers stay, nothing reads them
    p->clr.on = false;
    return DFTPAV_OK;
  }
  if (!std::isfinite(min_clearance) || !(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID; // NaN, +inf
  return p->clr.configure(p->h, (size_t)p->max_queries * p->R, min_clearance, check_dt);
}

extern "C" int dftpav_planner_last_clearance(dftpav_planner *p, const dftpav_clearance_out *out) {
  if (!p || !out || !p->clr.last || p->last_Q <= 0) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = p->clr.fetch(h, out, (size_t)p->last_Q * p->R)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

// ------------------------------------------------- the executing plans' swept footprints stamped into the map (stamp.hip)
extern "C" int dftpav_planner_stamp_slots(dftpav_planner *p, const unsigned char *select, double t0, double dt, int K, double inflate) {
  if (!p || !conflict_clocks_ok(t0, dt, K) || !(inflate >= 0.0) || !std::isfinite(inflate)) return DFTPAV_E_INVALID;
  dftpav_handle *h = p->h;
  if (!h->d_cells || !p->d_exec) return DFTPAV_E_INVALID; // no map; no table
  HIPCHK(h, hipSetDevice(h->device));
  const int S_pad = conflict_s_pad(p);
  const size_t n = (size_t)K * S_pad;
  if (n > (size_t)INT_MAX) return DFTPAV_E_UNSUPPORTED; // the box kernel counts its boxes in an int
  double *d_pose = nullptr;
  unsigned char *d_occupied = nullptr, *d_select = nullptr;
  auto fields = [&](auto take) {
    d_pose = (double *)take(sizeof(double) * 4 * n);
    d_occupied = (unsigned char *)take((size_t)S_pad);
    d_select = (unsigned char *)take((size_t)S_pad);
  };
  if (int rc = grow(h, h->d_stamp_ws, h->stamp_ws_bytes, carve(nullptr, fields))) return rc;
  carve(h->d_stamp_ws, fields);
  if (select) {
    if (h->stamp_sel_ev) HIPCHK(h, hipEventSynchronize(h->stamp_sel_ev)); // the last call's copy has read the vector
    else HIPCHK(h, hipEventCreateWithFlags(&h->stamp_sel_ev, hipEventDisableTiming));
    h->stamp_sel.assign((size_t)S_pad, 0); // the padding behind the last slot is unselected
    std::copy(select, select + p->max_queries, h->stamp_sel.begin());
    HIPCHK(h, hipMemcpyAsync(d_select, h->stamp_sel.data(), (size_t)S_pad, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->stamp_sel_ev, h->stream));
  }
  ConflictPoses P{};
  if (int rc = conflict_poses_into(p, d_pose, d_occupied, &h->stamp_ev, t0, dt, K, P)) return rc;
  h->stamp_posed = true;
  return stamp_boxes_on_stream(h, P.cx, P.cy, P.cs, P.sn, (int)n, select ? d_select : nullptr, S_pad, inflate);
}
