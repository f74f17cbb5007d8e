// capi_steps.cpp — the steps of a planning cycle around the solve, each a service of its own and chained on the stream by
// dftpav_plan_cycle: restarts, front-end resampling, Reeds-Shepp shots, the hybrid A* search, the map and its corridors, the
// collision re-check, the state read-out.
#include "capi_internal.h"

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
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_in, std::max<size_t>(1, (size_t)n_hyp * n_inner)));
  HIPCHK(h, tmp.alloc(d_du, (size_t)n_hyp * M));
  HIPCHK(h, tmp.alloc(d_oi, std::max<size_t>(1, B * n_inner)));
  HIPCHK(h, tmp.alloc(d_od, B * M));
  HIPCHK(h, hipMemcpyAsync(d_in, inner_pts, sizeof(double) * (size_t)n_hyp * n_inner, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_du, durations, sizeof(double) * (size_t)n_hyp * M, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_restarts(d_in, d_du, n_hyp, n_restarts, n_inner, M, sigma, dur_lo, dur_hi, seed, d_oi, d_od, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_inner_pts, d_oi, sizeof(double) * B * n_inner, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_durations, d_od, sizeof(double) * B * M, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
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
  DevScratch tmp(h);
  for (Buf &b : bufs) {
    if (!b.src && !b.dst) return DFTPAV_E_INVALID;
    HIPCHK(h, tmp.alloc_bytes(b.dev, b.bytes));
    if (b.src) HIPCHK(h, hipMemcpyAsync(*b.dev, b.src, b.bytes, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(*b.dev, 0, b.bytes, h->stream));
  }
  HIPCHK(h, launch_frontend(*fp, d_paths, d_len, max_path, d_ss, d_es, d_sc, n_hyp, D, h->stream));
  for (Buf &b : bufs)
    if (b.dst) HIPCHK(h, hipMemcpyAsync(b.dst, *b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
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
  std::vector<double> vv; // spacing of the outline points as the reference's running sum (shapes.cc:128)
  if (collides) {
    const double longest = std::max(h->params.veh_length, h->params.veh_width) + 1.0;
    for (double dl = vertex_res; dl < longest; dl += vertex_res) vv.push_back(dl);
  }
  if (vv.empty()) vv.push_back(1.0);
  double *d_from = nullptr, *d_to = nullptr, *d_len = nullptr, *d_seg = nullptr, *d_smp = nullptr, *d_v = nullptr;
  int *d_type = nullptr, *d_ns = nullptr, *d_col = nullptr;
  const size_t nn = (size_t)n, nsmp = nn * max_samples * 3;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_from, 3 * nn));
  HIPCHK(h, tmp.alloc(d_to, 3 * nn));
  HIPCHK(h, tmp.alloc(d_len, nn));
  HIPCHK(h, tmp.alloc(d_seg, 5 * nn));
  HIPCHK(h, tmp.alloc(d_smp, nsmp));
  HIPCHK(h, tmp.alloc(d_v, vv.size()));
  HIPCHK(h, tmp.alloc(d_type, nn));
  HIPCHK(h, tmp.alloc(d_ns, nn));
  HIPCHK(h, tmp.alloc(d_col, nn));
  h->cor_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_from, from, sizeof(double) * 3 * nn, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_to, to, sizeof(double) * 3 * nn, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_v, vv.data(), sizeof(double) * vv.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->cor_ev.record(0, h->stream));
  ShotArgs A{d_from, d_to, n, 1.0 / max_cur, checkl, max_samples, dev_grid(h), dev_footprint(h, d_v, (int)vv.size()),
             d_len, d_type, d_seg, d_smp, d_ns, d_col};
  if (!collides) A.grid.cells = nullptr; // no collision check
  HIPCHK(h, launch_shots(A, h->stream));
  HIPCHK(h, h->cor_ev.record(1, h->stream));
  HIPCHK(h, fetch_async(h, length, d_len, sizeof(double) * nn));
  HIPCHK(h, fetch_async(h, type, d_type, sizeof(int) * nn));
  HIPCHK(h, fetch_async(h, seg, d_seg, sizeof(double) * 5 * nn));
  HIPCHK(h, fetch_async(h, samples, d_smp, sizeof(double) * nsmp));
  HIPCHK(h, fetch_async(h, n_samples, d_ns, sizeof(int) * nn));
  HIPCHK(h, fetch_async(h, collides, d_col, sizeof(int) * nn));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cor_ev.complete();
  return DFTPAV_OK;
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

int dftpav::search_setup(dftpav_handle *h, const dftpav_search_params *sp, int n, SearchSetup &U) {
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
  S.grid = dev_grid(h);
  S.fp = DevFootprint{P.veh_width, P.veh_length, P.veh_d_cr, nullptr, (int)vv.size()}; // (v_tab: wire_search)
  S.inv_yaw_res = 1.0 / P.phi_grid_resolution; // kino_astar.cpp:421
  S.origin_sx = -0.5 * P.map_size_x;
  S.origin_sy = -0.5 * P.map_size_y;
  S.half_size_x = P.map_size_x * 0.5;
  S.half_size_y = P.map_size_y * 0.5;
  S.rho = rho;
  for (int k = 0; k < 3; k++) S.n_in[k] = n_in[k];
  S.n = n;
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
  if (int rc = search_setup(h, sp, n, U)) return rc;
  GoalFieldPlan G; // dftpav_set_search_heuristic; off: G.per_turn == 0 and nothing below differs
  if (int rc = search_heuristic_plan(h, start_states, end_states, n, U, G)) return rc;
  const size_t nn = (size_t)n, n_nodes = 6 * nn * out->max_nodes, n_paths = 3 * nn * out->max_path;
  double *d_tabs = nullptr, *d_st = nullptr, *d_en = nullptr, *d_nodes = nullptr, *d_paths = nullptr;
  int *d_ints = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_tabs, U.tabs.size()));
  HIPCHK(h, tmp.alloc(d_st, 4 * nn));
  HIPCHK(h, tmp.alloc(d_en, 4 * nn));
  HIPCHK(h, tmp.alloc(d_ints, 9 * nn));
  if (out->max_nodes > 0) HIPCHK(h, tmp.alloc(d_nodes, n_nodes));
  if (out->max_path > 0) HIPCHK(h, tmp.alloc(d_paths, n_paths));
  h->cor_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_tabs, U.tabs.data(), sizeof(double) * U.tabs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_st, start_states, sizeof(double) * 4 * nn, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_en, end_states, sizeof(double) * 4 * nn, hipMemcpyHostToDevice, h->stream));
  // rows past n_nodes / path_len read back as zeros
  if (d_nodes) HIPCHK(h, hipMemsetAsync(d_nodes, 0, sizeof(double) * n_nodes, h->stream));
  if (d_paths) HIPCHK(h, hipMemsetAsync(d_paths, 0, sizeof(double) * n_paths, h->stream));
  wire_search(U, d_tabs, d_st, d_en, d_ints, nn, out->max_nodes, d_nodes, out->max_path, d_paths);
  HIPCHK(h, h->cor_ev.record(0, h->stream));
  for (int q0 = 0; q0 < n; q0 += U.slots) {
    U.S.q0 = q0;
    if (G.per_turn)
      if (int rc = goal_field_turn(h, G, q0 / U.slots, &U.S, nullptr)) return rc;
    HIPCHK(h, launch_search(U.S, std::min(U.slots, n - q0), h->stream));
  }
  HIPCHK(h, h->cor_ev.record(1, h->stream));
  int *const fields[8] = {out->status, out->shot_success, out->used_3d, out->budget_hit, out->iters, out->nodes_used, out->n_nodes, out->path_len};
  for (int f = 0; f < 8; f++) HIPCHK(h, hipMemcpyAsync(fields[f], d_ints + f * nn, sizeof(int) * nn, hipMemcpyDeviceToHost, h->stream));
  if (d_nodes) HIPCHK(h, hipMemcpyAsync(out->nodes, d_nodes, sizeof(double) * n_nodes, hipMemcpyDeviceToHost, h->stream));
  if (d_paths) HIPCHK(h, hipMemcpyAsync(out->paths, d_paths, sizeof(double) * n_paths, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cor_ev.complete();
  for (int q = 0; q < n; q++)
    if (out->status[q] == 0) return DFTPAV_E_UNSUPPORTED; // a shot beyond the sample table (not reached: see the bound)
  return DFTPAV_OK;
}

void dftpav::wire_search(SearchSetup &U, double *d_tabs, double *d_start, double *d_end, int *d_ints, size_t n, int max_nodes,
                         double *d_nodes, int max_path, double *d_paths) {
  SearchArgs &S = U.S;
  S.in_tab = d_tabs;
  S.fp.v_tab = d_tabs + U.n_in_tab;
  S.l_tab = d_tabs + U.n_in_tab + U.n_vv;
  S.start = d_start;
  S.end = d_end;
  dftpav_search_out &O = S.out;
  O.max_nodes = max_nodes;
  O.max_path = max_path;
  O.status = d_ints;
  O.shot_success = d_ints + n;
  O.used_3d = d_ints + 2 * n;
  O.budget_hit = d_ints + 3 * n;
  O.iters = d_ints + 4 * n;
  O.nodes_used = d_ints + 5 * n;
  O.n_nodes = d_ints + 6 * n;
  O.path_len = d_ints + 7 * n;
  O.nodes = d_nodes;
  O.paths = d_paths;
}

// the maps that get the corridor's bit map: <= 40 KB of bits per workgroup, four workgroups per CU
static constexpr size_t kBitMapMaxCells = (size_t)8 * 40 * 1024;

// the table of a map's resolution on the device (h->d_dl is null): the sample offsets of CheckIfCollisionUsingLine
// (map_adapter.cpp:119): dl = 0, then dl += checkl; the longest segment is the far edge of a fully grown rectangle
static int map_line_table(dftpav_handle *h, double resolution) {
  const double checkl = resolution / 2.0;
  const double longest = std::max(h->params.veh_length, h->params.veh_width) + 2.0 * (10.0 + resolution) + 1.0;
  std::vector<double> dl;
  for (double v = 0.0; v < longest; v += checkl) dl.push_back(v);
  h->n_dl = (int)dl.size();
  HIPCHK(h, hipMalloc(&h->d_dl, sizeof(double) * dl.size()));
  HIPCHK(h, hipMemcpy(h->d_dl, dl.data(), sizeof(double) * dl.size(), hipMemcpyHostToDevice));
  return DFTPAV_OK;
}

extern "C" int dftpav_set_grid_map(dftpav_handle *h, const dftpav_grid_map *map) {
  if (!h || !map || !map->cells || map->size_x <= 0 || map->size_y <= 0 || !(map->resolution > 0.0)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->d_cells) (void)hipFree(h->d_cells);
  if (h->d_bits) (void)hipFree(h->d_bits);
  if (h->d_dl) (void)hipFree(h->d_dl);
  if (h->d_cells_base) (void)hipFree(h->d_cells_base); // a new map has no stamps
  h->d_cells = nullptr;
  h->d_bits = nullptr;
  h->d_dl = nullptr;
  h->d_cells_base = nullptr;
  const size_t ncell = (size_t)map->size_x * map->size_y;
  HIPCHK(h, hipMalloc(&h->d_cells, ncell));
  HIPCHK(h, hipMemcpy(h->d_cells, map->cells, ncell, hipMemcpyHostToDevice));
  h->map = *map;
  h->map.cells = nullptr;
  h->dist_stale = true; // the distance field, if a clearance call ever asks for one, is built again by that call
  if (ncell <= kBitMapMaxCells) {
    std::vector<unsigned> bits((ncell + 31) / 32, 0u);
    for (size_t i = 0; i < ncell; i++)
      if (map->cells[i] == 80) bits[i >> 5] |= 1u << (i & 31);
    HIPCHK(h, hipMalloc(&h->d_bits, sizeof(unsigned) * bits.size()));
    HIPCHK(h, hipMemcpy(h->d_bits, bits.data(), sizeof(unsigned) * bits.size(), hipMemcpyHostToDevice));
  }
  return map_line_table(h, map->resolution);
}

// uploads the states and runs the corridor kernel into `hpoly` (device, [n][16]) or into a batch's corridor
// the corridor kernel's arguments for n states (device) of the handle's map and vehicle
static CorridorArgs corridor_args(const dftpav_handle *h, const double *d_states, int n, double *d_hpoly, double *batch_cor, int Npts,
                                  int NptsPad, int replicate) {
  return CorridorArgs{dev_grid(h), h->d_bits, 0.0, d_states, n, h->params.veh_width, h->params.veh_length, h->params.veh_d_cr,
                      h->d_dl, h->n_dl, d_hpoly, batch_cor, Npts, NptsPad, replicate};
}

static int run_corridor(dftpav_handle *h, const double *states, int n_states, double *d_hpoly, double *batch_cor, int Npts,
                        int NptsPad, int replicate) {
  double *d_states = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_states, 3 * (size_t)n_states));
  h->cor_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_states, states, sizeof(double) * 3 * (size_t)n_states, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->cor_ev.record(0, h->stream));
  HIPCHK(h, launch_corridor(corridor_args(h, d_states, n_states, d_hpoly, batch_cor, Npts, NptsPad, replicate), h->stream));
  HIPCHK(h, h->cor_ev.record(1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cor_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_corridor_last_ms(dftpav_handle *h, float *ms) {
  if (!h || !ms || !h->cor_ev.reached()) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->cor_ev.elapsed(ms, 0, 1, false));
  return DFTPAV_OK;
}

extern "C" int dftpav_corridor_rectangles(dftpav_handle *h, const double *states, int n_states, double *hpoly) {
  if (!h || !states || !hpoly || n_states < 0) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (n_states == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  double *d_hpoly = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_hpoly, 16 * (size_t)n_states));
  if (int rc = run_corridor(h, states, n_states, d_hpoly, nullptr, 1, 1, 1)) return rc;
  HIPCHK(h, hipMemcpy(hpoly, d_hpoly, sizeof(double) * 16 * (size_t)n_states, hipMemcpyDeviceToHost));
  return DFTPAV_OK;
}

int dftpav::corridor_into_batch(dftpav_batch *b, const double *d_poses, int n_poses, int replicate) {
  dftpav_handle *h = b->h;
  HIPCHK(h, launch_corridor(corridor_args(h, d_poses, n_poses, nullptr, b->d_corridor, b->L.Npts, b->NptsPad, replicate), h->stream));
  b->have_corridor = true;
  b->cor_t_dirty = true;
  b->cor_rect = false;
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
int dftpav::ensure_coeffs(dftpav_batch *b, DevBatch &D) {
  dftpav_handle *h = b->h;
  if (int rc = finish_pending(b)) return rc;
  if (int rc = sync_dev(b, D)) return rc;
  if (!b->coef_override) HIPCHK(h, launch_for(b, D, kModeCoeffs));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_coeffs(dftpav_batch *b, double *coeffs, double *piece_dt) {
  if (!b || !b->uploaded || !b->solved) return DFTPAV_E_INVALID; // the coefficients are those of the solution x
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = finish_pending(b)) return rc;
  DevBatch D;
  if (int rc = sync_dev(b, D)) return rc;
  HIPCHK(h, launch_for(b, D, kModeCoeffs)); // (always: this call reports what follows from x, whatever the test hook installed)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (coeffs)
    HIPCHK(h, hipMemcpy(coeffs, b->d_coef, sizeof(double) * (size_t)b->B * 12 * b->L.Ntot, hipMemcpyDeviceToHost));
  if (piece_dt) HIPCHK(h, hipMemcpy(piece_dt, b->d_dt, sizeof(double) * (size_t)b->B * b->L.M, hipMemcpyDeviceToHost));
  return DFTPAV_OK;
}

int dftpav::validation_table(const dftpav_params &p, double check_dt, double vertex_res, int max_spacings, std::vector<double> &tab, int *n_t,
                             int *n_v) {
  tab.clear();
  double t = 0.0;
  for (int k = 0; k < 4096; k++, t += check_dt) tab.push_back(t);
  const size_t nt = tab.size();
  const double longest = std::max(p.veh_length, p.veh_width) + 1.0;
  for (double dl = vertex_res; dl < longest; dl += vertex_res) {
    tab.push_back(dl);
    if (max_spacings > 0 && tab.size() - nt >= (size_t)max_spacings) return DFTPAV_E_UNSUPPORTED; // an outline of that many points and more
  }
  if (tab.size() == nt) tab.push_back(vertex_res);
  *n_t = (int)nt;
  *n_v = (int)(tab.size() - nt);
  return DFTPAV_OK;
}
// test hook (host only, no device): the tables of the collision re-check as every caller of it gets them, out = sample times [*n_t] |
// spacings [*n_v].  A table beyond out's 8192 doubles (possible without a cap only) is refused with DFTPAV_E_UNSUPPORTED.
extern "C" int dftpav_debug_validation_table(const dftpav_params *p, double check_dt, double vertex_res, int max_spacings, double *out,
                                             int *n_t, int *n_v) {
  if (!p || !out || !n_t || !n_v || !(check_dt > 0.0) || !(vertex_res > 0.0) || max_spacings < 0) return DFTPAV_E_INVALID;
  std::vector<double> tab;
  if (int rc = validation_table(*p, check_dt, vertex_res, max_spacings, tab, n_t, n_v)) return rc;
  if (tab.size() > 8192) return DFTPAV_E_UNSUPPORTED;
  std::memcpy(out, tab.data(), sizeof(double) * tab.size());
  return DFTPAV_OK;
}

int dftpav::validate_on_stream(dftpav_batch *b, int n_traj, const double *d_tab, int n_t, int n_v, double check_dt, int *d_col, int *d_first) {
  dftpav_handle *h = b->h;
  const ValidateArgs A{dev_grid(h), dev_footprint(h, d_tab + n_t, n_v), SampleTable{d_tab, n_t, check_dt}, b->d_coef, b->d_dt, b->L, n_traj,
                       d_col, d_first};
  HIPCHK(h, launch_validate(A, h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_validate(dftpav_batch *b, double sample_dt, double vertex_res, int *collision, int *first_sample) {
  if (!b || !b->uploaded || !b->solved || !(sample_dt > 0.0) || !(vertex_res > 0.0)) return DFTPAV_E_INVALID; // nothing solved yet
  dftpav_handle *h = b->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  std::vector<double> tab;
  int n_t = 0, n_v = 0;
  if (int rc = validation_table(h->params, sample_dt, vertex_res, 0, tab, &n_t, &n_v)) return rc;
  const size_t B = (size_t)b->B;
  double *d_tab = nullptr;
  int *d_col = nullptr, *d_first = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_tab, tab.size()));
  HIPCHK(h, tmp.alloc(d_col, B));
  HIPCHK(h, tmp.alloc(d_first, B));
  h->cor_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->cor_ev.record(0, h->stream));
  if (int rc = validate_on_stream(b, b->B, d_tab, n_t, n_v, sample_dt, d_col, d_first)) return rc;
  HIPCHK(h, h->cor_ev.record(1, h->stream));
  HIPCHK(h, fetch_async(h, collision, d_col, sizeof(int) * B));
  HIPCHK(h, fetch_async(h, first_sample, d_first, sizeof(int) * B));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cor_ev.complete();
  return DFTPAV_OK;
}

// ------------------------------------------------- solved plans against the kinematic limits (limits.hip)
extern "C" void dftpav_default_limits(const dftpav_params *p, dftpav_limits *l) {
  // minco_config.pb.txt:83-85 (forward), :87-89 (backward), :91 (max_latacc); the reference has no steer limit of its own
  l->max_forward_vel = p->max_forward_vel;
  l->max_backward_vel = p->max_backward_vel;
  l->max_forward_acc = p->max_forward_acc;
  l->max_backward_acc = p->max_backward_acc;
  l->max_forward_cur = p->max_forward_cur;
  l->max_backward_cur = p->max_backward_cur;
  l->max_latacc = p->max_latacc;
  l->max_steer = HUGE_VAL;
}

bool dftpav::limits_common(const dftpav_params &p, const dftpav_limits &l, LimitsCommon &C) {
  const double both[kLimQ][2] = {{l.max_forward_vel, l.max_backward_vel}, {l.max_forward_acc, l.max_backward_acc}, {l.max_latacc, l.max_latacc},
                                 {l.max_forward_cur, l.max_backward_cur}, {l.max_steer, l.max_steer}};
  for (int q = 0; q < kLimQ; q++)
    for (int d = 0; d < 2; d++) {
      if (!(both[q][d] > 0.0)) return false;
      C.lim[q][d] = both[q][d];
    }
  C.wheel_base = p.veh_wheel_base;
  return true;
}

int dftpav::fetch_limits(dftpav_handle *h, const dftpav_limits_out *out, const LimitsCommon &C, size_t n) {
  HIPCHK(h, fetch_async(h, out->max_abs, C.max_abs, sizeof(double) * kLimQ * n));
  HIPCHK(h, fetch_async(h, out->arg, C.arg, sizeof(int) * kLimQ * n));
  HIPCHK(h, fetch_async(h, out->violated, C.violated, sizeof(int) * kLimQ * n));
  HIPCHK(h, fetch_async(h, out->feasible, C.feasible, sizeof(int) * n));
  return DFTPAV_OK;
}

int dftpav::check_limits_rows(dftpav_handle *h, double check_dt, size_t n, const dftpav_limits_out *out, LimitsCommon C,
                              const std::function<hipError_t(const LimitsCommon &)> &launch) {
  std::vector<double> tab;
  int n_t = 0, n_v = 0;
  if (int rc = validation_table(h->params, check_dt, 1.0, 0, tab, &n_t, &n_v)) return rc; // (the sample times are its first n_t entries)
  double *d_tab = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_tab, (size_t)n_t));
  double *d_max = nullptr;
  int *d_int = nullptr; // arg | violated | feasible
  HIPCHK(h, tmp.alloc(d_max, kLimQ * n));
  HIPCHK(h, tmp.alloc(d_int, (2 * kLimQ + 1) * n));
  limit_rows(C, d_max, d_int, n);
  C.tab = SampleTable{d_tab, n_t, check_dt};
  h->lim_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * (size_t)n_t, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->lim_ev.record(0, h->stream));
  HIPCHK(h, launch(C));
  HIPCHK(h, h->lim_ev.record(1, h->stream));
  if (int rc = fetch_limits(h, out, C, n)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->lim_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_check_limits(dftpav_batch *b, double check_dt, const dftpav_limits *l, const dftpav_limits_out *out) {
  if (!b || !l || !out || !b->uploaded || !b->solved || !(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  LimitsCommon C{};
  if (!limits_common(h->params, *l, C)) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  return check_limits_rows(h, check_dt, (size_t)b->B, out, C, [&](const LimitsCommon &done) {
    return launch_limits_batch(LimitsBatchArgs{done, b->d_coef, b->d_dt, b->L, b->B, nullptr, 1, nullptr}, h->stream);
  });
}

extern "C" int dftpav_limits_last_ms(dftpav_handle *h, float *ms) {
  if (!h || !ms || !h->lim_ev.reached()) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->lim_ev.elapsed(ms, 0, 1, false));
  return DFTPAV_OK;
}

// ------------------------------------------------- the distance field of the map, the clearance of solved plans (distfield.hip, clearance.hip)
int dftpav::ensure_dist_field(dftpav_handle *h) {
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (h->map.size_x > kDistMaxSide || h->map.size_y > kDistMaxSide) return DFTPAV_E_UNSUPPORTED;
  if (!h->dist_stale) return DFTPAV_OK;
  const size_t ncell = (size_t)h->map.size_x * h->map.size_y;
  if (h->dist_cells < ncell) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->d_dist) (void)hipFree(h->d_dist);
    h->d_dist = nullptr;
    h->dist_cells = 0;
    HIPCHK(h, hipMalloc(&h->d_dist, sizeof(int) * 2 * ncell));
    h->dist_cells = ncell;
  }
  const DistFieldArgs A{h->d_cells, h->map.size_x, h->map.size_y, h->d_dist + h->dist_cells, h->d_dist};
  h->field_ev.reset();
  HIPCHK(h, h->field_ev.record(0, h->stream));
  HIPCHK(h, launch_dist_field(A, h->stream));
  HIPCHK(h, h->field_ev.record(1, h->stream));
  h->field_ev.complete();
  h->dist_stale = false;
  return DFTPAV_OK;
}

extern "C" int dftpav_grid_distance_field(dftpav_handle *h, int *d2) {
  if (!h) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = ensure_dist_field(h)) return rc;
  HIPCHK(h, fetch_async(h, d2, h->d_dist, sizeof(int) * (size_t)h->map.size_x * h->map.size_y));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

ClearanceCommon dftpav::clearance_common(const dftpav_handle *h, const double *d_tab, int n_t, int n_v, double check_dt) {
  ClearanceCommon C{};
  C.grid = dev_grid(h);
  C.d2 = h->d_dist;
  C.fp = dev_footprint(h, d_tab + n_t, n_v);
  C.tab = SampleTable{d_tab, n_t, check_dt};
  return C;
}

int dftpav::fetch_clearance(dftpav_handle *h, const dftpav_clearance_out *out, const int *d_d2, const int *d_arg, const double *d_m, size_t n) {
  HIPCHK(h, fetch_async(h, out->min_d2, d_d2, sizeof(int) * n));
  HIPCHK(h, fetch_async(h, out->arg, d_arg, sizeof(int) * n));
  HIPCHK(h, fetch_async(h, out->clearance, d_m, sizeof(double) * n));
  return DFTPAV_OK;
}

int dftpav::check_clearance_rows(dftpav_handle *h, double check_dt, size_t n, const dftpav_clearance_out *out,
                                 const std::function<hipError_t(const ClearanceCommon &)> &launch) {
  if (int rc = ensure_dist_field(h)) return rc;
  std::vector<double> tab;
  int n_t = 0, n_v = 0;
  if (int rc = validation_table(h->params, check_dt, kClearanceVertexRes, 0, tab, &n_t, &n_v)) return rc;
  double *d_tab = nullptr, *d_m = nullptr;
  int *d_int = nullptr; // min_d2 | arg
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_tab, tab.size()));
  HIPCHK(h, tmp.alloc(d_m, n));
  HIPCHK(h, tmp.alloc(d_int, 2 * n));
  ClearanceCommon C = clearance_common(h, d_tab, n_t, n_v, check_dt);
  C.min_d2 = d_int;
  C.arg = d_int + n;
  C.clearance = d_m;
  h->clr_ev.reset(); // until the whole chain has run
  HIPCHK(h, hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, h->clr_ev.record(0, h->stream));
  HIPCHK(h, launch(C));
  HIPCHK(h, h->clr_ev.record(1, h->stream));
  if (int rc = fetch_clearance(h, out, C.min_d2, C.arg, C.clearance, n)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->clr_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_check_clearance(dftpav_batch *b, double check_dt, const dftpav_clearance_out *out) {
  if (!b || !out || !b->uploaded || !b->solved || !(check_dt > 0.0) || !std::isfinite(check_dt)) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  return check_clearance_rows(h, check_dt, (size_t)b->B, out, [&](const ClearanceCommon &C) {
    return launch_clearance_batch(ClearanceBatchArgs{C, b->d_coef, b->d_dt, b->L, b->B, nullptr, 1, nullptr, 0.0}, h->stream);
  });
}

extern "C" int dftpav_clearance_last_ms(dftpav_handle *h, float *field_ms, float *check_ms) {
  if (!h) return DFTPAV_E_INVALID;
  if (field_ms) *field_ms = 0.0f;
  if (check_ms) *check_ms = 0.0f;
  HIPCHK(h, hipSetDevice(h->device));
  if (field_ms && h->field_ev.reached()) HIPCHK(h, h->field_ev.elapsed(field_ms, 0, 1, true)); // (a build alone waits for nothing)
  if (check_ms && h->clr_ev.reached()) HIPCHK(h, h->clr_ev.elapsed(check_ms, 0, 1, false));
  return DFTPAV_OK;
}

// ------------------------------------------------- vehicle footprints stamped into the map (stamp.hip)
int dftpav::stamp_boxes_on_stream(dftpav_handle *h, const double *cx, const double *cy, const double *cs, const double *sn, int n_boxes,
                                  const unsigned char *d_select, int S_pad, double inflate) {
  const size_t ncell = (size_t)h->map.size_x * h->map.size_y;
  if (!h->d_cells_base) { // the first stamp of this map: what was uploaded is kept aside
    HIPCHK(h, hipMalloc(&h->d_cells_base, ncell));
    HIPCHK(h, hipMemcpyAsync(h->d_cells_base, h->d_cells, ncell, hipMemcpyDeviceToDevice, h->stream));
  }
  StampBoxArgs A{};
  A.cells = h->d_cells;
  A.bits = h->d_bits;
  A.size_x = h->map.size_x;
  A.size_y = h->map.size_y;
  A.resolution = h->map.resolution;
  A.origin_x = h->map.origin_x;
  A.origin_y = h->map.origin_y;
  A.cx = cx;
  A.cy = cy;
  A.cs = cs;
  A.sn = sn;
  A.n_boxes = n_boxes;
  A.select = d_select;
  A.S_pad = S_pad;
  A.hl = 0.5 * h->params.veh_length + inflate;
  A.hw = 0.5 * h->params.veh_width + inflate;
  h->dist_stale = true;
  HIPCHK(h, h->stamp_ev.record(1, h->stream));
  HIPCHK(h, launch_stamp_boxes(A, h->stream));
  HIPCHK(h, h->stamp_ev.record(2, h->stream));
  h->stamp_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_grid_stamp_poses(dftpav_handle *h, const double *poses, int n, double inflate) {
  if (!h || !poses || n < 0 || !(inflate >= 0.0) || !std::isfinite(inflate)) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (n == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> soa(4 * (size_t)n); // cx | cy | cs | sn, as the kernel reads the slot form's
  for (size_t i = 0; i < (size_t)n; i++)
    for (size_t c = 0; c < 4; c++) soa[c * n + i] = poses[4 * i + c];
  double *d = nullptr;
  DevScratch tmp(h); // (the call takes its boxes from the host: it ends with a wait, behind which the buffer goes)
  HIPCHK(h, tmp.alloc(d, soa.size()));
  HIPCHK(h, hipMemcpyAsync(d, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, h->stream));
  h->stamp_ev.reset();
  h->stamp_posed = false;
  return stamp_boxes_on_stream(h, d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, nullptr, 0, inflate);
}

extern "C" int dftpav_grid_clear_stamps(dftpav_handle *h) {
  if (!h || !h->d_cells) return DFTPAV_E_INVALID; // no map
  if (!h->d_cells_base) return DFTPAV_OK;         // nothing was stamped into this map
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ncell = (size_t)h->map.size_x * h->map.size_y;
  HIPCHK(h, hipMemcpyAsync(h->d_cells, h->d_cells_base, ncell, hipMemcpyDeviceToDevice, h->stream));
  if (h->d_bits) HIPCHK(h, launch_stamp_bits(StampBitsArgs{h->d_cells, h->d_bits, ncell}, h->stream));
  h->dist_stale = true;
  return DFTPAV_OK;
}

extern "C" int dftpav_grid_read_cells(dftpav_handle *h, unsigned char *cells, int *n_stamped) {
  if (!h || !h->d_cells) return DFTPAV_E_INVALID; // no map
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ncell = (size_t)h->map.size_x * h->map.size_y;
  std::vector<unsigned> partial; // (in front of tmp: it outlives the wait of tmp's destructor)
  DevScratch tmp(h);
  if (n_stamped && h->d_cells_base) {
    unsigned *d_partial = nullptr;
    partial.resize((size_t)stamp_count_blocks(ncell));
    HIPCHK(h, tmp.alloc(d_partial, partial.size()));
    HIPCHK(h, launch_stamp_count(StampCountArgs{h->d_cells, h->d_cells_base, ncell, d_partial}, h->stream));
    HIPCHK(h, hipMemcpyAsync(partial.data(), d_partial, sizeof(unsigned) * partial.size(), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, fetch_async(h, cells, h->d_cells, ncell));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (n_stamped) {
    unsigned n = 0;
    for (unsigned v : partial) n += v; // in the order of the workgroups
    *n_stamped = (int)n;
  }
  return DFTPAV_OK;
}

extern "C" int dftpav_stamp_last_ms(dftpav_handle *h, float *pose_ms, float *stamp_ms) {
  if (!h) return DFTPAV_E_INVALID;
  if (pose_ms) *pose_ms = 0.0f;
  if (stamp_ms) *stamp_ms = 0.0f;
  if (!h->stamp_ev.reached()) return DFTPAV_OK; // nothing was stamped yet
  HIPCHK(h, hipSetDevice(h->device));
  if (pose_ms && h->stamp_posed) HIPCHK(h, h->stamp_ev.elapsed(pose_ms, 0, 1, true)); // (a stamp waits for nothing)
  if (stamp_ms) HIPCHK(h, h->stamp_ev.elapsed(stamp_ms, 1, 2, true));
  return DFTPAV_OK;
}

// ------------------------------------------------- the map rendered from the arena's obstacle set (render.hip)
extern "C" int dftpav_grid_origin_centred(double ego_x, double ego_y, double extent_x, double extent_y, double out[2]) {
  if (!out || !std::isfinite(ego_x) || !std::isfinite(ego_y) || !std::isfinite(extent_x) || !std::isfinite(extent_y)) return DFTPAV_E_INVALID;
  out[0] = std::round(ego_x - extent_x / 2.0); // data_renderer.cc:156-160
  out[1] = std::round(ego_y - extent_y / 2.0);
  return DFTPAV_OK;
}

// the cell coordinate of a world coordinate: rint((p - origin) / resolution), halves to even; false beyond +-2^30 and for a NaN
static bool render_snap(double p, double origin, double resolution, int &out) {
  const double c = std::nearbyint((p - origin) / resolution);
  if (!(std::fabs(c) <= 1073741824.0)) return false;
  out = (int)c;
  return true;
}

extern "C" int dftpav_grid_render(dftpav_handle *h, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                                  unsigned char background, const dftpav_obstacle_set *obs) {
  if (!h || size_x <= 0 || size_y <= 0 || !(resolution > 0.0) || !std::isfinite(resolution) || !std::isfinite(origin_x) ||
      !std::isfinite(origin_y))
    return DFTPAV_E_INVALID;
  static const dftpav_obstacle_set none{};
  const dftpav_obstacle_set &O = obs ? *obs : none;
  if (O.n_poly < 0 || O.n_circle < 0 || O.n_point < 0) return DFTPAV_E_INVALID;
  if ((O.n_poly > 0 && !O.poly_off) || (O.n_circle > 0 && !O.circles) || (O.n_point > 0 && !O.points)) return DFTPAV_E_INVALID;
  // everything is checked and snapped before the handle changes: poly_off | boxes | edges | circles | points, as the kernels read them
  int n_vert = 0;
  if (O.n_poly > 0) {
    if (O.poly_off[0] != 0) return DFTPAV_E_INVALID;
    for (int p = 0; p < O.n_poly; p++) {
      const long long nv = (long long)O.poly_off[p + 1] - O.poly_off[p];
      if (nv < 0 || nv > DFTPAV_RENDER_MAX_VERTS) return DFTPAV_E_INVALID;
    }
    n_vert = O.poly_off[O.n_poly];
    if (n_vert > 0 && !O.poly_xy) return DFTPAV_E_INVALID;
  }
  std::vector<int> snapped((size_t)n_vert * 2);
  for (size_t i = 0; i < snapped.size(); i++) {
    if (!std::isfinite(O.poly_xy[i])) return DFTPAV_E_INVALID;
    if (!render_snap(O.poly_xy[i], i & 1 ? origin_y : origin_x, resolution, snapped[i])) return DFTPAV_E_INVALID;
  }
  std::vector<int4> boxes((size_t)O.n_poly), edges((size_t)n_vert), circles((size_t)O.n_circle);
  std::vector<int2> points((size_t)O.n_point);
  long long poly_rows = 0, circle_rows = 0; // the most rows of the grid that one polygon / circle spans
  const auto rows_inside = [&](long long lo, long long hi) { return std::min<long long>(hi, size_y - 1) - std::max<long long>(lo, 0) + 1; };
  for (int p = 0; p < O.n_poly; p++) {
    const int first = O.poly_off[p], nv = O.poly_off[p + 1] - first;
    int4 box = make_int4(INT_MAX, INT_MIN, INT_MAX, INT_MIN);
    for (int v = 0; v < nv; v++) {
      const int *a = &snapped[2 * (size_t)(first + v)], *b = &snapped[2 * (size_t)(first + (v + 1) % nv)];
      edges[(size_t)first + v] = make_int4(a[0], a[1], b[0], b[1]);
      box = make_int4(std::min(box.x, a[0]), std::max(box.y, a[0]), std::min(box.z, a[1]), std::max(box.w, a[1]));
    }
    boxes[p] = box;
    if (nv > 0) poly_rows = std::max(poly_rows, rows_inside(box.z, box.w));
  }
  for (int c = 0; c < O.n_circle; c++) {
    const double *q = O.circles + 3 * (size_t)c;
    int cx = 0, cy = 0;
    if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) || q[2] < 0.0) return DFTPAV_E_INVALID;
    if (!render_snap(q[0], origin_x, resolution, cx) || !render_snap(q[1], origin_y, resolution, cy)) return DFTPAV_E_INVALID;
    const double r = q[2] / resolution; // data_renderer.cc:178: truncated
    if (!(r <= 1073741824.0)) return DFTPAV_E_INVALID;
    circles[c] = make_int4(cx, cy, (int)r, 0);
    circle_rows = std::max(circle_rows, rows_inside((long long)cy - (int)r, (long long)cy + (int)r));
  }
  for (int i = 0; i < O.n_point; i++) {
    const double *q = O.points + 2 * (size_t)i;
    if (!std::isfinite(q[0]) || !std::isfinite(q[1])) return DFTPAV_E_INVALID;
    if (!render_snap(q[0], origin_x, resolution, points[i].x) || !render_snap(q[1], origin_y, resolution, points[i].y)) return DFTPAV_E_INVALID;
  }
  const auto chunks = [](long long rows) { return (int)std::min<long long>(kRenderMaxChunks, std::max<long long>(1, (rows + 3) / 4)); };

  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream)); // as dftpav_set_grid_map: what was enqueued read the map that goes
  RenderArgs A{};
  const auto fields = [&](auto take) {
    A.poly_off = (const int *)take(sizeof(int) * ((size_t)O.n_poly + 1));
    A.poly_box = (const int4 *)take(sizeof(int4) * boxes.size());
    A.edges = (const int4 *)take(sizeof(int4) * edges.size());
    A.circles = (const int4 *)take(sizeof(int4) * circles.size());
    A.points = (const int2 *)take(sizeof(int2) * points.size());
  };
  const size_t ws = carve(nullptr, fields);
  if (int rc = grow(h, h->d_render_ws, h->render_ws_bytes, ws)) return rc;
  carve(h->d_render_ws, fields);
  const size_t ncell = (size_t)size_x * (size_t)size_y;
  if (!h->d_cells || (size_t)h->map.size_x * (size_t)h->map.size_y != ncell) { // a map of the same size keeps its allocations
    if (h->d_cells) (void)hipFree(h->d_cells);
    if (h->d_bits) (void)hipFree(h->d_bits);
    h->d_cells = nullptr;
    h->d_bits = nullptr;
    HIPCHK(h, hipMalloc(&h->d_cells, ncell));
    if (ncell <= kBitMapMaxCells) HIPCHK(h, hipMalloc(&h->d_bits, sizeof(unsigned) * ((ncell + 31) / 32)));
  }
  if (h->d_cells_base) (void)hipFree(h->d_cells_base); // a new map has no stamps
  h->d_cells_base = nullptr;
  if (!h->d_dl || h->map.resolution != resolution) {
    if (h->d_dl) (void)hipFree(h->d_dl);
    h->d_dl = nullptr;
    if (int rc = map_line_table(h, resolution)) return rc;
  }
  h->map = dftpav_grid_map{nullptr, size_x, size_y, resolution, origin_x, origin_y};
  h->dist_stale = true;
  A.cells = h->d_cells;
  A.size_x = size_x;
  A.size_y = size_y;
  A.background = background;
  A.n_poly = O.n_poly;
  A.n_vert = n_vert;
  A.poly_chunks = chunks(poly_rows);
  A.n_circle = O.n_circle;
  A.circle_chunks = chunks(circle_rows);
  A.n_point = O.n_point;
  const auto upload = [&](const void *dst, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync((void *)dst, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
  };
  h->render_ev.reset(); // until the whole chain has run
  HIPCHK(h, upload(A.poly_off, O.poly_off, sizeof(int) * (O.n_poly > 0 ? (size_t)O.n_poly + 1 : 0)));
  HIPCHK(h, upload(A.poly_box, boxes.data(), sizeof(int4) * boxes.size()));
  HIPCHK(h, upload(A.edges, edges.data(), sizeof(int4) * edges.size()));
  HIPCHK(h, upload(A.circles, circles.data(), sizeof(int4) * circles.size()));
  HIPCHK(h, upload(A.points, points.data(), sizeof(int2) * points.size()));
  HIPCHK(h, h->render_ev.record(0, h->stream));
  HIPCHK(h, launch_render(A, h->stream));
  if (h->d_bits) HIPCHK(h, launch_stamp_bits(StampBitsArgs{h->d_cells, h->d_bits, ncell}, h->stream));
  HIPCHK(h, h->render_ev.record(1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream)); // the sources of the copies are this call's
  h->render_ev.complete();
  return DFTPAV_OK;
}

extern "C" int dftpav_render_last_ms(dftpav_handle *h, float *ms) {
  if (!h || !ms || !h->render_ev.reached()) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->render_ev.elapsed(ms, 0, 1, false));
  return DFTPAV_OK;
}

extern "C" int dftpav_batch_sample_states(dftpav_batch *b, double t0, double sample_dt, int n_samples, int filter_singularity,
                                          double *states, int *n_valid) {
  if (!b || !b->uploaded || !b->solved || !(sample_dt > 0.0) || n_samples <= 0 || !states) return DFTPAV_E_INVALID;
  dftpav_handle *h = b->h;
  HIPCHK(h, hipSetDevice(h->device));
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  const size_t nst = (size_t)b->B * (size_t)n_samples * 8;
  double *d_states = nullptr;
  int *d_valid = nullptr;
  DevScratch tmp(h);
  HIPCHK(h, tmp.alloc(d_states, nst));
  HIPCHK(h, tmp.alloc(d_valid, (size_t)b->B));
  h->cor_ev.reset(); // until the whole chain has run
  HIPCHK(h, h->cor_ev.record(0, h->stream));
  HIPCHK(h, launch_states(b->d_coef, b->d_dt, b->L, b->B, h->params.veh_wheel_base, t0, sample_dt, n_samples, filter_singularity != 0,
                          d_states, d_valid, h->stream));
  HIPCHK(h, h->cor_ev.record(1, h->stream));
  HIPCHK(h, hipMemcpyAsync(states, d_states, sizeof(double) * nst, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, fetch_async(h, n_valid, d_valid, sizeof(int) * (size_t)b->B));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cor_ev.complete();
  return DFTPAV_OK;
}

// ------------------------------------------------- one planning cycle, stream-ordered
// TrajPlanner::RunMINCOParking from getRectangleConst on (traj_manager.cpp:551-626) and the consumers of its result
// (CheckReplan's collision re-check, traj_server_ros.cpp:385-397; the state playback, :244-259,335-356) as ONE enqueue:
// upload of the boundary states / waypoints / durations, then on the handle's stream and without the host in between
//   constraint-point poses -> rectangles of every hypothesis (corridor.hip) -> solve (solver.hip) -> coefficients of the
//   solutions -> collision re-check (validate.hip) -> state read-out (states.hip).
// dftpav_plan_cycle returns when everything is enqueued; dftpav_plan_cycle_fetch waits and copies the results out.

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
  if (int rc = grow(h, pc.d_poses, pc.n_poses, 3 * n_poses)) return rc;
  HIPCHK(h, hipMemcpyAsync(pc.d_poses, pc.poses.data(), sizeof(double) * 3 * n_poses, hipMemcpyHostToDevice, h->stream));
  if (int rc = corridor_into_batch(b, pc.d_poses, (int)n_poses, n_restarts)) return rc; // (nothing waits between here and the solve)
  if (int rc = solve_impl(b, nullptr, false)) return rc;
  DevBatch D;
  if (int rc = ensure_coeffs(b, D)) return rc;
  int n_t = 0, n_v = 0;
  if (int rc = validation_table(h->params, check_dt, vertex_res, 0, pc.tab, &n_t, &n_v)) return rc;
  if (int rc = grow(h, pc.d_tab, pc.n_tab, pc.tab.size())) return rc;
  for (int **buf : {&pc.d_col, &pc.d_first, &pc.d_valid}) { // [B] each: a batch's size does not change
    size_t have = *buf ? (size_t)B : 0;
    if (int rc = grow(h, *buf, have, (size_t)B)) return rc;
  }
  if (int rc = grow(h, pc.d_rd, pc.n_rd, (size_t)B * n_samples * 8)) return rc;
  HIPCHK(h, hipMemcpyAsync(pc.d_tab, pc.tab.data(), sizeof(double) * pc.tab.size(), hipMemcpyHostToDevice, h->stream));
  if (int rc = validate_on_stream(b, b->B, pc.d_tab, n_t, n_v, check_dt, pc.d_col, pc.d_first)) return rc;
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

// ------------------------------------------------- the goal fields of the map and the search heuristic on them (goalfield.hip)
// The fields of one turn share the handle's workspace: 2 GiB of fields at most (one field, whatever its size, always fits).  A turn
// is a fixed range of queries, so what it may hold is decided by the call's largest field: the map's cells, or with windows the
// cells of the call's largest window.
static constexpr size_t kGoalFieldCapBytes = (size_t)2 << 30;
static int goal_field_per_turn(int slots, size_t largest_cells) {
  return (int)std::min<size_t>((size_t)slots, std::max<size_t>(1, kGoalFieldCapBytes / (sizeof(int) * std::max<size_t>(1, largest_cells))));
}

// the cell of a point by grid_occupied's rounding (footprint.h), as doubles; false: outside the grid (or NaN)
static bool goal_field_cell(const dftpav_grid_map &m, const double *xy, double &cx, double &cy) {
  cx = std::round((xy[0] - m.origin_x) / m.resolution);
  cy = std::round((xy[1] - m.origin_y) / m.resolution);
  return cx >= 0.0 && cx < (double)m.size_x && cy >= 0.0 && cy < (double)m.size_y;
}

extern "C" int dftpav_goal_window(const dftpav_grid_map *map_geometry, const double *start_xy, const double *goal_xy, double margin, int *win) {
  if (!map_geometry || !start_xy || !goal_xy || !win) return DFTPAV_E_INVALID;
  const dftpav_grid_map &m = *map_geometry;
  if (m.size_x < 1 || m.size_y < 1 || !(m.resolution > 0.0) || !std::isfinite(m.resolution) || !std::isfinite(m.origin_x) ||
      !std::isfinite(m.origin_y) || !(margin >= 0.0) || !std::isfinite(margin))
    return DFTPAV_E_INVALID;
  win[0] = win[1] = win[2] = win[3] = 0;
  double gx, gy, sx, sy;
  if (!goal_field_cell(m, goal_xy, gx, gy)) return 0; // seeds nothing: no window, no field
  (void)goal_field_cell(m, start_xy, sx, sy);          // a start may lie outside the grid: clamped into it
  sx = sx >= 0.0 ? std::min(sx, (double)(m.size_x - 1)) : 0.0;
  sy = sy >= 0.0 ? std::min(sy, (double)(m.size_y - 1)) : 0.0;
  const double md = std::ceil(margin / m.resolution);
  const long long mc = md < 2147483648.0 ? (long long)md : 2147483648ll; // (beyond any grid)
  const long long side[2] = {m.size_x, m.size_y}, tile[2] = {kGfTileX, kGfTileY};
  const long long s[2] = {(long long)sx, (long long)sy}, g[2] = {(long long)gx, (long long)gy};
  for (int k = 0; k < 2; k++) {
    const long long lo = std::max(0ll, std::min(s[k], g[k]) - mc), hi = std::min(side[k] - 1, std::max(s[k], g[k]) + mc);
    const long long c0 = lo / tile[k] * tile[k], c1 = std::min(side[k], (hi / tile[k] + 1) * tile[k]); // out to the field's tiles
    win[k] = (int)c0;
    win[2 + k] = (int)(c1 - c0);
  }
  return 1;
}

int dftpav::goal_field_plan(dftpav_handle *h, const double *start_xy, const double *xy, int stride, int n, int slots, double inflate_radius,
                            double margin, GoalFieldPlan &G) {
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (!(inflate_radius >= 0.0) || !std::isfinite(inflate_radius) || n < 1 || slots < 1) return DFTPAV_E_INVALID;
  const bool windowed = margin >= 0.0;
  if (windowed && (!start_xy || !std::isfinite(margin))) return DFTPAV_E_INVALID;
  if (int rc = ensure_dist_field(h)) return rc;
  const dftpav_grid_map &m = h->map;
  const size_t cells = (size_t)m.size_x * m.size_y;
  const int tiles_x = (m.size_x + kGfTileX - 1) / kGfTileX, tiles_y = (m.size_y + kGfTileY - 1) / kGfTileY;
  const size_t per_field = cells + (size_t)tiles_x * tiles_y;
  G = GoalFieldPlan{};
  G.windowed = windowed;
  // every query's window (windowed), and the largest of them: what a turn is sized by
  std::vector<int> qwin;
  size_t largest = cells;
  if (windowed) {
    qwin.assign(4 * (size_t)n, 0);
    largest = 0;
    for (int q = 0; q < n; q++) {
      int *w = qwin.data() + 4 * (size_t)q;
      if (dftpav_goal_window(&m, start_xy + (size_t)stride * q, xy + (size_t)stride * q, margin, w) < 0) return DFTPAV_E_INVALID;
      largest = std::max(largest, (size_t)w[2] * (size_t)w[3]);
    }
  }
  G.per_turn = goal_field_per_turn(slots, largest);
  // d2 <= T blocks; T stays below DFTPAV_DIST_FAR, what a map without an occupied cell holds everywhere
  const double t = std::floor(inflate_radius * inflate_radius / (m.resolution * m.resolution));
  G.T = t >= 2147483646.0 ? 2147483646 : (int)t;
  // per turn: the distinct goal cells inside the grid (windowed: the distinct pairs of goal cell and window), in the order of their
  // first query
  std::vector<int> &H = h->gf_host;
  H.assign((size_t)n, -1);
  std::vector<int> cell_list;
  G.turn_off.assign(1, 0);
  size_t most = 0, want_ws = 1;
  for (int q0 = 0; q0 < n; q0 += G.per_turn) {
    const size_t base = cell_list.size() / 2;
    size_t used = 0;
    int turn_tiles = 0;
    for (int q = q0; q < std::min(n, q0 + G.per_turn); q++) {
      double cx, cy;
      if (!goal_field_cell(m, xy + (size_t)stride * q, cx, cy)) continue; // seeds nothing: no field
      const int ix = (int)cx, iy = (int)cy;
      const int *w = windowed ? qwin.data() + 4 * (size_t)q : nullptr;
      size_t f = base;
      while (f < cell_list.size() / 2 &&
             (cell_list[2 * f] != ix || cell_list[2 * f + 1] != iy || (w && !std::equal(w, w + 4, G.win.begin() + 4 * f))))
        f++;
      if (f == cell_list.size() / 2) {
        cell_list.push_back(ix);
        cell_list.push_back(iy);
        if (w) {
          G.win.insert(G.win.end(), w, w + 4);
          G.off.push_back((long long)used);
          used += (size_t)w[2] * (size_t)w[3];
          turn_tiles = std::max(turn_tiles, ((w[2] + kGfTileX - 1) / kGfTileX) * ((w[3] + kGfTileY - 1) / kGfTileY));
        }
      }
      H[q] = (int)(f - base);
    }
    G.turn_off.push_back((int)(cell_list.size() / 2));
    const size_t ng = cell_list.size() / 2 - base;
    most = std::max(most, ng);
    if (windowed) {
      G.turn_ints.push_back(used);
      G.turn_tiles.push_back(turn_tiles);
      want_ws = std::max(want_ws, used + ng * (size_t)turn_tiles);
    }
  }
  if (!windowed) want_ws = std::max<size_t>(1, most) * per_field;
  G.n_goals = cell_list.size() / 2;
  H.insert(H.end(), cell_list.begin(), cell_list.end());
  size_t win_at = 0, off_at = 0;
  if (windowed) {
    win_at = H.size();
    H.insert(H.end(), G.win.begin(), G.win.end());
    if (H.size() % 2) H.push_back(0); // the offsets are 64-bit
    off_at = H.size();
    H.resize(H.size() + 2 * G.n_goals);
    if (G.n_goals) std::memcpy(H.data() + off_at, G.off.data(), sizeof(long long) * G.n_goals);
  }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t want_meta = H.size() + G.n_goals + 1;
  if (h->gf_meta_ints < want_meta || h->gf_ints < want_ws) HIPCHK(h, hipStreamSynchronize(h->stream)); // nothing in flight reads what is freed
  if (int rc = grow(h, h->d_gf_meta, h->gf_meta_ints, want_meta)) return rc;
  if (int rc = grow(h, h->d_gf, h->gf_ints, want_ws)) return rc;
  const size_t turns = G.turn_off.size() - 1;
  while (h->gf_ev.size() < turns) h->gf_ev.emplace_back();
  h->gf_timed = 0;
  HIPCHK(h, hipMemcpyAsync(h->d_gf_meta, H.data(), sizeof(int) * H.size(), hipMemcpyHostToDevice, h->stream));
  G.d_field_of = h->d_gf_meta;
  G.d_cells = h->d_gf_meta + n;
  G.d_reached = h->d_gf_meta + H.size();
  if (windowed) {
    G.d_win = h->d_gf_meta + win_at;
    G.d_off = (const long long *)(h->d_gf_meta + off_at);
  }
  return DFTPAV_OK;
}

int dftpav::goal_field_turn(dftpav_handle *h, const GoalFieldPlan &G, int t, SearchArgs *S, int **fields) {
  const dftpav_grid_map &m = h->map;
  const size_t cells = (size_t)m.size_x * m.size_y;
  const int ng = G.turn_off[t + 1] - G.turn_off[t];
  GoalFieldArgs A{};
  A.d2 = h->d_dist;
  A.size_x = m.size_x;
  A.size_y = m.size_y;
  A.T = G.T;
  A.tiles_x = (m.size_x + kGfTileX - 1) / kGfTileX;
  A.tiles_y = (m.size_y + kGfTileY - 1) / kGfTileY;
  A.goal_cell = G.d_cells + 2 * (size_t)G.turn_off[t];
  A.fields = h->d_gf;
  A.dirty = h->d_gf + (size_t)ng * cells;
  A.n_reached = G.d_reached + G.turn_off[t];
  // what the fills cover: the turn's fields, and their dirty maps behind them
  size_t field_ints = (size_t)ng * cells, dirty_ints = (size_t)ng * A.tiles_x * A.tiles_y;
  if (G.windowed) {
    A.window = G.d_win + 4 * (size_t)G.turn_off[t];
    A.offset = G.d_off + G.turn_off[t];
    A.dirty_stride = G.turn_tiles[t];
    A.dirty = h->d_gf + G.turn_ints[t];
    field_ints = G.turn_ints[t];
    dirty_ints = (size_t)ng * G.turn_tiles[t];
  }
  if (ng > 0) {
    HIPCHK(h, h->gf_ev[(size_t)h->gf_timed].record(0, h->stream));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)A.fields, DFTPAV_FIELD_UNREACHED, field_ints, h->stream));
    HIPCHK(h, hipMemsetAsync(A.dirty, 0, sizeof(int) * dirty_ints, h->stream));
    HIPCHK(h, launch_goal_fields(A, ng, h->stream));
    HIPCHK(h, h->gf_ev[(size_t)h->gf_timed].record(1, h->stream));
    h->gf_timed++;
  }
  if (S) {
    S->fields = h->d_gf; // (queries of a turn without a goal inside the grid have field_of -1 and read nothing)
    S->field_of = G.d_field_of;
    S->unit = G.unit;
    S->field_win = A.window; // (null without windows: the whole-map instance)
    S->field_off = A.offset;
  }
  if (fields) *fields = h->d_gf;
  return DFTPAV_OK;
}

int dftpav::search_heuristic_plan(dftpav_handle *h, const double *start_states, const double *end_states, int n, SearchSetup &U,
                                  GoalFieldPlan &G) {
  G = GoalFieldPlan{};
  if (int rc = search_rs_plan(h, U)) return rc; // dftpav_set_search_rs_heuristic; off: nothing
  if (!h->heu.enabled) return DFTPAV_OK;
  if (int rc = goal_field_plan(h, start_states, end_states, 4, n, U.slots, h->heu.inflate_radius, h->heu_margin, G)) return rc;
  G.unit = h->heu.scale * h->map.resolution / 5.0;
  U.slots = G.per_turn;
  return DFTPAV_OK;
}

extern "C" void dftpav_default_goal_field_params(dftpav_goal_field_params *gp) {
  if (!gp) return;
  gp->enabled = 0;
  gp->inflate_radius = 0.0;
  gp->scale = 1.0 / std::sqrt(1.16);
}

extern "C" int dftpav_set_search_heuristic(dftpav_handle *h, const dftpav_goal_field_params *gp) {
  if (!h) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (!gp || !gp->enabled) {
    h->heu.enabled = 0;
    return DFTPAV_OK;
  }
  if (!(gp->inflate_radius >= 0.0) || !std::isfinite(gp->inflate_radius) || !(gp->scale >= 0.0) || !std::isfinite(gp->scale))
    return DFTPAV_E_INVALID;
  if (h->map.size_x > kDistMaxSide || h->map.size_y > kDistMaxSide) return DFTPAV_E_UNSUPPORTED;
  h->heu = *gp;
  h->heu.enabled = 1;
  return DFTPAV_OK;
}

extern "C" int dftpav_grid_goal_field(dftpav_handle *h, const double *goals_xy, int n, double inflate_radius, int *field, int *n_reached) {
  if (!h || n < 0 || (n > 0 && !goals_xy)) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (!(inflate_radius >= 0.0) || !std::isfinite(inflate_radius)) return DFTPAV_E_INVALID;
  if (n == 0) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  GoalFieldPlan G;
  if (int rc = goal_field_plan(h, nullptr, goals_xy, 2, n, n, inflate_radius, -1.0, G)) return rc;
  const size_t cells = (size_t)h->map.size_x * h->map.size_y;
  const std::vector<int> field_of(h->gf_host.begin(), h->gf_host.begin() + n);
  const int turns = (int)G.turn_off.size() - 1;
  for (int t = 0; t < turns; t++) {
    int *F = nullptr;
    if (int rc = goal_field_turn(h, G, t, nullptr, &F)) return rc;
    for (int q = t * G.per_turn; field && q < std::min(n, (t + 1) * G.per_turn); q++) {
      int *dst = field + (size_t)q * cells;
      if (field_of[q] < 0) std::fill(dst, dst + cells, DFTPAV_FIELD_UNREACHED);
      else HIPCHK(h, hipMemcpyAsync(dst, F + (size_t)field_of[q] * cells, sizeof(int) * cells, hipMemcpyDeviceToHost, h->stream));
    }
  }
  std::vector<int> reached(G.n_goals + 1, 0);
  if (n_reached && G.n_goals) HIPCHK(h, hipMemcpyAsync(reached.data(), G.d_reached, sizeof(int) * G.n_goals, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int q = 0; n_reached && q < n; q++) n_reached[q] = field_of[q] < 0 ? 0 : reached[(size_t)G.turn_off[q / G.per_turn] + field_of[q]];
  return DFTPAV_OK;
}

extern "C" int dftpav_set_search_heuristic_window(dftpav_handle *h, double margin) {
  if (!h) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (std::isnan(margin) || margin == HUGE_VAL) return DFTPAV_E_INVALID;
  h->heu_margin = margin < 0.0 ? -1.0 : margin;
  return DFTPAV_OK;
}

extern "C" int dftpav_grid_goal_field_windowed(dftpav_handle *h, const double *starts_xy, const double *goals_xy, int n, double inflate_radius,
                                               double margin, int *windows, long long *offsets, int *field, int *n_reached) {
  if (!h || n < 0 || (n > 0 && (!goals_xy || !starts_xy))) return DFTPAV_E_INVALID;
  if (!h->d_cells) return DFTPAV_E_INVALID; // no map
  if (!(inflate_radius >= 0.0) || !std::isfinite(inflate_radius) || !(margin >= 0.0) || !std::isfinite(margin)) return DFTPAV_E_INVALID;
  if (n == 0) return DFTPAV_OK;
  // the packed layout: query q's rows [WY][WX] start at offsets[q], one after the other in query order
  std::vector<int> win(4 * (size_t)n, 0);
  std::vector<long long> off((size_t)n, 0);
  long long total = 0;
  for (int q = 0; q < n; q++) {
    int *w = win.data() + 4 * (size_t)q;
    if (dftpav_goal_window(&h->map, starts_xy + 2 * (size_t)q, goals_xy + 2 * (size_t)q, margin, w) < 0) return DFTPAV_E_INVALID;
    off[q] = total;
    total += (long long)w[2] * w[3];
  }
  if (windows) std::copy(win.begin(), win.end(), windows);
  if (offsets) std::copy(off.begin(), off.end(), offsets);
  if (!field && !n_reached) return DFTPAV_OK; // the sizes alone: nothing is built
  HIPCHK(h, hipSetDevice(h->device));
  GoalFieldPlan G;
  if (int rc = goal_field_plan(h, starts_xy, goals_xy, 2, n, n, inflate_radius, margin, G)) return rc;
  const std::vector<int> field_of(h->gf_host.begin(), h->gf_host.begin() + n);
  const int turns = (int)G.turn_off.size() - 1;
  for (int t = 0; t < turns; t++) {
    int *F = nullptr;
    if (int rc = goal_field_turn(h, G, t, nullptr, &F)) return rc;
    for (int q = t * G.per_turn; field && q < std::min(n, (t + 1) * G.per_turn); q++) {
      if (field_of[q] < 0) continue; // a window of no cells
      const size_t f = (size_t)G.turn_off[t] + field_of[q], ints = (size_t)win[4 * (size_t)q + 2] * win[4 * (size_t)q + 3];
      HIPCHK(h, hipMemcpyAsync(field + off[q], F + G.off[f], sizeof(int) * ints, hipMemcpyDeviceToHost, h->stream));
    }
  }
  std::vector<int> reached(G.n_goals + 1, 0);
  if (n_reached && G.n_goals) HIPCHK(h, hipMemcpyAsync(reached.data(), G.d_reached, sizeof(int) * G.n_goals, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int q = 0; n_reached && q < n; q++) n_reached[q] = field_of[q] < 0 ? 0 : reached[(size_t)G.turn_off[q / G.per_turn] + field_of[q]];
  return DFTPAV_OK;
}

extern "C" int dftpav_goal_field_last_ms(dftpav_handle *h, float *ms) {
  if (!h || !ms || h->gf_timed < 1) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  float sum = 0.0f;
  for (int k = 0; k < h->gf_timed; k++) {
    float one = 0.0f;
    HIPCHK(h, h->gf_ev[(size_t)k].elapsed(&one, 0, 1, false)); // (every call that builds fields waits for the stream)
    sum += one;
  }
  *ms = sum;
  return DFTPAV_OK;
}

// ------------------------------------------------- the Reeds-Shepp cost-to-go table and the search heuristic on it (rstable.hip)
static constexpr size_t kRsTableCapBytes = (size_t)256 << 20;

int dftpav::rs_geometry(const dftpav_rs_heuristic_params &gp, RsGeometry &g, size_t &entries) {
  if (gp.n_yaw < 1 || !std::isfinite(gp.cell) || !(gp.cell > 0.0) || !std::isfinite(gp.extent) || !(gp.extent >= 0.0) ||
      !std::isfinite(gp.scale) || !(gp.scale >= 0.0))
    return DFTPAV_E_INVALID;
  const double halfd = std::ceil(gp.extent / gp.cell);
  if (!(halfd < 32768.0)) return DFTPAV_E_UNSUPPORTED; // (a side beyond any table of 256 MiB; also keeps n an int)
  g.n_yaw = gp.n_yaw;
  g.half = (int)halfd;
  g.n = 2 * g.half + 1;
  g.cell = gp.cell;
  g.dth = 2.0 * M_PI / (double)gp.n_yaw;
  const double want = (double)g.n_yaw * (double)g.n * (double)g.n;
  if (want * sizeof(double) > (double)kRsTableCapBytes) return DFTPAV_E_UNSUPPORTED;
  entries = (size_t)g.n_yaw * g.n * g.n;
  return DFTPAV_OK;
}

int dftpav::ensure_rs_table(dftpav_handle *h, double rho, const dftpav_rs_heuristic_params &gp, RsGeometry &g) {
  size_t entries = 0;
  if (int rc = rs_geometry(gp, g, entries)) return rc;
  if (h->d_rs && h->rs_n_yaw == gp.n_yaw && h->rs_rho == rho && h->rs_extent == gp.extent && h->rs_cell == gp.cell) return DFTPAV_OK;
  HIPCHK(h, hipSetDevice(h->device));
  h->rs_n_yaw = 0; // nothing valid until the build below is in the stream
  if (h->rs_doubles < entries) HIPCHK(h, hipStreamSynchronize(h->stream)); // nothing in flight reads what is freed
  if (int rc = grow(h, h->d_rs, h->rs_doubles, entries)) return rc;
  RsTableArgs A{};
  A.T = h->d_rs;
  A.entries = (long long)entries;
  A.g = g;
  A.rho = rho;
  HIPCHK(h, h->rs_ev.record(0, h->stream));
  HIPCHK(h, launch_rs_table(A, h->stream));
  HIPCHK(h, h->rs_ev.record(1, h->stream));
  h->rs_ev.complete(); // (never reset: the read-out goes on answering after a build that failed)
  h->rs_builds++;
  h->rs_rho = rho;
  h->rs_extent = gp.extent;
  h->rs_cell = gp.cell;
  h->rs_n_yaw = gp.n_yaw;
  return DFTPAV_OK;
}

int dftpav::search_rs_plan(dftpav_handle *h, SearchSetup &U) {
  if (!h->rsh.enabled) return DFTPAV_OK;
  RsGeometry g{};
  if (int rc = ensure_rs_table(h, U.S.rho, h->rsh, g)) return rc;
  U.S.rs.tab = h->d_rs;
  U.S.rs.g = g;
  U.S.rs.scale = h->rsh.scale;
  return DFTPAV_OK;
}

extern "C" void dftpav_default_rs_heuristic_params(dftpav_rs_heuristic_params *gp) {
  if (!gp) return;
  gp->enabled = 0;
  gp->n_yaw = 72;
  gp->extent = 15.0; // the radius inside which the search tries the shot (kino_astar.cpp:91)
  gp->cell = 0.25;
  gp->scale = 1.0;
}

extern "C" int dftpav_set_search_rs_heuristic(dftpav_handle *h, const dftpav_rs_heuristic_params *gp) {
  if (!h) return DFTPAV_E_INVALID;
  if (!gp || !gp->enabled) {
    h->rsh.enabled = 0;
    return DFTPAV_OK;
  }
  RsGeometry g{};
  size_t entries = 0;
  if (int rc = rs_geometry(*gp, g, entries)) return rc;
  h->rsh = *gp;
  h->rsh.enabled = 1;
  return DFTPAV_OK;
}

extern "C" int dftpav_rs_table(dftpav_handle *h, double max_cur, const dftpav_rs_heuristic_params *gp, double *out, int *dims) {
  if (!h || !gp || !std::isfinite(max_cur) || !(max_cur > 0.0)) return DFTPAV_E_INVALID;
  RsGeometry g{};
  size_t entries = 0;
  if (int rc = rs_geometry(*gp, g, entries)) return rc;
  if (dims) {
    dims[0] = g.n_yaw;
    dims[1] = g.n;
    dims[2] = g.n;
  }
  if (!out) return DFTPAV_OK;
  if (int rc = ensure_rs_table(h, 1.0 / max_cur, *gp, g)) return rc;
  HIPCHK(h, hipMemcpyAsync(out, h->d_rs, sizeof(double) * entries, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DFTPAV_OK;
}

extern "C" int dftpav_rs_table_last_ms(dftpav_handle *h, float *ms, int *n_builds) {
  if (!h || !ms || !h->rs_ev.reached()) return DFTPAV_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->rs_ev.elapsed(ms, 0, 1, true));
  if (n_builds) *n_builds = h->rs_builds;
  return DFTPAV_OK;
}
