// TEST INFRASTRUCTURE ONLY: CPU restatement of the hybrid A* front end, the checker of dftpav_amd/csrc/search.hip.
//
//   TrajPlanner::getKinoPath (3D search, then 2D)  traj_planner/src/traj_manager.cpp:69-117
//   KinoAstar::search                              traj_planner/src/kino_astar.cpp:37-301
//   KinoAstar::stateTransit                        kino_astar.cpp:21-36
//   KinoAstar::is_shot_sucess / computeShotTraj    kino_astar.cpp:304-345 (ReedsSheppStateSpace: dftpav_amd/csrc/rs_math.h)
//   KinoAstar::retrievePath                        kino_astar.cpp:351-363
//   KinoAstar::init (constants), reset             kino_astar.cpp:372-463
//   KinoAstar::getKinoNode, up to SampleTraj       kino_astar.cpp:554-612
//   KinoAstar::posToIndex / yawToIndex             kino_astar.cpp:804-816
//   PathNode, NodeComparator, NodeHashTable        kino_astar.h:42-126; getSingularity / getHeu kino_astar.h:210-226
//   normalize_angle                                common/src/common/math/calculations.cc:18-23
//   CheckCollisionUsingPosAndYaw                   semantic_map_manager.cc:639-662, shapes.cc:110-149
//
// Written statement by statement from the cited lines, with the real std::priority_queue, std::unordered_map and a pool of
// PathNode pointers: nothing of the kernel's heap (kino_heap.h) or hash table is used by the search here.  The kernel's heap is
// checked against std::priority_queue by heap_selftest below.  The wall-clock budget max_seach_time is the iteration budget
// max_iters, as in the kernel (the one documented deviation).
//
// order 0: libm tan / sin / cos / atan2 / atan, as the reference calls them; order 1: the kernel's correctly rounded
// functions (cr_trig.h) replayed on the host; order 2: correctly rounded from binary128 (libquadmath) -- the kernel's
// results must equal order 2's bit for bit.  Everything else is IEEE fp64 in the reference's order, no contraction.
//
// oracle_kino_search_field is the same search with an optional goal field per query (dftpav_set_search_heuristic; the fields are
// the caller's, from oracle_goalfield/): getHeu's two call sites take fmax(getHeu, (double)F[cell] * unit), the term of
// kino_astar.cpp:247's commented-out getObsHeu line.  Without a field every statement is the one oracle_kino_search runs.
//
// oracle_kino_search_heu is that entry plus an optional Reeds-Shepp cost-to-go table (dftpav_set_search_rs_heuristic; the table is
// the caller's, from oracle_rs_table below): the heuristic becomes the maximum of the above and scale * the table's entry nearest
// the state as seen from the goal (RsTable::slot).  oracle_rs_table fills such a table through rs::Solver<TM<order>>.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <queue>
#include <random>
#include <unordered_map>
#include <vector>

#include "../dftpav_amd/csrc/kino_heap.h"
#include "../dftpav_amd/csrc/rs_math.h"
#include "../include/dftpav_hip.h"
#include "../oracle/step_trig.h"

namespace {

template <int O> struct TM { // the elementary functions of order O, as rs::Solver takes them
  static double sin(double x) { return step_trig::Trig{O}.sin(x); }
  static double cos(double x) { return step_trig::Trig{O}.cos(x); }
  static double tan(double x) { return step_trig::Trig{O}.tan(x); }
  static double atan(double x) { return step_trig::Trig{O}.atan(x); }
  static double atan2(double y, double x) { return step_trig::Trig{O}.atan2(y, x); }
};

const double kPi = 3.14159265358979323846; // M_PI / kPi of calculations.cc
enum { REACH_HORIZON = 1, REACH_END = 2, NO_PATH = 3 };
const char IN_CLOSE_SET = 'a', IN_OPEN_SET = 'b', NOT_EXPAND = 'c';

double normalize_angle(const double &theta) { // calculations.cc:18-23
  double theta_tmp = theta;
  theta_tmp -= (theta >= kPi) * 2 * kPi;
  theta_tmp += (theta < -kPi) * 2 * kPi;
  return theta_tmp;
}

struct PathNode { // kino_astar.h:42-61
  int index[2];
  int yaw_idx;
  double state[3];
  double g_score, f_score;
  double input[2];
  PathNode *parent = nullptr;
  char node_state = NOT_EXPAND;
  int singul = 0;
};
struct NodeComparator { // kino_astar.h:67-73
  bool operator()(PathNode *node1, PathNode *node2) const { return node1->f_score > node2->f_score; }
};
struct Key {
  int a, b, c;
  bool operator==(const Key &o) const { return a == o.a && b == o.b && c == o.c; }
};
struct KeyHash { // matrix_hash, kino_astar.h:75-85 (any hash gives the same finds)
  size_t operator()(const Key &k) const {
    size_t seed = 0;
    for (int e : {k.a, k.b, k.c}) seed ^= std::hash<int>()(e) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
    return seed;
  }
};

// The Reeds-Shepp cost-to-go table: `headings` slices of `side` x `side` poses around a goal at the origin heading along +x.
// Slice a, row b, column c is the pose ((c - reach) * pitch, (b - reach) * pitch, a * turn).
struct RsTable {
  const double *cost = nullptr;
  int headings = 0, reach = 0, side = 0;
  double pitch = 0.0, turn = 0.0, weight = 0.0;
  void shape(int n_yaw, double extent, double cell) {
    headings = n_yaw;
    reach = (int)std::ceil(extent / cell);
    side = reach + reach + 1;
    pitch = cell;
    turn = 2.0 * M_PI / (double)n_yaw;
  }
  // where a pose is filed, seen from a goal whose heading has cosine gc and sine gs: the flat offset, or -1 for a pose the table
  // does not cover (a NaN covers nothing)
  long long slot(const double *pose, const double *goal, double gc, double gs) const {
    const double ex = pose[0] - goal[0], ey = pose[1] - goal[1];
    const double ahead = gc * ex + gs * ey;   // along the goal's heading
    const double aside = gc * ey - gs * ex;   // to its left
    const double col = std::round(ahead / pitch) + (double)reach;
    const double row = std::round(aside / pitch) + (double)reach;
    const bool covered = col >= 0.0 && col < (double)side && row >= 0.0 && row < (double)side;
    if (!covered) return -1;
    const double steps = std::round((pose[2] - goal[2]) / turn);
    if (!(std::fabs(steps) < 9.0e18)) return -1;
    long long a = (long long)steps % (long long)headings;
    if (a < 0) a += headings;
    return (a * side + (long long)row) * side + (long long)col;
  }
};

struct Grid {
  const unsigned char *data;
  int sx, sy;
  double res, ox, oy;
};

template <int O> struct KinoAstar {
  typedef TM<O> M;
  typedef dftpav::rs::Solver<M> RS;
  const dftpav_search_params &P;
  Grid g;
  std::vector<PathNode> storage;
  std::vector<PathNode *> path_node_pool_;
  int use_node_num_ = 0, iter_num_ = 0;
  std::unordered_map<Key, PathNode *, KeyHash> data_2d_, data_3d_;
  std::priority_queue<PathNode *, std::vector<PathNode *>, NodeComparator> open_set_;
  std::vector<PathNode *> path_nodes_;
  double start_state_[4], end_state_[4];
  bool is_shot_succ_ = false;
  bool budget_hit = false;
  double resolution_, inv_yaw_resolution_, origin_[2], map_size_3d_[2], max_steer_, yaw_origin_ = -kPi;
  const int *field_ = nullptr; // the goal field of this query's goal [sy][sx], or none
  double unit_ = 0.0;
  RsTable rs_;                       // the Reeds-Shepp table, or none (cost == nullptr)
  double goal_c_ = 1.0, goal_s_ = 0.0; // cos / sin of the goal's heading, set by search() when there is a table

  KinoAstar(const dftpav_search_params &p, const Grid &grid) : P(p), g(grid) { // init, kino_astar.cpp:372-442
    storage.resize(P.allocate_num);
    for (int i = 0; i < P.allocate_num; i++) path_node_pool_.push_back(&storage[i]);
    map_size_3d_[0] = P.map_size_x;
    map_size_3d_[1] = P.map_size_y;
    resolution_ = P.map_resl;
    origin_[0] = -0.5 * map_size_3d_[0];
    origin_[1] = -0.5 * map_size_3d_[1];
    max_steer_ = M::atan(P.wheel_base * P.max_frontend_cur);
    inv_yaw_resolution_ = 1.0 / P.phi_grid_resolution;
  }
  void reset() { // kino_astar.cpp:445-463
    data_2d_.clear();
    data_3d_.clear();
    path_nodes_.clear();
    std::priority_queue<PathNode *, std::vector<PathNode *>, NodeComparator> empty_queue;
    open_set_.swap(empty_queue);
    for (int i = 0; i < use_node_num_; i++) {
      path_node_pool_[i]->parent = nullptr;
      path_node_pool_[i]->node_state = NOT_EXPAND;
    }
    use_node_num_ = 0;
    iter_num_ = 0;
    is_shot_succ_ = false;
  }
  // map ------------------------------------------------------------------------------------------------------------
  bool occupied(double x, double y) const {
    const double cx = std::round((x - g.ox) / g.res), cy = std::round((y - g.oy) / g.res);
    if (!(cx >= 0.0 && cx < (double)g.sx && cy >= 0.0 && cy < (double)g.sy)) return false; // outside the grid: free
    return g.data[(int)cx + g.sx * (int)cy] == 80;
  }
  bool edge_hits(double ax, double ay, double bx, double by) const { // shapes.cc:128-147: dl = res, res + res, ... < |b - a|
    const double dx = bx - ax, dy = by - ay;
    const double norm = std::sqrt(dx * dx + dy * dy);
    for (double dl = P.vertex_res; dl < norm; dl += P.vertex_res) {
      const double f = dl / norm;
      if (occupied(f * dx + ax, f * dy + ay)) return true;
    }
    return false;
  }
  bool collides(const double *s) const { // CheckIfCollisionUsingPosAndYaw(vp_, s), vp_ with its +0.2 margin
    const double cs = M::cos(s[2]), sn = M::sin(s[2]);
    const double W = P.veh_width, L = P.veh_length;
    const double x = s[0] + P.veh_d_cr * cs, y = s[1] + P.veh_d_cr * sn;
    const double c1x = x + 0.5 * L * cs + 0.5 * W * sn, c1y = y + 0.5 * L * sn - 0.5 * W * cs;
    const double c2x = x + 0.5 * L * cs - 0.5 * W * sn, c2y = y + 0.5 * L * sn + 0.5 * W * cs;
    const double c3x = x - 0.5 * L * cs - 0.5 * W * sn, c3y = y - 0.5 * L * sn + 0.5 * W * cs;
    const double c4x = x - 0.5 * L * cs + 0.5 * W * sn, c4y = y - 0.5 * L * sn - 0.5 * W * cs;
    if (edge_hits(c1x, c1y, c2x, c2y) || edge_hits(c2x, c2y, c3x, c3y) || edge_hits(c3x, c3y, c4x, c4y) || edge_hits(c4x, c4y, c1x, c1y))
      return true;
    return occupied(c1x, c1y) || occupied(c2x, c2y) || occupied(c3x, c3y) || occupied(c4x, c4y);
  }
  // helpers ----------------------------------------------------------------------------------------------------------
  static int getSingularity(double vel) { // kino_astar.h:210-219
    int singul = 0;
    if (std::fabs(vel) > 1e-2) {
      if (vel >= 0.0) singul = 1;
      else singul = -1;
    }
    return singul;
  }
  double getHeu(const double *x1, const double *x2) const { // kino_astar.h:221-226 (abs: the double overload)
    double dx = std::abs(x1[0] - x2[0]);
    double dy = std::abs(x1[1] - x2[1]);
    return P.tie_breaker * std::sqrt(dx * dx + dy * dy);
  }
  // getHeu, and with a goal field the maximum with the field's term: the cell by occupied()'s rounding, 0 outside the grid and
  // where the field did not reach
  double heu(const double *x1, const double *x2) const {
    const double e = getHeu(x1, x2);
    if (rs_.cost) {
      double m = e;
      if (field_) m = std::fmax(m, fieldTerm(x1));
      const long long at = rs_.slot(x1, x2, goal_c_, goal_s_);
      return std::fmax(m, at < 0 ? 0.0 : rs_.weight * rs_.cost[at]);
    }
    if (!field_) return e;
    return std::fmax(e, fieldTerm(x1));
  }
  double fieldTerm(const double *x1) const {
    const double cx = std::round((x1[0] - g.ox) / g.res), cy = std::round((x1[1] - g.oy) / g.res);
    double hobs = 0.0;
    if (cx >= 0.0 && cx < (double)g.sx && cy >= 0.0 && cy < (double)g.sy) {
      const int v = field_[(size_t)(int)cx + (size_t)g.sx * (size_t)(int)cy];
      if (v != 0x7fffffff) hobs = (double)v * unit_;
    }
    return hobs;
  }
  void posToIndex(const double *pt, int *idx) const { // kino_astar.cpp:804-809
    idx[0] = std::round((pt[0] - origin_[0]) / resolution_);
    idx[1] = std::round((pt[1] - origin_[1]) / resolution_);
  }
  int yawToIndex(double yaw) const { // kino_astar.cpp:811-816
    yaw = normalize_angle(yaw);
    int idx = std::floor((yaw - yaw_origin_) * inv_yaw_resolution_);
    return idx;
  }
  void stateTransit(const double *state0, double *state1, const double *ctrl_input) const { // kino_astar.cpp:21-36
    double psi = ctrl_input[0];
    double s = ctrl_input[1];
    if (psi != 0) {
      double k = P.wheel_base / M::tan(psi);
      state1[0] = state0[0] + k * (M::sin(state0[2] + s / k) - M::sin(state0[2]));
      state1[1] = state0[1] - k * (M::cos(state0[2] + s / k) - M::cos(state0[2]));
      state1[2] = state0[2] + s / k;
    } else {
      state1[0] = state0[0] + s * M::cos(state0[2]);
      state1[1] = state0[1] + s * M::sin(state0[2]);
      state1[2] = state0[2];
    }
  }
  PathNode *find(const int *idx, int yaw_idx, bool use3d) {
    auto &m = use3d ? data_3d_ : data_2d_;
    auto it = m.find(Key{idx[0], idx[1], use3d ? yaw_idx : 0});
    return it == m.end() ? nullptr : it->second;
  }
  void insert(const int *idx, int yaw_idx, bool use3d, PathNode *node) {
    (use3d ? data_3d_ : data_2d_).insert(std::make_pair(Key{idx[0], idx[1], use3d ? yaw_idx : 0}, node));
  }
  // the shot ---------------------------------------------------------------------------------------------------------
  void interpolate(const double *from, const double *to, const dftpav::rs::Path &path, double t, double *s) const {
    if (t >= 1.0) { // ReedsSheppStateSpace::interpolate copies the end states
      s[0] = to[0]; s[1] = to[1]; s[2] = to[2];
    } else if (t <= 0.0) {
      s[0] = from[0]; s[1] = from[1]; s[2] = from[2];
    } else {
      RS::interpolate(from, path, 1.0 / P.max_frontend_cur, t, s);
    }
  }
  bool is_shot_sucess(const double *state1, const double *state2) { // kino_astar.cpp:304-345
    const double rho = 1.0 / P.max_frontend_cur;
    const dftpav::rs::Path path = RS::between(state1, state2, rho);
    const double len = rho * path.total; // shotptr->distance
    for (double l = 0.0; l <= len; l += P.checkl) {
      double s[3];
      interpolate(state1, state2, path, l / len, s);
      if (collides(s)) return false;
    }
    is_shot_succ_ = true;
    return true;
  }
  void retrievePath(PathNode *end_node) { // kino_astar.cpp:351-363
    PathNode *cur_node = end_node;
    path_nodes_.push_back(cur_node);
    while (cur_node->parent != nullptr) {
      cur_node = cur_node->parent;
      path_nodes_.push_back(cur_node);
    }
    std::reverse(path_nodes_.begin(), path_nodes_.end());
  }

  int search(const double *start_state, const double *end_state, bool use3d) { // kino_astar.cpp:37-301
    bool initsearch = false;
    budget_hit = false;
    if (collides(start_state)) return NO_PATH; // :43-47
    if (collides(end_state)) return NO_PATH;   // :48-52
    std::memcpy(start_state_, start_state, sizeof start_state_);
    std::memcpy(end_state_, end_state, sizeof end_state_);
    if (rs_.cost) {
      goal_c_ = M::cos(end_state[2]);
      goal_s_ = M::sin(end_state[2]);
    }
    PathNode *cur_node = path_node_pool_[0]; // :59-76
    cur_node->parent = nullptr;
    std::memcpy(cur_node->state, start_state, 3 * sizeof(double));
    posToIndex(start_state, cur_node->index);
    cur_node->yaw_idx = yawToIndex(start_state[2]);
    cur_node->g_score = 0.0;
    cur_node->input[0] = 0.0;
    cur_node->input[1] = 0.0;
    cur_node->singul = getSingularity(start_state[3]);
    cur_node->f_score = P.lambda_heu * heu(cur_node->state, end_state);
    cur_node->node_state = IN_OPEN_SET;
    open_set_.push(cur_node);
    use_node_num_ += 1;
    insert(cur_node->index, yawToIndex(start_state[2]), use3d, cur_node);
    if (cur_node->singul == 0) initsearch = true;
    while (!open_set_.empty()) { // :78
      cur_node = open_set_.top();
      const double ddx = cur_node->state[0] - end_state_[0], ddy = cur_node->state[1] - end_state_[1];
      if (std::sqrt(ddx * ddx + ddy * ddy) < 15.0 && initsearch) is_shot_sucess(cur_node->state, end_state_); // :90-93
      if (is_shot_succ_) { // :97-114
        retrievePath(cur_node);
        return REACH_END;
      }
      if (iter_num_ >= P.max_iters) { // :115-132, the budget in iterations
        budget_hit = true;
        retrievePath(cur_node);
        if (cur_node->parent == nullptr) return NO_PATH;
        return REACH_END;
      }
      open_set_.pop(); // :134-136
      cur_node->node_state = IN_CLOSE_SET;
      iter_num_ += 1;
      double cur_state[3], pro_state[3];
      std::memcpy(cur_state, cur_node->state, sizeof cur_state);
      std::vector<std::array<double, 2>> inputs; // :141-171
      const double res = 0.5;
      if (!initsearch) {
        if (start_state_[3] > 0) {
          for (double arc = resolution_; arc <= 2 * resolution_ + 1e-3; arc += resolution_)
            for (double steer = -max_steer_; steer <= max_steer_ + 1e-3; steer += res * max_steer_ * 1.0) inputs.push_back({steer, arc});
        } else {
          for (double arc = -resolution_; arc >= -2 * resolution_ - 1e-3; arc -= resolution_)
            for (double steer = -max_steer_; steer <= max_steer_ + 1e-3; steer += res * max_steer_ * 1.0) inputs.push_back({steer, arc});
        }
        initsearch = true;
      } else {
        for (double arc = -P.step_arc; arc <= P.step_arc + 1e-3; arc += 0.5 * P.step_arc) {
          if (std::fabs(arc) < 1.0e-2) continue;
          for (double steer = -max_steer_; steer <= max_steer_ + 1e-3; steer += res * max_steer_ * 1.0) inputs.push_back({steer, arc});
        }
      }
      for (auto &input : inputs) { // :173-295
        int singul = input[1] > 0 ? 1 : -1;
        stateTransit(cur_state, pro_state, input.data());
        if (pro_state[0] <= origin_[0] || pro_state[0] >= map_size_3d_[0] * 0.5 || pro_state[1] <= origin_[1] ||
            pro_state[1] >= map_size_3d_[1] * 0.5)
          continue;
        int pro_id[2];
        posToIndex(pro_state, pro_id);
        double pro_yaw_id = yawToIndex(pro_state[2]);
        PathNode *pro_node = find(pro_id, (int)pro_yaw_id, use3d);
        if (pro_node != nullptr && pro_node->node_state == IN_CLOSE_SET) continue;
        const int diff0 = pro_id[0] - cur_node->index[0], diff1 = pro_id[1] - cur_node->index[1];
        int diff_yaw = pro_yaw_id - cur_node->yaw_idx;
        if (diff0 == 0 && diff1 == 0 && ((!use3d) || diff_yaw == 0)) continue;
        double xt[3];
        bool is_occ = false;
        for (int k = 1; k <= P.check_num; ++k) { // :212-224
          double tmparc = input[1] * double(k) / double(P.check_num);
          double tmpctrl[2] = {input[0], tmparc};
          stateTransit(cur_state, xt, tmpctrl);
          is_occ = collides(xt);
          if (is_occ) break;
        }
        if (is_occ) continue;
        double tmp_g_score = 0.0; // :229-246
        double tmp_f_score = 0.0;
        int lastDir = cur_node->singul;
        if (singul > 0) tmp_g_score += std::fabs(input[1]) * P.traj_forward_penalty;
        else tmp_g_score += std::fabs(input[1]) * P.traj_back_penalty;
        if (singul * lastDir < 0) tmp_g_score += P.traj_gear_switch_penalty;
        tmp_g_score += P.traj_steer_penalty * std::fabs(input[0]) * std::fabs(input[1]);
        tmp_g_score += P.traj_steer_change_penalty * std::fabs(input[0] - cur_node->input[0]);
        tmp_g_score += cur_node->g_score;
        tmp_f_score = tmp_g_score + P.lambda_heu * heu(pro_state, end_state);
        if (pro_node == nullptr) { // :252-275
          pro_node = path_node_pool_[use_node_num_];
          pro_node->index[0] = pro_id[0];
          pro_node->index[1] = pro_id[1];
          std::memcpy(pro_node->state, pro_state, sizeof pro_state);
          pro_node->yaw_idx = pro_yaw_id;
          pro_node->f_score = tmp_f_score;
          pro_node->g_score = tmp_g_score;
          pro_node->input[0] = input[0];
          pro_node->input[1] = input[1];
          pro_node->parent = cur_node;
          pro_node->node_state = IN_OPEN_SET;
          pro_node->singul = singul;
          open_set_.push(pro_node);
          insert(pro_id, (int)pro_yaw_id, use3d, pro_node);
          use_node_num_ += 1;
          if (use_node_num_ == P.allocate_num) return NO_PATH; // "run out of memory"
        } else if (pro_node->node_state == IN_OPEN_SET) { // :276-290: in place, no re-heapify
          if (tmp_g_score < pro_node->g_score) {
            pro_node->index[0] = pro_id[0];
            pro_node->index[1] = pro_id[1];
            std::memcpy(pro_node->state, pro_state, sizeof pro_state);
            pro_node->yaw_idx = pro_yaw_id;
            pro_node->f_score = tmp_f_score;
            pro_node->g_score = tmp_g_score;
            pro_node->input[0] = input[0];
            pro_node->input[1] = input[1];
            pro_node->parent = cur_node;
            pro_node->singul = singul;
          }
        }
      }
    }
    return NO_PATH; // "open set empty, no path"
  }

  // getKinoNode up to SampleTraj, kino_astar.cpp:554-612
  std::vector<std::array<double, 3>> sampleTraj() {
    std::vector<std::array<double, 3>> roughSampleList;
    PathNode *node = path_nodes_.back();
    while (node->parent != nullptr) {
      for (int k = P.check_num; k > 0; k--) {
        double state[3];
        double tmparc = node->input[1] * double(k) / double(P.check_num);
        double tmpctrl[2] = {node->input[0], tmparc};
        stateTransit(node->parent->state, state, tmpctrl);
        state[2] = normalize_angle(state[2]);
        roughSampleList.push_back({state[0], state[1], state[2]});
      }
      node = node->parent;
    }
    start_state_[2] = normalize_angle(start_state_[2]);
    roughSampleList.push_back({start_state_[0], start_state_[1], start_state_[2]});
    std::reverse(roughSampleList.begin(), roughSampleList.end());
    if (is_shot_succ_) {
      const double state1[3] = {roughSampleList.back()[0], roughSampleList.back()[1], roughSampleList.back()[2]};
      const double state2[3] = {end_state_[0], end_state_[1], end_state_[2]};
      const double rho = 1.0 / P.max_frontend_cur;
      const dftpav::rs::Path path = RS::between(state1, state2, rho);
      double shotLength = rho * path.total;
      for (double l = P.checkl; l < shotLength; l += P.checkl) {
        double s[3];
        interpolate(state1, state2, path, l / shotLength, s);
        roughSampleList.push_back({s[0], s[1], normalize_angle(s[2])});
      }
      end_state_[2] = normalize_angle(end_state_[2]);
      roughSampleList.push_back({end_state_[0], end_state_[1], end_state_[2]});
    }
    return roughSampleList; // the truncate loop (:603-611) keeps every pose
  }
};

template <int O>
void run_queries(const Grid &g, const dftpav_search_params &P, const double *start, const double *end, int n, int nthreads,
                 const dftpav_search_out &out, const int *fields = nullptr, const int *field_of = nullptr, double unit = 0.0,
                 const RsTable *rs = nullptr) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
  for (int q = 0; q < n; q++) {
    KinoAstar<O> ka(P, g);
    if (fields && field_of && field_of[q] >= 0) {
      ka.field_ = fields + (size_t)field_of[q] * g.sx * g.sy;
      ka.unit_ = unit;
    }
    if (rs && rs->cost) ka.rs_ = *rs;
    const double *st = start + 4 * (size_t)q, *en = end + 4 * (size_t)q;
    // getKinoPath, traj_manager.cpp:79-103
    ka.reset();
    bool use3d = P.use3d != 0;
    int status = ka.search(st, en, use3d);
    if (status == NO_PATH && use3d && P.retry_2d) {
      ka.reset();
      use3d = false;
      status = ka.search(st, en, false);
    }
    out.status[q] = status;
    out.shot_success[q] = ka.is_shot_succ_ ? 1 : 0;
    out.used_3d[q] = use3d ? 1 : 0;
    out.budget_hit[q] = ka.budget_hit ? 1 : 0;
    out.iters[q] = ka.iter_num_;
    out.nodes_used[q] = ka.use_node_num_;
    out.n_nodes[q] = 0;
    out.path_len[q] = 0;
    if (status != REACH_END) continue;
    const int m = (int)ka.path_nodes_.size();
    out.n_nodes[q] = m;
    for (int j = 0; j < m && j < out.max_nodes; j++) {
      const PathNode *nd = ka.path_nodes_[j];
      double *o = out.nodes + ((size_t)q * out.max_nodes + j) * 6;
      o[0] = nd->state[0];
      o[1] = nd->state[1];
      o[2] = nd->state[2];
      o[3] = nd->input[0];
      o[4] = nd->input[1];
      o[5] = (double)nd->singul;
    }
    const std::vector<std::array<double, 3>> traj = ka.sampleTraj();
    out.path_len[q] = (int)traj.size();
    for (int i = 0; i < (int)traj.size() && i < out.max_path; i++)
      for (int d = 0; d < 3; d++) out.paths[((size_t)q * out.max_path + i) * 3 + d] = traj[i][d];
  }
}

} // namespace

extern "C" void oracle_kino_search(const unsigned char *grid, int size_x, int size_y, double resolution, double origin_x,
                                   double origin_y, const dftpav_search_params *sp, const double *start_states,
                                   const double *end_states, int n, int order, int nthreads, const dftpav_search_out *out) {
  const Grid g{grid, size_x, size_y, resolution, origin_x, origin_y};
  if (nthreads < 1) nthreads = 1;
  if (order == 0) run_queries<0>(g, *sp, start_states, end_states, n, nthreads, *out);
  else if (order == 1) run_queries<1>(g, *sp, start_states, end_states, n, nthreads, *out);
  else run_queries<2>(g, *sp, start_states, end_states, n, nthreads, *out);
}

// the same with goal fields: fields [k][size_y][size_x], field_of [n] (the field of query q, -1: none), unit; fields == NULL: none
extern "C" void oracle_kino_search_field(const unsigned char *grid, int size_x, int size_y, double resolution, double origin_x,
                                         double origin_y, const dftpav_search_params *sp, const double *start_states,
                                         const double *end_states, int n, int order, int nthreads, const dftpav_search_out *out,
                                         const int *fields, const int *field_of, double unit) {
  const Grid g{grid, size_x, size_y, resolution, origin_x, origin_y};
  if (nthreads < 1) nthreads = 1;
  if (order == 0) run_queries<0>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit);
  else if (order == 1) run_queries<1>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit);
  else run_queries<2>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit);
}

// the same with, besides, a Reeds-Shepp table rs_tab [n_yaw][n][n] of (extent, cell) weighted by scale; rs_tab == NULL: none
extern "C" void oracle_kino_search_heu(const unsigned char *grid, int size_x, int size_y, double resolution, double origin_x,
                                       double origin_y, const dftpav_search_params *sp, const double *start_states,
                                       const double *end_states, int n, int order, int nthreads, const dftpav_search_out *out,
                                       const int *fields, const int *field_of, double unit, const double *rs_tab, int n_yaw,
                                       double extent, double cell, double scale) {
  const Grid g{grid, size_x, size_y, resolution, origin_x, origin_y};
  if (nthreads < 1) nthreads = 1;
  RsTable rs;
  if (rs_tab) {
    rs.shape(n_yaw, extent, cell);
    rs.cost = rs_tab;
    rs.weight = scale;
  }
  if (order == 0) run_queries<0>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit, &rs);
  else if (order == 1) run_queries<1>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit, &rs);
  else run_queries<2>(g, *sp, start_states, end_states, n, nthreads, *out, fields, field_of, unit, &rs);
}

// the table itself: out [n_yaw][n][n], entry (k, j, i) = rho * the normalised length of the shortest Reeds-Shepp path from
// ((i - half) cell, (j - half) cell, k dth) to the origin heading along +x -- is_shot_sucess's `len` for that pair of poses
template <int O> static void fill_rs_table(double rho, const RsTable &t, double *out) {
  const double goal[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < t.headings; a++)
    for (int b = 0; b < t.side; b++)
      for (int c = 0; c < t.side; c++) {
        const double pose[3] = {(double)(c - t.reach) * t.pitch, (double)(b - t.reach) * t.pitch, (double)a * t.turn};
        out[((size_t)a * t.side + b) * t.side + c] = rho * dftpav::rs::Solver<TM<O>>::between(pose, goal, rho).total;
      }
}
extern "C" void oracle_rs_table(int order, double rho, int n_yaw, double extent, double cell, double *out) {
  RsTable t;
  t.shape(n_yaw, extent, cell);
  if (order == 0) fill_rs_table<0>(rho, t, out);
  else if (order == 1) fill_rs_table<1>(rho, t, out);
  else fill_rs_table<2>(rho, t, out);
}

// RsTable::slot for m poses [m][3] seen from `goal` [3]: the flat offset of each, or -1 (the lookup rule, for its own test)
extern "C" void oracle_rs_slot(int order, int n_yaw, double extent, double cell, const double *goal, const double *poses, int m,
                               long long *slot) {
  RsTable t;
  t.shape(n_yaw, extent, cell);
  const step_trig::Trig tr{order};
  const double gc = tr.cos(goal[2]), gs = tr.sin(goal[2]);
  for (int p = 0; p < m; p++) slot[p] = t.slot(poses + 3 * (size_t)p, goal, gc, gs);
}

// stateTransit of one order, for checking every returned node against its parent and input
extern "C" void oracle_state_transit(int order, double wheel_base, const double *state0, const double *ctrl, double *state1) {
  dftpav_search_params p{};
  p.wheel_base = wheel_base;
  const Grid g{nullptr, 0, 0, 1.0, 0.0, 0.0};
  if (order == 0) KinoAstar<0>(p, g).stateTransit(state0, state1, ctrl);
  else if (order == 1) KinoAstar<1>(p, g).stateTransit(state0, state1, ctrl);
  else KinoAstar<2>(p, g).stateTransit(state0, state1, ctrl);
}

// kino_heap.h beside std::priority_queue<PathNode *, ..., NodeComparator> over n_ops random operations (push, pop and
// in-place key changes of nodes in the queue, keys drawn from a handful of values so that ties are everywhere).  After
// every operation the whole underlying arrays are compared.  Returns -1, or the index of the first operation after which
// they differ.
extern "C" long long heap_selftest(unsigned long long seed, long long n_ops) {
  struct PQ : std::priority_queue<PathNode *, std::vector<PathNode *>, NodeComparator> {
    const std::vector<PathNode *> &vec() const { return c; }
  };
  std::mt19937_64 rng(seed);
  std::vector<PathNode> nodes((size_t)n_ops + 1);
  std::vector<int> h_node(nodes.size()), h_pos(nodes.size());
  std::vector<double> h_key(nodes.size());
  dftpav::KinoHeap heap{h_node.data(), h_key.data(), h_pos.data(), 0};
  PQ pq;
  std::vector<int> in_queue; // node ids in the queue
  std::vector<int> where(nodes.size(), -1);
  int next = 0;
  for (long long op = 0; op < n_ops; op++) {
    const unsigned r = (unsigned)(rng() % 100);
    const double key = (double)(rng() % 8) * 0.5;
    if (r < 45 || pq.empty()) { // push a new node
      PathNode &nd = nodes[next];
      nd.f_score = key;
      pq.push(&nd);
      heap.push(next, key);
      where[next] = (int)in_queue.size();
      in_queue.push_back(next);
      next++;
    } else if (r < 75) { // pop
      PathNode *t = pq.top();
      const int id = (int)(t - nodes.data());
      if (heap.top() != id) return op;
      pq.pop();
      heap.pop();
      const int w = where[id];
      where[in_queue.back()] = w;
      in_queue[w] = in_queue.back();
      in_queue.pop_back();
      where[id] = -1;
    } else { // change the key of a queued node in place (kino_astar.cpp:284)
      const int id = in_queue[rng() % in_queue.size()];
      nodes[id].f_score = key;
      heap.set_key(id, key);
    }
    const std::vector<PathNode *> &v = pq.vec();
    if ((int)v.size() != heap.size) return op;
    for (size_t i = 0; i < v.size(); i++)
      if ((int)(v[i] - nodes.data()) != h_node[i] || v[i]->f_score != h_key[i] || h_pos[h_node[i]] != (int)i) return op;
  }
  return -1;
}
