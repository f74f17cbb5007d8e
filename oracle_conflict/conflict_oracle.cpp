// TEST INFRASTRUCTURE ONLY: CPU yardstick of the conflict check between executing plans (dftpav_planner_check_conflicts,
// dftpav_planner_sample_poses; dftpav_amd/csrc/conflict.hip).  It shares no header with the kernels (oracle/step_trig.h brings the
// trigonometry by order), and is written from the definition in include/dftpav_hip.h.
//
// The pose.  The reference's objects -- Piece, Trajectory (getPos, getAngle), the container of chained segments with its times -- are
// oracle_shared/ref_objects.h's, cited there.  The segment of a clock is exe_traj_index_ as TrajPlannerServer::PublishData steps it
// (traj_planner/src/traj_server_ros.cpp:248-252), derived from the clock alone; outside its plan the vehicle is held at the plan's
// first or last pose.  The box is the one CheckCollisionUsingPosAndYaw builds (semantic_map_manager.cc:645-646, shapes.cc:110-149).
// order 0: the host's libm, as the reference calls it; order 2: correctly rounded from binary128 -- the yardstick of the kernels.
//
// The pairs.  A plain triple loop over (i, j, k); every minimum is taken by an explicit lexicographic comparison.  Nothing is
// tiled, staged, masked or reduced.
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "../oracle_shared/ref_objects.h"

namespace {

using namespace ref_objects;

const double INF = std::numeric_limits<double>::infinity();
const double QNAN = std::numeric_limits<double>::quiet_NaN();

struct Box { // the oriented box of a pose: centre, the heading's cosine and sine, the four corners
  Vec2 c;
  double cs, sn;
  Vec2 corner[4];
};

Box make_box(double cx, double cy, double cos_theta, double sin_theta, const Vehicle &vp) {
  Box b;
  b.c = Vec2{cx, cy};
  b.cs = cos_theta;
  b.sn = sin_theta;
  const double x = cx, y = cy, L = vp.length, W = vp.width;
  b.corner[0] = Vec2{x + 0.5 * L * cos_theta + 0.5 * W * sin_theta, y + 0.5 * L * sin_theta - 0.5 * W * cos_theta};
  b.corner[1] = Vec2{x + 0.5 * L * cos_theta - 0.5 * W * sin_theta, y + 0.5 * L * sin_theta + 0.5 * W * cos_theta};
  b.corner[2] = Vec2{x - 0.5 * L * cos_theta - 0.5 * W * sin_theta, y - 0.5 * L * sin_theta + 0.5 * W * cos_theta};
  b.corner[3] = Vec2{x - 0.5 * L * cos_theta + 0.5 * W * sin_theta, y - 0.5 * L * sin_theta - 0.5 * W * cos_theta};
  return b;
}

// step 2, one owner: do its x or y axis separate it from `other`?
bool owner_separates(const Box &own, const Box &other, const Vehicle &vp) {
  int above_x = 0, below_x = 0, above_y = 0, below_y = 0;
  for (int q = 0; q < 4; q++) {
    const double px = other.corner[q].x, py = other.corner[q].y;
    const double lx = own.cs * (px - own.c.x) + own.sn * (py - own.c.y);
    const double ly = own.cs * (py - own.c.y) - own.sn * (px - own.c.x);
    if (lx > vp.length / 2) above_x++;
    if (lx < -vp.length / 2) below_x++;
    if (ly > vp.width / 2) above_y++;
    if (ly < -vp.width / 2) below_y++;
  }
  return above_x == 4 || below_x == 4 || above_y == 4 || below_y == 4;
}

// step 3, one point against one segment
double point_segment_d2(Vec2 p, Vec2 a, Vec2 b) {
  double u = ((p.x - a.x) * (b.x - a.x) + (p.y - a.y) * (b.y - a.y)) / ((b.x - a.x) * (b.x - a.x) + (b.y - a.y) * (b.y - a.y));
  if (!(u > 0.0)) u = 0.0;
  else if (u > 1.0) u = 1.0;
  const Vec2 q{a.x + u * (b.x - a.x), a.y + u * (b.y - a.y)};
  const double ex = p.x - q.x, ey = p.y - q.y;
  return ex * ex + ey * ey;
}

double separation(const Box &A, const Box &B, const Vehicle &vp) {
  if (!owner_separates(A, B, vp) && !owner_separates(B, A, vp)) return 0.0;
  double m = INF;
  for (int side = 0; side < 2; side++) {
    const Box &P = side == 0 ? A : B, &E = side == 0 ? B : A;
    for (int q = 0; q < 4; q++)
      for (int e = 0; e < 4; e++) {
        const double d = point_segment_d2(P.corner[q], E.corner[e], E.corner[(e + 1) % 4]);
        if (d < m) m = d;
      }
  }
  return std::sqrt(m);
}

struct Pose {
  bool occupied;
  double cx, cy, cs, sn;
};

// the pose of one row of the table at clock t
Pose pose_at(const std::vector<LocalTrajData> &executing_traj_, double t, const Vehicle &vp, const Trig &T) {
  Pose r{false, QNAN, QNAN, QNAN, QNAN};
  const int n_seg = (int)executing_traj_.size();
  if (n_seg == 0) return r;
  int e = n_seg - 1;
  for (int i = 0; i < n_seg; i++)
    if (!(executing_traj_.at(i).end_time <= t)) {
      e = i;
      break;
    }
  const LocalTrajData &d = executing_traj_.at(e);
  double tt = t - d.start_time;
  if (tt < 0) tt = 0;
  if (tt > d.duration) tt = d.duration;
  const Vec2 pos = d.traj.getPos(tt);
  const double yaw = d.traj.getAngle(tt, T);
  const double cos_theta = T.cos(yaw), sin_theta = T.sin(yaw);
  r.occupied = true;
  r.cs = cos_theta;
  r.sn = sin_theta;
  r.cx = pos.x + vp.d_cr * cos_theta; // semantic_map_manager.cc:645-646
  r.cy = pos.y + vp.d_cr * sin_theta;
  return r;
}

std::vector<std::vector<LocalTrajData>> containers(int n, int max_seg, int row_pieces, const int *n_seg, const int *singul,
                                                   const int *piece_nums, const double *coeff_dt, const double *coeffs,
                                                   const double *t_start) {
  std::vector<std::vector<LocalTrajData>> all;
  for (int s = 0; s < n; s++)
    all.push_back(fill_container(n_seg[s], singul + (size_t)s * max_seg, piece_nums + (size_t)s * max_seg, coeff_dt + (size_t)s * max_seg,
                                 coeffs + (size_t)s * row_pieces * 12, t_start[s]));
  return all;
}

} // namespace

// n plans, padded as the executing table: n_seg / t_start [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs
// [n][row_pieces][6][2] with the pieces of a plan's segments following one another.  veh: width, length, d_cr.
// poses [K][n][4]: cx, cy, cs, sn; NaN rows for n_seg == 0.
extern "C" void oracle_conflict_poses(int n, int max_seg, int row_pieces, const int *n_seg, const int *singul, const int *piece_nums,
                                      const double *coeff_dt, const double *coeffs, const double *t_start, double t0, double dt, int K,
                                      const double *veh, int order, double *poses) {
  const Trig T{order};
  const Vehicle vp{veh[0], veh[1], veh[2]};
  const auto all = containers(n, max_seg, row_pieces, n_seg, singul, piece_nums, coeff_dt, coeffs, t_start);
  for (int k = 0; k < K; k++) {
    const double t = t0 + (double)k * dt;
    for (int s = 0; s < n; s++) {
      const Pose p = pose_at(all[s], t, vp, T);
      double *o = poses + ((size_t)k * n + s) * 4;
      o[0] = p.cx;
      o[1] = p.cy;
      o[2] = p.cs;
      o[3] = p.sn;
    }
  }
}

// the separation of two poses (cx, cy, cs, sn), steps 2 and 3 alone
extern "C" double oracle_conflict_sep(const double *a, const double *b, const double *veh) {
  const Vehicle vp{veh[0], veh[1], veh[2]};
  return separation(make_box(a[0], a[1], a[2], a[3], vp), make_box(b[0], b[1], b[2], b[3], vp), vp);
}

// The five rows [n]; counts[0] = pair-samples (i != j, both occupied) examined, counts[1] = those inside the broad phase (may be NULL)
extern "C" void oracle_conflicts(int n, int max_seg, int row_pieces, const int *n_seg, const int *singul, const int *piece_nums,
                                 const double *coeff_dt, const double *coeffs, const double *t_start, double t0, double dt, int K,
                                 double margin, double range, const double *veh, int order, double *min_sep, int *sep_sample,
                                 int *sep_partner, int *conflict_sample, int *conflict_partner, long long *counts) {
  const Trig T{order};
  const Vehicle vp{veh[0], veh[1], veh[2]};
  const auto all = containers(n, max_seg, row_pieces, n_seg, singul, piece_nums, coeff_dt, coeffs, t_start);
  std::vector<Pose> pose((size_t)K * n);
  for (int k = 0; k < K; k++)
    for (int s = 0; s < n; s++) pose[(size_t)k * n + s] = pose_at(all[s], t0 + (double)k * dt, vp, T);
  const double L = vp.length, W = vp.width;
  const double rad = std::sqrt(0.25 * L * L + 0.25 * W * W);
  const double R = range + 2.0 * rad;
  long long examined = 0, inside = 0;
  for (int i = 0; i < n; i++) {
    double best = INF;
    int best_k = -1, best_j = -1, first_k = -1, first_j = -1;
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      for (int k = 0; k < K; k++) {
        const Pose &a = pose[(size_t)k * n + i], &b = pose[(size_t)k * n + j];
        if (!a.occupied || !b.occupied) continue;
        examined++;
        const double dx = a.cx - b.cx, dy = a.cy - b.cy;
        const double d2 = dx * dx + dy * dy;
        if (!(d2 <= R * R)) continue;
        inside++;
        const double sep = separation(make_box(a.cx, a.cy, a.cs, a.sn, vp), make_box(b.cx, b.cy, b.cs, b.sn, vp), vp);
        // (sep, k, j) < (best, best_k, best_j), or the first
        if (best_k < 0 || sep < best || (sep == best && (k < best_k || (k == best_k && j < best_j)))) {
          best = sep;
          best_k = k;
          best_j = j;
        }
        if (sep <= margin && (first_k < 0 || k < first_k || (k == first_k && j < first_j))) {
          first_k = k;
          first_j = j;
        }
      }
    }
    min_sep[i] = best;
    sep_sample[i] = best_k;
    sep_partner[i] = best_j;
    conflict_sample[i] = first_k;
    conflict_partner[i] = first_j;
  }
  if (counts) {
    counts[0] = examined;
    counts[1] = inside;
  }
}
