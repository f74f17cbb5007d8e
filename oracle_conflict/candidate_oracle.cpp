// TEST INFRASTRUCTURE ONLY: CPU yardstick of the candidate conflict check (dftpav_batch_check_conflicts, dftpav_batch_sample_poses and
// the conflict filter of dftpav_plan_queries; dftpav_amd/csrc/cand_conflict.hip).  It shares no header with the kernels
// (oracle/step_trig.h brings the trigonometry by order) and is written from the definition in include/dftpav_hip.h.
//
// A candidate is one trajectory of a batch -- the batch's layout, its pieces and piece durations -- with a start clock.  Its pose at a
// clock is the pose of the container RunMINCOParking would fill from it at that start (oracle_shared/ref_objects.h: fill_container,
// the chain of start / end times), read as the conflict check reads a slot: the segment exe_traj_index_ reaches at the clock, the
// local time clamped into the segment, Trajectory::getPos / getAngle, the box centre d_cr ahead.  The slots are read the same way.
// order 0: the host's libm; order 2: correctly rounded -- the yardstick of the kernels.
//
// The rows.  Plain loops over (candidate, slot, sample); every minimum is an explicit lexicographic comparison.  The box, the
// separating-axis test and the point-to-segment distance are restated here from the definition, not shared with conflict_oracle.cpp:
// the two files stand alone.
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "../oracle_shared/ref_objects.h"

namespace {

using namespace ref_objects;

const double INF = std::numeric_limits<double>::infinity();
const double QNAN = std::numeric_limits<double>::quiet_NaN();

struct Pose {
  bool occupied;
  double cx, cy, cs, sn;
};

// the pose of one container at clock t
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

// the four corners of the box of a pose, shapes.cc:110-149
void corners_of(const Pose &p, const Vehicle &vp, Vec2 corner[4]) {
  const double x = p.cx, y = p.cy, L = vp.length, W = vp.width, cos_theta = p.cs, sin_theta = p.sn;
  corner[0] = Vec2{x + 0.5 * L * cos_theta + 0.5 * W * sin_theta, y + 0.5 * L * sin_theta - 0.5 * W * cos_theta};
  corner[1] = Vec2{x + 0.5 * L * cos_theta - 0.5 * W * sin_theta, y + 0.5 * L * sin_theta + 0.5 * W * cos_theta};
  corner[2] = Vec2{x - 0.5 * L * cos_theta - 0.5 * W * sin_theta, y - 0.5 * L * sin_theta + 0.5 * W * cos_theta};
  corner[3] = Vec2{x - 0.5 * L * cos_theta + 0.5 * W * sin_theta, y - 0.5 * L * sin_theta - 0.5 * W * cos_theta};
}

// step 2: does an axis of `own` separate it from the box with these corners?
bool axis_of_owner_separates(const Pose &own, const Vec2 other[4], const Vehicle &vp) {
  bool all_above_x = true, all_below_x = true, all_above_y = true, all_below_y = true;
  for (int q = 0; q < 4; q++) {
    const double lx = own.cs * (other[q].x - own.cx) + own.sn * (other[q].y - own.cy);
    const double ly = own.cs * (other[q].y - own.cy) - own.sn * (other[q].x - own.cx);
    if (!(lx > vp.length / 2)) all_above_x = false;
    if (!(lx < -vp.length / 2)) all_below_x = false;
    if (!(ly > vp.width / 2)) all_above_y = false;
    if (!(ly < -vp.width / 2)) all_below_y = false;
  }
  return all_above_x || all_below_x || all_above_y || all_below_y;
}

// steps 2 and 3
double separation(const Pose &A, const Pose &B, const Vehicle &vp) {
  Vec2 ca[4], cb[4];
  corners_of(A, vp, ca);
  corners_of(B, vp, cb);
  if (!axis_of_owner_separates(A, cb, vp) && !axis_of_owner_separates(B, ca, vp)) return 0.0;
  double m = INF;
  for (int side = 0; side < 2; side++) {
    const Vec2 *P = side == 0 ? ca : cb, *E = side == 0 ? cb : ca;
    for (int q = 0; q < 4; q++)
      for (int e = 0; e < 4; e++) {
        const Vec2 p = P[q], a = E[e], b = E[(e + 1) % 4];
        double u = ((p.x - a.x) * (b.x - a.x) + (p.y - a.y) * (b.y - a.y)) / ((b.x - a.x) * (b.x - a.x) + (b.y - a.y) * (b.y - a.y));
        if (!(u > 0.0)) u = 0.0;
        else if (u > 1.0) u = 1.0;
        const Vec2 foot{a.x + u * (b.x - a.x), a.y + u * (b.y - a.y)};
        const double ex = p.x - foot.x, ey = p.y - foot.y;
        const double d = ex * ex + ey * ey;
        if (d < m) m = d;
      }
  }
  return std::sqrt(m);
}

// candidate c of the batch as the container an adoption at t_start would fill
std::vector<LocalTrajData> candidate(int c, int M, int n_pieces, const int *singul, const int *piece_nums, const double *piece_dt,
                                     const double *coeffs, double t_start) {
  return fill_container(M, singul, piece_nums, piece_dt + (size_t)c * M, coeffs + (size_t)c * n_pieces * 12, t_start);
}

} // namespace

// B candidates of one layout: singul / piece_nums [M], piece_dt [B][M], coeffs [B][n_pieces][6][2].  poses [K][B][4]: cx, cy, cs, sn.
extern "C" void oracle_candidate_poses(int B, int M, int n_pieces, const int *singul, const int *piece_nums, const double *piece_dt,
                                       const double *coeffs, double t_start, double t0, double dt, int K, const double *veh, int order,
                                       double *poses) {
  const Trig T{order};
  const Vehicle vp{veh[0], veh[1], veh[2]};
  for (int c = 0; c < B; c++) {
    const auto cont = candidate(c, M, n_pieces, singul, piece_nums, piece_dt, coeffs, t_start);
    for (int k = 0; k < K; k++) {
      const Pose p = pose_at(cont, t0 + (double)k * dt, vp, T);
      double *o = poses + ((size_t)k * B + c) * 4;
      o[0] = p.cx;
      o[1] = p.cy;
      o[2] = p.cs;
      o[3] = p.sn;
    }
  }
}

// The candidates against n slots padded as the executing table (conflict_oracle.cpp: oracle_conflicts).  own [B] or NULL.  The five rows [B].
extern "C" void oracle_candidate_conflicts(int B, int M, int n_pieces, const int *singul, const int *piece_nums, const double *piece_dt,
                                           const double *coeffs, double t_start, int n, int max_seg, int row_pieces, const int *t_n_seg,
                                           const int *t_singul, const int *t_piece_nums, const double *t_coeff_dt, const double *t_coeffs,
                                           const double *t_t_start, double t0, double dt, int K, double margin, double range,
                                           const double *veh, int order, const int *own, double *min_sep, int *sep_sample,
                                           int *sep_partner, int *conflict_sample, int *conflict_partner) {
  const Trig T{order};
  const Vehicle vp{veh[0], veh[1], veh[2]};
  std::vector<Pose> slot((size_t)K * n);
  for (int s = 0; s < n; s++) {
    const auto cont = fill_container(t_n_seg[s], t_singul + (size_t)s * max_seg, t_piece_nums + (size_t)s * max_seg,
                                     t_coeff_dt + (size_t)s * max_seg, t_coeffs + (size_t)s * row_pieces * 12, t_t_start[s]);
    for (int k = 0; k < K; k++) slot[(size_t)k * n + s] = pose_at(cont, t0 + (double)k * dt, vp, T);
  }
  const double L = vp.length, W = vp.width;
  const double rad = std::sqrt(0.25 * L * L + 0.25 * W * W);
  const double R = range + 2.0 * rad;
  for (int c = 0; c < B; c++) {
    const auto cont = candidate(c, M, n_pieces, singul, piece_nums, piece_dt, coeffs, t_start);
    std::vector<Pose> mine((size_t)K);
    for (int k = 0; k < K; k++) mine[k] = pose_at(cont, t0 + (double)k * dt, vp, T);
    double best = INF;
    int best_k = -1, best_j = -1, first_k = -1, first_j = -1;
    for (int j = 0; j < n; j++) {
      if (own && j == own[c]) continue;
      for (int k = 0; k < K; k++) {
        const Pose &a = mine[k];
        const Pose &b = slot[(size_t)k * n + j];
        if (!a.occupied || !b.occupied) continue;
        const double dx = a.cx - b.cx, dy = a.cy - b.cy;
        const double d2 = dx * dx + dy * dy;
        if (!(d2 <= R * R)) continue;
        const double sep = separation(a, b, vp);
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
    min_sep[c] = best;
    sep_sample[c] = best_k;
    sep_partner[c] = best_j;
    conflict_sample[c] = first_k;
    conflict_partner[c] = first_j;
  }
}
