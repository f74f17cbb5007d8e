// TEST INFRASTRUCTURE ONLY: CPU yardstick of dftpav_grid_distance_field and of the clearance calls (dftpav_amd/csrc/distfield.hip,
// clearance.hip).  It shares no header with the kernels (oracle/step_trig.h brings the trigonometry by order).
//
// The field.  oracle_field_brute is the definition, literally: every cell against every occupied cell.  oracle_field is Meijster's
// two-phase algorithm (A. Meijster, J. Roerdink, W. Hesselink, "A general algorithm for computing distance transforms in linear
// time", 2000) in integer arithmetic, the column phase FIRST and the lower envelope of parabolas along the rows second -- the
// kernels scan the rows first and then walk the columns outward, so neither the axis order nor the second phase is theirs.
//
// The clearance.  The reference's objects -- Piece, Trajectory (getPos, getAngle), the container of chained segments, the grid's cell
// rule and the dense outline CheckCollisionUsingPosAndYaw walks -- are oracle_shared/ref_objects.h's, cited there (that header shares none
// with the kernels either); the sampling loop is TrajPlannerServer::CheckReplan's, traj_planner/src/traj_server_ros.cpp:385-387.
// The reference asks each vertex "is this cell OCCUPIED"; here the same vertex, in the same cell, reads the field instead, and the
// running minimum over vertices and samples is kept in sample order, replaced only on `<`.  A vertex outside the grid is skipped.
// Nothing is tabulated, strided or reduced.  order 0: the host's libm, as the reference calls it; order 2: correctly rounded from
// binary128 -- the yardstick of the device kernel.
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "../oracle_shared/ref_objects.h"

namespace {

const int FAR = INT_MAX;

// ---------------------------------------------------------------- the field
void field_brute(const unsigned char *cells, int sx, int sy, int *d2) {
  for (int iy = 0; iy < sy; iy++)
    for (int ix = 0; ix < sx; ix++) {
      long long best = FAR;
      for (int jy = 0; jy < sy; jy++)
        for (int jx = 0; jx < sx; jx++)
          if (cells[jx + (size_t)sx * jy] == 80) {
            const long long d = (long long)(ix - jx) * (ix - jx) + (long long)(iy - jy) * (iy - jy);
            if (d < best) best = d;
          }
      d2[ix + (size_t)sx * iy] = (int)best;
    }
}

inline long long floor_div(long long a, long long b) { // b > 0
  long long q = a / b;
  if (a % b != 0 && a < 0) q--;
  return q;
}

void field_meijster(const unsigned char *cells, int sx, int sy, int *d2) {
  const long long INF = 1ll << 20; // beyond every distance of a map whose sides are <= 16384; INF * INF fits easily
  std::vector<long long> G((size_t)sx * sy);
  // phase 1, along y: G = the distance along the column to its nearest occupied cell
  for (int x = 0; x < sx; x++) {
    G[x] = cells[x] == 80 ? 0 : INF;
    for (int y = 1; y < sy; y++) G[x + (size_t)sx * y] = cells[x + (size_t)sx * y] == 80 ? 0 : std::min(INF, G[x + (size_t)sx * (y - 1)] + 1);
    for (int y = sy - 2; y >= 0; y--)
      if (G[x + (size_t)sx * (y + 1)] < G[x + (size_t)sx * y]) G[x + (size_t)sx * y] = std::min(INF, G[x + (size_t)sx * (y + 1)] + 1);
  }
  // phase 2, along x: the lower envelope of f(x, i) = (x - i)^2 + G(i)^2
  std::vector<int> s(sx), t(sx);
  for (int y = 0; y < sy; y++) {
    const long long *g = &G[(size_t)sx * y];
    auto f = [&](long long x, long long i) { return (x - i) * (x - i) + g[i] * g[i]; };
    auto sep = [&](long long i, long long u) { return floor_div(u * u - i * i + g[u] * g[u] - g[i] * g[i], 2 * (u - i)); };
    int q = 0;
    s[0] = 0;
    t[0] = 0;
    for (int u = 1; u < sx; u++) {
      while (q >= 0 && f(t[q], s[q]) > f(t[q], u)) q--;
      if (q < 0) {
        q = 0;
        s[0] = u;
      } else {
        const long long w = 1 + sep(s[q], u);
        if (w < sx) {
          q++;
          s[q] = u;
          t[q] = (int)w;
        }
      }
    }
    for (int u = sx - 1; u >= 0; u--) {
      const long long v = f(u, s[q]);
      d2[u + (size_t)sx * y] = v >= INF * INF ? FAR : (int)v;
      if (u == t[q]) q--;
    }
  }
}

// ---------------------------------------------------------------- the clearance
using namespace ref_objects;

// CheckCollisionUsingPosAndYaw's walk over the vertices (semantic_map_manager.cc:639-662), reading the field at the cell the
// reference would probe: the smallest d2 of the vertices inside the grid, FAR if none is
int pose_min_d2(const Grid &g, const int *d2, Vec2 pos, double yaw, const Vehicle &vp, double vres, const Trig &T) {
  int m = FAR;
  visit_outline(pos.x, pos.y, yaw, vp, vres, T, [&](Vec2 v) {
    const ptrdiff_t i = g.cell_index(v.x, v.y);
    if (i >= 0 && d2[i] < m) m = d2[i];
    return false;
  });
  return m;
}

} // namespace

extern "C" void oracle_field(const unsigned char *cells, int size_x, int size_y, int *d2) { field_meijster(cells, size_x, size_y, d2); }
extern "C" void oracle_field_brute(const unsigned char *cells, int size_x, int size_y, int *d2) { field_brute(cells, size_x, size_y, d2); }

// n plans, padded: n_seg [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs [n][row_pieces][6][2] with the pieces of a plan's
// segments following one another.  veh: width, length, d_cr.  min_d2 / arg / clearance / n_samples [n].
extern "C" void oracle_clearance(const unsigned char *cells, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                                 int n, int max_seg, int row_pieces, const int *n_seg, const int *singul, const int *piece_nums,
                                 const double *coeff_dt, const double *coeffs, double check_dt, const double *veh, double vertex_res,
                                 int order, int *min_d2, int *arg, double *clearance, int *n_samples) {
  const Trig T{order};
  std::vector<int> field((size_t)size_x * size_y);
  field_meijster(cells, size_x, size_y, field.data());
  const Grid g{cells, size_x, size_y, resolution, origin_x, origin_y};
  const Vehicle vp{veh[0], veh[1], veh[2]};
  for (int s = 0; s < n; s++) {
    // the container as RunMINCOParking fills it (traj_manager.cpp:618-625)
    const std::vector<LocalTrajData> executing_traj_ = fill_container(n_seg[s], singul + (size_t)s * max_seg, piece_nums + (size_t)s * max_seg,
                                                                      coeff_dt + (size_t)s * max_seg, coeffs + (size_t)s * row_pieces * 12, 0.0);
    int best = FAR, where = -1, k = 0;
    for (size_t i = 0; i < executing_traj_.size(); i++) {                           // traj_server_ros.cpp:385
      for (double t = 0.0; t < executing_traj_.at(i).duration; t += check_dt) {     // :386-387
        const Trajectory &traj = executing_traj_.at(i).traj;
        const Vec2 pos = traj.getPos(t);
        const double yaw = traj.getAngle(t, T);
        const int d = pose_min_d2(g, field.data(), pos, yaw, vp, vertex_res, T);
        if (d < best) {
          best = d;
          where = k;
        }
        k++;
      }
    }
    min_d2[s] = best;
    arg[s] = where;
    clearance[s] = best == FAR ? std::numeric_limits<double>::infinity() : resolution * std::sqrt((double)best);
    if (n_samples) n_samples[s] = k;
  }
}
