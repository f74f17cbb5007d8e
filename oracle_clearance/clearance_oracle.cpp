// TEST INFRASTRUCTURE ONLY: CPU yardstick of dftpav_grid_distance_field and of the clearance calls (dftpav_amd/csrc/distfield.hip,
// clearance.hip).  It shares no header with the kernels (oracle/step_trig.h brings the trigonometry by order).
//
// The field.  oracle_field_brute is the definition, literally: every cell against every occupied cell.  oracle_field is Meijster's
// two-phase algorithm (A. Meijster, J. Roerdink, W. Hesselink, "A general algorithm for computing distance transforms in linear
// time", 2000) in integer arithmetic, the column phase FIRST and the lower envelope of parabolas along the rows second -- the
// kernels scan the rows first and then walk the columns outward, so neither the axis order nor the second phase is theirs.
//
// The clearance.  The reference's objects, restated from the cited lines:
//   TrajPlannerServer::CheckReplan, the sampling loop   traj_planner/src/traj_server_ros.cpp:385-387
//   Piece::getPos / getdSigma                           plan_utils/poly_traj_utils.hpp:77-87, 179-192
//   Trajectory::getTotalDuration / locatePieceIdx       poly_traj_utils.hpp:425-434, 510-528
//   Trajectory::getPos / getAngle, Piece::getAngle      poly_traj_utils.hpp:554-558, 626-630, 237-244
//   TrajContainer::addSingulTraj, the chained segments  plan_utils/traj_container.hpp:58-73
//   SemanticMapManager::CheckCollisionUsingPosAndYaw    semantic_map_manager.cc:639-662
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox   common/src/common/basics/shapes.cc:110-149 (res = 0.1, shapes.h:200-201)
//   GridMapND::GetCoordUsingGlobalPosition              common/src/common/basics/semantics.cc:169-179, 214-221
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

#include "../oracle/step_trig.h"

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
using step_trig::Trig;

struct Vec2 {
  double x, y;
};

struct Piece { // plan_utils::Piece.  c[k][0] / c[k][1]: the coefficient of t^k of x / y (the layout of dftpav_batch_coeffs)
  double duration;
  const double *c;
  Vec2 getPos(double t) const { // :77-87
    Vec2 pos{0.0, 0.0};
    double tn = 1.0;
    for (int i = 0; i <= 5; i++) {
      pos.x += tn * c[2 * i];
      pos.y += tn * c[2 * i + 1];
      tn *= t;
    }
    return pos;
  }
  Vec2 getdSigma(double t) const { // :179-192
    Vec2 vel{0.0, 0.0};
    double tn = 1.0;
    int n = 1;
    for (int i = 1; i <= 5; i++) {
      vel.x += n * tn * c[2 * i];
      vel.y += n * tn * c[2 * i + 1];
      tn *= t;
      n++;
    }
    return vel;
  }
};

struct Trajectory {
  std::vector<Piece> pieces;
  int singul;
  const Trig *T;
  double getTotalDuration() const { // :425-434
    double totalDuration = 0.0;
    for (size_t i = 0; i < pieces.size(); i++) totalDuration += pieces[i].duration;
    return totalDuration;
  }
  int locatePieceIdx(double &t) const { // :510-528
    const int N = (int)pieces.size();
    int idx;
    double dur;
    for (idx = 0; idx < N && t > (dur = pieces[idx].duration); idx++) t -= dur;
    if (idx == N) {
      idx--;
      t += pieces[idx].duration;
    }
    return idx;
  }
  Vec2 getPos(double t) const { // :554-558 (t by value: locatePieceIdx rewrites the copy)
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getPos(t);
  }
  double getAngle(double t) const { // :626-630, with Piece::getAngle (:237-244) written out
    int pieceIdx = locatePieceIdx(t);
    Vec2 dsigma = pieces[pieceIdx].getdSigma(t);
    return T->atan2(singul * dsigma.y, singul * dsigma.x);
  }
};

struct LocalTrajData { // traj_container.hpp:28-38
  Trajectory traj;
  double duration, start_time, end_time;
};

struct GridMap {
  const unsigned char *cells;
  const int *d2;
  int sx, sy;
  double res, ox, oy;
};

// GetDenseVerticesOfOrientedBoundingBox, shapes.cc:110-149: the dense points of the four edges, then the four corners
void dense_vertices(double x, double y, double angle, double W, double L, double res, const Trig &T, std::vector<Vec2> *vertices) {
  const double cs = T.cos(angle), sn = T.sin(angle);
  Vec2 corner[4];
  corner[0] = Vec2{x + 0.5 * L * cs + 0.5 * W * sn, y + 0.5 * L * sn - 0.5 * W * cs};
  corner[1] = Vec2{x + 0.5 * L * cs - 0.5 * W * sn, y + 0.5 * L * sn + 0.5 * W * cs};
  corner[2] = Vec2{x - 0.5 * L * cs - 0.5 * W * sn, y - 0.5 * L * sn + 0.5 * W * cs};
  corner[3] = Vec2{x - 0.5 * L * cs + 0.5 * W * sn, y - 0.5 * L * sn - 0.5 * W * cs};
  vertices->clear();
  for (int e = 0; e < 4; e++) {
    const Vec2 a = corner[e], b = corner[(e + 1) % 4];
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double norm = std::sqrt(dx * dx + dy * dy);
    for (double dl = res; dl < norm; dl += res) {
      const double f = dl / norm;
      vertices->push_back(Vec2{f * dx + a.x, f * dy + a.y});
    }
  }
  for (int e = 0; e < 4; e++) vertices->push_back(corner[e]);
}

// CheckCollisionUsingPosAndYaw's walk over the vertices (semantic_map_manager.cc:639-662), reading the field: the smallest d2 of
// the vertices inside the grid, FAR if none is
int pose_min_d2(const GridMap &g, Vec2 pos, double yaw, double W, double L, double dcr, double vres, const Trig &T, std::vector<Vec2> *scratch) {
  const double cx = pos.x + dcr * T.cos(yaw), cy = pos.y + dcr * T.sin(yaw); // the obb centre, :645-646
  dense_vertices(cx, cy, yaw, W, L, vres, T, scratch);
  int m = FAR;
  for (const Vec2 &v : *scratch) {
    const double gx = std::round((v.x - g.ox) / g.res), gy = std::round((v.y - g.oy) / g.res);
    if (!(gx >= 0.0 && gx < (double)g.sx && gy >= 0.0 && gy < (double)g.sy)) continue;
    const int d = g.d2[(int)gx + (size_t)g.sx * (int)gy];
    if (d < m) m = d;
  }
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
  const GridMap g{cells, field.data(), size_x, size_y, resolution, origin_x, origin_y};
  std::vector<Vec2> vertices;
  for (int s = 0; s < n; s++) {
    std::vector<LocalTrajData> executing_traj_; // the container as RunMINCOParking fills it (traj_manager.cpp:618-625)
    double world = 0.0;
    int p0 = 0;
    for (int i = 0; i < n_seg[s]; i++) {
      LocalTrajData d;
      d.traj.singul = singul[s * max_seg + i];
      d.traj.T = &T;
      for (int k = 0; k < piece_nums[s * max_seg + i]; k++)
        d.traj.pieces.push_back(Piece{coeff_dt[s * max_seg + i], coeffs + ((size_t)s * row_pieces + p0 + k) * 12});
      p0 += piece_nums[s * max_seg + i];
      d.duration = d.traj.getTotalDuration();
      d.start_time = world;
      d.end_time = d.start_time + d.duration;
      world = d.end_time;
      executing_traj_.push_back(d);
    }
    int best = FAR, where = -1, k = 0;
    for (size_t i = 0; i < executing_traj_.size(); i++) {                           // traj_server_ros.cpp:385
      for (double t = 0.0; t < executing_traj_.at(i).duration; t += check_dt) {     // :386-387
        const Trajectory &traj = executing_traj_.at(i).traj;
        const Vec2 pos = traj.getPos(t);
        const double yaw = traj.getAngle(t);
        const int d = pose_min_d2(g, pos, yaw, veh[0], veh[1], veh[2], vertex_res, T, &vertices);
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
