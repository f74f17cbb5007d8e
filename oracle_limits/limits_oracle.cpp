// TEST INFRASTRUCTURE ONLY: CPU restatement of the kinematic quantities the reference can read off a plan, maximised over the
// samples its replan check walks -- what dftpav_batch_check_limits / dftpav_planner_check_limits compute on the device
// (dftpav_amd/csrc/limits.hip), written from the reference's statements.
//
//   Piece::getCurv / getVel / getAcc / getLatAcc / getSteer        plan_utils/poly_traj_utils.hpp:247-300
//   Piece::getdSigma / getddSigma                                  poly_traj_utils.hpp:179-211
//   Trajectory::getVel / getAcc / getLatAcc / getCurv / getSteer   poly_traj_utils.hpp:606-645
//   Trajectory::getTotalDuration / locatePieceIdx                  poly_traj_utils.hpp:425-434, 510-528
//   TrajContainer::addSingulTraj, the chained segments             plan_utils/traj_container.hpp:58-73
//   TrajPlannerServer::CheckReplan, the sampling loop              traj_planner/src/traj_server_ros.cpp:385-386
//
// Laid out as the reference's objects: a Piece, a Trajectory of pieces, a container entry per gear segment, and CheckReplan's two
// loops with the running t += check_dt.  Every getter evaluates dsigma (and its norm) again, as the reference's does.  The maxima
// are plain running maxima in sample order, replaced only on `>`; the one addition is the NaN rule of the header (a NaN sample
// replaces a number once and is then kept).  Nothing is tabulated, strided or reduced.
// order 0: the host's libm, as the reference calls it (std::pow(., 3), std::atan).  order 2: both correctly rounded from binary128
// (oracle/step_trig.h) -- the yardstick of the device kernel.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../oracle/step_trig.h"

namespace {

using step_trig::Trig;

struct Vec2 {
  double x, y;
  double norm() const { return std::sqrt(x * x + y * y); }
};

// plan_utils::Piece.  c[k][0] / c[k][1]: the coefficient of t^k of x / y (the layout of dftpav_batch_coeffs)
struct Piece {
  double duration;
  const double *c;
  int singul;
  double wheel_base;
  const Trig *T;
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
  Vec2 getddSigma(double t) const { // :194-211
    Vec2 acc{0.0, 0.0};
    double tn = 1.0;
    int m = 1, n = 2;
    for (int i = 2; i <= 5; i++) {
      acc.x += m * n * tn * c[2 * i];
      acc.y += m * n * tn * c[2 * i + 1];
      tn *= t;
      m++;
      n++;
    }
    return acc;
  }
  double getCurv(const double &t) const {
    Vec2 dsigma = getdSigma(t);
    Vec2 ddsigma = getddSigma(t);
    if (dsigma.norm() < 1e-6) {
      return 0.0;
    } else {
      return singul * (dsigma.x * ddsigma.y - dsigma.y * ddsigma.x) / T->cube(dsigma.norm());
    }
  }
  double getVel(const double &t) const {
    Vec2 dsigma = getdSigma(t);
    return singul * dsigma.norm();
  }
  double getAcc(const double &t) const {
    Vec2 dsigma = getdSigma(t);
    Vec2 ddsigma = getddSigma(t);
    if (dsigma.norm() < 1e-6) {
      return 0.0;
    } else {
      return singul * (dsigma.x * ddsigma.x + dsigma.y * ddsigma.y) / dsigma.norm();
    }
  }
  double getLatAcc(const double &t) const {
    Vec2 dsigma = getdSigma(t);
    Vec2 ddsigma = getddSigma(t);
    if (dsigma.norm() < 1e-6) {
      return 0.0;
    } else {
      return singul * (dsigma.x * ddsigma.y - dsigma.y * ddsigma.x) / dsigma.norm();
    }
  }
  double getSteer(const double &t) const { return T->atan(wheel_base * getCurv(t)); }
};

struct Trajectory {
  std::vector<Piece> pieces;
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
  // :606-645 (t by value: locatePieceIdx rewrites the copy)
  double getVel(double t) const {
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getVel(t);
  }
  double getAcc(double t) const {
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getAcc(t);
  }
  double getLatAcc(double t) const {
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getLatAcc(t);
  }
  double getCurv(double t) const {
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getCurv(t);
  }
  double getSteer(double t) const {
    int pieceIdx = locatePieceIdx(t);
    return pieces[pieceIdx].getSteer(t);
  }
};

struct LocalTrajData { // traj_container.hpp:28-38
  Trajectory traj;
  double duration, start_time, end_time;
};

struct RunningMax { // replaced only on `>`; a NaN replaces a number once and is then kept (the header's rule)
  double m = 0.0;
  int arg = -1;
  void take(double a, int k) {
    if (arg < 0 || a > m || (a != a && m == m)) {
      m = a;
      arg = k;
    }
  }
};

} // namespace

// n plans, padded: n_seg [n], singul / piece_nums / coeff_dt [n][max_seg], coeffs [n][row_pieces][6][2] with the pieces of a plan's
// segments following one another.  limits [8] in the order of dftpav_limits.  max_abs / arg / violated [n][5] (velocity, acceleration,
// lateral acceleration, curvature, steer), feasible [n]; a plan without a segment gives a zero row with arg -1.  samples (or null)
// [n][max_samples][8]: the loop's t, the segment, the local time locatePieceIdx leaves, then the five quantities signed, in sample
// order; n_samples [n] counts every sample, the stored ones are the first max_samples.
extern "C" void oracle_limits(int n, int max_seg, int row_pieces, const int *n_seg, const int *singul, const int *piece_nums,
                              const double *coeff_dt, const double *coeffs, double check_dt, double wheel_base, const double *limits,
                              int order, double *max_abs, int *arg, int *violated, int *feasible, int max_samples, double *samples,
                              int *n_samples) {
  const Trig T{order};
  for (int s = 0; s < n; s++) {
    std::vector<LocalTrajData> executing_traj_; // the container as RunMINCOParking fills it (traj_manager.cpp:618-625)
    double world = 0.0;
    int p0 = 0;
    for (int i = 0; i < n_seg[s]; i++) {
      LocalTrajData d;
      for (int k = 0; k < piece_nums[s * max_seg + i]; k++)
        d.traj.pieces.push_back(Piece{coeff_dt[s * max_seg + i], coeffs + ((size_t)s * row_pieces + p0 + k) * 12, singul[s * max_seg + i], wheel_base, &T});
      p0 += piece_nums[s * max_seg + i];
      d.duration = d.traj.getTotalDuration();
      d.start_time = world;
      d.end_time = d.start_time + d.duration;
      world = d.end_time;
      executing_traj_.push_back(d);
    }
    RunningMax mx[5];
    int viol[5] = {0, 0, 0, 0, 0};
    int k = 0;
    for (size_t i = 0; i < executing_traj_.size(); i++) { // traj_server_ros.cpp:385
      const int sg = singul[s * max_seg + (int)i];
      const double lim[5] = {sg > 0 ? limits[0] : limits[1], sg > 0 ? limits[2] : limits[3], limits[6], sg > 0 ? limits[4] : limits[5], limits[7]};
      for (double t = 0.0; t < executing_traj_.at(i).duration; t += check_dt) { // :386
        const Trajectory &traj = executing_traj_.at(i).traj;
        const double q[5] = {traj.getVel(t), traj.getAcc(t), traj.getLatAcc(t), traj.getCurv(t), traj.getSteer(t)};
        for (int j = 0; j < 5; j++) {
          const double a = std::fabs(q[j]);
          mx[j].take(a, k);
          if (a > lim[j] || a != a) viol[j] = 1;
        }
        if (samples && k < max_samples) {
          double *row = samples + ((size_t)s * max_samples + k) * 8;
          double tl = t;
          traj.locatePieceIdx(tl);
          row[0] = t;
          row[1] = (double)i;
          row[2] = tl;
          for (int j = 0; j < 5; j++) row[3 + j] = q[j];
        }
        k++;
      }
    }
    if (n_samples) n_samples[s] = k;
    int any = 0;
    for (int j = 0; j < 5; j++) {
      max_abs[s * 5 + j] = mx[j].m;
      arg[s * 5 + j] = mx[j].arg;
      violated[s * 5 + j] = viol[j];
      any |= viol[j];
    }
    feasible[s] = (n_seg[s] > 0 && !any) ? 1 : 0;
  }
}
