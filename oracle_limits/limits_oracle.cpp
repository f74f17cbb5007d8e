// TEST INFRASTRUCTURE ONLY: CPU restatement of the kinematic quantities the reference can read off a plan, maximised over the
// samples its replan check walks -- what dftpav_batch_check_limits / dftpav_planner_check_limits compute on the device
// (dftpav_amd/csrc/limits.hip), written from the reference's statements.
//
//   TrajPlannerServer::CheckReplan, the sampling loop              traj_planner/src/traj_server_ros.cpp:385-386
//
// Piece and Trajectory with their five kinematic getters, and the container of chained segments, are oracle_shared/ref_objects.h's, cited
// there.
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

#include "../oracle_shared/ref_objects.h"

namespace {

using namespace ref_objects;

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
    // the container as RunMINCOParking fills it (traj_manager.cpp:618-625)
    const std::vector<LocalTrajData> executing_traj_ = fill_container(n_seg[s], singul + (size_t)s * max_seg, piece_nums + (size_t)s * max_seg,
                                                                      coeff_dt + (size_t)s * max_seg, coeffs + (size_t)s * row_pieces * 12, 0.0);
    RunningMax mx[5];
    int viol[5] = {0, 0, 0, 0, 0};
    int k = 0;
    for (size_t i = 0; i < executing_traj_.size(); i++) { // traj_server_ros.cpp:385
      const int sg = singul[s * max_seg + (int)i];
      const double lim[5] = {sg > 0 ? limits[0] : limits[1], sg > 0 ? limits[2] : limits[3], limits[6], sg > 0 ? limits[4] : limits[5], limits[7]};
      for (double t = 0.0; t < executing_traj_.at(i).duration; t += check_dt) { // :386
        const Trajectory &traj = executing_traj_.at(i).traj;
        const double q[5] = {traj.getVel(t), traj.getAcc(t), traj.getLatAcc(t), traj.getCurv(t, T), traj.getSteer(t, wheel_base, T)};
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
