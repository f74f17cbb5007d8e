// piece_eval.h — the reference's trajectory read-out as the step kernels around the solve share it (validate.hip, states.hip,
// replan.hip, limits.hip; search.hip takes normalize_angle): one statement of each, held bit-equal to the order-2 oracles.
//
//   Trajectory::locatePieceIdx / getTotalDuration / GetState   plan_utils/poly_traj_utils.hpp:510-528, 425-434, 378-406
//   Piece::getPos / getdSigma / getddSigma                     poly_traj_utils.hpp:77-87, 179-211
//   normalize_angle                                            common/src/common/math/calculations.cc:18-23
//   TrajPlannerServer::FilterSingularityState                  traj_planner/src/traj_server_ros.cpp:335-356
//   TrajPlannerServer::CheckReplan, the sampling loop          traj_server_ros.cpp:385-387
//
// Plain functions over values and pointers: a kernel keeps its own data sources (kernel arguments, LDS, a row of the executing
// table) and hands in what it loaded.  A piece is 12 doubles c[6][2] (power k, x | y), a segment N pieces of one duration dtp.
// The names live in dftpav::pe: traj_math.h's piece_pos(const SurEval &, ...) family reads the solver's other layout.
#pragma once
#include "cr_trig.h"

namespace dftpav {

// the sample times of CheckReplan, t = 0, dt, dt + dt, ...: the host tabulates the first n_t values of that running sum
// (validation_table), so a thread sees exactly the value the sequential loop would have reached
struct SampleTable {
  const double *t_tab;
  int n_t;
  double sample_dt;
};

namespace pe {

// locatePieceIdx: the piece tt falls into; tt becomes the time inside it.  (The walk runs on a local copy: through the reference
// the compiler leaves a longer loop body in every caller.)
__device__ inline int locate_piece(int N, double dtp, double &tt) {
  double t = tt;
  int idx = 0;
  while (idx < N && t > dtp) {
    t -= dtp;
    idx++;
  }
  if (idx == N) {
    idx--;
    t += dtp;
  }
  tt = t;
  return idx;
}
__device__ inline void piece_pos(const double *c, double tt, double &px, double &py) { // Piece::getPos
  px = 0.0;
  py = 0.0;
  double tn = 1.0;
#pragma unroll
  for (int k = 0; k <= 5; k++) {
    px += tn * c[2 * k];
    py += tn * c[2 * k + 1];
    tn *= tt;
  }
}
__device__ inline void piece_vel(const double *c, double tt, double &vx, double &vy) { // Piece::getdSigma
  vx = 0.0;
  vy = 0.0;
  double tn = 1.0;
#pragma unroll
  for (int k = 1; k <= 5; k++) {
    vx += (double)k * tn * c[2 * k];
    vy += (double)k * tn * c[2 * k + 1];
    tn *= tt;
  }
}
__device__ inline void piece_acc(const double *c, double tt, double &ax, double &ay) { // Piece::getddSigma
  ax = 0.0;
  ay = 0.0;
  double tn = 1.0;
#pragma unroll
  for (int k = 2; k <= 5; k++) {
    ax += (double)((k - 1) * k) * tn * c[2 * k];
    ay += (double)((k - 1) * k) * tn * c[2 * k + 1];
    tn *= tt;
  }
}

// Trajectory::getTotalDuration of a segment: the piece durations summed in order
__device__ inline double segment_duration(int N, double dtp) {
  double d = 0.0;
  for (int p = 0; p < N; p++) d += dtp;
  return d;
}

// The tail of Trajectory::GetState from dsigma, ddsigma and the direction sg.  (The reference calls libm's atan2, pow(vel, 3)
// and atan; here the correctly rounded ones, as oracle order 2.)  limits.hip does not use it: Piece::getAcc / getCurv divide by
// the norm and branch on it, not on vel.
struct StateTail {
  double angle, vel, curv, acc, steer;
};
__device__ inline StateTail get_state_tail(double vx, double vy, double ax, double ay, double sg, double wheel_base) {
  StateTail s;
  s.angle = crt::atan2(sg * vy, sg * vx);
  s.vel = sg * sqrt(vx * vx + vy * vy);
  s.curv = 0.0;
  s.acc = 0.0;
  s.steer = 0.0;
  if (!(fabs(s.vel) < 1e-6)) {
    s.curv = (vx * ay - vy * ax) / crt::cube_cr(s.vel);
    s.acc = (vx * ax + vy * ay) / s.vel;
    s.steer = crt::atan(wheel_base * s.curv);
  }
  return s;
}

__device__ inline double normalize_angle(double theta) {
  const double pi = 3.14159265358979323846;
  double tmp = theta;
  tmp -= (double)((theta >= pi) * 2) * pi;
  tmp += (double)((theta < -pi) * 2) * pi;
  return tmp;
}

// FilterSingularityState: a slow state (|vel| < kBigEPS) takes the previous heading when its own differs from it by more than
// the steering limit allows in the dt since.  True: hold hist_angle.  max_rate = tan(M_PI / 4) / 2.85 * 0.1 with the tangent
// correctly rounded, which is what glibc returns.  (Written as a branch: returned as one && expression it becomes selects in
// the publisher's serial chain.)
__device__ inline bool filter_singularity(double angle, double vel, double hist_angle, double dt) {
  const double max_rate = 0x1.fffffffffffffp-1 / 2.85 * 0.1;
  const double max_change = max_rate * dt;
  if (fabs(vel) < 0.1 && fabs(normalize_angle(angle - hist_angle)) > max_change) return true;
  return false;
}

// number of samples t_k < dur: the table is increasing; past its end the running sum is continued
__device__ inline int samples_below(const SampleTable &tab, double dur) {
  int lo = 0, hi = tab.n_t;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab.t_tab[mid] < dur) lo = mid + 1;
    else hi = mid;
  }
  int cnt = lo;
  if (cnt == tab.n_t) {
    for (double t = tab.t_tab[tab.n_t - 1] + tab.sample_dt; t < dur; t += tab.sample_dt) cnt++;
  }
  return cnt;
}
// t_k: from the table, past its end the continued running sum
__device__ inline double sample_time(const SampleTable &tab, int k) {
  if (k < tab.n_t) return tab.t_tab[k];
  double t = tab.t_tab[tab.n_t - 1];
  for (int j = tab.n_t - 1; j < k; j++) t += tab.sample_dt;
  return t;
}
// the segment of global sample q; count[i] = samples of the segments before segment i
__device__ inline int sample_segment(const int *count, int M, int q) {
  int i = 0;
  while (i + 1 < M && q >= count[i + 1]) i++;
  return i;
}

} // namespace pe
} // namespace dftpav
