// TEST INFRASTRUCTURE ONLY (see oracle/dftpav_oracle.h): CPU restatement of the read-out of an optimised
// trajectory, the other half of SURVEY.md §8(f)-2 — Trajectory::GetState over a time grid, played back the
// way the server walks the gear segments.
//
//   TrajPlannerServer::PublishData (which segment is played)   traj_planner/src/traj_server_ros.cpp:244-259
//
// Trajectory::GetState, the container and its chain of start / end times, and the rule of FilterSingularityState are
// oracle_shared/ref_objects.h's, cited there.
//
// Sample k carries the time stamp t_k = t0 + k * dt (time 0 = start of the first segment).  The segment
// played at t is the first one whose end_time is not <= t (the server moves on by one segment per tick when
// `end_time <= t`; ticks are far denser than segments); past the last segment nothing is published, which
// ends the valid prefix.  With `filter` the heading of a near-standstill sample is held at the previous
// published heading when it jumps, exactly as the server does with its history's last entry.
//
// order 0: libm atan2 / atan / pow / tan, as the reference.  order 1: the double-double functions the HIP kernels call
// (dftpav_amd/csrc/cr_trig.h through step_trig.h) compiled for the host.  order 2: the same calls correctly rounded from
// binary128 -- the yardstick of the device kernel.  tan(M_PI / 4) is 0x1.fffffffffffffp-1 at every order (glibc returns the
// correctly rounded value).  Everything else is IEEE arithmetic in the reference's order.
// PINNED (round 5): order 0 is bit-equal to the reference's own code -- the cited functions cut verbatim out of
// /root/reference (oracle/ref_slices.py) and compiled into oracle/_ref/libdftpav_ref_next.so (oracle/ref_next_driver.cpp) --
// on the scenarios the GPU tests of this step use (tests/test_ref_pin.py::test_states_oracle_is_bit_equal_to_GetState_and_the_servers_playback).
#include <cmath>
#include <cstdint>

#include "../oracle_shared/ref_objects.h"

using namespace ref_objects;

// coeffs: [B][Ntot][6][2], entry [k][d] = coefficient of t^k; piece_dt: [B][M]; states: [B][n_samples][8] =
// (time_stamp, x, y, angle, curvature, velocity, acceleration, steer); rows past n_valid[b] are zero.
extern "C" void oracle_sample_states(const double *coeffs, const double *piece_dt, const int *piece_nums, const int *singuls,
                                     int M, int B, double wheel_base, double t0, double sample_dt, int n_samples, int filter,
                                     int order, double *states, int *n_valid) {
  const Trig T{order};
  int Ntot = 0;
  for (int i = 0; i < M; i++) Ntot += piece_nums[i];
  for (int b = 0; b < B; b++) {
    double *out = states + (size_t)b * n_samples * 8;
    const std::vector<LocalTrajData> traj = fill_container(M, singuls, piece_nums, piece_dt + (size_t)b * M, coeffs + (size_t)b * Ntot * 12, 0.0);
    int valid = 0;
    bool have_hist = false;
    double hist_t = 0.0, hist_angle = 0.0;
    for (int k = 0; k < n_samples; k++) {
      double *s = out + 8 * k;
      for (int q = 0; q < 8; q++) s[q] = 0.0;
      State state;
      state.time_stamp = t0 + (double)k * sample_dt;
      int i = 0;
      while (i < M && traj[i].end_time <= state.time_stamp) i++;
      if (i >= M) continue; // exe_traj_index_ > final_traj_index_: nothing published
      valid = k + 1;
      traj[i].traj.GetState(state.time_stamp - traj[i].start_time, &state, wheel_base, T);
      if (filter && have_hist) FilterSingularityState(hist_t, hist_angle, &state, T);
      have_hist = true;
      hist_t = state.time_stamp;
      hist_angle = state.angle;
      s[0] = state.time_stamp; s[1] = state.vec_position.x; s[2] = state.vec_position.y; s[3] = state.angle;
      s[4] = state.curvature; s[5] = state.velocity; s[6] = state.acceleration; s[7] = state.steer;
    }
    n_valid[b] = valid;
  }
}
