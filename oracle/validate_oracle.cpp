// TEST INFRASTRUCTURE ONLY (see oracle/dftpav_oracle.h): CPU restatement of the step that consumes the
// solve path's result, SURVEY.md §8(f)-2 — the sampled collision re-check of an optimised trajectory.
//
//   TrajPlannerServer::CheckReplan, collision part   traj_planner/src/traj_server_ros.cpp:385-397
//
// Trajectory::getPos / getAngle, the container of chained segments and CheckCollisionUsingPosAndYaw with the grid probe are
// oracle_shared/ref_objects.h's, cited there.
//
// Every segment of a trajectory is sampled at t = 0, dt, dt + dt, ... < duration; at each sample the
// vehicle's outline (dense points along the four edges, then the corners) is tested against the
// occupancy grid.  The result per trajectory is whether any sample collides and the index of the first
// one (counted over the segments in order).
//
// order 0: libm cos / sin / atan2, as the reference.  order 1: the double-double functions the HIP kernels call
// (dftpav_amd/csrc/cr_trig.h through step_trig.h) compiled for the host.  order 2: the same calls correctly rounded from
// binary128 -- the yardstick of the device kernel.  Everything else is IEEE arithmetic in the reference's order.
// PINNED (round 5): order 0 is bit-equal to the reference's own code -- the cited functions cut verbatim out of
// /root/reference (oracle/ref_slices.py) and compiled into oracle/_ref/libdftpav_ref_next.so (oracle/ref_next_driver.cpp) --
// on the scenarios the GPU tests of this step use (tests/test_ref_pin.py::test_validate_oracle_is_bit_equal_to_CheckReplan).
#include <cmath>
#include <cstdint>

#include "../oracle_shared/ref_objects.h"

using namespace ref_objects;

// coeffs: [B][Ntot][6][2], entry [k][d] = coefficient of s^k (what dftpav_batch_coeffs / oracle coeffs return);
// piece_dt: [B][M] piece duration of each segment
extern "C" void oracle_validate_trajectories(const unsigned char *grid, int size_x, int size_y, double resolution, double origin_x,
                                             double origin_y, const double *coeffs, const double *piece_dt, const int *piece_nums,
                                             const int *singuls, int M, int B, double veh_width, double veh_length,
                                             double veh_dcr, double sample_dt, double vertex_res, int order, int *collision,
                                             int *first_sample) {
  const Trig T{order};
  const Grid map{grid, size_x, size_y, resolution, origin_x, origin_y};
  const Vehicle vp{veh_width, veh_length, veh_dcr};
  int Ntot = 0;
  for (int i = 0; i < M; i++) Ntot += piece_nums[i];
  for (int b = 0; b < B; b++) {
    const std::vector<LocalTrajData> traj = fill_container(M, singuls, piece_nums, piece_dt + (size_t)b * M, coeffs + (size_t)b * Ntot * 12, 0.0);
    int hit = 0, first = -1, counter = 0;
    for (size_t i = 0; i < traj.size() && !hit; i++) {
      for (double t = 0.0; t < traj[i].duration; t += sample_dt, counter++) { // traj_server_ros.cpp:386-387
        const Vec2 pos = traj[i].traj.getPos(t);
        const double yaw = traj[i].traj.getAngle(t, T);
        if (collides(map, vp, pos.x, pos.y, yaw, vertex_res, T)) {
          hit = 1;
          first = counter;
          break;
        }
      }
    }
    collision[b] = hit;
    first_sample[b] = first;
  }
}
