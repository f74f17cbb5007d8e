// TEST INFRASTRUCTURE ONLY: CPU restatement of one tick of the reference's replan loop for a table of executing plans --
// what dftpav_replan_check computes on the device (dftpav_amd/csrc/replan.hip), written from the reference's statements.
//
//   TrajPlannerServer::PlanCycleCallback, completion   traj_planner/src/traj_server_ros.cpp:149-158
//   TrajPlannerServer::PublishData, exe_traj_index_    traj_server_ros.cpp:248-252
//   TrajPlannerServer::CheckReplan                     traj_server_ros.cpp:359-402
//   TrajPlannerServer::Replan (stamp, pidx, GetState)  traj_server_ros.cpp:414, 445-461
//   TrajPlanner::getKinoPath, start state and control  traj_manager.cpp:74-75
//
// The objects it walks -- Piece, Trajectory (GetState), the container and its chain of times, the grid probe, the dense outline of
// CheckCollisionUsingPosAndYaw, normalize_angle and the rule of FilterSingularityState -- are oracle_shared/ref_objects.h's, cited there.
//
// The program is laid out as the reference's objects are: a Piece (duration, six coefficient columns, direction), a Trajectory
// of pieces, a container entry per gear segment (duration, start_time, end_time), a server holding the executing container, its
// indices, the goal and the desired-state history.  Loops are the reference's loops (running sums t += 0.05, dl += res; early
// returns); nothing is tabulated or parallel.  order 0: the host's libm, as the reference calls it.  order 2: atan2 / atan /
// cos / sin / tan / pow(., 3) correctly rounded from binary128 (oracle/step_trig.h) -- the yardstick of the device kernel.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../oracle_shared/ref_objects.h"

namespace {

using namespace ref_objects;

enum { kOccupied = 0, kComplete, kExeIndex, kCloseTurn, kNear, kTargetMoved, kCollision, kFirstSample, kReplan, kInts };

} // namespace

// Every array is padded as the device table: singul / piece_nums / coeff_dt [slots][max_seg], coeffs
// [slots][max_seg * max_pieces][6][2] (the pieces of a slot's segments one after another), end_state [slots][4], hist
// [slots][2] (stamp, angle), t_start [slots].  goals / ego may be null.  o_int [9][slots] in the order of dftpav_replan_out's
// int fields; times [slots][max_seg][3] = duration, start_time, end_time; pidx / t_local [slots]: the segment the desired state
// was read from and the time handed to GetState (-1 / 0 where none was read).
extern "C" void oracle_replan_check(const unsigned char *grid, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                                    int slots, int max_seg, int max_pieces, const int *n_seg, const int *singul, const int *piece_nums,
                                    const double *coeff_dt, const double *coeffs, const double *end_state, const double *hist,
                                    const int *have_hist, const double *t_start, double t_now, double budget, const double *goals,
                                    const double *ego, double veh_width, double veh_length, double veh_dcr, double wheel_base,
                                    double check_dt, double vertex_res, int order, int *o_int, double *desired, double *start_state,
                                    double *start_ctrl, double *times, int *pidx_out, double *t_local) {
  const Trig T{order};
  const Grid map{grid, size_x, size_y, resolution, origin_x, origin_y};
  const Vehicle vp{veh_width, veh_length, veh_dcr};
  for (int s = 0; s < slots; s++) {
    int *o[kInts];
    for (int k = 0; k < kInts; k++) {
      o[k] = o_int + (size_t)k * slots + s;
      *o[k] = 0;
    }
    *o[kFirstSample] = -1;
    for (int k = 0; k < 8; k++) desired[8 * s + k] = 0.0;
    for (int k = 0; k < 4; k++) start_state[4 * s + k] = 0.0;
    for (int k = 0; k < 2; k++) start_ctrl[2 * s + k] = 0.0;
    for (int k = 0; k < 3 * max_seg; k++) times[(size_t)s * 3 * max_seg + k] = 0.0;
    pidx_out[s] = -1;
    t_local[s] = 0.0;
    State desired_state;
    bool have_desired = false;
    desired_state.time_stamp = t_now + budget; // traj_server_ros.cpp:414
    if (n_seg[s] == 0) {
      // executing_traj_ == nullptr: CheckReplan returns true (:361); Replan plans from the ego state (:411-416)
      if (ego) {
        const double *e = ego + 6 * s;
        desired_state.vec_position.x = e[0];
        desired_state.vec_position.y = e[1];
        desired_state.angle = e[2];
        desired_state.velocity = e[3];
        desired_state.steer = e[4];
        desired_state.acceleration = e[5];
        desired_state.curvature = 0.0;
        have_desired = true;
        *o[kReplan] = 1;
      }
    } else {
      *o[kOccupied] = 1;
      // the executing container, as RunMINCOParking fills it (traj_manager.cpp:618-625)
      const size_t row = (size_t)s * max_seg;
      std::vector<LocalTrajData> executing_traj =
          fill_container(n_seg[s], singul + row, piece_nums + row, coeff_dt + row, coeffs + row * max_pieces * 12, t_start[s]);
      for (size_t i = 0; i < executing_traj.size(); i++) {
        times[(row + i) * 3] = executing_traj[i].duration;
        times[(row + i) * 3 + 1] = executing_traj[i].start_time;
        times[(row + i) * 3 + 2] = executing_traj[i].end_time;
      }
      const int final_traj_index = (int)executing_traj.size() - 1;
      const double current_time = t_now;
      if (current_time > executing_traj.at(final_traj_index).end_time) { // :150 "Mission complete"
        *o[kComplete] = 1;
      } else {
        // exe_traj_index_ as PublishData advances it (:248-252), from 0, for the clock of this tick; on the last segment it stays
        int exe_traj_index = 0;
        while (exe_traj_index < final_traj_index && executing_traj.at(exe_traj_index).end_time <= current_time) exe_traj_index += 1;
        *o[kExeIndex] = exe_traj_index;
        // ---- CheckReplan, :359-402
        const double *end_pt = (goals ? goals : end_state) + 4 * s;
        bool is_near = false, is_collision = false, is_close_turnPoint = false;
        const double cur_time = current_time;
        const Vec2 localTarget = executing_traj.back().traj.getPos(executing_traj.back().duration);
        double totaltrajTime = 0.0;
        for (size_t i = 0; i < executing_traj.size(); i++) totaltrajTime += executing_traj.at(i).duration;
        if (exe_traj_index == final_traj_index) is_close_turnPoint = false;
        else {
          if ((executing_traj.at(exe_traj_index).end_time - cur_time) < 2.5) is_close_turnPoint = true;
        }
        if ((executing_traj.back().end_time - cur_time) < 2 * totaltrajTime / 3.0) is_near = true;
        else is_near = false;
        const double ex = localTarget.x - end_pt[0], ey = localTarget.y - end_pt[1];
        const bool moved = std::sqrt(ex * ex + ey * ey) > 0.1;
        const bool early = is_near && !is_close_turnPoint && moved; // the return of :381-383
        *o[kCloseTurn] = is_close_turnPoint;
        *o[kNear] = is_near;
        *o[kTargetMoved] = moved;
        int counter = 0;
        for (size_t i = 0; i < executing_traj.size() && !is_collision; i++) { // :385-397
          for (double t = 0.0; t < executing_traj.at(i).duration; t += check_dt) {
            const Vec2 pos = executing_traj.at(i).traj.getPos(t);
            const double yaw = executing_traj.at(i).traj.getAngle(t, T);
            if (collides(map, vp, pos.x, pos.y, yaw, vertex_res, T)) {
              is_collision = true;
              *o[kFirstSample] = counter;
              break;
            }
            counter++;
          }
        }
        *o[kCollision] = is_collision;
        *o[kReplan] = early || is_collision;
        // ---- Replan, :442-461
        int pidx = exe_traj_index;
        while (true) {
          if (desired_state.time_stamp <= executing_traj.at(pidx).start_time + executing_traj.at(pidx).duration) {
            break;
          } else {
            pidx++;
            if (pidx >= (int)executing_traj.size()) {
              pidx--;
              break;
            }
          }
        }
        const double t = desired_state.time_stamp - executing_traj.at(pidx).start_time;
        executing_traj.at(pidx).traj.GetState(t, &desired_state, wheel_base, T);
        if (have_hist[s]) FilterSingularityState(hist[2 * s], hist[2 * s + 1], &desired_state, T); // hist.empty(): kWrongStatus, untouched
        have_desired = true;
        pidx_out[s] = pidx;
        t_local[s] = t;
      }
    }
    if (have_desired) {
      double *d = desired + 8 * s;
      d[0] = desired_state.time_stamp;
      d[1] = desired_state.vec_position.x;
      d[2] = desired_state.vec_position.y;
      d[3] = desired_state.angle;
      d[4] = desired_state.curvature;
      d[5] = desired_state.velocity;
      d[6] = desired_state.acceleration;
      d[7] = desired_state.steer;
      // getKinoPath, traj_manager.cpp:74-75
      start_state[4 * s] = desired_state.vec_position.x;
      start_state[4 * s + 1] = desired_state.vec_position.y;
      start_state[4 * s + 2] = desired_state.angle;
      start_state[4 * s + 3] = desired_state.velocity;
      start_ctrl[2 * s] = desired_state.steer;
      start_ctrl[2 * s + 1] = desired_state.acceleration;
    }
  }
}
