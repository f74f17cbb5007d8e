// TEST INFRASTRUCTURE ONLY: CPU restatement of one tick of the reference's replan loop for a table of executing plans --
// what dftpav_replan_check computes on the device (dftpav_amd/csrc/replan.hip), written from the reference's statements.
//
//   TrajPlannerServer::PlanCycleCallback, completion   traj_planner/src/traj_server_ros.cpp:149-158
//   TrajPlannerServer::PublishData, exe_traj_index_    traj_server_ros.cpp:248-252
//   TrajPlannerServer::CheckReplan                     traj_server_ros.cpp:359-402
//   TrajPlannerServer::Replan (stamp, pidx, GetState)  traj_server_ros.cpp:414, 445-461
//   TrajPlannerServer::FilterSingularityState          traj_server_ros.cpp:335-356
//   normalize_angle, kPi, kBigEPS                      common/src/common/math/calculations.cc:18-23, basics.h:76
//   Trajectory::GetState / getPos / getAngle / getTotalDuration / locatePieceIdx   plan_utils/poly_traj_utils.hpp:378-406, 425-434, 510-528
//   Piece::getPos / getdSigma / getddSigma / getAngle / getStateExpPos             poly_traj_utils.hpp:77-87, 179-211, 237-244, 303-340
//   TrajContainer::addSingulTraj, the chain of times   plan_utils/traj_container.hpp:58-73, traj_manager.cpp:618-625
//   TrajPlanner::getKinoPath, start state and control  traj_manager.cpp:74-75
//   SemanticMapManager::CheckCollisionUsingPosAndYaw   semantic_map_manager.cc:639-662
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox  common/src/common/basics/shapes.cc:110-149
//   GridMapND::CheckIfEqualUsingGlobalPosition         common/src/common/basics/semantics.cc:169-179, 214-221
//
// The program is laid out as the reference's objects are: a Piece (duration, six coefficient columns, direction), a Trajectory
// of pieces, a container entry per gear segment (duration, start_time, end_time), a server holding the executing container, its
// indices, the goal and the desired-state history.  Loops are the reference's loops (running sums t += 0.05, dl += res; early
// returns); nothing is tabulated or parallel.  order 0: the host's libm, as the reference calls it.  order 2: atan2 / atan /
// cos / sin / tan / pow(., 3) correctly rounded from binary128 (oracle/step_trig.h) -- the yardstick of the device kernel.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../oracle/step_trig.h"

namespace {

using step_trig::Trig;

constexpr double kPi = 3.14159265358979323846; // acos(-1.0), basics.h
constexpr double kBigEPS = 1e-1;               // basics.h:76

struct Vec2 {
  double x, y;
};

// plan_utils::Piece: coefficient of t^k in column k of `c` (c[k][0] x, c[k][1] y) -- the layout dftpav_batch_coeffs returns;
// the reference keeps the columns in the opposite order and walks them from the constant term upwards, as here
struct Piece {
  double duration;
  const double *c; // [6][2]
  int singul;
  Vec2 getPos(double t) const { // poly_traj_utils.hpp:77-87
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
    Vec2 d{0.0, 0.0};
    double tn = 1.0;
    int n = 1;
    for (int i = 1; i <= 5; i++) {
      d.x += n * tn * c[2 * i];
      d.y += n * tn * c[2 * i + 1];
      tn *= t;
      n++;
    }
    return d;
  }
  Vec2 getddSigma(double t) const { // :194-211
    Vec2 dd{0.0, 0.0};
    double tn = 1.0;
    int m = 1, n = 2;
    for (int i = 2; i <= 5; i++) {
      dd.x += m * n * tn * c[2 * i];
      dd.y += m * n * tn * c[2 * i + 1];
      tn *= t;
      m++;
      n++;
    }
    return dd;
  }
  double getAngle(double t, const Trig &T) const { // :237-244
    const Vec2 d = getdSigma(t);
    return T.atan2(singul * d.y, singul * d.x);
  }
};

struct State { // common::State, the fields the server reads
  double time_stamp, x, y, angle, curvature, velocity, acceleration, steer;
};

struct Trajectory {
  std::vector<Piece> pieces;
  double getTotalDuration() const { // :425-434
    double total = 0.0;
    for (size_t i = 0; i < pieces.size(); i++) total += pieces[i].duration;
    return total;
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
  Vec2 getPos(double t) const {
    const int idx = locatePieceIdx(t);
    return pieces[idx].getPos(t);
  }
  double getAngle(double t, const Trig &T) const {
    const int idx = locatePieceIdx(t);
    return pieces[idx].getAngle(t, T);
  }
  void GetState(double t, State *state, double wheel_base, const Trig &T) const { // :378-406 with getStateExpPos :303-340
    double inner_t = t;
    if (inner_t > getTotalDuration()) inner_t = getTotalDuration();
    const int idx = locatePieceIdx(inner_t);
    const Piece &p = pieces[idx];
    const Vec2 pos = p.getPos(inner_t);
    const Vec2 ds = p.getdSigma(inner_t), dds = p.getddSigma(inner_t);
    const double theta = T.atan2(p.singul * ds.y, p.singul * ds.x);
    const double vel = p.singul * std::sqrt(ds.x * ds.x + ds.y * ds.y);
    double curv, acc, phi;
    if (std::fabs(vel) < 1e-6) {
      curv = 0.0;
      acc = 0.0;
      phi = 0.0;
    } else {
      curv = (ds.x * dds.y - ds.y * dds.x) / T.cube(vel);
      acc = (ds.x * dds.x + ds.y * dds.y) / vel;
      phi = T.atan(wheel_base * curv);
    }
    state->x = pos.x;
    state->y = pos.y;
    state->angle = theta;
    state->curvature = curv;
    state->velocity = vel;
    state->acceleration = acc;
    state->steer = phi;
  }
};

struct LocalTrajData { // traj_container.hpp:28-38
  Trajectory traj;
  double duration, start_time, end_time;
};

struct Map {
  const unsigned char *data;
  int sx, sy;
  double res, ox, oy;
  bool occupied(double x, double y) const { // semantics.cc:169-179, 214-221: round to the cell, outside is not occupied
    const double cx = std::round((x - ox) / res), cy = std::round((y - oy) / res);
    if (!(cx >= 0.0 && cx < (double)sx && cy >= 0.0 && cy < (double)sy)) return false;
    return data[(int)cx + sx * (int)cy] == 80;
  }
};

struct Vehicle {
  double width, length, d_cr, wheel_base;
};

// CheckCollisionUsingPosAndYaw: the dense outline of the oriented box (edges first, then the corners), first hit returns
bool collides(const Map &map, const Vehicle &vp, double px, double py, double yaw, double res, const Trig &T) {
  const double cos_theta = T.cos(yaw), sin_theta = T.sin(yaw);
  const double x = px + vp.d_cr * cos_theta, y = py + vp.d_cr * sin_theta; // semantic_map_manager.cc:645-646
  const double L = vp.length, W = vp.width;
  const Vec2 corner[4] = {{x + 0.5 * L * cos_theta + 0.5 * W * sin_theta, y + 0.5 * L * sin_theta - 0.5 * W * cos_theta},
                          {x + 0.5 * L * cos_theta - 0.5 * W * sin_theta, y + 0.5 * L * sin_theta + 0.5 * W * cos_theta},
                          {x - 0.5 * L * cos_theta - 0.5 * W * sin_theta, y - 0.5 * L * sin_theta + 0.5 * W * cos_theta},
                          {x - 0.5 * L * cos_theta + 0.5 * W * sin_theta, y - 0.5 * L * sin_theta - 0.5 * W * cos_theta}};
  for (int e = 0; e < 4; e++) { // shapes.cc:128-143
    const Vec2 a = corner[e], b = corner[(e + 1) % 4];
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double len = std::sqrt(dx * dx + dy * dy);
    for (double dl = res; dl < len; dl += res) {
      const double f = dl / len;
      if (map.occupied(f * dx + a.x, f * dy + a.y)) return true;
    }
  }
  for (int e = 0; e < 4; e++)
    if (map.occupied(corner[e].x, corner[e].y)) return true;
  return false;
}

inline double normalize_angle(double theta) { // calculations.cc:18-23
  double tmp = theta;
  tmp -= (double)((theta >= kPi) * 2) * kPi;
  tmp += (double)((theta < -kPi) * 2) * kPi;
  return tmp;
}

// FilterSingularityState against hist.back() = (hist_stamp, hist_angle)
void filter_singularity(double hist_stamp, double hist_angle, State *s, const Trig &T) {
  const double duration = s->time_stamp - hist_stamp;
  const double max_steer = kPi / 4.0; // M_PI / 4.0: the same double
  const double singular_velocity = kBigEPS;
  const double max_orientation_rate = T.tan(max_steer) / 2.85 * singular_velocity;
  const double max_orientation_change = max_orientation_rate * duration;
  if (std::fabs(s->velocity) < singular_velocity && std::fabs(normalize_angle(s->angle - hist_angle)) > max_orientation_change)
    s->angle = hist_angle;
}

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
  const Map map{grid, size_x, size_y, resolution, origin_x, origin_y};
  const Vehicle vp{veh_width, veh_length, veh_dcr, wheel_base};
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
    State desired_state{};
    bool have_desired = false;
    desired_state.time_stamp = t_now + budget; // traj_server_ros.cpp:414
    if (n_seg[s] == 0) {
      // executing_traj_ == nullptr: CheckReplan returns true (:361); Replan plans from the ego state (:411-416)
      if (ego) {
        const double *e = ego + 6 * s;
        desired_state.x = e[0];
        desired_state.y = e[1];
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
      std::vector<LocalTrajData> executing_traj;
      {
        double world = t_start[s];
        int p0 = 0;
        for (int i = 0; i < n_seg[s]; i++) {
          LocalTrajData d;
          for (int k = 0; k < piece_nums[s * max_seg + i]; k++)
            d.traj.pieces.push_back(Piece{coeff_dt[s * max_seg + i], coeffs + ((size_t)s * max_seg * max_pieces + p0 + k) * 12, singul[s * max_seg + i]});
          p0 += piece_nums[s * max_seg + i];
          d.duration = d.traj.getTotalDuration();
          d.start_time = world;
          d.end_time = d.start_time + d.duration;
          world = d.end_time;
          executing_traj.push_back(d);
          times[((size_t)s * max_seg + i) * 3] = d.duration;
          times[((size_t)s * max_seg + i) * 3 + 1] = d.start_time;
          times[((size_t)s * max_seg + i) * 3 + 2] = d.end_time;
        }
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
        executing_traj.at(pidx).traj.GetState(t, &desired_state, vp.wheel_base, T);
        if (have_hist[s]) filter_singularity(hist[2 * s], hist[2 * s + 1], &desired_state, T); // hist.empty(): kWrongStatus, untouched
        have_desired = true;
        pidx_out[s] = pidx;
        t_local[s] = t;
      }
    }
    if (have_desired) {
      double *d = desired + 8 * s;
      d[0] = desired_state.time_stamp;
      d[1] = desired_state.x;
      d[2] = desired_state.y;
      d[3] = desired_state.angle;
      d[4] = desired_state.curvature;
      d[5] = desired_state.velocity;
      d[6] = desired_state.acceleration;
      d[7] = desired_state.steer;
      // getKinoPath, traj_manager.cpp:74-75
      start_state[4 * s] = desired_state.x;
      start_state[4 * s + 1] = desired_state.y;
      start_state[4 * s + 2] = desired_state.angle;
      start_state[4 * s + 3] = desired_state.velocity;
      start_ctrl[2 * s] = desired_state.steer;
      start_ctrl[2 * s + 1] = desired_state.acceleration;
    }
  }
}
