// One tick of the replan loop for every executing plan of a planner's table (docs/NEXT_ROWS.md §4.15).
//
//   TrajPlannerServer::PlanCycleCallback, completion  traj_planner/src/traj_server_ros.cpp:149-158
//   TrajPlannerServer::PublishData, exe_traj_index_   traj_server_ros.cpp:248-252
//   TrajPlannerServer::CheckReplan                    traj_server_ros.cpp:359-402
//   TrajPlannerServer::Replan, desired state          traj_server_ros.cpp:414, 445-461
//   TrajPlannerServer::FilterSingularityState         traj_server_ros.cpp:335-356
//   Trajectory::GetState / locatePieceIdx             plan_utils/poly_traj_utils.hpp:378-406, 510-528
//   Piece::getPos / getdSigma / getddSigma / getStateExpPos   poly_traj_utils.hpp:77-87, 179-211, 303-340
//   TrajPlanner::getKinoPath, start state and control traj_manager.cpp:74-75
//   SemanticMapManager::CheckCollisionUsingPosAndYaw  semantic_map_manager.cc:639-662, shapes.cc:110-149
//
// One workgroup of 256 threads per slot; the layout (segments, pieces, directions) is read from the slot's own row of the
// table, so plans of different layouts are checked in one launch.  Thread 0 makes the scalar decisions in the reference's
// statements and order and reads the desired state; all threads then take the collision samples of CheckReplan exactly as
// validate.hip takes them (tabulated running sums, an atomic minimum over the samples), so collision / first_sample are the
// bits dftpav_batch_validate gives for the same plan.  The read-out and the outline walk are piece_eval.h's and footprint.h's,
// as in validate.hip / states.hip: those kernels read a launch-wide DevLayout, this one a row of the table.
// fp64, no contraction, cr_trig.h wherever the reference calls libm: bit-identical to oracle_replan/replan_oracle.cpp in
// order 2.  The kernel writes nothing into the table.
//
// publish_kernel, further down, is the other half of the server's loop: the 100 Hz publisher (PublishData, traj_server_ros.cpp:195-318).
#include <hip/hip_runtime.h>

#include "plan_args.h"

namespace dftpav {

__global__ void __launch_bounds__(256) replan_check_kernel(ReplanArgs A) {
  __shared__ int s_count[kMaxSeg + 1];  // samples of the segments before segment i
  __shared__ int s_piece0[kMaxSeg + 1]; // first piece of segment i in the slot's row
  __shared__ int s_first, s_go, s_rule;
  const int s = blockIdx.x, tid = threadIdx.x;
  const ExecTable &T = A.T;
  const int S = T.n_slots, MS = T.max_seg;
  const int *pn = T.piece_nums + (size_t)s * MS, *sg = T.singul + (size_t)s * MS;
  const double *dtv = T.coeff_dt + (size_t)s * MS;
  const double *cb = T.coeffs + (size_t)s * MS * T.max_pieces * 12;
  const int M = T.n_seg[s];
  if (tid == 0) {
    const double *dur = T.duration + (size_t)s * MS, *st = T.start_time + (size_t)s * MS, *en = T.end_time + (size_t)s * MS;
    int o[kRcInts];
    for (int k = 0; k < kRcInts; k++) o[k] = 0;
    o[kRcFirstSample] = -1;
    double des[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool have_des = false;
    int go = 0, rule = 0;
    const double stamp = A.t_now + A.budget; // traj_server_ros.cpp:414
    if (M == 0) {
      // executing_traj_ == nullptr: CheckReplan returns true (:361), Replan plans from the ego state with the stamp (:411-416)
      if (A.ego) {
        const double *e = A.ego + 6 * (size_t)s;
        o[kRcReplan] = 1;
        des[0] = stamp; des[1] = e[0]; des[2] = e[1]; des[3] = e[2]; des[4] = 0.0; des[5] = e[3]; des[6] = e[5]; des[7] = e[4];
        have_des = true;
      }
    } else {
      o[kRcOccupied] = 1;
      const int last = M - 1;
      if (A.t_now > en[last]) { // :150
        o[kRcComplete] = 1;
      } else {
        // exe_traj_index_, :248-252, derived from t_now (at t_now == the last end_time it stays on the last segment)
        int exe = 0;
        while (exe < last && en[exe] <= A.t_now) exe++;
        o[kRcExeIndex] = exe;
        int acc = 0, p0 = 0;
        for (int i = 0; i < M; i++) {
          s_piece0[i] = p0;
          p0 += pn[i];
          s_count[i] = acc;
          acc += pe::samples_below(A.tab, dur[i]);
        }
        s_count[M] = acc;
        s_piece0[M] = p0;
        // CheckReplan, :366-383
        const double *goal = (A.goals ? A.goals : T.end_state) + 4 * (size_t)s;
        double ltx, lty;
        {
          double tt = dur[last];
          const int idx = pe::locate_piece(pn[last], dtv[last], tt);
          pe::piece_pos(cb + (size_t)(s_piece0[last] + idx) * 12, tt, ltx, lty);
        }
        double total = 0.0;
        for (int i = 0; i < M; i++) total += dur[i];
        int close_turn = 0;
        if (exe != last) {
          if ((en[exe] - A.t_now) < 2.5) close_turn = 1;
        }
        const int near = (en[last] - A.t_now) < 2 * total / 3.0 ? 1 : 0;
        const double gx = ltx - goal[0], gy = lty - goal[1];
        const int moved = sqrt(gx * gx + gy * gy) > 0.1 ? 1 : 0;
        o[kRcCloseTurn] = close_turn;
        o[kRcNear] = near;
        o[kRcTargetMoved] = moved;
        rule = (near && !close_turn && moved) ? 1 : 0;
        // Replan, :445-458: the segment the stamp falls into, walked from exe_traj_index_
        int pidx = exe;
        while (true) {
          if (stamp <= st[pidx] + dur[pidx]) {
            break;
          } else {
            pidx++;
            if (pidx >= M) {
              pidx--;
              break;
            }
          }
        }
        const double t = stamp - st[pidx];
        // Trajectory::GetState, poly_traj_utils.hpp:378-406
        double inner = t;
        if (inner > dur[pidx]) inner = dur[pidx];
        const int idx = pe::locate_piece(pn[pidx], dtv[pidx], inner);
        const double *c = cb + (size_t)(s_piece0[pidx] + idx) * 12;
        double px, py, vx, vy, ax, ay;
        pe::piece_pos(c, inner, px, py);
        pe::piece_vel(c, inner, vx, vy);
        pe::piece_acc(c, inner, ax, ay);
        pe::StateTail g = pe::get_state_tail(vx, vy, ax, ay, (double)sg[pidx], A.wheel_base);
        if (T.have_hist[s]) { // FilterSingularityState against desired_state_hist_.back(), :335-356, :460
          const double hist_angle = T.hist[2 * (size_t)s + 1];
          if (pe::filter_singularity(g.angle, g.vel, hist_angle, stamp - T.hist[2 * (size_t)s])) g.angle = hist_angle;
        }
        des[0] = stamp; des[1] = px; des[2] = py; des[3] = g.angle; des[4] = g.curv; des[5] = g.vel; des[6] = g.acc; des[7] = g.steer;
        have_des = true;
        go = 1;
      }
    }
    for (int k = 0; k < kRcInts; k++) A.o_int[(size_t)k * S + s] = o[k];
    for (int k = 0; k < 8; k++) A.desired[8 * (size_t)s + k] = des[k];
    // getKinoPath, traj_manager.cpp:74-75: start_state << vec_position, angle, velocity; init_ctrl << steer, acceleration
    A.start_state[4 * (size_t)s] = have_des ? des[1] : 0.0;
    A.start_state[4 * (size_t)s + 1] = have_des ? des[2] : 0.0;
    A.start_state[4 * (size_t)s + 2] = have_des ? des[3] : 0.0;
    A.start_state[4 * (size_t)s + 3] = have_des ? des[5] : 0.0;
    A.start_ctrl[2 * (size_t)s] = have_des ? des[7] : 0.0;
    A.start_ctrl[2 * (size_t)s + 1] = have_des ? des[6] : 0.0;
    s_first = 0x7fffffff;
    s_go = go;
    s_rule = rule;
  }
  __syncthreads();
  if (!s_go) return; // an empty or completed slot: nothing else is computed (the whole workgroup leaves)
  // the collision loop of CheckReplan, :385-397, sample by sample as validate.hip
  const int total = s_count[M];
  for (int q = tid; q < total; q += blockDim.x) {
    const int i = pe::sample_segment(s_count, M, q);
    double tt = pe::sample_time(A.tab, q - s_count[i]);
    const int idx = pe::locate_piece(pn[i], dtv[i], tt);
    const double *c = cb + (size_t)(s_piece0[i] + idx) * 12;
    double px, py, vx, vy;
    pe::piece_pos(c, tt, px, py);
    pe::piece_vel(c, tt, vx, vy);
    const double sgn = (double)sg[i];
    const double yaw = crt::atan2(sgn * vy, sgn * vx);
    double cs, sn;
    crt::sincos(yaw, sn, cs);
    const bool hit = footprint_hits(A.grid, A.fp, px, py, cs, sn);
    if (hit) atomicMin(&s_first, q);
  }
  __syncthreads();
  if (tid == 0) {
    const bool any = s_first != 0x7fffffff;
    A.o_int[(size_t)kRcCollision * S + s] = any ? 1 : 0;
    A.o_int[(size_t)kRcFirstSample * S + s] = any ? s_first : -1;
    A.o_int[(size_t)kRcReplan * S + s] = (s_rule || any) ? 1 : 0; // the early return of :381-383, then the loop
  }
}

// The winners of a dftpav_plan_queries call into slots of the table: one workgroup per (query, slot) pair copies the pieces;
// thread 0 copies the layout row and chains the times as TrajContainer::addSingulTraj does (traj_container.hpp:58-73,
// traj_manager.cpp:618-625): duration = the piece durations summed in order, end = start + duration, the next segment
// starts at that end.
__global__ void __launch_bounds__(256) exec_adopt_kernel(ExecAdoptArgs A) {
  const int q = A.pairs[2 * blockIdx.x], s = A.pairs[2 * blockIdx.x + 1], tid = threadIdx.x;
  const ExecTable &T = A.T;
  const int MS = T.max_seg;
  const size_t row = (size_t)MS * T.max_pieces * 12;
  const double *src = A.q_coeffs + (size_t)q * row;
  double *dst = T.coeffs + (size_t)s * row;
  for (size_t k = tid; k < row; k += blockDim.x) dst[k] = src[k];
  if (tid == 0) {
    const int M = A.q_n_seg[q];
    T.n_seg[s] = M;
    double world = A.t_start;
    for (int i = 0; i < MS; i++) {
      const bool used = i < M;
      const int N = used ? A.q_piece_nums[(size_t)q * MS + i] : 0;
      const double dtp = used ? A.q_dt[(size_t)q * MS + i] : 0.0;
      T.singul[(size_t)s * MS + i] = used ? A.q_singul[(size_t)q * MS + i] : 0;
      T.piece_nums[(size_t)s * MS + i] = N;
      T.coeff_dt[(size_t)s * MS + i] = dtp;
      const double d = pe::segment_duration(N, dtp);
      T.duration[(size_t)s * MS + i] = used ? d : 0.0;
      T.start_time[(size_t)s * MS + i] = used ? world : 0.0;
      T.end_time[(size_t)s * MS + i] = used ? world + d : 0.0;
      if (used) world = world + d;
    }
    for (int k = 0; k < 4; k++) T.end_state[4 * (size_t)s + k] = A.q_goal[4 * (size_t)q + k];
    if (A.desired) { // desired_state_hist_.push_back(desired_state), traj_server_ros.cpp:461
      T.hist[2 * (size_t)s] = A.desired[8 * (size_t)s];
      T.hist[2 * (size_t)s + 1] = A.desired[8 * (size_t)s + 3];
      T.have_hist[s] = 1;
    } else {
      T.hist[2 * (size_t)s] = 0.0;
      T.hist[2 * (size_t)s + 1] = 0.0;
      T.have_hist[s] = 0;
    }
  }
}

// K ticks of the 100 Hz publisher for every slot of the table (docs/NEXT_ROWS.md §4.16).
//
//   TrajPlannerServer::PublishData, the trajectory feedback   traj_server_ros.cpp:240-289
//   TrajPlannerServer::FilterSingularityState                 traj_server_ros.cpp:335-356
//   Trajectory::GetState / locatePieceIdx                     poly_traj_utils.hpp:378-406, 510-528
//
// One workgroup of kPubChunk threads per slot takes the ticks in chunks of kPubChunk.  The two recurrences of a tick are serial and
// cheap and run on thread 0: the index walk (:248-252, compares only) before the evaluation, the filter chain (:257-258, a
// subtraction, normalize_angle and a compare against the previous filtered angle and stamp) after it.  The state evaluation (double-double
// atan2 / atan) is independent per tick once its segment is known: every thread takes one tick.  exe_index and the history back are
// carried from chunk to chunk in LDS and written back at the end.  The idle branch (:210-237) is not reproduced: such ticks publish nothing
// and change nothing.  The table is not written.
__global__ void __launch_bounds__(kPubChunk) publish_kernel(PublishArgs A) {
  __shared__ int s_piece0[kMaxSeg + 1];
  __shared__ int s_seg[kPubChunk];      // the segment of tick j of the chunk, -1: nothing is published
  __shared__ double s_ang[kPubChunk], s_vel[kPubChunk];
  __shared__ int s_code[kPubChunk];
  __shared__ int s_exe, s_have;
  __shared__ double s_hist[2];
  const int s = blockIdx.x, tid = threadIdx.x;
  const ExecTable &T = A.T;
  const int S = T.n_slots, MS = T.max_seg;
  const int *pn = T.piece_nums + (size_t)s * MS, *sg = T.singul + (size_t)s * MS;
  const double *dtv = T.coeff_dt + (size_t)s * MS;
  const double *cb = T.coeffs + (size_t)s * MS * T.max_pieces * 12;
  const double *dur = T.duration + (size_t)s * MS, *st = T.start_time + (size_t)s * MS, *en = T.end_time + (size_t)s * MS;
  const int M = T.n_seg[s];
  if (tid == 0) {
    int p0 = 0;
    for (int i = 0; i < M; i++) {
      s_piece0[i] = p0;
      p0 += pn[i];
    }
    s_piece0[M] = p0;
    s_exe = A.P.exe_index[s];
    s_have = A.P.have[s];
    s_hist[0] = A.P.hist[2 * (size_t)s];
    s_hist[1] = A.P.hist[2 * (size_t)s + 1];
  }
  for (int k0 = 0; k0 < A.K; k0 += kPubChunk) {
    __syncthreads(); // the set-up above; the previous chunk's reads of s_seg / s_code / s_ang
    const int nk = min(kPubChunk, A.K - k0);
    if (tid == 0) { // the index walk
      int exe = s_exe;
      const int last = M - 1; // final_traj_index_
      for (int j = 0; j < nk; j++) {
        int seg = -1;
        // :210-211 executing_traj_ == nullptr || exe_traj_index_ > final_traj_index_ || duration < 1e-5: the idle branch, not reproduced
        if (M > 0 && exe >= 0 && exe <= last && !(dur[exe] < 1e-5)) {
          const double t = A.t[k0 + j];
          if (en[exe] <= t) exe += 1; // :248-250, one step per tick
          if (exe <= last) seg = exe; // :251-252
        }
        s_seg[j] = seg;
      }
      s_exe = exe;
    }
    __syncthreads();
    const int k = k0 + tid;
    const int seg = tid < nk ? s_seg[tid] : -1;
    double row[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (seg >= 0) {
      const double t = A.t[k];
      // Trajectory::GetState(t - start_time), poly_traj_utils.hpp:378-406
      double inner = t - st[seg];
      if (inner > dur[seg]) inner = dur[seg];
      const int idx = pe::locate_piece(pn[seg], dtv[seg], inner);
      const double *c = cb + (size_t)(s_piece0[seg] + idx) * 12;
      double px, py, vx, vy, ax, ay;
      pe::piece_pos(c, inner, px, py);
      pe::piece_vel(c, inner, vx, vy);
      pe::piece_acc(c, inner, ax, ay);
      const pe::StateTail g = pe::get_state_tail(vx, vy, ax, ay, (double)sg[seg], A.wheel_base);
      row[0] = t; row[1] = px; row[2] = py; row[3] = g.angle; row[4] = g.curv; row[5] = g.vel; row[6] = g.acc; row[7] = g.steer;
      s_ang[tid] = g.angle;
      s_vel[tid] = g.vel;
    }
    __syncthreads();
    if (tid == 0) { // the filter chain: FilterSingularityState against ctrl_state_hist_.back(), then push_back (:257-258)
      int have = s_have;
      double h_stamp = s_hist[0], h_angle = s_hist[1];
      for (int j = 0; j < nk; j++) {
        int code = 0;
        if (s_seg[j] >= 0) {
          const double t = A.t[k0 + j];
          double angle = s_ang[j];
          code = 1;
          if (have) {
            if (pe::filter_singularity(angle, s_vel[j], h_angle, t - h_stamp)) {
              angle = h_angle;
              code = 2;
            }
          }
          s_ang[j] = angle;
          h_stamp = t;
          h_angle = angle;
          have = 1;
        }
        s_code[j] = code;
      }
      s_have = have;
      s_hist[0] = h_stamp;
      s_hist[1] = h_angle;
    }
    __syncthreads();
    if (tid < nk) {
      const int code = s_code[tid];
      if (code) row[3] = s_ang[tid];
      if (A.states) {
        double *o = A.states + ((size_t)k * S + s) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = row[q];
      }
      if (A.published) A.published[(size_t)k * S + s] = code;
    }
  }
  __syncthreads();
  if (tid == 0) {
    A.P.exe_index[s] = s_exe;
    A.P.have[s] = s_have;
    A.P.hist[2 * (size_t)s] = s_hist[0];
    A.P.hist[2 * (size_t)s + 1] = s_hist[1];
  }
}

// exe_traj_index_ = 0 for the slots an adoption fills (traj_server_ros.cpp:177); ctrl_state_hist_ stays (the reference keeps it across
// replans), is dropped, or is seeded from the slot's desired state: one thread per adopted pair
__global__ void __launch_bounds__(256) pub_reset_kernel(PubResetArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int s = A.pairs[2 * i + 1], mode = A.mode[i];
  A.P.exe_index[s] = 0;
  if (mode == kPubDrop) {
    A.P.hist[2 * (size_t)s] = 0.0;
    A.P.hist[2 * (size_t)s + 1] = 0.0;
    A.P.have[s] = 0;
  } else if (mode == kPubSeed) {
    A.P.hist[2 * (size_t)s] = A.desired[8 * (size_t)s];
    A.P.hist[2 * (size_t)s + 1] = A.desired[8 * (size_t)s + 3];
    A.P.have[s] = 1;
  }
}

hipError_t launch_replan_check(const ReplanArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(replan_check_kernel, dim3(A.T.n_slots), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_exec_adopt(const ExecAdoptArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(exec_adopt_kernel, dim3(A.n), dim3(256), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_publish(const PublishArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(publish_kernel, dim3(A.T.n_slots), dim3(kPubChunk), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_pub_reset(const PubResetArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(pub_reset_kernel, dim3((A.n + 255) / 256), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
