// The device glue of dftpav_plan_queries (include/dftpav_hip.h): TrajPlanner::RunOnceParking from getKinoPath on
// (traj_manager.cpp:194-217) for a batch of queries whose searched paths have different layouts.  The stages themselves are the
// kernels of search.hip, frontend.hip, corridor.hip, solver_ref*.hip and validate.hip; what is here sits between them:
//
//   plan_paths_kernel    a query without a usable searched path (no path, arrived, a path longer than its padding) gets a
//                        two-pose stand-in, so that the resampling kernel can run over every query of the call; its rows are
//                        never read
//   plan_pack_kernel     once per layout group: gathers the group's queries out of the padded front-end arrays into the batch's
//                        own arrays, draws the restarts (the generator of restart.hip, keyed by (seed, query index in the call,
//                        restart)) and does the set-up half of OptimizeTrajectory that dftpav_batch_upload does on the host
//                        (traj_optimizer.cpp:30-33 mini_T, :65-76 clamping of the boundary |v| and |a|, :96-115 x0 with
//                        RealT2VirtualT, the junction position and its angle); gathers the constraint-point poses
//   plan_select_kernel   per query the cheapest restart that succeeded, does not collide and carries no reject flag, and its x /
//                        coefficients into the compact per-query outputs
//   penalty_gate_kernel  with dftpav_planner_set_penalty_filter, in front of the selection: per (query, restart) the five terms of
//                        the solution's cost into their row, and the reject flag set where a penalty sum is above its cap
//
// The reject flags are one array per call, cleared by the host: each post-solve filter (limits.hip, clearance.hip, the gate) only
// sets the flag of a trajectory it rejects, by the one thread that owns that trajectory, so their order does not show.
//
// fp64, no contraction, the host code's statements in the host code's order; atan2 is the correctly rounded one (cr_trig.h),
// as the oracle's order 2.  Plain vector stores only.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "traj_math.h"
#include "cr_trig.h"
#include "restart_rng.h"
#include "plan_args.h"

namespace dftpav {

__global__ void __launch_bounds__(256) plan_paths_kernel(const int *__restrict__ status, const int *__restrict__ path_len,
                                                         const int *__restrict__ skip, int n, int max_path, double *__restrict__ paths,
                                                         int *__restrict__ fe_len) {
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q >= n) return;
  const int len = path_len[q];
  if (status[q] == DFTPAV_SEARCH_REACH_END && len >= 2 && len <= max_path && skip[q] == 0) {
    fe_len[q] = len;
    return;
  }
  double *P = paths + (size_t)q * max_path * 3; // max_path >= 2
  P[0] = 0.0; P[1] = 0.0; P[2] = 0.0;
  P[3] = 1.0; P[4] = 0.0; P[5] = 0.0;
  fe_len[q] = 2;
}

// RealT2VirtualT, traj_optimizer.cpp:360-369 (capi.cpp: real_to_virtual)
__device__ inline double plan_real_to_virtual(double rt, double mini_T) {
  return rt > 1.0 + mini_T ? (sqrt(2.0 * rt - 1.0 - 2 * mini_T) - 1.0) : (1.0 - sqrt(2.0 / (rt - mini_T) - 1.0));
}
// traj_optimizer.cpp:65-76 (capi.cpp: clamp_col)
__device__ inline void plan_clamp(double &c0, double &c1, double lim) {
  const double nrm = sqrt(c0 * c0 + c1 * c1);
  if (nrm >= lim) {
    const double nx = c0 / nrm, ny = c1 / nrm;
    c0 = nx * (lim - 1.0e-2);
    c1 = ny * (lim - 1.0e-2);
  }
}

// one workgroup per member of the group
__global__ void __launch_bounds__(256) plan_pack_kernel(PlanPackArgs A) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int q = A.members[m];
  const DevLayout &L = A.L;
  const int M = L.M, n = L.n, R = A.n_restarts;
  const size_t MS = (size_t)A.fe.max_seg, MP = (size_t)A.fe.max_pieces, MST = (size_t)A.fe.max_states;
  // the constraint-point poses of the hypothesis, segment after segment (statelist of getRectangleConst)
  for (int p = tid; p < L.Npts; p += 256) {
    int i = 0;
    while (i + 1 < M && p >= L.seg_pt0[i + 1]) i++;
    const int local = p - L.seg_pt0[i];
    const double *src = A.fe.states + (((size_t)q * MS + i) * MST + local) * 3;
    double *dst = A.poses + ((size_t)m * L.Npts + p) * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
  }
  const int nw = L.x_tau0 / 2; // inner waypoints of all segments
  const int per = nw + 2 * M;  // work items per trajectory: a waypoint, a duration, a segment's boundary states
  for (int w = tid; w < R * per; w += 256) {
    const int r = w / per, k = w - r * per;
    const size_t t = (size_t)m * R + r;
    double *x = A.x0 + t * n;
    const unsigned long long s0 = restart_stream(A.seed, q, r);
    if (k < nw) { // restart.hip: waypoint k of the flattened inner points
      int i = 0;
      while (i + 1 < M && 2 * k >= L.seg_x0[i + 1]) i++;
      const int j = k - L.seg_x0[i] / 2;
      const double *src = A.fe.inner_pts + (((size_t)q * MS + i) * (MP - 1) + j) * 2;
      const double bx = src[0], by = src[1];
      double dx = 0.0, dy = 0.0;
      if (r > 0) {
        const double u1 = u01(s0, 2ull * k), u2 = u01(s0, 2ull * k + 1);
        const double rad = sqrt(-2.0 * p_log(u1)), ang = 6.283185307179586476925 * u2;
        dx = A.sigma * (rad * p_cos(ang));
        dy = A.sigma * (rad * p_sin(ang));
      }
      x[2 * k] = bx + dx;
      x[2 * k + 1] = by + dy;
    } else if (k < nw + M) { // restart.hip: the duration of segment i; then RealT2VirtualT
      const int i = k - nw;
      const double dur = A.fe.piece_dt[(size_t)q * MS + i] * A.fe.piece_nums[(size_t)q * MS + i];
      double f = 1.0;
      if (r > 0) f = A.lo + (A.hi - A.lo) * u01(s0, 2ull * nw + i);
      double T = dur * f;
      if (T < A.mini_T) {       // traj_optimizer.cpp:30-33: OptimizeTrajectory refuses; the query is reported without a plan,
        A.mini_t_flag[q] = 1;   // and this trajectory solves a stand-in duration so that its solve stays finite
        T = 1.0;
      }
      x[L.x_tau0 + i] = plan_real_to_virtual(T, A.mini_T);
    } else { // boundary states of segment i, clamped; the junction behind it
      const int i = k - nw - M;
      const double *Is = A.fe.ini_states + ((size_t)q * MS + i) * 6, *Fs = A.fe.fin_states + ((size_t)q * MS + i) * 6;
      double I0 = Is[0], I1 = Is[1], I2 = Is[2], I3 = Is[3], I4 = Is[4], I5 = Is[5];
      double F0 = Fs[0], F1 = Fs[1], F2 = Fs[2], F3 = Fs[3], F4 = Fs[4], F5 = Fs[5];
      const int back = L.singuls[i] > 0 ? 0 : 1;
      const double mv = A.max_vel[back], ma = A.max_acc[back];
      plan_clamp(I2, I3, mv);
      plan_clamp(F2, F3, mv);
      plan_clamp(I4, I5, ma);
      plan_clamp(F4, F5, ma);
      double *Io = A.iniS + (t * M + i) * 6, *Fo = A.finS + (t * M + i) * 6;
      Io[0] = I0; Io[1] = I1; Io[2] = I2; Io[3] = I3; Io[4] = I4; Io[5] = I5;
      Fo[0] = F0; Fo[1] = F1; Fo[2] = F2; Fo[3] = F3; Fo[4] = F4; Fo[5] = F5;
      if (i < M - 1) {
        x[L.x_gear0 + 2 * i + 0] = F0;
        x[L.x_gear0 + 2 * i + 1] = F1;
        x[L.x_ang0 + i] = crt::atan2(F3, F2);
      }
    }
  }
}

// one wave per member: a lane takes the restarts r = lane, lane + 64, ... in rising order, then the lanes are reduced
__global__ void __launch_bounds__(64) plan_select_kernel(PlanSelectArgs A) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int q = A.members ? A.members[m] : m;
  const int R = A.R;
  double best = 0.0;
  int idx = INT_MAX; // none yet
  for (int r = lane; r < R; r += 64) {
    const size_t t = (size_t)m * R + r, o = (size_t)q * R + r;
    const double c = A.cost[t];
    const int suc = A.success[t], col = A.collision[t];
    if (suc != 0 && col == 0 && (A.reject == nullptr || A.reject[t] == 0) && c == c && (idx == INT_MAX || c < best)) {
      best = c;
      idx = r;
    }
    if (A.r_cost) {
      A.r_cost[o] = c;
      A.r_status[o] = A.status[t];
      A.r_success[o] = suc;
      A.r_iters[o] = A.iters[t];
      A.r_evals[o] = A.evals[t];
      A.r_collision[o] = col;
      A.r_first_sample[o] = A.first_sample[t];
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double oc = __shfl_xor(best, off);
    const int oi = __shfl_xor(idx, off);
    if (oi != INT_MAX && (idx == INT_MAX || oc < best || (oc == best && oi < idx))) {
      best = oc;
      idx = oi;
    }
  }
  if (lane == 0) A.winner[q] = idx == INT_MAX ? -1 : idx;
  if (idx == INT_MAX) return; // the compact rows stay zero
  const size_t t = (size_t)m * R + idx;
  if (lane == 0 && A.w_cost) {
    A.w_cost[q] = best;
    A.w_iters[q] = A.iters[t];
  }
  if (A.w_x)
    for (int k = lane; k < A.n; k += 64) A.w_x[(size_t)q * A.x_stride + k] = A.x[t * A.n + k];
  if (A.w_coef)
    for (int k = lane; k < A.n_coef; k += 64) A.w_coef[(size_t)q * A.coef_stride + k] = A.coef[t * A.n_coef + k];
  if (A.w_dt)
    for (int k = lane; k < A.M; k += 64) A.w_dt[(size_t)q * A.dt_stride + k] = A.dt[t * A.M + k];
}

// The residual-penalty gate between the terms launch and the selection.  !(t <= cap): a NaN term is rejected, +inf caps reject
// no finite term, -0.0 <= 0.0 holds.
__global__ void __launch_bounds__(256) penalty_gate_kernel(PenaltyGateArgs A) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= A.n) return;
  const size_t row = A.members ? (size_t)A.members[t / A.R] * A.R + t % A.R : (size_t)t;
  const double *tm = A.terms + (size_t)t * kCostTerms;
  if (A.r_terms)
    for (int k = 0; k < kCostTerms; k++) A.r_terms[row * kCostTerms + k] = tm[k];
  const int rejected = (!(tm[kTermCorridor] <= A.cap_corridor) | !(tm[kTermSurround] <= A.cap_surround) | !(tm[kTermFeas] <= A.cap_feas)) ? 1 : 0;
  if (A.r_rejected) A.r_rejected[row] = rejected;
  if (A.reject && rejected) A.reject[t] = 1;
}

hipError_t launch_plan_paths(const int *status, const int *path_len, const int *skip, int n, int max_path, double *paths, int *fe_len,
                             hipStream_t stream) {
  hipLaunchKernelGGL(plan_paths_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, status, path_len, skip, n, max_path, paths, fe_len);
  return hipGetLastError();
}
hipError_t launch_plan_pack(const PlanPackArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(plan_pack_kernel, dim3(A.n_members), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_penalty_gate(const PenaltyGateArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(penalty_gate_kernel, dim3((A.n + 255) / 256), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_plan_select(const PlanSelectArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(plan_select_kernel, dim3(A.n_members), dim3(64), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
