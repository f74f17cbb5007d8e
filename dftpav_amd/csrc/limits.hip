// Kinematic limits of solved plans on the device (docs/NEXT_ROWS.md §4.17): per trajectory the largest |velocity|, |longitudinal
// acceleration|, |lateral acceleration|, |curvature| and |steer| over the samples CheckReplan walks, where each is first reached,
// and whether it exceeds its limit.  The reference computes these quantities but checks none of them after the solve.
//
//   Piece::getCurv / getVel / getAcc / getLatAcc / getSteer        plan_utils/poly_traj_utils.hpp:247-300
//   Trajectory::getVel / getAcc / getLatAcc / getCurv / getSteer   poly_traj_utils.hpp:606-645
//   Trajectory::locatePieceIdx, Piece::getdSigma / getddSigma      poly_traj_utils.hpp:510-528, 179-211
//   TrajPlannerServer::CheckReplan, the sampling loop              traj_planner/src/traj_server_ros.cpp:385-386
//
// One workgroup of 256 threads per trajectory, the samples strided over the threads (t = 0, dt, dt + dt, ... < duration of each
// gear segment, taken from the host's table of that running sum exactly as validate.hip takes them; a sample's global index is
// validate's first_sample index).  A thread keeps five (value, index) pairs and a mask of violated limits; the pairs are reduced
// inside a wave by cross-lane exchanges and across the four waves through LDS.  No atomics.  The 12 coefficients of a piece
// come from L2, as in states.hip.  fp64, no contraction, sqrt(x * x + y * y) for dsigma.norm(), cr_trig.h's cube and atan where
// the reference calls pow(., 3) and std::atan: bit-identical to oracle_limits/limits_oracle.cpp in order 2.
//
// The rules of the reduction (they make the result independent of its order):
//   max_abs   the maximum of |q| over the samples; arg the LOWEST global sample index at which it is reached.
//   NaN       a NaN sample is a violation of its limit, whatever the limit, and is reported as the maximum (max_abs NaN) at
//             the FIRST NaN sample; later samples, NaN or not, do not replace it.  Both fall out of comparisons written as
//             !(a <= m): they are true for a NaN a.
//   violated  1 if !(|q| <= limit) at any sample -- |q| > limit, strictly, for numbers; a limit of +inf never fires for a number.
//   no sample max_abs 0, arg -1, nothing violated (a segment list without a sample; an empty slot of the table gives a zero row,
//             feasible included, with arg -1).
// Two entry kernels share one device function: limits_batch_kernel reads a solved batch (launch-wide DevLayout, the coefficients
// dftpav_batch_coeffs produces), limits_table_kernel the rows of the executing table (layout per slot, as replan_check_kernel).
// Neither writes what it reads.  The piece evaluators and the sample table are piece_eval.h's; the quantities are Piece::getVel
// ... getSteer, which divide by the norm and branch on it, not GetState's tail.
#include <hip/hip_runtime.h>

#include <climits>

#include "limits_args.h"
#include "traj_segments.h"

namespace dftpav {

namespace {

struct LimRed { // what lane 0 of each wave leaves for the last step
  double m[4][kLimQ];
  int i[4][kLimQ];
  int mask[4];
};

// (b, ib) into (a, ia): the larger value, a NaN before every number, the lower index between equals (and between NaNs).
// (-1.0, INT_MAX) is "no sample yet": every |q| replaces it.
__device__ inline void lm_merge(double &a, int &ia, double b, int ib) {
  const bool a_nan = a != a;
  if ((!(b <= a) && !a_nan) || ((b == a || (a_nan && b != b)) && ib < ia)) {
    a = b;
    ia = ib;
  }
}

// the samples of one trajectory (its segments in S, its pieces at cb) into result row `row`; returns feasible (thread 0 only)
__device__ inline int lm_trajectory(const LimitsCommon &C, const SegTable &S, LimRed &Rd, int M, const double *cb, size_t row) {
  const int tid = threadIdx.x;
  const int total = S.count[M];
  double m[kLimQ];
  int mi[kLimQ];
#pragma unroll
  for (int k = 0; k < kLimQ; k++) {
    m[k] = -1.0;
    mi[k] = INT_MAX;
  }
  int mask = 0;
  for (int q = tid; q < total; q += blockDim.x) {
    const int i = pe::sample_segment(S.count, M, q);
    double tt = pe::sample_time(C.tab, q - S.count[i]);
    const int idx = pe::locate_piece(S.pn[i], S.dt[i], tt);
    const double *c = cb + (size_t)(S.piece0[i] + idx) * 12;
    double vx, vy, ax, ay;
    pe::piece_vel(c, tt, vx, vy);
    pe::piece_acc(c, tt, ax, ay);
    const double sg = (double)S.sg[i];
    const double norm = sqrt(vx * vx + vy * vy); // dsigma.norm()
    double v[kLimQ];
    v[kLimVel] = sg * norm; // getVel, :263-268
    if (norm < 1e-6) {      // getAcc / getLatAcc / getCurv: their branch at rest (a NaN norm takes the other one)
      v[kLimAcc] = 0.0;
      v[kLimLatAcc] = 0.0;
      v[kLimCur] = 0.0;
    } else {
      v[kLimAcc] = sg * (vx * ax + vy * ay) / norm;                  // getAcc, :271-281
      v[kLimLatAcc] = sg * (vx * ay - vy * ax) / norm;               // getLatAcc, :283-293
      v[kLimCur] = sg * (vx * ay - vy * ax) / crt::cube_cr(norm);    // getCurv, :247-260 (the reference: pow(norm, 3) of libm)
    }
    v[kLimSteer] = crt::atan(C.wheel_base * v[kLimCur]); // getSteer, :297-300 (the reference: std::atan)
    const int back = S.sg[i] > 0 ? 0 : 1;
#pragma unroll
    for (int j = 0; j < kLimQ; j++) {
      const double a = fabs(v[j]);
      if (!(a <= m[j]) && !(m[j] != m[j])) { // this thread's samples come in rising order: the first of equals stays
        m[j] = a;
        mi[j] = q;
      }
      if (!(a <= C.lim[j][back])) mask |= 1 << j;
    }
  }
  // within the wave
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int j = 0; j < kLimQ; j++) {
      const double om = __shfl_xor(m[j], off);
      const int oi = __shfl_xor(mi[j], off);
      lm_merge(m[j], mi[j], om, oi);
    }
    mask |= __shfl_xor(mask, off);
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < kLimQ; j++) {
      Rd.m[wave][j] = m[j];
      Rd.i[wave][j] = mi[j];
    }
    Rd.mask[wave] = mask;
  }
  __syncthreads();
  // across the four waves
  if (tid < kLimQ) {
    double a = Rd.m[0][tid];
    int ia = Rd.i[0][tid];
    for (int w = 1; w < 4; w++) lm_merge(a, ia, Rd.m[w][tid], Rd.i[w][tid]);
    const bool none = ia == INT_MAX;
    const int all = Rd.mask[0] | Rd.mask[1] | Rd.mask[2] | Rd.mask[3];
    C.max_abs[row * kLimQ + tid] = none ? 0.0 : a;
    C.arg[row * kLimQ + tid] = none ? -1 : ia;
    C.violated[row * kLimQ + tid] = (all >> tid) & 1;
    if (tid == 0) {
      C.feasible[row] = all == 0 ? 1 : 0;
      return all == 0 ? 1 : 0;
    }
  }
  return 0;
}

} // namespace

__global__ void __launch_bounds__(256) limits_batch_kernel(LimitsBatchArgs A) {
  __shared__ SegTable S;
  __shared__ LimRed Rd;
  const int b = blockIdx.x, tid = threadIdx.x;
  const DevLayout &L = A.L;
  const int M = L.M;
  if (tid == 0) fill_from_batch(S, A.C.tab, L, A.piece_dt + (size_t)b * M);
  __syncthreads();
  const size_t row = A.members ? (size_t)A.members[b / A.R] * A.R + b % A.R : (size_t)b;
  const int feasible = lm_trajectory(A.C, S, Rd, M, A.coeffs + (size_t)b * L.Ntot * 12, row);
  if (tid == 0 && A.reject && !feasible) A.reject[b] = 1;
}

__global__ void __launch_bounds__(256) limits_table_kernel(LimitsTableArgs A) {
  __shared__ SegTable S;
  __shared__ LimRed Rd;
  const int s = blockIdx.x, tid = threadIdx.x;
  const ExecTable &T = A.T;
  const int MS = T.max_seg;
  const int M = T.n_seg[s];
  if (M == 0) { // an empty slot: a zero row, arg -1
    if (tid < kLimQ) {
      A.C.max_abs[(size_t)s * kLimQ + tid] = 0.0;
      A.C.arg[(size_t)s * kLimQ + tid] = -1;
      A.C.violated[(size_t)s * kLimQ + tid] = 0;
      if (tid == 0) A.C.feasible[s] = 0;
    }
    return;
  }
  if (tid == 0) fill_from_slot(S, A.C.tab, T, s);
  __syncthreads();
  (void)lm_trajectory(A.C, S, Rd, M, T.coeffs + (size_t)s * MS * T.max_pieces * 12, (size_t)s);
}

hipError_t launch_limits_batch(const LimitsBatchArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(limits_batch_kernel, dim3(A.B), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_limits_table(const LimitsTableArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(limits_table_kernel, dim3(A.T.n_slots), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
