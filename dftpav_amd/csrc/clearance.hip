// Clearance of solved plans on the device (docs/NEXT_ROWS.md §4.19): how close the vehicle's outline comes to the map's occupied
// cells over the samples CheckReplan walks -- the collision re-check's yes / no as a distance.
//
//   TrajPlannerServer::CheckReplan, the sampling loop   traj_planner/src/traj_server_ros.cpp:385-387
//   Trajectory::getPos / getAngle / locatePieceIdx      plan_utils/poly_traj_utils.hpp:510-528, 77-87, 179-192, 237-244
//   SemanticMapManager::CheckCollisionUsingPosAndYaw    semantic_map_manager.cc:639-662 (the probe points)
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox   common/src/common/basics/shapes.cc:110-149
//
// The samples are validate.hip's (t = 0, dt, dt + dt, ... < duration of each gear segment, from the host's table of that running
// sum; a sample's global index is validate's first_sample index) and the pose is formed statement for statement as validate_kernel
// forms it.  The probe points are footprint_hits' (footprint.h); a point's value is the distance field (distfield.hip) at its cell,
// a point outside the grid is skipped.  Per trajectory:
//   min_d2     the minimum over all probe points of all samples; DFTPAV_DIST_FAR (INT32_MAX) without a sample, with every probe
//              out of range, or on a map without an occupied cell
//   arg        the LOWEST global sample index at which min_d2 is reached; -1 when min_d2 is FAR
//   clearance  resolution * sqrt((double)min_d2), +inf for FAR
// One workgroup of 256 threads per trajectory, the samples strided over the threads, every sample visited.  A thread keeps a
// (d2, sample) pair under the lexicographic minimum -- associative and commutative, so the reduction's order does not show -- reduced
// inside a wave by cross-lane exchanges and across the four waves through LDS.  No atomics.  Two entry kernels share one device
// function, as in limits.hip: clearance_batch_kernel reads a solved batch, clearance_table_kernel the rows of the executing table.
// Neither writes what it reads.  min_d2 == 0 exactly when validate_kernel reports a collision (same samples, same points, d2 == 0
// exactly on the occupied cells), and arg is then its first_sample.
#include <hip/hip_runtime.h>

#include <climits>

#include "clearance_args.h"
#include "traj_segments.h"

namespace dftpav {

namespace {

struct ClrRed { // what lane 0 of each wave leaves for the last step
  int d[4], i[4];
};

// (b, ib) into (a, ia) under the lexicographic minimum
__device__ inline void cl_merge(int &a, int &ia, int b, int ib) {
  if (b < a || (b == a && ib < ia)) {
    a = b;
    ia = ib;
  }
}

__device__ inline double cl_metres(const ClearanceCommon &C, int d2) {
  return d2 == INT_MAX ? __longlong_as_double(0x7ff0000000000000ll) : C.grid.resolution * sqrt((double)d2);
}

// the samples of one trajectory (its segments in S, its pieces at cb) into result row `row`; returns min_d2 (thread 0 only)
__device__ inline int cl_trajectory(const ClearanceCommon &C, const SegTable &S, ClrRed &Rd, int M, const double *cb, size_t row) {
  const int tid = threadIdx.x;
  const int total = S.count[M];
  int best = INT_MAX, bi = INT_MAX;
  for (int q = tid; q < total; q += blockDim.x) {
    const int i = pe::sample_segment(S.count, M, q);
    double tt = pe::sample_time(C.tab, q - S.count[i]);
    const int idx = pe::locate_piece(S.pn[i], S.dt[i], tt);
    const double *c = cb + (size_t)(S.piece0[i] + idx) * 12;
    double px, py, vx, vy;
    pe::piece_pos(c, tt, px, py);
    pe::piece_vel(c, tt, vx, vy);
    const double sg = (double)S.sg[i];
    const double yaw = crt::atan2(sg * vy, sg * vx); // (the reference: libm; here correctly rounded, as oracle order 2)
    double cs, sn;
    crt::sincos(yaw, sn, cs);
    const int d = footprint_min_d2(C.grid, C.d2, C.fp, px, py, cs, sn);
    if (d < best) { // this thread's samples come in rising order: the first of equals stays
      best = d;
      bi = q;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) { // within the wave
    const int od = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    cl_merge(best, bi, od, oi);
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    Rd.d[wave] = best;
    Rd.i[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) { // across the four waves
    for (int w = 1; w < 4; w++) cl_merge(best, bi, Rd.d[w], Rd.i[w]);
    C.min_d2[row] = best;
    C.arg[row] = best == INT_MAX ? -1 : bi;
    C.clearance[row] = cl_metres(C, best);
    return best;
  }
  return INT_MAX;
}

} // namespace

__global__ void __launch_bounds__(256) clearance_batch_kernel(ClearanceBatchArgs A) {
  __shared__ SegTable S;
  __shared__ ClrRed Rd;
  const int b = blockIdx.x, tid = threadIdx.x;
  const DevLayout &L = A.L;
  const int M = L.M;
  if (tid == 0) fill_from_batch(S, A.C.tab, L, A.piece_dt + (size_t)b * M);
  __syncthreads();
  const size_t row = A.members ? (size_t)A.members[b / A.R] * A.R + b % A.R : (size_t)b;
  const int d2 = cl_trajectory(A.C, S, Rd, M, A.coeffs + (size_t)b * L.Ntot * 12, row);
  if (tid == 0 && A.reject && !(cl_metres(A.C, d2) >= A.min_clearance)) A.reject[b] = 1;
}

__global__ void __launch_bounds__(256) clearance_table_kernel(ClearanceTableArgs A) {
  __shared__ SegTable S;
  __shared__ ClrRed Rd;
  const int s = blockIdx.x, tid = threadIdx.x;
  const ExecTable &T = A.T;
  const int MS = T.max_seg;
  const int M = T.n_seg[s];
  if (M == 0) { // an empty slot
    if (tid == 0) {
      A.C.min_d2[s] = INT_MAX;
      A.C.arg[s] = -1;
      A.C.clearance[s] = cl_metres(A.C, INT_MAX);
    }
    return;
  }
  if (tid == 0) fill_from_slot(S, A.C.tab, T, s);
  __syncthreads();
  (void)cl_trajectory(A.C, S, Rd, M, T.coeffs + (size_t)s * MS * T.max_pieces * 12, (size_t)s);
}

hipError_t launch_clearance_batch(const ClearanceBatchArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(clearance_batch_kernel, dim3(A.B), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_clearance_table(const ClearanceTableArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(clearance_table_kernel, dim3(A.T.n_slots), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
