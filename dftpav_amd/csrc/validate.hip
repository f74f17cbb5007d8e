// Collision re-check of optimised trajectories on the device: the step after the solve.
//
//   TrajPlannerServer::CheckReplan, collision part   traj_planner/src/traj_server_ros.cpp:385-397
//   Trajectory::getPos / getAngle / locatePieceIdx    plan_utils/poly_traj_utils.hpp:510-528, 77-87, 179-192, 237-244
//   SemanticMapManager::CheckCollisionUsingPosAndYaw  semantic_map_manager.cc:639-662
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox common/src/common/basics/shapes.cc:110-149
//
// One workgroup per trajectory, one thread per time sample (t = 0, dt, dt + dt, ... < duration of each
// segment).  The samples are independent; a thread evaluates the pose, walks the ~140 outline points of
// the vehicle through the occupancy grid and, on a hit, lowers the trajectory's first-collision index with
// an atomic minimum — the reference stops at the first colliding sample, the minimum is the same answer.
// Both running sums of the reference (the sample times and the spacing along an edge) are tabulated on the
// host so that a thread sees exactly the value the sequential loop would have reached.  fp64, no
// contraction, cr_trig.h's atan2 / sincos where the reference calls libm: bit-identical to
// oracle/validate_oracle.cpp in order 2.  The read-out and the outline walk are piece_eval.h's and footprint.h's.
#include <hip/hip_runtime.h>

#include "step_args.h"

namespace dftpav {

__global__ void __launch_bounds__(256) validate_kernel(ValidateArgs A) {
  __shared__ int s_count[kMaxSeg + 1]; // samples of the segments before segment i
  __shared__ int s_first;
  const int b = blockIdx.x, tid = threadIdx.x;
  const DevLayout &L = A.L;
  const int M = L.M;
  if (tid == 0) {
    int acc = 0;
    for (int i = 0; i < M; i++) {
      const double dtp = A.piece_dt[(size_t)b * M + i];
      s_count[i] = acc;
      acc += pe::samples_below(A.tab, pe::segment_duration(L.piece_nums[i], dtp));
    }
    s_count[M] = acc;
    s_first = 0x7fffffff;
  }
  __syncthreads();
  const int total = s_count[M];
  const double *cb = A.coeffs + (size_t)b * L.Ntot * 12;
  for (int q = tid; q < total; q += blockDim.x) {
    const int i = pe::sample_segment(s_count, M, q);
    double tt = pe::sample_time(A.tab, q - s_count[i]);
    const int idx = pe::locate_piece(L.piece_nums[i], A.piece_dt[(size_t)b * M + i], tt);
    const double *c = cb + (size_t)(L.seg_piece0[i] + idx) * 12;
    double px, py, vx, vy;
    pe::piece_pos(c, tt, px, py);
    pe::piece_vel(c, tt, vx, vy);
    const double sg = (double)L.singuls[i];
    const double yaw = crt::atan2(sg * vy, sg * vx); // (the reference: libm; here correctly rounded, as oracle order 2)
    double cs, sn;
    crt::sincos(yaw, sn, cs);
    const bool hit = footprint_hits(A.grid, A.fp, px, py, cs, sn);
    if (hit) atomicMin(&s_first, q);
  }
  __syncthreads();
  if (tid == 0) {
    const bool any = s_first != 0x7fffffff;
    A.collision[b] = any ? 1 : 0;
    A.first_sample[b] = any ? s_first : -1;
  }
}

hipError_t launch_validate(const ValidateArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(validate_kernel, dim3(A.B), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
