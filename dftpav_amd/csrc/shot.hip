// Reeds-Shepp shots on the device (hypothesis generation): the analytic connection of a
// pose to the goal that the reference's front end tries from its search nodes.
//
//   KinoAstar::computeShotTraj / is_shot_sucess      traj_planner/src/kino_astar.cpp:304-345
//   ompl::base::ReedsSheppStateSpace(1 / max_cur_)   kino_astar.cpp:423 (OMPL is not vendored: rs_math.h restates
//     ::distance, ::interpolate                        the published algorithm behind it)
//   SemanticMapManager::CheckCollisionUsingPosAndYaw semantic_map_manager.cc:639-662 (through map_adapter.cpp:110-115)
//   ShapeUtils::GetDenseVerticesOfOrientedBoundingBox common/src/common/basics/shapes.cc:110-149
//
// One wave per (from, to) pair.  Every lane computes the shortest path (the 48 candidate words are straight-line
// code, nothing to share), lane 0 lays down the sample offsets l = 0, checkl, checkl + checkl, ... <= length as
// the reference's running sum, then the samples are independent: a lane interpolates its pose and, if a map is
// installed, walks the vehicle outline through the occupancy grid (footprint.h).  fp64, no contraction, portable
// sin / cos / atan2: bit-identical to oracle/shot_oracle.cpp in order 1.
#include <hip/hip_runtime.h>

#include "rs_math.h"
#include "step_args.h"

namespace dftpav {

__global__ void __launch_bounds__(64) shot_kernel(ShotArgs A) {
  extern __shared__ double l_tab[]; // [max_samples]
  __shared__ int s_cnt, s_hit;
  const int i = blockIdx.x, lane = threadIdx.x;
  typedef rs::Solver<rs::PortableMath> RS;
  double from[3], to[3];
  for (int k = 0; k < 3; k++) {
    from[k] = A.from[3 * (size_t)i + k];
    to[k] = A.to[3 * (size_t)i + k];
  }
  const rs::Path path = RS::between(from, to, A.rho);
  const double len = A.rho * path.total; // ReedsSheppStateSpace::distance
  if (lane == 0) {
    A.length[i] = len;
    A.type[i] = path.type;
    for (int k = 0; k < 5; k++) A.seg[5 * (size_t)i + k] = path.len[k];
    int cnt = 0;
    for (double l = 0.0; l <= len; l += A.checkl) { // kino_astar.cpp:338
      if (cnt < A.max_samples) l_tab[cnt] = l;
      cnt++;
    }
    s_cnt = cnt;
    s_hit = 0;
  }
  __syncthreads();
  const int cnt = s_cnt, stored = cnt < A.max_samples ? cnt : A.max_samples;
  double *out = A.samples + (size_t)i * A.max_samples * 3;
  for (int k = lane; k < A.max_samples; k += 64) {
    double s[3] = {0.0, 0.0, 0.0};
    if (k < stored) {
      const double t = l_tab[k] / len;
      if (t >= 1.0) { // ReedsSheppStateSpace::interpolate: the end states are copied as they are
        s[0] = to[0]; s[1] = to[1]; s[2] = to[2];
      } else if (t <= 0.0) {
        s[0] = from[0]; s[1] = from[1]; s[2] = from[2];
      } else {
        RS::interpolate(from, path, A.rho, t, s);
      }
      if (A.grid.cells != nullptr && footprint_hits(A.grid, A.fp, s[0], s[1], p_cos(s[2]), p_sin(s[2]))) atomicOr(&s_hit, 1);
    }
    out[3 * k] = s[0];
    out[3 * k + 1] = s[1];
    out[3 * k + 2] = s[2];
  }
  __syncthreads();
  if (lane == 0) {
    A.n_samples[i] = cnt;
    if (A.collides) A.collides[i] = s_hit;
  }
}

hipError_t launch_shots(const ShotArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(shot_kernel, dim3(A.n), dim3(64), sizeof(double) * (size_t)A.max_samples, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
