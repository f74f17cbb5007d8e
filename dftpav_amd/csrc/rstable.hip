// The Reeds-Shepp cost-to-go table: the non-holonomic, obstacle-free term of the hybrid A* heuristic (Dolgov et al.'s second
// term; the first, holonomic with obstacles, is goalfield.hip).
//
//   T[k][j][i] = rho * rs::Solver<CrMath>::between(from, to, rho).total,
//   from = ((double)(i - half) * cell, (double)(j - half) * cell, (double)k * dth),   to = (0, 0, 0):
//
// the length of the shortest Reeds-Shepp path from a pose in the goal's frame to the goal, the expression sr_shot_free
// (search.hip) forms for `len`, with the same solver instance; fp64, no contraction, bit-identical to oracle_search/'s
// oracle_rs_table in order 2.  It depends on rho and the table's geometry only -- not on the map, not on the goal -- so a handle
// builds it once (capi_steps.cpp) and the search reads one double per heuristic.
//
// One thread per entry in workgroups of 256, as a grid-stride loop over the entry count (the tail is guarded by that count, not
// by a rounded-up size).  Consecutive lanes are consecutive i: a wave stores 64 contiguous doubles.  No LDS, no atomics.  The
// solver is the word ladder of rs_math.h as it stands, one candidate after the other with a branch per candidate; lanes of a
// wave hold neighbouring poses, which mostly take the same branches.
#include <hip/hip_runtime.h>

#include "rstable_args.h"

namespace dftpav {

__global__ void __launch_bounds__(kRsThreads) rs_table_kernel(RsTableArgs A) {
  typedef rs::Solver<CrMath> RS;
  const RsGeometry &g = A.g;
  const long long stride = (long long)gridDim.x * kRsThreads, plane = (long long)g.n * g.n;
  const double to[3] = {0.0, 0.0, 0.0};
  for (long long e = (long long)blockIdx.x * kRsThreads + threadIdx.x; e < A.entries; e += stride) {
    const int k = (int)(e / plane), r = (int)(e % plane), j = r / g.n, i = r % g.n;
    const double from[3] = {(double)(i - g.half) * g.cell, (double)(j - g.half) * g.cell, (double)k * g.dth};
    A.T[e] = A.rho * RS::between(from, to, A.rho).total;
  }
}

hipError_t launch_rs_table(const RsTableArgs &A, hipStream_t stream) {
  if (A.entries < 1) return hipSuccess;
  const long long blocks = (A.entries + kRsThreads - 1) / kRsThreads;
  hipLaunchKernelGGL(rs_table_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kRsThreads), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
