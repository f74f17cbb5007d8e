// The conflict trigger of the replan tick (docs/NEXT_ROWS.md §4.29): which slot of the executing table gives way to which, and when.
// The poses, the clocks and steps 1 to 3 of the separation are the conflict check's (conflict.hip, conflict_sep.h), in the same
// expressions; what is new is the restriction of the partners and the flag.
//
//   can_yield(s)     the slot holds a plan and !(t_now > end_time[n_seg - 1]): the completion test of replan_check_kernel
//                    (traj_server_ros.cpp:150), read from the table's row.  A completed slot stands where its plan ended and the
//                    tick plans nothing for it: it cannot give way, so whoever meets it must.
//   precedes(j, i)   for occupied i != j: !can_yield(j) || j < i.  A lower slot index is a higher priority: the order of the tick's
//                    query list, and so the priority of joint selection.
//   per occupied i   yield_sample, yield_partner: the lexicographic minimum of (k, j) over the pair-samples with
//                    sep(i, j, k) <= margin and precedes(j, i); -1, -1 when there is none.  yield = can_yield(i) && yield_sample >= 0.
//   an empty slot    0, -1, -1.
// The rows are existential and lexicographic, so no order of reduction shows; every output is an integer.  A pair outside the broad
// phase, or with a pose that is not finite, contributes nothing.  Nothing of the table is written.
//
// Two kernels behind conflict_pose_kernel.  trigger_pair_kernel has conflict_pair_kernel's shape -- one workgroup of 256 threads per
// (I-tile, J-tile) of 64 x 64 slots, a lane a slot i, the four waves on the samples k = wave, wave + 4, ..., the J-tile's 64 poses
// staged per wave in LDS -- and does less:
//   - a precedence mask per lane, formed once per workgroup: the lower-slot term is all ones below the diagonal, none above it and
//     the bits below the lane on it; ORed with the J-tile's cannot-yield ballot, ANDed with its occupancy, the lane's own bit cleared;
//   - the mask is ANDed into the broad phase's survivors before the narrow phase: only pairs that could make i yield reach cf_sep;
//   - a tile pair whose masks are all empty walks no sample (a fleet all under way: every tile pair above the diagonal);
//   - a lane meets its (k, j) in rising order within its wave, so its first hit is its wave's minimum and it searches no further;
//     the wave leaves its loop when a ballot shows no lane still searching.
// The four waves merge through LDS by the lexicographic rule; a partial row is written per (slot, J-tile).  trigger_reduce_kernel:
// one thread per slot merges its partial rows and writes yield.  No atomics, no scratch, fp64 without contraction.
#include <hip/hip_runtime.h>

#include "conflict_sep.h"
#include "conflict_trigger_args.h"

namespace dftpav {

// can_yield of slot s < S_pad (false for an empty slot and for the padding behind the last slot)
__device__ inline bool trigger_can_yield(const TriggerYield &Y, int s) {
  if (Y.flags) return Y.flags[s] != 0;
  if (s >= Y.T.n_slots) return false;
  const int M = Y.T.n_seg[s];
  if (M <= 0) return false;
  return !(Y.t_now > Y.T.end_time[(size_t)s * Y.T.max_seg + (M - 1)]);
}

__global__ void __launch_bounds__(256) trigger_pair_kernel(TriggerPairArgs A) {
  __shared__ double s_pose[4][4][kConflictTile]; // [wave][cx | cy | cs | sn][j]: the J-tile at the wave's sample
  __shared__ int s_idx[4][2][kConflictTile];     // [wave][sample | partner][lane], for the merge
  const ConflictPoses &P = A.P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.y * kConflictTile;
  const int i = blockIdx.x * kConflictTile + lane; // < S_pad
  // the precedence mask of the lane: bit j, slot j0 + j is occupied, is not i, and precedes i (every wave forms the same)
  const bool occ_j = P.occupied[j0 + lane] != 0;
  const unsigned long long occupied_j = __ballot(occ_j);
  const unsigned long long cannot_j = __ballot(occ_j && !trigger_can_yield(A.Y, j0 + lane));
  unsigned long long prec = blockIdx.y < blockIdx.x ? ~0ull : (blockIdx.y > blockIdx.x ? 0ull : (1ull << lane) - 1ull);
  prec = (prec | cannot_j) & occupied_j;
  if (blockIdx.x == blockIdx.y) prec &= ~(1ull << lane); // the tile against itself: not i against i
  if (P.occupied[i] == 0) prec = 0ull;                    // an empty slot has no row
  int fk = -1, fj = -1;
  double(*sp)[kConflictTile] = s_pose[wave];
  // a tile pair whose masks are all empty walks no sample: the first ballot is false (every wave decides alike)
  for (int k = wave; k < P.K; k += 4) {
    if (__ballot(prec != 0ull && fk < 0) == 0ull) break; // no lane still searching
    const size_t row = (size_t)k * P.S_pad;
    sp[0][lane] = P.cx[row + j0 + lane];
    sp[1][lane] = P.cy[row + j0 + lane];
    sp[2][lane] = P.cs[row + j0 + lane];
    sp[3][lane] = P.sn[row + j0 + lane];
    const double xi = P.cx[row + i], yi = P.cy[row + i], ci = P.cs[row + i], si = P.sn[row + i];
    // (a wave's LDS accesses complete in order; the fence keeps the compiler from moving the reads above the stores)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unsigned long long cand = 0ull; // the broad phase: bit j, slot j0 + j passes
#pragma unroll 8
    for (int j = 0; j < kConflictTile; j++) {
      const double dx = xi - sp[0][j], dy = yi - sp[1][j];
      const double d2 = dx * dx + dy * dy;
      if (d2 <= A.V.reach2) cand |= 1ull << j;
    }
    cand &= prec;            // only a pair that could make i yield reaches the narrow phase
    if (fk >= 0) cand = 0ull; // the lane has its minimum
    while (cand) {
      const int j = __ffsll((long long)cand) - 1;
      cand &= cand - 1ull;
      const double sep = cf_sep(xi, yi, ci, si, sp[0][j], sp[1][j], sp[2][j], sp[3][j], A.V.half_l, A.V.half_w);
      if (sep <= A.V.margin) { // rising (k, j): the first hit is the wave's minimum
        fk = k;
        fj = j0 + j;
        cand = 0ull;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next sample's stores stay behind these reads
    __builtin_amdgcn_wave_barrier();
  }
  s_idx[wave][0][lane] = fk;
  s_idx[wave][1][lane] = fj;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < 4; w++) cf_merge_first(fk, fj, s_idx[w][0][lane], s_idx[w][1][lane]);
    const size_t o = (size_t)blockIdx.y * P.S_pad + i;
    A.part.sample[o] = fk;
    A.part.partner[o] = fj;
  }
}

__global__ void __launch_bounds__(256) trigger_reduce_kernel(TriggerReduceArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_slots) return;
  int fk = -1, fj = -1;
  for (int t = 0; t < A.tiles; t++) {
    const size_t o = (size_t)t * A.S_pad + i;
    cf_merge_first(fk, fj, A.part.sample[o], A.part.partner[o]);
  }
  A.out.sample[i] = fk;
  A.out.partner[i] = fj;
  A.yield[i] = (fk >= 0 && A.occupied[i] != 0 && trigger_can_yield(A.Y, i)) ? 1 : 0;
}

hipError_t launch_trigger_pairs(const TriggerPairArgs &A, hipStream_t stream) {
  const int tiles = A.P.S_pad / kConflictTile;
  hipLaunchKernelGGL(trigger_pair_kernel, dim3(tiles, tiles), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_trigger_reduce(const TriggerReduceArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(trigger_reduce_kernel, dim3((A.n_slots + 255) / 256), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
