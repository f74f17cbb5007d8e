// Footprint conflicts of candidate plans against the executing table (docs/NEXT_ROWS.md §4.26): does the vehicle of trajectory c of
// a batch, were it adopted at t_start, come within `margin` of the vehicle of an occupied slot at the same clock, when first, and
// who with.  The read-out dftpav_batch_check_conflicts / dftpav_batch_sample_poses, and the conflict filter in front of the
// selection of dftpav_plan_queries.  The definition is normative in include/dftpav_hip.h; restated:
//
//   candidate   trajectory c of a batch: the batch's layout (M, piece_nums, singuls), its piece coefficients [Ntot][6][2] and piece
//               durations [M] as dftpav_batch_coeffs returns them, and an absolute start clock t_start.
//   clocks      t_k = t0 + (double)k * dt, k < K <= DFTPAV_CONFLICT_MAX_SAMPLES, as the conflict check's.
//   pose of a candidate at clock t: the pose its slot would have after dftpav_planner_adopt(..., t_start).  The segment times are
//               chained by pe::segment_duration and the additions of exec_adopt_kernel: world = t_start, d = segment_duration(N_i,
//               dt_i), start = world, end = world + d, and the next segment starts at that end.  Segment, local time, clamping,
//               position, heading and box centre are the statements of conflict_pose_kernel: the first segment e with
//               !(end[e] <= t), else the last; tt = t - start[e] clamped to [0, d[e]]; pe::locate_piece, pe::piece_pos, pe::piece_vel;
//               yaw = crt::atan2(sg * vy, sg * vx); crt::sincos; c = pos + veh_d_cr * (cs, sn).  Held still before t_start and after
//               the last end.
//   pose of a slot: conflict_pose_kernel's, unchanged (conflict.hip; launched by the host once per call).
//   separation  of candidate c and occupied slot j != own[c] at sample k: steps 1 to 3 of the conflict check in the same
//               expressions -- the broad phase on the centres against R = range + 2.0 * rad, the separating-axis test, the 32
//               corner-to-edge distances (conflict_sep.h, shared with conflict.hip).
//   own slot    own[c]: the slot the candidate would replace, -1: none.  It takes no part; neither does an empty slot or a pose that
//               is not finite on either side.
//   rows        per candidate, lexicographic minima: min_sep, sep_sample, sep_partner = min (sep, k, j); conflict_sample,
//               conflict_partner = min (k, j) over sep <= margin.  Nothing contributed: +inf, -1, -1, -1, -1.
// Nothing of the table, the publisher's state or the batch is written.
//
// Not claimed: candidates of one call are not tested against each other unless joint selection is on (joint_select.hip, §4.28); a
// slot that replans in the same tick is tested as its old plan; between samples nothing is tested; one vehicle size; the moving
// obstacles of dftpav_set_surround take no part.  The filter only rejects: what starts a replanning when two executing plans meet is
// the conflict trigger of dftpav_replan_tick (conflict_trigger.hip, §4.29).
//
// Two kernels.  cand_pair_kernel is conflict_pair_kernel's shape with the I side evaluated instead of loaded: one workgroup of 256
// threads per 64 candidates, a lane a candidate, the four waves the samples k = wave, wave + 4, ...  Per sample a lane evaluates its
// candidate's pose once, in registers; the wave then walks every J-tile of the table's poses: it stages the tile's 64 poses in its
// own 2 KB of LDS, forms the broad phase's 64-bit mask from broadcast reads, clears the own slot's bit, and hands the survivors to
// cf_sep in rising j.  A lane visits its (k, j) in rising order, so its minima are replaced on `<` alone; the four waves merge
// through LDS by the full lexicographic rule and wave 0 writes the row.  The filter's variant writes row members[c / R] * R + c % R
// and stores 1 into reject[c] where conflict_sample >= 0: only that lane, only where it rejects (§4.17).  cand_pose_kernel writes the
// poses [K][B][4] for the read-out.  Both take the per-candidate segment durations from LDS (CandSegs, cand_pose.h), filled once per
// workgroup.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "cand_conflict_args.h"
#include "cand_pose.h"
#include "conflict_sep.h"

namespace dftpav {

__global__ void __launch_bounds__(256) cand_pose_kernel(CandPoseArgs A) {
  __shared__ CandSegs S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * kConflictTile + lane;
  const int k = blockIdx.y * 4 + wave;
  cand_fill_segments(S, A.C, blockIdx.x * kConflictTile);
  if (c >= A.C.B || k >= A.K) return;
  double cx, cy, cs, sn;
  cand_pose(A.C, S, c, lane, A.C.t0 + (double)k * A.C.dt, cx, cy, cs, sn);
  double *o = A.poses + ((size_t)k * A.C.B + c) * 4;
  o[0] = cx;
  o[1] = cy;
  o[2] = cs;
  o[3] = sn;
}

__global__ void __launch_bounds__(256) cand_pair_kernel(CandPairArgs A) {
  __shared__ CandSegs S;
  __shared__ double s_pose[4][4][kConflictTile]; // [wave][cx | cy | cs | sn][j]: a J-tile at the wave's sample
  __shared__ double s_sep[4][kConflictTile];     // the waves' minima, for the merge
  __shared__ int s_idx[4][4][kConflictTile];     // [wave][sep_sample | sep_partner | conflict_sample | conflict_partner][lane]
  const ConflictPoses &P = A.P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * kConflictTile + lane;
  const bool valid = c < A.C.B;
  cand_fill_segments(S, A.C, blockIdx.x * kConflictTile);
  int own = -1;
  if (valid && A.own) own = A.own[A.members ? A.members[c / A.R] : c];
  double bs = kCfInf;
  int bk = -1, bj = -1, fk = -1, fj = -1;
  double(*sp)[kConflictTile] = s_pose[wave];
  for (int k = wave; k < P.K; k += 4) {
    double xi = kCfNaN, yi = kCfNaN, ci = kCfNaN, si = kCfNaN; // a lane behind the last candidate: passes no broad phase
    if (valid) cand_pose(A.C, S, c, lane, A.C.t0 + (double)k * A.C.dt, xi, yi, ci, si);
    const size_t row = (size_t)k * P.S_pad;
    for (int j0 = 0; j0 < P.S_pad; j0 += kConflictTile) {
      sp[0][lane] = P.cx[row + j0 + lane];
      sp[1][lane] = P.cy[row + j0 + lane];
      sp[2][lane] = P.cs[row + j0 + lane];
      sp[3][lane] = P.sn[row + j0 + lane];
      // (a wave's LDS accesses complete in order; the fence keeps the compiler from moving the reads above the stores)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (__ballot(sp[0][lane] == sp[0][lane]) != 0) { // a tile of empty slots (NaN) is not walked
        unsigned long long cand = 0ull;                // the broad phase: bit j, slot j0 + j passes
#pragma unroll 8
        for (int j = 0; j < kConflictTile; j++) {
          const double dx = xi - sp[0][j], dy = yi - sp[1][j];
          const double d2 = dx * dx + dy * dy;
          if (d2 <= A.V.reach2) cand |= 1ull << j;
        }
        const int oj = own - j0; // the own slot's bit, where this tile holds it
        if ((unsigned)oj < (unsigned)kConflictTile) cand &= ~(1ull << oj);
        while (cand) {
          const int j = __ffsll((long long)cand) - 1;
          cand &= cand - 1ull;
          const double sep = cf_sep(xi, yi, ci, si, sp[0][j], sp[1][j], sp[2][j], sp[3][j], A.V.half_l, A.V.half_w);
          if (sep < bs) { // rising (k, j): the first of equals stays
            bs = sep;
            bk = k;
            bj = j0 + j;
          }
          if (fk < 0 && sep <= A.V.margin) {
            fk = k;
            fj = j0 + j;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next tile's stores stay behind these reads
      __builtin_amdgcn_wave_barrier();
    }
  }
  s_sep[wave][lane] = bs;
  s_idx[wave][0][lane] = bk;
  s_idx[wave][1][lane] = bj;
  s_idx[wave][2][lane] = fk;
  s_idx[wave][3][lane] = fj;
  __syncthreads();
  if (wave == 0 && valid) {
    for (int w = 1; w < 4; w++) {
      cf_merge_sep(bs, bk, bj, s_sep[w][lane], s_idx[w][0][lane], s_idx[w][1][lane]);
      cf_merge_first(fk, fj, s_idx[w][2][lane], s_idx[w][3][lane]);
    }
    const size_t o = A.members ? (size_t)A.members[c / A.R] * A.R + c % A.R : (size_t)c;
    A.rows.min_sep[o] = bs;
    A.rows.sep_sample[o] = bk;
    A.rows.sep_partner[o] = bj;
    A.rows.conflict_sample[o] = fk;
    A.rows.conflict_partner[o] = fj;
    if (A.reject && fk >= 0) A.reject[c] = 1;
  }
}

hipError_t launch_cand_poses(const CandPoseArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(cand_pose_kernel, dim3((A.C.B + kConflictTile - 1) / kConflictTile, (A.K + 3) / 4), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_cand_pairs(const CandPairArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(cand_pair_kernel, dim3((A.C.B + kConflictTile - 1) / kConflictTile), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
