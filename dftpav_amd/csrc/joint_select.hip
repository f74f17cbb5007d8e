// Joint selection (docs/NEXT_ROWS.md §4.28): the candidate plans of one dftpav_plan_queries call tested against each other, so that
// two queries of the call cannot both win with plans that cross at the same clock.  An option of the conflict filter; the definition
// is normative in include/dftpav_hip.h; restated:
//
//   candidate   (q, r), restart r of query q of a call of Q queries with R restarts; index i = q * R + r.  Its pose at the filter's
//               clocks t_k = t_call + (double)k * dt is cand_pose()'s with t_start = t_call (cand_pose.h, shared with cand_conflict.hip).
//   priority    the call's query order: q' < q has priority over q.
//   conf(a, b)  for candidates of two queries: a k < K with sep_k(a, b) <= margin, sep_k the conflict check's steps 1 to 3 (the broad
//               phase against range + 2.0 * rad, then cf_sep of conflict_sep.h).  Outside the broad phase, or with a pose that is not
//               finite on either side, a pair-sample contributes nothing.
//   greedy      for q = 0 .. Q - 1 in turn: blocked(q, r) when a q' < q with a winner w(q') >= 0 exists and conf((q, r), (q', w(q')));
//               w(q) the cheapest restart that is eligible and not blocked, ties to the lowest r, -1 if none.  Only winners block.
//   rows        per candidate, against the winners of the queries below its own, the partner index the query index: min_sep,
//               sep_sample, sep_partner = min (sep, k, q'); conflict_sample, conflict_partner = min (k, q') over sep <= margin;
//               +inf, -1, -1, -1, -1 where nothing contributed.  blocked(q, r) == (conflict_sample >= 0).
//   effect      a blocked restart gets the call's reject flag, stored by the one lane that owns the candidate (§4.17), and
//               plan_select_kernel, launched afterwards, arrives at w(q).
//
// Not claimed: priorities other than call order; no excusing of a replanning slot's old plan (the table test stays as it is);
// nothing between samples; one vehicle size; greedy, not jointly optimal -- a lower-priority query can end without a plan where a
// different choice for a higher one would have served both.
//
// Four kernels, fp64 without contraction, plain vector stores, no atomics, no scratch, no grid-wide wait; every loop is bounded by Q,
// R, K or a tile count.
//   joint_pose_kernel    cand_pose_kernel's shape per layout group: the poses through `members` into the call-wide arrays
//                        cx | cy | cs | sn [K][C_pad]; the lanes of sample 0 also gather cost, eligibility and the flag index.
//   joint_pair_kernel    conflict_pair_kernel's shape: workgroup (I-tile, J-tile) of 256 threads, a lane an I-candidate, the four waves
//                        the samples k = wave, wave + 4, ...; a wave stages the J-tile's poses in its own 2 KB of LDS, forms the broad
//                        phase's mask from broadcast reads, keeps the bits of candidates of queries below its own that are not set
//                        yet, and sets bit j where cf_sep <= margin.  The waves' words are OR-ed through LDS and wave 0 stores one
//                        64-bit word per (I-candidate, J-tile).  A J-tile with no candidate of a query below the I-tile's highest query
//                        is not walked (its words are never read); a J-tile of NaN poses is skipped on the ballot.
//   joint_greedy_kernel  one workgroup, q in order.  `chosen`, a bit per candidate, sits in LDS (C_pad / 64 words, 1 KB at the cap).  A
//                        wave takes the restarts r = wave, wave + 4, ...: the words of the restart's row are ANDed against `chosen`,
//                        strided over the lanes, and a ballot says blocked.  The cheapest eligible unblocked restart is kept on `<`
//                        in rising r, the four waves merge by plan_select_kernel's rule, thread 0 sets the `chosen` bit, and a
//                        barrier ends the query.
//   joint_rows_kernel    cand_pair_kernel's shape: the "table" is the winners' poses read in place through wcand, J-tiles of 64
//                        queries, the partner rule q' < q in place of j != own.
#include <hip/hip_runtime.h>

#include <climits>

#include "joint_args.h"
#include "cand_pose.h"
#include "conflict_sep.h"

namespace dftpav {

namespace {

// the bits j < n of a tile
__device__ inline unsigned long long joint_below(int n) { return n <= 0 ? 0ull : (n >= kConflictTile ? ~0ull : (1ull << n) - 1ull); }

// the broad phase of the lane's pose against the 64 staged poses: bit j, the pair passes
__device__ inline unsigned long long joint_broad(double xi, double yi, const double (*sp)[kConflictTile], double reach2) {
  unsigned long long cand = 0ull;
#pragma unroll 8
  for (int j = 0; j < kConflictTile; j++) {
    const double dx = xi - sp[0][j], dy = yi - sp[1][j];
    const double d2 = dx * dx + dy * dy;
    if (d2 <= reach2) cand |= 1ull << j;
  }
  return cand;
}

} // namespace

__global__ void __launch_bounds__(256) joint_pose_kernel(JointPoseArgs A) {
  __shared__ CandSegs S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * kConflictTile + lane;
  const int k = blockIdx.y * 4 + wave;
  cand_fill_segments(S, A.C, blockIdx.x * kConflictTile);
  if (c >= A.C.B || k >= A.P.K) return;
  const size_t i = (size_t)A.members[c / A.R] * A.R + c % A.R;
  double cx, cy, cs, sn;
  cand_pose(A.C, S, c, lane, A.C.t0 + (double)k * A.C.dt, cx, cy, cs, sn);
  const size_t o = (size_t)k * A.P.C_pad + i;
  A.P.cx[o] = cx;
  A.P.cy[o] = cy;
  A.P.cs[o] = cs;
  A.P.sn[o] = sn;
  if (k == 0) { // what the selection reads of the candidate, once
    const double f = A.f[c];
    A.J.cost[i] = f;
    A.J.eligible[i] = A.success[c] != 0 && A.collision[c] == 0 && A.reject[c] == 0 && f == f ? 1 : 0;
    A.J.flag[i] = A.flag0 + c;
  }
}

__global__ void __launch_bounds__(256) joint_pair_kernel(JointPairArgs A) {
  __shared__ double s_pose[4][4][kConflictTile];       // [wave][cx | cy | cs | sn][j]: the J-tile at the wave's sample
  __shared__ unsigned long long s_word[4][kConflictTile];
  const JointPoses &P = A.P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int it = blockIdx.x, jt = blockIdx.y, j0 = jt * kConflictTile;
  const int i = it * kConflictTile + lane;
  const int i_last = min(A.C - 1, it * kConflictTile + kConflictTile - 1);
  if (j0 / A.R >= i_last / A.R) return; // no candidate of a query below the I-tile's highest: the whole workgroup leaves
  // the partners of a candidate are the candidates of the queries below its own: the bits j with j0 + j < q * R
  const unsigned long long lower = i < A.C ? joint_below(i / A.R * A.R - j0) : 0ull;
  unsigned long long word = 0ull;
  double(*sp)[kConflictTile] = s_pose[wave];
  for (int k = wave; k < P.K; k += 4) {
    const size_t row = (size_t)k * P.C_pad;
    const double xi = P.cx[row + i], yi = P.cy[row + i], ci = P.cs[row + i], si = P.sn[row + i];
    sp[0][lane] = P.cx[row + j0 + lane];
    sp[1][lane] = P.cy[row + j0 + lane];
    sp[2][lane] = P.cs[row + j0 + lane];
    sp[3][lane] = P.sn[row + j0 + lane];
    // (a wave's LDS accesses complete in order; the fence keeps the compiler from moving the reads above the stores)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (__ballot(sp[0][lane] == sp[0][lane]) != 0) { // a tile of NaN poses is not walked
      unsigned long long cand = joint_broad(xi, yi, sp, A.V.reach2) & lower & ~word; // a bit that is set stays set
      while (cand) {
        const int j = __ffsll((long long)cand) - 1;
        cand &= cand - 1ull;
        const double sep = cf_sep(xi, yi, ci, si, sp[0][j], sp[1][j], sp[2][j], sp[3][j], A.V.half_l, A.V.half_w);
        if (sep <= A.V.margin) word |= 1ull << j;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next sample's stores stay behind these reads
    __builtin_amdgcn_wave_barrier();
  }
  s_word[wave][lane] = word;
  __syncthreads();
  if (wave == 0) A.bits[(size_t)i * A.tiles + jt] = word | s_word[1][lane] | s_word[2][lane] | s_word[3][lane];
}

__global__ void __launch_bounds__(256) joint_greedy_kernel(JointGreedyArgs A) {
  __shared__ unsigned long long s_chosen[DFTPAV_JOINT_MAX_CANDIDATES / kConflictTile];
  __shared__ double s_best[4];
  __shared__ int s_idx[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int R = A.R;
  for (int w = threadIdx.x; w < A.tiles; w += 256) s_chosen[w] = 0ull;
  __syncthreads();
  for (int q = 0; q < A.Q; q++) {
    const int n_words = (q * R + kConflictTile - 1) / kConflictTile; // the words that hold a candidate of a query below q
    const bool open = A.minit == nullptr || A.minit[q] == 0;
    double best = 0.0;
    int idx = INT_MAX; // none yet
    for (int r = wave; r < R; r += 4) {
      const size_t i = (size_t)q * R + r;
      bool hit = false;
      for (int w = lane; w < n_words; w += kConflictTile) hit = hit || (A.bits[i * A.tiles + w] & s_chosen[w]) != 0ull;
      const bool blk = __ballot(hit) != 0;
      const double c = A.J.cost[i];
      if (lane == 0) { // the lane that owns the candidate
        A.blocked[i] = blk ? 1 : 0;
        if (blk && A.reject) {
          const int fl = A.J.flag[i];
          if (fl >= 0) A.reject[fl] = 1;
        }
      }
      if (open && !blk && A.J.eligible[i] != 0 && c == c && (idx == INT_MAX || c < best)) { // rising r: the first of equals stays
        best = c;
        idx = r;
      }
    }
    if (lane == 0) {
      s_best[wave] = best;
      s_idx[wave] = idx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; w++) {
        const double oc = s_best[w];
        const int oi = s_idx[w];
        if (oi != INT_MAX && (idx == INT_MAX || oc < best || (oc == best && oi < idx))) {
          best = oc;
          idx = oi;
        }
      }
      const int win = idx == INT_MAX ? -1 : idx;
      A.winner[q] = win;
      A.wcand[q] = win < 0 ? -1 : q * R + win;
      if (win >= 0) {
        const int i = q * R + win;
        s_chosen[i / kConflictTile] |= 1ull << (i % kConflictTile);
      }
    }
    __syncthreads(); // the next query reads `chosen`
  }
}

__global__ void __launch_bounds__(256) joint_rows_kernel(JointRowsArgs A) {
  __shared__ double s_pose[4][4][kConflictTile]; // [wave][cx | cy | cs | sn][j]: the winners of 64 queries at the wave's sample
  __shared__ double s_sep[4][kConflictTile];     // the waves' minima, for the merge
  __shared__ int s_idx[4][4][kConflictTile];     // [wave][sep_sample | sep_partner | conflict_sample | conflict_partner][lane]
  const JointPoses &P = A.P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * kConflictTile + lane;
  const bool valid = i < A.C;
  const int q = valid ? i / A.R : 0;
  const int q_last = min(A.C - 1, (int)blockIdx.x * kConflictTile + kConflictTile - 1) / A.R; // the tile's highest query
  double bs = kCfInf;
  int bk = -1, bj = -1, fk = -1, fj = -1;
  double(*sp)[kConflictTile] = s_pose[wave];
  for (int k = wave; k < P.K; k += 4) {
    const size_t row = (size_t)k * P.C_pad;
    double xi = kCfNaN, yi = kCfNaN, ci = kCfNaN, si = kCfNaN; // a lane behind the last candidate: passes no broad phase
    if (valid) xi = P.cx[row + i], yi = P.cy[row + i], ci = P.cs[row + i], si = P.sn[row + i];
    for (int q0 = 0; q0 < q_last; q0 += kConflictTile) { // the queries below the tile's highest
      const int w = q0 + lane < A.Q ? A.wcand[q0 + lane] : -1;
      sp[0][lane] = w >= 0 ? P.cx[row + w] : kCfNaN;
      sp[1][lane] = w >= 0 ? P.cy[row + w] : kCfNaN;
      sp[2][lane] = w >= 0 ? P.cs[row + w] : kCfNaN;
      sp[3][lane] = w >= 0 ? P.sn[row + w] : kCfNaN;
      // (a wave's LDS accesses complete in order; the fence keeps the compiler from moving the reads above the stores)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (__ballot(sp[0][lane] == sp[0][lane]) != 0) { // 64 queries without a winner are not walked
        unsigned long long cand = joint_broad(xi, yi, sp, A.V.reach2) & joint_below(q - q0); // the partners: q' < q
        while (cand) {
          const int j = __ffsll((long long)cand) - 1;
          cand &= cand - 1ull;
          const double sep = cf_sep(xi, yi, ci, si, sp[0][j], sp[1][j], sp[2][j], sp[3][j], A.V.half_l, A.V.half_w);
          if (sep < bs) { // rising (k, q'): the first of equals stays
            bs = sep;
            bk = k;
            bj = q0 + j;
          }
          if (fk < 0 && sep <= A.V.margin) {
            fk = k;
            fj = q0 + j;
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
    A.rows.min_sep[i] = bs;
    A.rows.sep_sample[i] = bk;
    A.rows.sep_partner[i] = bj;
    A.rows.conflict_sample[i] = fk;
    A.rows.conflict_partner[i] = fj;
  }
}

hipError_t launch_joint_poses(const JointPoseArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(joint_pose_kernel, dim3((A.C.B + kConflictTile - 1) / kConflictTile, (A.P.K + 3) / 4), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_joint_pairs(const JointPairArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(joint_pair_kernel, dim3(A.tiles, A.tiles), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_joint_greedy(const JointGreedyArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(joint_greedy_kernel, dim3(1), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_joint_rows(const JointRowsArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(joint_rows_kernel, dim3((A.C + kConflictTile - 1) / kConflictTile), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
