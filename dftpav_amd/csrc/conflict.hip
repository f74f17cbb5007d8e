// Footprint conflicts between the executing plans of a planner's table, slot against slot (docs/NEXT_ROWS.md §4.23): do the
// vehicles of two slots come within `margin` of one another at the same clock, when first, and who with.  A read-out beside
// limits.hip and clearance.hip; it feeds nothing back.
//
//   TrajPlannerServer::PublishData, exe_traj_index_          traj_planner/src/traj_server_ros.cpp:248-252
//   Trajectory::getPos / getAngle / locatePieceIdx           plan_utils/poly_traj_utils.hpp:554-558, 626-630, 510-528
//   Piece::getPos / getdSigma / getAngle                     poly_traj_utils.hpp:77-87, 179-192, 237-244
//   SemanticMapManager::CheckCollisionUsingPosAndYaw, the box   semantic_map_manager.cc:645-646, shapes.cc:110-149
//
// The clocks are t_k = t0 + (double)k * dt, k = 0 .. K - 1, absolute, on the clock of the table's start_time / end_time.
//
// The pose of an occupied slot at clock t is the vehicle as the publisher would drive it, held still outside its plan.
//   segment e   the first i in [0, n_seg) with !(end_time[i] <= t), else n_seg - 1 (replan_check_kernel's derivation).
//   local time  tt = t - start_time[e]; tt < 0 becomes 0; tt > duration[e] becomes duration[e].
//   position    Trajectory::getPos(tt): pe::locate_piece's subtraction walk, pe::piece_pos.
//   heading     Trajectory::getAngle(tt) = atan2(singul * sigma'_y, singul * sigma'_x) by crt::atan2; cs, sn by crt::sincos.
//   footprint   the obb centre c = pos + veh_d_cr * (cs, sn) and the four corners, in the expressions and the corner order of
//               footprint_hits (footprint.h).
//
// The separation of two occupied slots i != j at sample k, fp64 without contraction:
//   1. broad phase: dx = cx_i - cx_j, dy = cy_i - cy_j, d2 = dx * dx + dy * dy; R = range + 2.0 * rad, rad = sqrt(0.25 * L * L +
//      0.25 * W * W) computed once on the host.  The pair-sample contributes nothing when !(d2 <= R * R).  This is part of the
//      definition, not an optimisation; a pose that is not finite contributes nothing.
//   2. overlap: the separating-axis test on the four axes, (cs, sn) and (-sn, cs) of both boxes.  For the axis owner A the other's
//      four corners in A's frame: lx = cs * (px - cx) + sn * (py - cy), ly = cs * (py - cy) - sn * (px - cx).  A's x axis separates
//      when all four lx > L / 2 or all four lx < -L / 2, its y axis likewise with W / 2.  No axis separates: sep = 0.0.
//   3. otherwise sep = sqrt(m), m the minimum of the 32 squared point-to-segment distances, each box's four corners against the
//      other's four edges: u = ((p - a) . (b - a)) / ((b - a) . (b - a)) clamped to [0, 1] (!(u > 0) gives 0), q = a + u * (b - a),
//      and |p - q|^2 is summed as ex * ex + ey * ey.
//   4. sep(i, j, k) and sep(j, i, k) are the same bits: dx and dy are only squared, and steps 2 and 3 are conjunctions and minima
//      over one set of values whichever box is named first (cf_sep, conflict_sep.h, computes both boxes' corners by one expression and
//      visits both halves of either step).
//
// Per slot i, each a lexicographic minimum, so the order of reduction does not show:
//   min_sep, sep_sample, sep_partner    the minimum of (sep, k, j) over all contributing pair-samples
//   conflict_sample, conflict_partner   the minimum of (k, j) over the pair-samples with sep <= margin
// An empty slot and a slot with nothing inside the broad phase give +inf, -1, -1, -1, -1.  Nothing of the table is written.
//
// Three kernels.  conflict_pose_kernel: one thread per (sample, slot), four samples of 64 slots per workgroup, each thread reading
// its slot's row of the table; the poses go out sample-major as four arrays [K][S_pad] (S_pad: whole tiles of 64; NaN for empty
// slots and the padding), so a wave of the pair kernel reads the 64 slots of a tile at one sample as 512 contiguous bytes per array.
// conflict_pair_kernel: an N-body tiling, one workgroup of 256 threads per (I-tile, J-tile) of 64 x 64 slots; its four waves take
// the samples k = wave, wave + 4, ...; a lane is one slot i.  Per sample a wave stages the J-tile's 64 poses in its own 2 KB of LDS,
// every lane walks j = 0 .. 63 reading one address (a broadcast) for the broad phase and keeps the survivors as a 64-bit mask;
// only those enter the overlap and distance code, in rising j, under divergence.  A lane visits its (k, j) in rising order, so
// its minima are replaced on `<` alone; the four waves merge through LDS and the workgroup writes one partial row per (slot,
// J-tile).  conflict_reduce_kernel: one thread per slot merges its partial rows.  No atomics.
#include <hip/hip_runtime.h>

#include "conflict_args.h"
#include "conflict_sep.h"

namespace dftpav {

__global__ void __launch_bounds__(256) conflict_pose_kernel(ConflictPoseArgs A) {
  const ExecTable &T = A.T;
  const int s = blockIdx.x * kConflictTile + (threadIdx.x & 63); // < S_pad: the grid covers whole tiles
  const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (k >= A.P.K) return;
  const int M = s < T.n_slots ? T.n_seg[s] : 0; // the padding behind the last slot is empty
  if (k == 0) A.P.occupied[s] = M > 0 ? 1 : 0;
  double cx = kCfNaN, cy = kCfNaN, cs = kCfNaN, sn = kCfNaN;
  if (M > 0) {
    const int MS = T.max_seg;
    const int *pn = T.piece_nums + (size_t)s * MS, *sg = T.singul + (size_t)s * MS;
    const double *dtv = T.coeff_dt + (size_t)s * MS;
    const double *dur = T.duration + (size_t)s * MS, *st = T.start_time + (size_t)s * MS, *en = T.end_time + (size_t)s * MS;
    const double t = A.t0 + (double)k * A.dt;
    int e = 0, p0 = 0; // the segment, and its first piece: the pieces of a slot's segments follow one another
    while (e < M - 1 && en[e] <= t) {
      p0 += pn[e];
      e++;
    }
    double tt = t - st[e];
    if (tt < 0.0) tt = 0.0;
    if (tt > dur[e]) tt = dur[e];
    const int idx = pe::locate_piece(pn[e], dtv[e], tt);
    const double *c = T.coeffs + ((size_t)s * MS * T.max_pieces + (size_t)(p0 + idx)) * 12;
    double px, py, vx, vy;
    pe::piece_pos(c, tt, px, py);
    pe::piece_vel(c, tt, vx, vy);
    const double sgn = (double)sg[e];
    const double yaw = crt::atan2(sgn * vy, sgn * vx);
    crt::sincos(yaw, sn, cs);
    cx = px + A.dcr * cs;
    cy = py + A.dcr * sn;
  }
  const size_t o = (size_t)k * A.P.S_pad + s;
  A.P.cx[o] = cx;
  A.P.cy[o] = cy;
  A.P.cs[o] = cs;
  A.P.sn[o] = sn;
}

__global__ void __launch_bounds__(256) conflict_pair_kernel(ConflictPairArgs A) {
  __shared__ double s_pose[4][4][kConflictTile]; // [wave][cx | cy | cs | sn][j]: the J-tile at the wave's sample
  __shared__ double s_sep[4][kConflictTile];     // the waves' minima, for the merge
  __shared__ int s_idx[4][4][kConflictTile];     // [wave][sep_sample | sep_partner | conflict_sample | conflict_partner][lane]
  const ConflictPoses &P = A.P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.y * kConflictTile;
  const int i = blockIdx.x * kConflictTile + lane; // < S_pad
  // a tile without a plan on either side: no sample is walked (every wave decides alike)
  const bool any = __ballot(P.occupied[i] != 0) != 0 && __ballot(P.occupied[j0 + lane] != 0) != 0;
  const int K = any ? P.K : 0;
  double bs = kCfInf;
  int bk = -1, bj = -1, fk = -1, fj = -1;
  double(*sp)[kConflictTile] = s_pose[wave];
  for (int k = wave; k < K; k += 4) {
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
    if (blockIdx.x == blockIdx.y) cand &= ~(1ull << lane); // the tile against itself: not i against i
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
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the next sample's stores stay behind these reads
    __builtin_amdgcn_wave_barrier();
  }
  s_sep[wave][lane] = bs;
  s_idx[wave][0][lane] = bk;
  s_idx[wave][1][lane] = bj;
  s_idx[wave][2][lane] = fk;
  s_idx[wave][3][lane] = fj;
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < 4; w++) {
      cf_merge_sep(bs, bk, bj, s_sep[w][lane], s_idx[w][0][lane], s_idx[w][1][lane]);
      cf_merge_first(fk, fj, s_idx[w][2][lane], s_idx[w][3][lane]);
    }
    const size_t o = (size_t)blockIdx.y * P.S_pad + i;
    A.part.min_sep[o] = bs;
    A.part.sep_sample[o] = bk;
    A.part.sep_partner[o] = bj;
    A.part.conflict_sample[o] = fk;
    A.part.conflict_partner[o] = fj;
  }
}

__global__ void __launch_bounds__(256) conflict_reduce_kernel(ConflictReduceArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n_slots) return;
  double bs = kCfInf;
  int bk = -1, bj = -1, fk = -1, fj = -1;
  for (int t = 0; t < A.tiles; t++) {
    const size_t o = (size_t)t * A.S_pad + i;
    cf_merge_sep(bs, bk, bj, A.part.min_sep[o], A.part.sep_sample[o], A.part.sep_partner[o]);
    cf_merge_first(fk, fj, A.part.conflict_sample[o], A.part.conflict_partner[o]);
  }
  A.out.min_sep[i] = bs;
  A.out.sep_sample[i] = bk;
  A.out.sep_partner[i] = bj;
  A.out.conflict_sample[i] = fk;
  A.out.conflict_partner[i] = fj;
}

hipError_t launch_conflict_poses(const ConflictPoseArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(conflict_pose_kernel, dim3(A.P.S_pad / kConflictTile, (A.P.K + 3) / 4), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_conflict_pairs(const ConflictPairArgs &A, hipStream_t stream) {
  const int tiles = A.P.S_pad / kConflictTile;
  hipLaunchKernelGGL(conflict_pair_kernel, dim3(tiles, tiles), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_conflict_reduce(const ConflictReduceArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(conflict_reduce_kernel, dim3((A.n_slots + 255) / 256), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
