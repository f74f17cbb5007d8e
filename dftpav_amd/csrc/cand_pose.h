// cand_pose.h — the pose of a candidate plan at a clock, stated once for the kernels that evaluate it: cand_conflict.hip (candidate
// against slot, docs/NEXT_ROWS.md §4.26) and joint_select.hip (candidate against candidate, §4.28).  The statements are those of
// the definition in include/dftpav_hip.h; a kernel keeps its own CandSegs in LDS and fills it once per workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "cand_conflict_args.h"

namespace dftpav {

// the segments of a workgroup's 64 candidates: the layout's rows, and per candidate the piece duration and the duration of each
struct CandSegs {
  double dur[kMaxSeg][kConflictTile], dtp[kMaxSeg][kConflictTile];
  int pn[kMaxSeg], sg[kMaxSeg], p0[kMaxSeg];
};

// filled by the whole workgroup of 256 threads for the candidates c0 .. c0 + 63; ends with a barrier
__device__ inline void cand_fill_segments(CandSegs &S, const CandBatch &C, int c0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int M = C.L.M, c = c0 + lane;
  for (int i = wave; i < M; i += 4) {
    const double dtp = c < C.B ? C.piece_dt[(size_t)c * M + i] : 0.0;
    S.dtp[i][lane] = dtp;
    S.dur[i][lane] = pe::segment_duration(C.L.piece_nums[i], dtp);
  }
  if ((int)threadIdx.x < M) {
    S.pn[threadIdx.x] = C.L.piece_nums[threadIdx.x];
    S.sg[threadIdx.x] = C.L.singuls[threadIdx.x];
    S.p0[threadIdx.x] = C.L.seg_piece0[threadIdx.x];
  }
  __syncthreads();
}

// the pose of candidate c (< B; its segments in column `lane` of S) at clock t: conflict_pose_kernel's statements over the chained times
__device__ inline void cand_pose(const CandBatch &C, const CandSegs &S, int c, int lane, double t, double &cx, double &cy, double &cs,
                                 double &sn) {
  const int M = C.L.M;
  int e = 0;
  double st = C.t_start, d = S.dur[0][lane], en = st + d; // exec_adopt_kernel: world = t_start; end = world + d
  while (e < M - 1 && en <= t) {
    e++;
    st = en; // the next segment starts at that end
    d = S.dur[e][lane];
    en = st + d;
  }
  double tt = t - st;
  if (tt < 0.0) tt = 0.0;
  if (tt > d) tt = d;
  const int idx = pe::locate_piece(S.pn[e], S.dtp[e][lane], tt);
  const double *q = C.coeffs + ((size_t)c * C.L.Ntot + (size_t)(S.p0[e] + idx)) * 12;
  double px, py, vx, vy;
  pe::piece_pos(q, tt, px, py);
  pe::piece_vel(q, tt, vx, vy);
  const double sgn = (double)S.sg[e];
  const double yaw = crt::atan2(sgn * vy, sgn * vx);
  crt::sincos(yaw, sn, cs);
  cx = px + C.dcr * cs;
  cy = py + C.dcr * sn;
}

} // namespace dftpav
