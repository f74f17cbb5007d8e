// traj_segments.h — the gear segments of one trajectory as the sampled read-outs keep them in LDS (limits.hip, clearance.hip): per
// segment its first piece, piece count, direction and piece duration, and the running count of CheckReplan's samples in front of
// it (traj_server_ros.cpp:385-387; a sample's global index is validate's first_sample index).  One thread fills the table, the
// workgroup reads it after a barrier.  validate.hip, replan.hip and states.hip keep their segments in kernel arguments and scalar
// registers and do not use it.
#pragma once
#include "plan_args.h"

namespace dftpav {

struct SegTable {
  int count[kMaxSeg + 1]; // samples of the segments before segment i; count[M]: all of them
  int piece0[kMaxSeg], pn[kMaxSeg], sg[kMaxSeg];
  double dt[kMaxSeg];
};

// trajectory b of a solved batch: the launch-wide layout, the duration of a segment summed from its piece duration piece_dt[i]
__device__ inline void fill_from_batch(SegTable &S, const SampleTable &tab, const DevLayout &L, const double *piece_dt) {
  const int M = L.M;
  int acc = 0;
  for (int i = 0; i < M; i++) {
    const double dtp = piece_dt[i];
    S.piece0[i] = L.seg_piece0[i];
    S.pn[i] = L.piece_nums[i];
    S.sg[i] = L.singuls[i];
    S.dt[i] = dtp;
    S.count[i] = acc;
    acc += pe::samples_below(tab, pe::segment_duration(L.piece_nums[i], dtp));
  }
  S.count[M] = acc;
}

// slot s of the executing table (n_seg[s] > 0): the slot's own layout row, the duration of a segment as the table stores it
__device__ inline void fill_from_slot(SegTable &S, const SampleTable &tab, const ExecTable &T, int s) {
  const int MS = T.max_seg;
  const int M = T.n_seg[s];
  int acc = 0, p0 = 0;
  for (int i = 0; i < M; i++) {
    S.piece0[i] = p0; // the pieces of a slot's segments follow one another
    S.pn[i] = T.piece_nums[(size_t)s * MS + i];
    S.sg[i] = T.singul[(size_t)s * MS + i];
    S.dt[i] = T.coeff_dt[(size_t)s * MS + i];
    p0 += S.pn[i];
    S.count[i] = acc;
    acc += pe::samples_below(tab, T.duration[(size_t)s * MS + i]);
  }
  S.count[M] = acc;
}

} // namespace dftpav
