// conflict_trigger_args.h — what the host half of the conflict trigger (dftpav_planner_check_yield, the trigger stage of
// dftpav_replan_tick, dftpav_debug_conflict_trigger) hands the kernels of conflict_trigger.hip.  docs/NEXT_ROWS.md §4.29.
#pragma once
#include "conflict_args.h"

namespace dftpav {

// can_yield(s): the slot holds a plan and !(t_now > end_time[n_seg - 1]), read from the table's rows; the debug hook brings the
// flags themselves (flags [S_pad], 0 behind the last slot) and no table is read.
struct TriggerYield {
  ExecTable T;                // read only; not read when flags is set
  double t_now;
  const unsigned char *flags; // nullptr: from the table
};

// The lexicographic minimum (k, j) of one slot over the pair-samples that could make it yield: over one J-tile (the partial rows
// [tiles][S_pad]) or over all of them (the outputs [slots]).  -1, -1: none.
struct TriggerRows {
  int *sample, *partner;
};

// trigger_pair_kernel: workgroup (I-tile, J-tile) writes the partial row jt * S_pad + i of every slot i of its I-tile
struct TriggerPairArgs {
  ConflictPoses P; // read only
  TriggerYield Y;
  TriggerRows part;
  PairConsts V;
};
static_assert(offsetof(TriggerPairArgs, V) == offsetof(TriggerPairArgs, part) + sizeof(TriggerRows) && sizeof(TriggerPairArgs) == offsetof(TriggerPairArgs, V) + 32,
              "the four doubles lie where they lay");

// trigger_reduce_kernel: slot i's partial rows merged into its output row; yield = can_yield(i) && sample >= 0
struct TriggerReduceArgs {
  TriggerRows part, out;
  int *yield; // [slots]
  TriggerYield Y;
  const unsigned char *occupied; // [S_pad], the poses'
  int n_slots, S_pad, tiles;
};

} // namespace dftpav
