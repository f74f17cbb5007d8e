// search_args.h — what the host half of dftpav_kino_search (capi.cpp) hands the search kernel (search.hip).
#pragma once
#include "../../include/dftpav_hip.h"
#include "footprint.h"
#include "piece_eval.h"
#include "rstable_args.h"

namespace dftpav {

constexpr int kSearchThreads = 256; // one workgroup per query
constexpr int kSearchMaxIn = 32;    // inputs per expansion
constexpr int kSearchMaxCheck = 8;  // check_num
constexpr int kSearchMaxShot = 1024; // shot sample offsets in the table

struct SearchNode { // PathNode, kino_astar.h:42-61
  double x, y, yaw, g, f, steer, arc;
  int parent, ix, iy, yaw_idx, singul;
  int state;
};

struct SearchArgs {
  dftpav_search_params sp;
  DevGrid grid;
  DevFootprint fp; // the search's own vehicle, from sp (veh_*: vp_ + 0.2 m, kino_astar.cpp:426-427)
  const double *l_tab; // shot sample offsets: 0, checkl, checkl + checkl, ...
  int n_l;
  const double *in_tab; // [3][kSearchMaxIn][2] (steer, arc): first expansion forward, backward, later expansions
  int n_in[3];
  double inv_yaw_res, origin_sx, origin_sy, half_size_x, half_size_y, rho; // origin_ = -0.5 map_size (kino_astar.cpp:408-409)
  const double *start, *end; // [n][4]
  int q0, n;
  // workspace, per slot (query in flight)
  SearchNode *pool;
  int *h_node, *h_pos, *path_idx; // [slots][allocate_num]
  double *h_key;
  int *table; // [slots][hcap]
  int hcap;
  dftpav_search_out out; // device pointers
  // the goal fields of dftpav_set_search_heuristic (goalfield.hip); read only by the kernel launched with a field
  const int *fields;   // [distinct goals of this launch][size_y][size_x]
  const int *field_of; // [n] the field of query q, -1: none (a goal outside the grid)
  double unit;         // metres of heuristic per unit of the field: scale * resolution / 5
  // the Reeds-Shepp table of dftpav_set_search_rs_heuristic (rstable.hip); read only by the kernel launched with a table
  RsLookup rs;
  // windowed fields (dftpav_set_search_heuristic_window): field f covers the window field_win[f] = (X0, Y0, WX, WY) of the grid
  // and is [WY][WX] at fields + field_off[f].  nullptr: whole-map fields, as `fields` says; read only by the kernel launched with windowed fields
  const int *field_win;       // [distinct fields of this launch][4]
  const long long *field_off; // [distinct fields of this launch], in ints
};

} // namespace dftpav
