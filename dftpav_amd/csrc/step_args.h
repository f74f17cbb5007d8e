// step_args.h — what the host half of the steps around a solve (capi_steps.cpp) hands validate.hip, shot.hip and corridor.hip.
#pragma once
#include "device_types.h"
#include "footprint.h"
#include "piece_eval.h"

namespace dftpav {

// validate_kernel: the collision re-check of the first B trajectories of a solved batch
struct ValidateArgs {
  DevGrid grid;
  DevFootprint fp;
  SampleTable tab;
  const double *coeffs;   // [B][Ntot][6][2]
  const double *piece_dt; // [B][M]
  DevLayout L;
  int B;
  int *collision, *first_sample; // [B]
};

// shot_kernel: n Reeds-Shepp shots
struct ShotArgs {
  const double *from, *to; // [n][3]
  int n;
  double rho, checkl;
  int max_samples;
  DevGrid grid; // grid.cells == nullptr: no collision check
  DevFootprint fp;
  double *length;  // [n]
  int *type;       // [n]
  double *seg;     // [n][5]
  double *samples; // [n][max_samples][3]
  int *n_samples;  // [n]
  int *collides;   // [n]
};

// corridor_kernel: the rectangles of n states
struct CorridorArgs {
  DevGrid grid;
  const unsigned *bits; // the same map, one bit per cell (set = OCCUPIED), or nullptr when it does not fit in LDS
  double res_rcp;       // 1.0 / grid.resolution (launch_corridor sets it)
  const double *states; // [n][3]
  int n;
  double veh_width, veh_length, veh_dcr;
  const double *dl; // running sum 0, checkl, checkl + checkl, ...
  int n_dl;
  double *hpoly; // [n][4][4], or nullptr:
  // the solve path's own layout, [trajectory][4 * plane + component][NptsPad] with unit normals
  // (traj_optimizer.cpp:49-52), state i being point i % Npts of trajectory i / Npts
  double *batch_cor;
  int Npts, NptsPad;
  int replicate; // every trajectory i / Npts is written `replicate` times: trajectories t * replicate + r (restarts share a corridor)
};

} // namespace dftpav
