// rstable_args.h — the Reeds-Shepp cost-to-go table of dftpav_set_search_rs_heuristic: what the host hands the kernel of
// rstable.hip, and the geometry by which the search kernel (search.hip) reads the table.
#pragma once
#include "../../include/dftpav_hip.h"
#include "cr_trig.h"
#include "rs_math.h"

namespace dftpav {

enum { kRsThreads = 256 }; // workgroup of rs_table_kernel

struct CrMath { // the shot's elementary functions, correctly rounded: what rs::Solver takes in search.hip and rstable.hip
  DFTPAV_HD static double sin(double x) { return crt::sin(x); }
  DFTPAV_HD static double cos(double x) { return crt::cos(x); }
  DFTPAV_HD static double atan2(double y, double x) { return crt::atan2(y, x); }
};

// T [n_yaw][n][n], n = 2 half + 1: T[k][j][i] is the Reeds-Shepp length from ((i - half) cell, (j - half) cell, k dth) to (0, 0, 0)
struct RsGeometry {
  int n_yaw, half, n;
  double cell, dth;
};

struct RsTableArgs {
  double *T;
  long long entries; // n_yaw * n * n
  RsGeometry g;
  double rho;
};

// what search_kernel<FIELD, true> reads; tab == nullptr: the kernels without the term
struct RsLookup {
  const double *tab;
  RsGeometry g;
  double scale;
};

} // namespace dftpav
