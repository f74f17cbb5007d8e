// conflict_sep.h — the separation of two footprints and the lexicographic merges of the rows, stated once for the kernels that
// relate poses: conflict.hip (slot against slot, docs/NEXT_ROWS.md §4.23) and cand_conflict.hip (candidate against slot, §4.26).
// Steps 2 and 3 of the definition in include/dftpav_hip.h: fp64, no contraction, the expressions and the corner order of
// footprint_hits (footprint.h).  Plain device functions over values; a kernel keeps its own poses.
#pragma once
#include <hip/hip_runtime.h>

namespace dftpav {

constexpr double kCfInf = __builtin_huge_val();
constexpr double kCfNaN = __builtin_nan("");

// the four corners of the box about (cx, cy) with heading (cs, sn): footprint_hits' c1 .. c4
__device__ inline void cf_corners(double cx, double cy, double cs, double sn, double hl, double hw, double *X, double *Y) {
  X[0] = cx + hl * cs + hw * sn; Y[0] = cy + hl * sn - hw * cs;
  X[1] = cx + hl * cs - hw * sn; Y[1] = cy + hl * sn + hw * cs;
  X[2] = cx - hl * cs - hw * sn; Y[2] = cy - hl * sn + hw * cs;
  X[3] = cx - hl * cs + hw * sn; Y[3] = cy - hl * sn - hw * cs;
}

// does one of the owner's two axes separate it from the box with the corners (X, Y)?
__device__ inline bool cf_separates(double cx, double cy, double cs, double sn, const double *X, const double *Y, double hl, double hw) {
  bool xp = true, xn = true, yp = true, yn = true;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const double dx = X[q] - cx, dy = Y[q] - cy;
    const double lx = cs * dx + sn * dy, ly = cs * dy - sn * dx;
    xp = xp && lx > hl;
    xn = xn && lx < -hl;
    yp = yp && ly > hw;
    yn = yn && ly < -hw;
  }
  return xp || xn || yp || yn;
}

// the smallest squared distance of the corners (PX, PY) to the four edges of the box with the corners (EX, EY), folded into m
__device__ inline double cf_corners_to_edges(const double *PX, const double *PY, const double *EX, const double *EY, double m) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const double ax = EX[e], ay = EY[e];
    const double abx = EX[(e + 1) & 3] - ax, aby = EY[(e + 1) & 3] - ay;
    const double den = abx * abx + aby * aby;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const double apx = PX[q] - ax, apy = PY[q] - ay;
      double u = (apx * abx + apy * aby) / den;
      u = !(u > 0.0) ? 0.0 : (u > 1.0 ? 1.0 : u);
      const double qx = ax + u * abx, qy = ay + u * aby;
      const double ex = PX[q] - qx, ey = PY[q] - qy;
      const double d = ex * ex + ey * ey;
      m = d < m ? d : m;
    }
  }
  return m;
}

// steps 2 and 3 for the boxes a and b
__device__ inline double cf_sep(double ax, double ay, double ac, double as, double bx, double by, double bc, double bs, double hl, double hw) {
  double AX[4], AY[4], BX[4], BY[4];
  cf_corners(ax, ay, ac, as, hl, hw, AX, AY);
  cf_corners(bx, by, bc, bs, hl, hw, BX, BY);
  const bool sa = cf_separates(ax, ay, ac, as, BX, BY, hl, hw);
  const bool sb = cf_separates(bx, by, bc, bs, AX, AY, hl, hw);
  if (!(sa || sb)) return 0.0;
  double m = kCfInf;
  m = cf_corners_to_edges(AX, AY, BX, BY, m);
  m = cf_corners_to_edges(BX, BY, AX, AY, m);
  return sqrt(m);
}

// (sep, k, j) of b into a under the lexicographic minimum; k < 0: nothing
__device__ inline void cf_merge_sep(double &as, int &ak, int &aj, double bs, int bk, int bj) {
  if (bk >= 0 && (ak < 0 || bs < as || (bs == as && (bk < ak || (bk == ak && bj < aj))))) {
    as = bs;
    ak = bk;
    aj = bj;
  }
}
// (k, j) likewise
__device__ inline void cf_merge_first(int &ak, int &aj, int bk, int bj) {
  if (bk >= 0 && (ak < 0 || bk < ak || (bk == ak && bj < aj))) {
    ak = bk;
    aj = bj;
  }
}

} // namespace dftpav
