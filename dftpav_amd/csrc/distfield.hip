// Exact Euclidean distance transform of the handle's occupancy grid (docs/NEXT_ROWS.md §4.19): for every cell the squared distance,
// in cell units, to the nearest OCCUPIED (80) cell,
//
//   d2[ix + size_x * iy] = min over cells (jx, jy) with cells[jx + size_x * jy] == 80 of (ix - jx)^2 + (iy - jy)^2,
//
// DFTPAV_DIST_FAR (INT32_MAX) everywhere on a map without an occupied cell.  int32, integer arithmetic only: the field is exact.
// A side is at most 16384 cells (the host refuses a larger map), so g * g + dy * dy <= 2 * 16383^2 < 2^31 - 1.
//
// Separable, two kernels, no atomics:
//   dist_rows_kernel   g[ix, iy] = the distance along x to the nearest occupied cell of row iy (FAR if the row has none).  One wave
//                      per row; the row is walked in chunks of 64 cells, once left to right and once right to left.  Within a
//                      chunk "the last occupied index at or before lane l" is an inclusive maximum scan over the lanes (six
//                      __shfl_up steps), "the next at or after" a minimum scan (__shfl_down); the carry between chunks is the
//                      scan's last lane, broadcast.  No serial loop over the cells of a row.
//   dist_cols_kernel   d2[ix, iy] = min over jy of g[ix, jy]^2 + (iy - jy)^2.  Lanes run along ix (memory is ix-fastest: a wave
//                      reads 64 contiguous g values per row); a thread walks outward from its own row, dy = 1, 2, ..., and stops
//                      when dy * dy >= best -- no farther row can lower the minimum, so the exit is exact and the work is
//                      proportional to the answer -- or when both rows are off the map.  g comes from L2: the rows a wave's
//                      neighbours in iy read are the same ones.
// A workgroup of either kernel is 64 x 4 threads: one wave along x, four rows (kDistTileX, kDistTileY).
#include <hip/hip_runtime.h>

#include <climits>

#include "clearance_args.h"

namespace dftpav {

__global__ void __launch_bounds__(256) dist_rows_kernel(DistFieldArgs A) {
  const int lane = threadIdx.x; // blockDim = (64, 4): a wave is one row
  const int iy = blockIdx.x * kDistTileY + threadIdx.y;
  if (iy >= A.size_y) return; // the whole wave
  const unsigned char *row = A.cells + (size_t)iy * A.size_x;
  int *g = A.g + (size_t)iy * A.size_x;
  const int n_chunks = (A.size_x + kDistTileX - 1) / kDistTileX;
  // left to right: g = ix - (the last occupied index <= ix)
  int carry = -1;
  for (int c = 0; c < n_chunks; c++) {
    const int ix = c * kDistTileX + lane;
    const bool in = ix < A.size_x;
    int last = (in && row[ix] == 80) ? ix : -1;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(last, off);
      if (lane >= off && o > last) last = o;
    }
    if (carry > last) last = carry;
    if (in) g[ix] = last >= 0 ? ix - last : INT_MAX;
    carry = __shfl(last, 63);
  }
  // right to left: the minimum with (the next occupied index >= ix) - ix
  carry = INT_MAX;
  for (int c = n_chunks - 1; c >= 0; c--) {
    const int ix = c * kDistTileX + lane;
    const bool in = ix < A.size_x;
    int next = (in && row[ix] == 80) ? ix : INT_MAX;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_down(next, off);
      if (lane + off < 64 && o < next) next = o;
    }
    if (carry < next) next = carry;
    if (in && next != INT_MAX) {
      const int d = next - ix;
      if (d < g[ix]) g[ix] = d;
    }
    carry = __shfl(next, 0);
  }
}

__global__ void __launch_bounds__(256) dist_cols_kernel(DistFieldArgs A) {
  const int ix = blockIdx.x * kDistTileX + threadIdx.x;
  const int iy = blockIdx.y * kDistTileY + threadIdx.y;
  if (ix >= A.size_x || iy >= A.size_y) return;
  const int *g = A.g + ix;
  const size_t sx = (size_t)A.size_x;
  int best = g[sx * iy];
  if (best != INT_MAX) best *= best;
  for (int dy = 1;; dy++) {
    const int up = iy - dy, dn = iy + dy;
    if (up < 0 && dn >= A.size_y) break;
    const int dd = dy * dy;
    if (dd >= best) break;
    if (up >= 0) {
      const int v = g[sx * up];
      if (v != INT_MAX && v * v + dd < best) best = v * v + dd;
    }
    if (dn < A.size_y) {
      const int v = g[sx * dn];
      if (v != INT_MAX && v * v + dd < best) best = v * v + dd;
    }
  }
  A.d2[sx * iy + ix] = best;
}

hipError_t launch_dist_field(const DistFieldArgs &A, hipStream_t stream) {
  const dim3 block(kDistTileX, kDistTileY);
  const unsigned by = (unsigned)((A.size_y + kDistTileY - 1) / kDistTileY);
  hipLaunchKernelGGL(dist_rows_kernel, dim3(by), block, 0, stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_cols_kernel, dim3((unsigned)((A.size_x + kDistTileX - 1) / kDistTileX), by), block, 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
