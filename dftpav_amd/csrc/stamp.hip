// Vehicle footprints stamped into the handle's grid map on the device (docs/NEXT_ROWS.md §4.24): every stage that plans or checks a
// plan reads the occupancy grid alone, so another vehicle reaches them as occupied cells.  The boxes are rows of
// dftpav_planner_sample_poses -- conflict_pose_kernel's output as it lies -- or the caller's own.
//
// A box (cx, cy, cs, sn) with hl = 0.5 * veh_length + inflate, hw = 0.5 * veh_width + inflate covers the cell (ix, iy) iff, in fp64
// without contraction,
//   X = origin_x + (double)ix * resolution,  Y = origin_y + (double)iy * resolution
//   dx = X - cx,  dy = Y - cy
//   lx = cs * dx + sn * dy,  ly = cs * dy - sn * dx          (the frame of conflict.hip's cf_separates)
//   fabs(lx) <= hl && fabs(ly) <= hw
// and a box with a member that is not finite covers nothing.  A covered cell of the working map becomes 80.  This is defined over
// every cell of the grid; the range of cells a wave walks is an optimisation.  It is the axis-aligned box of the covered set --
// half extents (|cs| hl + |sn| hw) / (cs^2 + sn^2) and (|sn| hl + |cs| hw) / (cs^2 + sn^2), exact for any (cs, sn), unit or not --
// widened by a cell on every side for the rounding of its own arithmetic, and the whole grid where that arithmetic gives a NaN.
//
// Three kernels.  stamp_box_kernel: one wave per box, four per workgroup; a wave whose box is unselected, not finite or wholly outside
// the grid leaves at once, the others walk the rows of their clipped range with the 64 lanes on 64 consecutive ix from a multiple of
// 32, and the covered lanes store the byte.  Every writer writes 80, so the stores of overlapping boxes race to the same result.
// Where the map has a bit map, the wave's ballot is the two 32-bit words of its 64 cells; lanes 0 and 32 OR theirs in, split over
// two words where the row's first bit is not word-aligned (the bit of a cell is ix + size_x * iy).  stamp_bits_kernel makes the bit map
// again from the bytes after the base copy was put back.  stamp_count_kernel counts the cells that are 80 now and were not in the
// base: integer partial sums, one per workgroup, added on the host in order.
#include <hip/hip_runtime.h>

#include "stamp_args.h"

namespace dftpav {

namespace {

// the first and the last cell of [a, b] (already widened) inside [0, n): a NaN gives the whole side
__device__ inline int stamp_lo(double a, int n) { return a > 0.0 ? (a < (double)n ? (int)a : n) : 0; }
__device__ inline int stamp_hi(double b, int n) { return b < (double)(n - 1) ? (b >= 0.0 ? (int)b : -1) : n - 1; }

// of the four bytes of c: those that are 80 while b's are not
__device__ inline unsigned stamp_new4(unsigned c, unsigned b) {
  unsigned n = 0;
#pragma unroll
  for (int q = 0; q < 32; q += 8) n += ((c >> q) & 0xffu) == 80u && ((b >> q) & 0xffu) != 80u ? 1u : 0u;
  return n;
}
// the bits of four bytes: bit q set where byte q is 80
__device__ inline unsigned stamp_bits4(unsigned c) {
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) m |= ((c >> (8 * q)) & 0xffu) == 80u ? 1u << q : 0u;
  return m;
}

} // namespace

__global__ void __launch_bounds__(256) stamp_box_kernel(StampBoxArgs A) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= A.n_boxes) return;
  if (A.select && A.select[b % A.S_pad] == 0) return;
  const double cx = A.cx[b], cy = A.cy[b], cs = A.cs[b], sn = A.sn[b];
  if (!(__builtin_isfinite(cx) && __builtin_isfinite(cy) && __builtin_isfinite(cs) && __builtin_isfinite(sn))) return;
  const double r2 = cs * cs + sn * sn;
  const double ex = (fabs(cs) * A.hl + fabs(sn) * A.hw) / r2, ey = (fabs(sn) * A.hl + fabs(cs) * A.hw) / r2;
  const int ix0 = stamp_lo(floor((cx - ex - A.origin_x) / A.resolution) - 1.0, A.size_x);
  const int ix1 = stamp_hi(ceil((cx + ex - A.origin_x) / A.resolution) + 1.0, A.size_x);
  const int iy0 = stamp_lo(floor((cy - ey - A.origin_y) / A.resolution) - 1.0, A.size_y);
  const int iy1 = stamp_hi(ceil((cy + ey - A.origin_y) / A.resolution) + 1.0, A.size_y);
  if (ix0 > ix1 || iy0 > iy1) return; // wholly outside
  for (int iy = iy0; iy <= iy1; iy++) { // 0 <= iy < size_y
    const double Y = A.origin_y + (double)iy * A.resolution;
    const double dy = Y - cy;
    const size_t row = (size_t)iy * (size_t)A.size_x;
    for (long long x0 = ix0 & ~31; x0 <= ix1; x0 += 64) {
      const long long ix = x0 + lane; // >= 0
      bool covered = false;
      if (ix < A.size_x) {
        const double X = A.origin_x + (double)ix * A.resolution;
        const double dx = X - cx;
        const double lx = cs * dx + sn * dy, ly = cs * dy - sn * dx;
        covered = fabs(lx) <= A.hl && fabs(ly) <= A.hw;
      }
      if (covered) A.cells[row + (size_t)ix] = 80;
      if (A.bits) {
        const unsigned long long m = __ballot(covered);
        const unsigned half = lane < 32 ? (unsigned)m : (unsigned)(m >> 32);
        if ((lane & 31) == 0 && half) { // (a set bit is a cell of the grid, so both words lie inside the bit map)
          const size_t g = row + (size_t)ix; // the bit of this half's first cell
          const unsigned sh = (unsigned)(g & 31);
          atomicOr(&A.bits[g >> 5], half << sh);
          if (sh && (half >> (32 - sh))) atomicOr(&A.bits[(g >> 5) + 1], half >> (32 - sh));
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) stamp_bits_kernel(StampBitsArgs A) {
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t c0 = w * 32;
  if (c0 >= A.n_cells) return;
  unsigned m = 0;
  if (c0 + 32 <= A.n_cells) { // (the map is a device allocation: 32 w is aligned for the loads)
    const uint4 lo = *(const uint4 *)(A.cells + c0), hi = *(const uint4 *)(A.cells + c0 + 16);
    m = stamp_bits4(lo.x) | stamp_bits4(lo.y) << 4 | stamp_bits4(lo.z) << 8 | stamp_bits4(lo.w) << 12 | stamp_bits4(hi.x) << 16 |
        stamp_bits4(hi.y) << 20 | stamp_bits4(hi.z) << 24 | stamp_bits4(hi.w) << 28;
  } else {
    for (size_t i = c0; i < A.n_cells; i++) m |= A.cells[i] == 80 ? 1u << (i - c0) : 0u;
  }
  A.bits[w] = m;
}

__global__ void __launch_bounds__(256) stamp_count_kernel(StampCountArgs A) {
  __shared__ unsigned s_n[4];
  unsigned n = 0;
  const size_t n16 = A.n_cells / 16;
  const uint4 *c = (const uint4 *)A.cells, *b = (const uint4 *)A.base;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 cw = c[i], bw = b[i];
    n += stamp_new4(cw.x, bw.x) + stamp_new4(cw.y, bw.y) + stamp_new4(cw.z, bw.z) + stamp_new4(cw.w, bw.w);
  }
  if (blockIdx.x == 0) // the bytes behind the last whole sixteen
    for (size_t i = n16 * 16 + threadIdx.x; i < A.n_cells; i += 256) n += A.cells[i] == 80 && A.base[i] != 80 ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) A.partial[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

hipError_t launch_stamp_boxes(const StampBoxArgs &A, hipStream_t stream) {
  if (A.n_boxes <= 0) return hipSuccess;
  hipLaunchKernelGGL(stamp_box_kernel, dim3((unsigned)(((long long)A.n_boxes + 3) / 4)), dim3(256), 0, stream, A);
  return hipGetLastError();
}
hipError_t launch_stamp_bits(const StampBitsArgs &A, hipStream_t stream) {
  const size_t words = (A.n_cells + 31) / 32;
  hipLaunchKernelGGL(stamp_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, A);
  return hipGetLastError();
}
int stamp_count_blocks(size_t n_cells) {
  const size_t want = (n_cells / 16 + 255) / 256;
  return (int)(want < 1 ? 1 : (want > (size_t)kStampCountBlocks ? (size_t)kStampCountBlocks : want));
}
hipError_t launch_stamp_count(const StampCountArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(stamp_count_kernel, dim3(stamp_count_blocks(A.n_cells)), dim3(256), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
