// The grid map rendered on the device from the arena's obstacle set (docs/NEXT_ROWS.md §4.25): what DataRenderer::GetObstacleMap and
// FakeMapper do every cycle on the host (data_renderer.cc:146-259) -- wipe the grid to a background byte, fill the obstacle circles
// and polygons, set the remembered obstacle points -- so that a cycle is "render, stamp, plan, clear" and no map crosses the bus.
//
// The definition (normative in include/dftpav_hip.h, "the rendered map"), restated.  Every cell starts as `background`; a covered
// cell becomes 80; every writer writes 80, so order and overlap do not show.  All arithmetic is fp64 without contraction.  A world
// coordinate snaps to a cell coordinate as rint((p - origin) / resolution), halves to even; the host does it (render_args.h), the
// kernels start from the integers.
//   Polygon with snapped vertices (X_v, Y_v); edge e from vertex e to vertex e + 1, cyclic.  One whose snapped bounding box misses
//   the grid covers nothing.
//     interior, for each row y in [max(minY, 0), min(maxY, size_y - 1)]:
//       edge e crosses the row iff (Y0 <= y && Y1 > y) || (Y1 <= y && Y0 > y)
//       its abscissa is t = (double)(y - Y0) / (double)(Y1 - Y0), x = (double)X0 + t * (double)(X1 - X0)
//       the abscissae of the row sorted ascending (equal values are interchangeable); each pair (a, b) at positions (2k, 2k + 1)
//       covers ix in [max(ceil(a), 0), min(floor(b), size_x - 1)]
//     outline, for each edge: n = max(|X1 - X0|, |Y1 - Y0|) + 1 steps, step k the cell
//       (rint((double)k * sx + (double)X0), rint((double)k * sy + (double)Y0)), sx = (double)(X1 - X0) / (double)(n - 1), sy
//       likewise; the last step is exactly (X1, Y1); n == 1 is the single cell (X0, Y0); steps outside the grid are dropped
//   Circle with the snapped centre (cx, cy) and r = (int)(radius / resolution): the cells with integer dx * dx + dy * dy <= r * r,
//   clipped to the grid.
//   Point: its snapped cell, if that lies inside the grid.
//
// Five kernels.  render_fill_kernel: the background in 16-byte stores.  render_poly_kernel: a wave per (polygon, row) -- the rows of
// a polygon are dealt round the waves of its workgroups -- with lane e holding edge e; a ballot of the crossing lanes, each of which
// ranks its abscissa among the others' through lane reads (at most 64 values: no sort in LDS); then the 64 lanes sweep each pair's
// span, 64 consecutive ix from a multiple of 64 per step, with byte stores.  render_outline_kernel: a wave per edge, a lane per step;
// along the edge's longer axis the step is exactly one cell, so the steps inside the grid on that axis are an integer range and only
// they are walked.  render_circle_kernel: a wave per (circle, row), the half width of the row from an integer square root.
// render_point_kernel: a thread per point.  All writers store the same byte, so their races end in the same map; nothing is atomic.
#include <hip/hip_runtime.h>

#include "render_args.h"

namespace dftpav {

namespace {

// lane j's value of v, j the same in every lane
__device__ inline double render_lane_read(double v, int j) {
  const int u = __builtin_amdgcn_readfirstlane(j);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), u), __builtin_amdgcn_readlane(__double2loint(v), u));
}

// the cells [i0, i1] of row `row` (both inside the grid) by the wave's 64 lanes
__device__ inline void render_span(unsigned char *row, long long i0, long long i1, int lane) {
  for (long long x0 = i0 & ~63LL; x0 <= i1; x0 += 64) {
    const long long ix = x0 + lane;
    if (ix >= i0 && ix <= i1) row[ix] = 80;
  }
}

} // namespace

__global__ void __launch_bounds__(256) render_fill_kernel(unsigned char *cells, size_t n_cells, unsigned char background) {
  const unsigned w = 0x01010101u * background;
  const uint4 v = make_uint4(w, w, w, w);
  const size_t n16 = n_cells / 16; // (the map is a device allocation: aligned for the stores)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) ((uint4 *)cells)[i] = v;
  if (blockIdx.x == 0) // the bytes behind the last whole sixteen
    for (size_t i = n16 * 16 + threadIdx.x; i < n_cells; i += 256) cells[i] = background;
}

__global__ void __launch_bounds__(256) render_poly_kernel(RenderArgs A) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x; // < n_poly
  const int first = A.poly_off[p], nv = A.poly_off[p + 1] - first;
  if (nv <= 0) return;
  const int4 box = A.poly_box[p];
  if (box.y < 0 || box.w < 0 || box.x >= A.size_x || box.z >= A.size_y) return; // wholly outside
  const long long y_lo = box.z > 0 ? box.z : 0, y_hi = box.w < A.size_y - 1 ? box.w : A.size_y - 1;
  int4 e = make_int4(0, 0, 0, 0);
  if (lane < nv) e = A.edges[first + lane]; // (nv <= 64: the host refuses more)
  const long long X0 = e.x, Y0 = e.y, X1 = e.z, Y1 = e.w;
  const int wave = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = gridDim.y * 4;
  for (long long y = y_lo + wave; y <= y_hi; y += waves) { // 0 <= y < size_y
    const bool cross = lane < nv && ((Y0 <= y && Y1 > y) || (Y1 <= y && Y0 > y));
    const unsigned long long m = __ballot(cross);
    if (!m) continue;
    double x = 0.0;
    if (cross) {
      const double t = (double)(y - Y0) / (double)(Y1 - Y0);
      x = (double)X0 + t * (double)(X1 - X0);
    }
    int rank = 0; // of a crossing lane's abscissa among the row's; equal values in lane order
    for (unsigned long long mm = m; mm; mm &= mm - 1) {
      const int j = __builtin_ctzll(mm);
      const double xj = render_lane_read(x, j);
      rank += (xj < x || (xj == x && j < lane)) ? 1 : 0;
    }
    unsigned char *row = A.cells + (size_t)y * (size_t)A.size_x;
    const int pairs = __popcll(m) / 2;
    for (int k = 0; k < pairs; k++) {
      const unsigned long long ma = __ballot(cross && rank == 2 * k), mb = __ballot(cross && rank == 2 * k + 1); // one lane each
      const double a = render_lane_read(x, __builtin_ctzll(ma)), b = render_lane_read(x, __builtin_ctzll(mb));
      long long i0 = (long long)ceil(a), i1 = (long long)floor(b); // (between the polygon's abscissae: within +-2^30 and an ulp)
      if (i0 < 0) i0 = 0;
      if (i1 > A.size_x - 1) i1 = A.size_x - 1;
      render_span(row, i0, i1, lane);
    }
  }
}

__global__ void __launch_bounds__(256) render_outline_kernel(RenderArgs A) {
  const int lane = threadIdx.x & 63;
  const long long ei = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (ei >= A.n_vert) return;
  const int4 e = A.edges[ei];
  const long long X0 = e.x, Y0 = e.y, X1 = e.z, Y1 = e.w;
  const long long dx = X1 - X0, dy = Y1 - Y0, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const long long n1 = adx > ady ? adx : ady; // n - 1
  if (n1 == 0) {
    if (lane == 0 && X0 >= 0 && X0 < A.size_x && Y0 >= 0 && Y0 < A.size_y) A.cells[(size_t)Y0 * (size_t)A.size_x + (size_t)X0] = 80;
    return;
  }
  const double sx = (double)dx / (double)n1, sy = (double)dy / (double)n1;
  // along the longer axis s is +-1.0 and step k lies at exactly c0 + s k: the steps inside the grid on that axis are a range of k
  const bool by_x = adx == n1;
  const long long c0 = by_x ? X0 : Y0, s = by_x ? (dx < 0 ? -1 : 1) : (dy < 0 ? -1 : 1), size = by_x ? A.size_x : A.size_y;
  long long k_lo = s > 0 ? -c0 : c0 - (size - 1), k_hi = s > 0 ? size - 1 - c0 : c0;
  if (k_lo < 0) k_lo = 0;
  if (k_hi > n1) k_hi = n1;
  for (long long k = k_lo + lane; k <= k_hi; k += 64) {
    long long x, y;
    if (k == n1) {
      x = X1;
      y = Y1;
    } else {
      x = (long long)rint((double)k * sx + (double)X0);
      y = (long long)rint((double)k * sy + (double)Y0);
    }
    if (x >= 0 && x < A.size_x && y >= 0 && y < A.size_y) A.cells[(size_t)y * (size_t)A.size_x + (size_t)x] = 80;
  }
}

__global__ void __launch_bounds__(256) render_circle_kernel(RenderArgs A) {
  const int lane = threadIdx.x & 63;
  const int4 c = A.circles[blockIdx.x]; // < n_circle
  const long long cx = c.x, cy = c.y, r = c.z; // 0 <= r <= 2^30
  if (cx + r < 0 || cx - r >= A.size_x) return;
  const long long y_lo = cy - r > 0 ? cy - r : 0, y_hi = cy + r < A.size_y - 1 ? cy + r : A.size_y - 1;
  const int wave = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), waves = gridDim.y * 4;
  for (long long y = y_lo + wave; y <= y_hi; y += waves) { // 0 <= y < size_y, |y - cy| <= r
    const long long d = y - cy, rem = r * r - d * d;        // >= 0, <= 2^60
    long long w = (long long)sqrt((double)rem);             // the largest w with w * w <= rem: the estimate, then exactly
    while (w * w > rem) w--;
    while ((w + 1) * (w + 1) <= rem) w++;
    const long long i0 = cx - w > 0 ? cx - w : 0, i1 = cx + w < A.size_x - 1 ? cx + w : A.size_x - 1;
    render_span(A.cells + (size_t)y * (size_t)A.size_x, i0, i1, lane);
  }
}

__global__ void __launch_bounds__(256) render_point_kernel(RenderArgs A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_point) return;
  const int2 p = A.points[i];
  if (p.x >= 0 && p.x < A.size_x && p.y >= 0 && p.y < A.size_y) A.cells[(size_t)p.y * (size_t)A.size_x + (size_t)p.x] = 80;
}

hipError_t launch_render(const RenderArgs &A, hipStream_t stream) {
  const size_t n_cells = (size_t)A.size_x * (size_t)A.size_y;
  const size_t want = (n_cells / 16 + 255) / 256;
  hipLaunchKernelGGL(render_fill_kernel, dim3((unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want))), dim3(256), 0, stream, A.cells,
                     n_cells, A.background);
  if (hipError_t e = hipGetLastError()) return e;
  if (A.n_poly > 0 && A.n_vert > 0) {
    hipLaunchKernelGGL(render_poly_kernel, dim3((unsigned)A.n_poly, (unsigned)A.poly_chunks), dim3(256), 0, stream, A);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(render_outline_kernel, dim3((unsigned)(((long long)A.n_vert + 3) / 4)), dim3(256), 0, stream, A);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (A.n_circle > 0) {
    hipLaunchKernelGGL(render_circle_kernel, dim3((unsigned)A.n_circle, (unsigned)A.circle_chunks), dim3(256), 0, stream, A);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (A.n_point > 0) {
    hipLaunchKernelGGL(render_point_kernel, dim3((unsigned)(((long long)A.n_point + 255) / 256)), dim3(256), 0, stream, A);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

} // namespace dftpav
