// The obstacle-aware cost-to-go of the grid map (docs/NEXT_ROWS.md §4.20): for a goal cell c*, F[c] is the cost of the cheapest
// 8-connected path between c and c*, an axial step 5, a diagonal step 7, int32, integer arithmetic only.  It is what the hybrid A*
// search takes as max(getHeu, .) when dftpav_set_search_heuristic is on: the term the reference left commented out at
// kino_astar.cpp:247 (`lambda_heu_ * getObsHeu(pro_state.head(2))`; no getObsHeu exists there), the "holonomic with obstacles"
// heuristic of Dolgov et al.
//
//   blocked     a cell with d2 <= T, d2 the distance field of the map (distfield.hip), T = floor(r^2 / resolution^2)
//   moves       the field spreads from c*: a step from a cell n that has a value into a neighbour c inside the grid is allowed iff
//               c is not blocked; a diagonal step additionally needs the two cells it passes between (n.x, c.y) and (c.x, n.y) not
//               blocked -- no corner cutting.  Both conditions are symmetric in the diagonal's side cells, so F[c] is also the cost
//               of walking from c to c* under "every cell entered after c, c* excepted, is free".
//   seed        F[c*] = 0 whether c* is blocked or not (a blocked c* spreads to its free neighbours, and is entered by nothing)
//   unreached   DFTPAV_FIELD_UNREACHED (INT32_MAX).  A path enters a cell at most once: F <= 7 * 16384^2 < 2^31 on the largest map.
//
// F is the unique fixed point of F[c] = min(F[c], F[n] + w(n, c)) over these moves above the seed -- Dijkstra's values (what
// oracle_goalfield/ computes with a binary heap) -- so any schedule of relaxations that runs until nothing changes gives the same
// integers.  The schedule here:
//
// ONE workgroup of 256 threads per field, and nothing but that workgroup ever touches the field or its dirty map: no barrier, wait
// or atomic between workgroups, no host round trip.  The workgroup takes a dirty tile of 64 x 32 cells with a one-cell halo into
// LDS (66 x 34 words, 8976 bytes); bit 31 of a word is the cell's blocked flag (halo cells outside the grid: blocked, unreached), so
// one LDS read gives a neighbour's value and whether a diagonal may pass it.  It relaxes the tile to the tile's own fixed point in
// place: a row sweep (a thread owns 8 consecutive cells of a row and relaxes them left to right, then right to left, in registers,
// from the three rows it read), then a column sweep (8 consecutive cells of a column, lanes along x: conflict-free), a barrier
// between them and a workgroup-wide "changed" vote (__syncthreads_or) after each pair.  A cell is written by its owner only, a
// value read from a neighbour is old or new and either is the cost of a real path, so the races between a sweep's reads and writes
// are harmless; a pair of sweeps in which nobody wrote has read one unchanging state, which is therefore the fixed point.  The tile
// is written back where it differs from the field, the up to eight neighbour tiles whose facing border (or corner) cell changed
// are marked dirty, and the next dirty tile is taken: the nearest one ahead in tile order, the direction turning round at either
// end (a front moving against the order then needs a turn, not a full scan per tile row).  The kernel ends when no tile is dirty.
//
// Termination: every store lowers an integer that is bounded below by 0, so there are finitely many stores; a sweep pair
// repeats only after a store, and a tile is marked dirty only after a store to a border cell; so finitely many tile passes of
// finitely many sweeps.  Exactness at the end: no tile is dirty, so every tile was relaxed to its fixed point against halo values
// that have not changed since (a change would have marked it); hence no move anywhere lowers a value.
//
// The windowed instance, goal_field_kernel<true> (dftpav_set_search_heuristic_window, docs/NEXT_ROWS.md §4.22): the field of a
// window (X0, Y0, WX, WY) of the grid that dftpav_goal_window chose -- a rectangle of whole tiles of the tiling above (X0 a
// multiple of 64, Y0 of 32; its last column and row of tiles partial only where the grid's are), the goal cell inside it --
// stored compactly as [WY][WX].  It is the field above of the cropped map: every rule is the same, a cell outside the window
// is what a cell outside the grid is (blocked and unreached in a halo, never written), and blocked is still d2 <= T with d2 the
// distance field of the WHOLE map, read at the cell's grid coordinates, so an obstacle outside the window inflates into it.  A
// cell whose only way to c* leaves the window stays unreached.  The kernel runs in the window's own coordinates: tile t of the
// window is tile (X0 / 64 + t % tiles_x, Y0 / 32 + t / tiles_x) of the grid, its dirty map has one word per tile of the window,
// and the grid's coordinates appear in the one expression that reads d2.  Still one workgroup per field and nothing between
// workgroups.  goal_field_kernel<false> is the kernel of before: the same instructions, registers and LDS, but for one
// constant, the offset of the implicit arguments behind GoalFieldArgs, which is 24 bytes longer; launch_goal_fields picks.
//
// Termination, windowed: the argument above names the grid nowhere.  The window has finitely many cells, every store lowers an
// int32 that is bounded below by 0, a sweep pair repeats and a tile is marked only after a store; so finitely many tile passes
// over a finite tile set.  Exactness likewise, for the moves that stay inside the window.
//
// Resources (gfx950, the code object's notes): goal_field_kernel<false> 121 VGPRs, 62 SGPRs, 9256 bytes of LDS (the tile's 8976,
// the votes), no scratch, 4 waves per SIMD; goal_field_kernel<true> 122 VGPRs, 64 SGPRs, the same LDS, no scratch, 4 waves per SIMD.
#include <hip/hip_runtime.h>

#include <climits>

#include "goalfield_args.h"

namespace dftpav {

constexpr unsigned kGfBlockedBit = 0x80000000u, kGfValueMask = 0x7fffffffu;

// the relaxed value of a non-blocked cell m from its eight neighbours (u: up, d: down, l, r and the four diagonals).  An unreached
// neighbour gives 0x7fffffff + w as an unsigned candidate, which is above every value: no test for it.
__device__ inline unsigned gf_cell(unsigned ul, unsigned u, unsigned ur, unsigned l, unsigned m, unsigned r, unsigned dl, unsigned d,
                                   unsigned dr) {
  if (m & kGfBlockedBit) return m; // never entered (a blocked seed keeps its 0)
  unsigned best = m;
  best = min(best, (u & kGfValueMask) + kGfAxial);
  best = min(best, (d & kGfValueMask) + kGfAxial);
  best = min(best, (l & kGfValueMask) + kGfAxial);
  best = min(best, (r & kGfValueMask) + kGfAxial);
  const unsigned bu = u >> 31, bd = d >> 31, bl = l >> 31, br = r >> 31;
  if (!(bu | bl)) best = min(best, (ul & kGfValueMask) + kGfDiagonal);
  if (!(bu | br)) best = min(best, (ur & kGfValueMask) + kGfDiagonal);
  if (!(bd | bl)) best = min(best, (dl & kGfValueMask) + kGfDiagonal);
  if (!(bd | br)) best = min(best, (dr & kGfValueMask) + kGfDiagonal);
  return best;
}

// One sweep over the 8 cells base[ALONG], ..., base[8 * ALONG] of this thread (base[0] and base[9 * ALONG] belong to the neighbours
// along the line, base[. +- ACROSS] to the lines beside it): forwards, then backwards, in registers; the cells that came out lower
// are stored.  Returns whether any was.
template <int ALONG, int ACROSS> __device__ inline int gf_sweep(unsigned *base) {
  unsigned U[10], M[10], D[10], O[8];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    U[k] = base[k * ALONG - ACROSS];
    M[k] = base[k * ALONG];
    D[k] = base[k * ALONG + ACROSS];
  }
#pragma unroll
  for (int k = 0; k < 8; k++) O[k] = M[k + 1];
#pragma unroll
  for (int i = 1; i <= 8; i++) M[i] = gf_cell(U[i - 1], U[i], U[i + 1], M[i - 1], M[i], M[i + 1], D[i - 1], D[i], D[i + 1]);
#pragma unroll
  for (int i = 8; i >= 1; i--) M[i] = gf_cell(U[i - 1], U[i], U[i + 1], M[i - 1], M[i], M[i + 1], D[i - 1], D[i], D[i + 1]);
  int changed = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (M[k + 1] != O[k]) {
      base[(k + 1) * ALONG] = M[k + 1];
      changed = 1;
    }
  return changed;
}

// WINDOW: the field of a window of the grid (see the header).  (x, y), sx, sy, the tiles and the dirty map below are then the
// window's own -- cell (x, y) of the field is cell (wx0 + x, wy0 + y) of the grid -- and the grid is met in one place, where d2 is read.
template <bool WINDOW> __global__ void __launch_bounds__(kGfThreads) goal_field_kernel(GoalFieldArgs A) {
  __shared__ unsigned tile[kGfRows * kGfStride];
  __shared__ int s_ahead, s_min, s_max, s_mark, s_count;
  const int lane = threadIdx.x, g = blockIdx.x;
  const int wx0 = WINDOW ? A.window[4 * g] : 0, wy0 = WINDOW ? A.window[4 * g + 1] : 0;
  const int sx = WINDOW ? A.window[4 * g + 2] : A.size_x, sy = WINDOW ? A.window[4 * g + 3] : A.size_y;
  const int tiles_x = WINDOW ? (sx + kGfTileX - 1) / kGfTileX : A.tiles_x, tiles_y = WINDOW ? (sy + kGfTileY - 1) / kGfTileY : A.tiles_y;
  const int n_tiles = tiles_x * tiles_y;
  int *F = WINDOW ? A.fields + A.offset[g] : A.fields + (size_t)g * sx * sy;
  int *dirty = A.dirty + (WINDOW ? (size_t)g * A.dirty_stride : (size_t)g * n_tiles);
  if (lane == 0) { // the seed (inside the grid, and inside its window: the host's check)
    const int gx = A.goal_cell[2 * g] - wx0, gy = A.goal_cell[2 * g + 1] - wy0;
    F[(size_t)gy * sx + gx] = 0;
    // every tile that holds the seed, in its cells or in its halo: the seed's own tile does not "change" it, so a seed on a tile's
    // border would never mark the tile beside it
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int x = gx + dx, y = gy + dy;
        if (x >= 0 && x < sx && y >= 0 && y < sy) dirty[(y / kGfTileY) * tiles_x + x / kGfTileX] = 1;
      }
    s_count = 0;
  }
  int reached = lane == 0 ? 1 : 0; // cells this thread took from unreached to a value
  // the thread's 8 cells of a row sweep (row lane / 8, columns 8 (lane % 8) ...) and of a column sweep (column lane % 64, rows
  // 8 (lane / 64) ...), each as the address of the cell in front of them
  unsigned *const row_base = tile + ((lane >> 3) + 1) * kGfStride + 8 * (lane & 7);
  unsigned *const col_base = tile + (8 * (lane >> 6)) * kGfStride + (lane & 63) + 1;
  int cursor = 0, dir = 1;
  for (;;) {
    __syncthreads(); // the marks of the last pass (and the seed) are written, its votes are read
    if (lane == 0) {
      s_ahead = dir > 0 ? INT_MAX : -1;
      s_min = INT_MAX;
      s_max = -1;
      s_mark = 0;
    }
    __syncthreads();
    for (int t = lane; t < n_tiles; t += kGfThreads)
      if (dirty[t]) {
        atomicMin(&s_min, t);
        atomicMax(&s_max, t);
        if (dir > 0 && t >= cursor) atomicMin(&s_ahead, t);
        if (dir < 0 && t <= cursor) atomicMax(&s_ahead, t);
      }
    __syncthreads();
    if (s_max < 0) break; // no tile is dirty
    int t = s_ahead;
    if (dir > 0 && t == INT_MAX) {
      dir = -1;
      t = s_max;
    } else if (dir < 0 && t < 0) {
      dir = 1;
      t = s_min;
    }
    cursor = t + dir;
    const int tx = t % tiles_x, ty = t / tiles_x;
    const int x0 = tx * kGfTileX, y0 = ty * kGfTileY;
    if (lane == 0) dirty[t] = 0;
    for (int c = lane; c < kGfRows * kGfStride; c += kGfThreads) {
      const int cy = c / kGfStride, cx = c - cy * kGfStride;
      const int x = x0 - 1 + cx, y = y0 - 1 + cy;
      unsigned v = kGfBlockedBit | kGfValueMask;
      if (x >= 0 && x < sx && y >= 0 && y < sy) {
        const size_t idx = (size_t)y * sx + x;
        const size_t map_idx = WINDOW ? (size_t)(wy0 + y) * A.size_x + (size_t)(wx0 + x) : idx; // d2 is the whole map's
        v = (unsigned)F[idx] | (A.d2[map_idx] <= A.T ? kGfBlockedBit : 0u);
      }
      tile[c] = v;
    }
    __syncthreads();
    int changed;
    do {
      changed = gf_sweep<1, kGfStride>(row_base);
      __syncthreads();
      changed |= gf_sweep<kGfStride, 1>(col_base);
    } while (__syncthreads_or(changed));
    // write back what differs; bits 0..7 of the mark: the neighbour tile at (dx, dy) = (k % 3 - 1, k / 3 - 1), k = bit + (bit >= 4)
    int mark = 0;
    for (int c = lane; c < kGfTileX * kGfTileY; c += kGfThreads) {
      const int cy = c / kGfTileX, cx = c - cy * kGfTileX;
      const int x = x0 + cx, y = y0 + cy;
      if (x >= sx || y >= sy) continue;
      const size_t idx = (size_t)y * sx + x;
      const int v = (int)(tile[(cy + 1) * kGfStride + cx + 1] & kGfValueMask), old = F[idx];
      if (v == old) continue;
      F[idx] = v;
      if (old == INT_MAX) reached++;
      // the tiles that see this cell in their halo: beside it in x, in y, and across the corner
      const int ex = cx == 0 ? -1 : cx == kGfTileX - 1 ? 1 : 0, ey = cy == 0 ? -1 : cy == kGfTileY - 1 ? 1 : 0;
      if (ex) mark |= ex < 0 ? 1 << 3 : 1 << 4;
      if (ey) mark |= ey < 0 ? 1 << 1 : 1 << 6;
      if (ex && ey) mark |= ey < 0 ? (ex < 0 ? 1 << 0 : 1 << 2) : (ex < 0 ? 1 << 5 : 1 << 7);
    }
    if (mark) atomicOr(&s_mark, mark);
    __syncthreads();
    if (lane < 8 && ((s_mark >> lane) & 1)) {
      const int k = lane + (lane >= 4 ? 1 : 0);
      const int nx = tx + k % 3 - 1, ny = ty + k / 3 - 1;
      if (nx >= 0 && nx < tiles_x && ny >= 0 && ny < tiles_y) dirty[ny * tiles_x + nx] = 1;
    }
  }
  if (reached) atomicAdd(&s_count, reached);
  __syncthreads();
  if (lane == 0) A.n_reached[g] = s_count;
}

hipError_t launch_goal_fields(const GoalFieldArgs &A, int n, hipStream_t stream) {
  if (A.window) hipLaunchKernelGGL(goal_field_kernel<true>, dim3((unsigned)n), dim3(kGfThreads), 0, stream, A);
  else hipLaunchKernelGGL(goal_field_kernel<false>, dim3((unsigned)n), dim3(kGfThreads), 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
