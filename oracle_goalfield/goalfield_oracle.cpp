// TEST INFRASTRUCTURE ONLY: CPU yardstick of dftpav_grid_goal_field (dftpav_amd/csrc/goalfield.hip): Dijkstra with a binary heap.
//
// For a goal at (x, y) on a grid map, cell c* = round((p - origin) / resolution), F[c] is the cost of the cheapest 8-connected path
// between c and c*: an axial step 5, a diagonal step 7, int32.  A cell is blocked iff d2 <= T, d2 the squared cell distance to the
// nearest occupied cell (the caller's: pygoalfield.py takes it from oracle_clearance's Meijster restatement, or from the brute
// force there) and T = (int)floor(r * r / (resolution * resolution)).  The search spreads from c*: a step enters a cell inside the
// grid that is not blocked; a diagonal step also needs the two cells it passes between not blocked.  c* is seeded with 0 whether
// it is blocked or not; a goal outside the grid seeds nothing; unreached cells hold INT32_MAX.
//
// Nothing of the kernel is shared: no tiles, no sweeps -- a std::priority_queue of (cost, cell), lazy deletion.
#include <climits>
#include <cmath>
#include <cstddef>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace {
const int kUnreached = INT_MAX;

int threshold(double r, double res) {
  const double t = std::floor(r * r / (res * res));
  return t >= 2147483646.0 ? 2147483646 : (int)t;
}
} // namespace

extern "C" int oracle_goal_threshold(double inflate_radius, double resolution) { return threshold(inflate_radius, resolution); }

// d2 [size_y][size_x]; goals_xy [n][2]; field [n][size_y][size_x]; n_reached [n]; cell [n][2]: the goal's cell, (-1, -1) outside
extern "C" void oracle_goal_field(const int *d2, int size_x, int size_y, double resolution, double origin_x, double origin_y,
                                  const double *goals_xy, int n, double inflate_radius, int *field, int *n_reached, int *cell) {
  const int T = threshold(inflate_radius, resolution);
  const size_t cells = (size_t)size_x * size_y;
  std::vector<char> blocked(cells);
  for (size_t i = 0; i < cells; i++) blocked[i] = d2[i] <= T;
  for (int g = 0; g < n; g++) {
    int *F = field + (size_t)g * cells;
    for (size_t i = 0; i < cells; i++) F[i] = kUnreached;
    n_reached[g] = 0;
    cell[2 * g] = cell[2 * g + 1] = -1;
    const double cx = std::round((goals_xy[2 * g] - origin_x) / resolution), cy = std::round((goals_xy[2 * g + 1] - origin_y) / resolution);
    if (!(cx >= 0.0 && cx < (double)size_x && cy >= 0.0 && cy < (double)size_y)) continue;
    const int gx = (int)cx, gy = (int)cy;
    cell[2 * g] = gx;
    cell[2 * g + 1] = gy;
    typedef std::pair<long long, int> Item; // cost, cell
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> open;
    F[gx + size_x * gy] = 0;
    open.push(Item(0, gx + size_x * gy));
    while (!open.empty()) {
      const Item it = open.top();
      open.pop();
      const int c = it.second;
      if (it.first != F[c]) continue; // an entry that a cheaper one replaced
      n_reached[g]++;
      const int x = c % size_x, y = c / size_x;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          if (!dx && !dy) continue;
          const int nx = x + dx, ny = y + dy;
          if (nx < 0 || nx >= size_x || ny < 0 || ny >= size_y) continue;
          if (blocked[nx + size_x * ny]) continue;
          if (dx && dy && (blocked[nx + size_x * y] || blocked[x + size_x * ny])) continue; // no corner cutting
          const long long cost = it.first + (dx && dy ? 7 : 5);
          if (cost < F[nx + size_x * ny]) {
            F[nx + size_x * ny] = (int)cost;
            open.push(Item(cost, nx + size_x * ny));
          }
        }
    }
  }
}
