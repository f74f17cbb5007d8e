"""Queries for the hybrid A* front end (dftpav_kino_search): small hand-made maps that each exercise one branch of
KinoAstar::search (kino_astar.cpp:37-301), and goals on the reference's default arena that the direct shot cannot reach.

Every scene is (name, grid [size_y][size_x] uint8 (80 = occupied), resolution, origin, start [4], goal [4]); start and
goal are (x, y, yaw, v) as TrajPlanner::getKinoPath passes them (traj_manager.cpp:74)."""
import numpy as np

from . import scenarios as sc

RES = 0.2
ORIGIN = (-20.0, -20.0)
SIZE = 200                      # 40 m x 40 m


def _grid():
    return np.full((SIZE, SIZE), 127, dtype=np.uint8)


def _box(g, x0, y0, x1, y1):
    """occupies the cells whose centres lie in [x0, x1] x [y0, y1]"""
    xs = ORIGIN[0] + np.arange(SIZE) * RES
    ys = ORIGIN[1] + np.arange(SIZE) * RES
    ix = (xs >= x0 - 1e-9) & (xs <= x1 + 1e-9)
    iy = (ys >= y0 - 1e-9) & (ys <= y1 + 1e-9)
    g[np.ix_(iy, ix)] = 80
    return g


def empty():
    """nothing in the way: a start at rest reaches the goal by the shot from the start node (iteration 0)"""
    return "empty", _grid(), RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([8.0, 3.0, 0.5, 0.0])


def moving_start():
    """a start moving forwards: the first expansion takes only the forward arcs map_resl and 2 map_resl (:143-151)"""
    return "moving", _grid(), RES, ORIGIN, np.array([0.0, 0.0, 0.3, 1.5]), np.array([9.0, 2.0, 0.3, 0.0])


def wall_gap():
    """a wall across the way with a gap to one side: the shot from the start collides, the search goes round"""
    g = _box(_grid(), 5.0, -20.0, 6.0, 3.0)
    g = _box(g, 5.0, 9.0, 6.0, 20.0)
    return "wall-gap", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([12.0, 0.0, 0.0, 0.0])


def reverse():
    """a goal behind a start that is rolling backwards: the first expansion is reverse only (:152-159)"""
    g = _box(_grid(), -20.0, 3.0, 20.0, 4.0)
    g = _box(g, -20.0, -4.0, 20.0, -3.0)
    return "reverse", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, -1.0]), np.array([-8.0, 0.0, 0.0, 0.0])


def enclosed():
    """a start boxed in by walls (the goal outside): the open set runs dry, in 3D and in the 2D retry (:298-300)"""
    g = _grid()
    for x0, y0, x1, y1 in ((-3.5, -3.0, 5.5, -2.0), (-3.5, 2.0, 5.5, 3.0), (-3.5, -3.0, -2.5, 3.0), (4.5, -3.0, 5.5, 3.0)):
        g = _box(g, x0, y0, x1, y1)
    return "enclosed", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([12.0, 0.0, 0.0, 0.0])


def occupied_start():
    g = _box(_grid(), -1.0, -1.0, 1.0, 1.0)
    return "occupied-start", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([10.0, 0.0, 0.0, 0.0])


def occupied_goal():
    g = _box(_grid(), 9.0, -1.0, 11.0, 1.0)
    return "occupied-goal", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([10.0, 0.0, 0.0, 0.0])


def small_scenes():
    return [empty(), moving_start(), wall_gap(), reverse(), enclosed(), occupied_start(), occupied_goal()]


MAZE_MAX_ITERS = 2000           # the oracle (order 2) ends on this budget with nodes_used = 5337 (4162 at 1500, 6638 at 2500)


def maze():
    """two staggered walls between start and goal: a search of thousands of nodes (a deep heap with in-place key changes).  Not one
    of small_scenes(): at the default budget it runs its 20 000 iterations out, with 28 677 nodes.  Run it with
    max_iters = MAZE_MAX_ITERS, the smallest multiple of 500 at which the oracle uses 5000 nodes or more; it ends on that budget."""
    g = _box(_grid(), -8.0, -20.0, -7.0, 10.0)
    g = _box(g, -1.0, -10.0, 0.0, 20.0)
    return "maze", g, RES, ORIGIN, np.array([-15.0, -5.0, 0.0, 0.0]), np.array([3.0, 0.0, 0.0, 0.0])


PARALLEL_SLOT_MAX_ITERS = 2000  # the oracle (order 2) ends by a free shot after 506 pops (1713 nodes) without the Reeds-Shepp table
RS_SMALL = dict(n_yaw=16, extent=6.0, cell=0.5)   # the table geometry of the tests: 16 x 25 x 25 entries


def parallel_slot():
    """a bay 10 m long between two blocks with a wall behind it, beside the lane the vehicle stands in; the goal is the start moved
    3.5 m sideways into the bay, heading unchanged.  Straight-line distance and goal field are small from the first node on; what is
    left to do is all heading.  The shot from the start collides with the rear block.  Not one of small_scenes(); run it with
    max_iters = PARALLEL_SLOT_MAX_ITERS."""
    g = _box(_grid(), 6.0, -6.5, 11.0, -1.5)
    g = _box(g, -9.0, -6.5, -4.0, -1.5)
    g = _box(g, -9.0, -6.5, 11.0, -4.9)
    return "parallel-slot", g, RES, ORIGIN, np.array([0.0, 0.0, 0.0, 0.0]), np.array([0.0, -3.5, 0.0, 0.0])


# goals on the default arena (sc.default_sim_map): free poses near the ego vehicle whose direct shot from the ego start
# collides (checked by tests/test_search_oracle.py)
ARENA_GOALS = np.array([
    [-62.7, 34.3, 0.0, 0.0],
    [-44.4, 24.5, 2.8, 0.0],
    [-63.5, 33.4, -2.9, 0.0],
    [-50.4, 22.9, 0.6, 0.0],
    [-43.8, 39.1, 1.5, 0.0],
    [-45.3, 24.3, 2.6, 0.0],
    [-43.3, 37.7, -0.8, 0.0],
    [-44.9, 23.6, 2.8, 0.0],
    [-43.6, 21.6, 0.0, 0.0],
    [-61.5, 34.5, -2.4, 0.0],
    [-50.0, 24.2, -2.1, 0.0],
    [-47.0, 22.8, 3.0, 0.0],
])


def arena():
    """(grid, resolution, origin, start [4], goals [k][4]) on the default arena, the ego vehicle at rest"""
    grid, origin, res, ego = sc.default_sim_map()
    start = np.array([ego[0], ego[1], ego[2], 0.0])
    return grid, res, origin, start, ARENA_GOALS.copy()


def arena_plan_queries():
    """(grid, resolution, origin, starts [14][4], goals [14][4]) for dftpav_plan_queries on the default arena: ARENA_GOALS from the
    ego start, then a goal inside an obstacle (no path) and one closer than 1 m to the start (arrived)."""
    grid, res, origin, start, goals = arena()
    extra = np.array([[-47.8, 40.0, 0.0, 0.0],
                      [start[0] + 0.6, start[1] + 0.3, start[2], 0.0]])
    goals = np.concatenate([goals, extra])
    return grid, res, origin, np.repeat(start[None], len(goals), 0), goals


# ---- maps for the goal field (dftpav_grid_goal_field, tests/test_goalfield_oracle.py and tests/test_gpu_goalfield.py).  Each is
# (name, grid [size_y][size_x] uint8, resolution, origin); cell (ix, iy) has its centre at origin + resolution * (ix, iy).
FIELD_RES = 0.25
FIELD_ORIGIN = (-3.0, 2.0)
FIELD_EXACT_RADIUS = 0.75       # r^2 / res^2 = 9 exactly: cells at the cell distance 3 from an occupied one have d2 == T


def cell_centre(ix, iy, res=FIELD_RES, origin=FIELD_ORIGIN):
    return (origin[0] + res * ix, origin[1] + res * iy)


def field_free(size_x, size_y):
    """no occupied cell: the distance field is FAR everywhere and nothing is blocked, whatever the radius"""
    return "free-%dx%d" % (size_x, size_y), np.full((size_y, size_x), 127, dtype=np.uint8), FIELD_RES, FIELD_ORIGIN


def field_random(size_x, size_y, density, seed):
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((size_y, size_x)) < density, 80, 127).astype(np.uint8)
    return "random-%dx%d-%g" % (size_x, size_y, density), g, FIELD_RES, FIELD_ORIGIN


def field_pocket(size_x=67, size_y=35):
    """a ring of occupied cells round a free pocket: the pocket stays unreached from outside, and the outside from within"""
    g = np.full((size_y, size_x), 127, dtype=np.uint8)
    x0, y0, x1, y1 = size_x // 2 - 4, size_y // 2 - 3, size_x // 2 + 4, size_y // 2 + 3
    g[y0:y1 + 1, x0:x1 + 1] = 80
    g[y0 + 1:y1, x0 + 1:x1] = 127
    return "pocket", g, FIELD_RES, FIELD_ORIGIN


def field_corner_pair(size_x=65, size_y=33):
    """two occupied cells that touch at a corner, across the corner where four tiles of 64 x 32 would meet: the diagonal between
    them is not taken"""
    g = np.full((size_y, size_x), 127, dtype=np.uint8)
    g[31, 63] = 80
    g[32, 64] = 80
    return "corner-pair", g, FIELD_RES, FIELD_ORIGIN


def field_serpentine(size_x=130, size_y=70):
    """walls every fourth row, open at alternating ends: the only path from the bottom row to the top runs the full width of every
    corridor, through every tile of 64 x 32 several times, and the walls stop any other spreading -- a tile is revisited"""
    g = np.full((size_y, size_x), 127, dtype=np.uint8)
    for k, y in enumerate(range(3, size_y, 4)):
        g[y, :] = 80
        if k % 2 == 0:
            g[y, size_x - 2:] = 127
        else:
            g[y, :2] = 127
    return "serpentine", g, FIELD_RES, FIELD_ORIGIN
