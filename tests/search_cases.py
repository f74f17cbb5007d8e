"""The searches that tests/test_search_oracle.py (the CPU restatement alone: does the case still take its branch?) and
tests/test_gpu_search.py (the device against the restatement, bit for bit) share: one table of cases, one cached oracle run per case.

A case is (scene, parameter changes, yaw): scene "wall_gap" / "maze" is one query, "arena" the 12 default-arena goals from the ego
start in one call; yaw, if given, replaces the yaw of start and goal."""
import functools
import math

import numpy as np

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_search import pysearch as ps

REACH_END, NO_PATH = 2, 3

CASES = {"default-wall-gap": ("wall_gap", {}, None), "default-arena": ("arena", {}, None)}
# 1. the budget exit
BUDGET = {f"budget-wall-gap-max_iters={m}-retry_2d={r}": ("wall_gap", dict(max_iters=m, retry_2d=r), None)
          for m in (0, 1, 5, 30) for r in (0, 1)}
BUDGET["budget-arena-max_iters=50"] = ("arena", dict(max_iters=50), None)
# 2. node-pool exhaustion, in a hash table of 128, 128, 512 (wall_gap) and 1024 (arena) slots
POOL = {f"pool-wall-gap-allocate_num={a}-retry_2d={r}": ("wall_gap", dict(allocate_num=a, retry_2d=r), None)
        for a in (40, 64, 200) for r in (0, 1)}
POOL.update({f"pool-arena-allocate_num=300-retry_2d={r}": ("arena", dict(allocate_num=300, retry_2d=r), None) for r in (0, 1)})
# 3. the bounds of the search space (wall_gap lies in x 0 .. 12, its way round the wall in y 3 .. 9)
BOUNDS = {f"bounds-{x}x{y}": ("wall_gap", dict(map_size_x=float(x), map_size_y=float(y)), None)
          for x, y in ((30, 14), (26, 12), (24.2, 20))}
# 4. one parameter off its default
PARAMS = {"steer-change-wall-gap": ("wall_gap", dict(traj_steer_change_penalty=2.0), None),
          "steer-change-arena": ("arena", dict(traj_steer_change_penalty=2.0), None)}
PARAMS.update({f"{k}={v}": ("wall_gap", {k: v}, None) for k, v in (
    ("check_num", 3), ("check_num", 8), ("step_arc", 0.6), ("phi_grid_resolution", 0.15), ("max_frontend_cur", 0.5),
    ("checkl", 0.1), ("map_resl", 0.2), ("vertex_res", 0.25), ("lambda_heu", 1.0))})
# 5. start and goal yaws outside [-pi, pi): normalize_angle wraps once, which brings 7.0 inside (0.72) and leaves 10.0 outside
# (3.72: it would need two; its yaw cells lie beyond the last cell of a wrapped yaw)
YAWS = {f"yaw={name}": ("wall_gap", {}, y) for name, y in (
    ("4.0", 4.0), ("-3.5", -3.5), ("pi", math.pi), ("-pi", -math.pi), ("7.0", 7.0), ("10.0", 10.0))}
# 6. a large search
MAZE = {"maze": ("maze", dict(max_iters=ss.MAZE_MAX_ITERS), None)}
for group in (BUDGET, POOL, BOUNDS, PARAMS, YAWS, MAZE):
    CASES.update(group)
NEW_CASES = [c for c in CASES if not c.startswith("default-")]


def queries(case):
    """(grid, resolution, origin, starts [n][4], goals [n][4], SearchParams) of a case"""
    scene, changes, yaw = CASES[case]
    if scene == "arena":
        grid, res, org, start, goals = ss.arena()
        S, E = np.repeat(start[None], len(goals), 0), goals
    else:
        _, grid, res, org, st, en = getattr(ss, scene)()
        S, E = st[None].copy(), en[None].copy()
    if yaw is not None:
        S[:, 2] = yaw
        E[:, 2] = yaw
    return grid, res, org, S, E, SearchParams.default().copy(**changes)


@functools.lru_cache(maxsize=None)
def oracle(case):
    """the restatement's answer in order 2, computed once per session; read only"""
    grid, res, org, S, E, sp = queries(case)
    r = ps.kino_search(grid, res, org, S, E, sp=sp, order=2, nthreads=8 if len(S) > 1 else 1)
    for v in r.values():
        v.setflags(write=False)
    return r
