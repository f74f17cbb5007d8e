"""Shared by the goal-window tests (test_goal_window_cpu.py, test_gpu_goal_window.py, test_gpu_search_window.py): a numpy restatement
of the window rule of dftpav_goal_window, and the yardsticks of the windowed goal field and of the search that reads it, both made
from the unchanged oracles -- oracle_goalfield on the cropped map with the whole map's distance field, and oracle_search with that
field pasted into a whole-size array of UNREACHED."""
import math

import numpy as np

from oracle_goalfield import pygoalfield as pg

TILE_X, TILE_Y = 64, 32
U = pg.UNREACHED


def _round(v):
    """C's round(): to the nearest integer, halves away from zero (v - floor(v) is exact for a double)"""
    a = abs(v)
    r = math.floor(a) + (1 if a - math.floor(a) >= 0.5 else 0)
    return r if v >= 0.0 else -r


def window_rule(size_x, size_y, res, origin, start_xy, goal_xy, margin):
    """(X0, Y0, WX, WY), or None for a goal outside the grid: the rule as the issue states it, in Python integers"""
    gx, gy = _round((goal_xy[0] - origin[0]) / res), _round((goal_xy[1] - origin[1]) / res)
    if not (0 <= gx < size_x and 0 <= gy < size_y):
        return None
    sx, sy = _round((start_xy[0] - origin[0]) / res), _round((start_xy[1] - origin[1]) / res)
    sx, sy = min(max(sx, 0), size_x - 1), min(max(sy, 0), size_y - 1)
    m = int(math.ceil(margin / res))
    x0, x1 = max(0, min(sx, gx) - m), min(size_x - 1, max(sx, gx) + m)
    y0, y1 = max(0, min(sy, gy) - m), min(size_y - 1, max(sy, gy) + m)
    X0, X1 = x0 // TILE_X * TILE_X, min(size_x, (x1 // TILE_X + 1) * TILE_X)
    Y0, Y1 = y0 // TILE_Y * TILE_Y, min(size_y, (y1 // TILE_Y + 1) * TILE_Y)
    return X0, Y0, X1 - X0, Y1 - Y0


def goal_cell(res, origin, goal_xy):
    return _round((goal_xy[0] - origin[0]) / res), _round((goal_xy[1] - origin[1]) / res)


def cropped_field(grid, res, origin, goal_xy, r, win, d2_full=None):
    """the windowed field's yardstick: oracle_goalfield on the map cropped to win, its origin shifted, blocked by the WHOLE map's
    distance field -> (field [WY][WX], n_reached).  The cell the oracle found is checked against the goal's own, shifted.

    The oracle is handed the centre of the goal's cell, not the goal's own point: origin + res * X0 is a rounded sum, and a goal on
    the border between two cells of the grid -- ARENA_GOALS[0]: (-62.7 + 202) / 0.2 = 696.5 -- rounds to the other one in the
    shifted frame (the check below found it).  The field depends on the goal through its cell only."""
    X0, Y0, WX, WY = win
    d2 = pg.distance_field(grid) if d2_full is None else d2_full
    crop = np.ascontiguousarray(grid[Y0:Y0 + WY, X0:X0 + WX])
    gx, gy = goal_cell(res, origin, goal_xy)
    shifted = (origin[0] + res * X0, origin[1] + res * Y0)
    centre = np.array([[shifted[0] + res * (gx - X0), shifted[1] + res * (gy - Y0)]])
    o = pg.goal_field(crop, res, shifted, centre, r, d2=np.ascontiguousarray(d2[Y0:Y0 + WY, X0:X0 + WX]))
    assert tuple(o["cell"][0]) == (gx - X0, gy - Y0), (tuple(o["cell"][0]), (gx - X0, gy - Y0))
    return o["field"][0], int(o["n_reached"][0])


def windowed_fields(grid, res, origin, starts_xy, goals_xy, r, margin):
    """per (start, goal) pair: (windows [n][4] -- zeros for a goal outside the grid --, the list of cropped fields, n_reached [n])"""
    sy, sx = grid.shape
    d2 = pg.distance_field(grid)
    wins, fields, reached, seen = [], [], [], {}
    for st, go in zip(np.asarray(starts_xy, dtype=np.float64), np.asarray(goals_xy, dtype=np.float64)):
        w = window_rule(sx, sy, res, origin, st, go, margin)
        if w is None:
            wins.append((0, 0, 0, 0))
            fields.append(np.zeros((0, 0), dtype=np.int32))
            reached.append(0)
            continue
        key = (goal_cell(res, origin, go), w)
        if key not in seen:
            seen[key] = cropped_field(grid, res, origin, go, r, w, d2)
        wins.append(w)
        fields.append(seen[key][0])
        reached.append(seen[key][1])
    return np.array(wins, dtype=np.int32).reshape(-1, 4), fields, np.array(reached, dtype=np.int32)


def search_fields(grid, res, origin, start_states, end_states, r, margin, scale=pg.DEFAULT_SCALE):
    """what oracle_search.pysearch.kino_search takes for the search with windowed fields: per distinct (goal cell, window) the
    cropped field pasted into a whole-size array of UNREACHED -> dict(fields, field_of, unit)"""
    st = np.asarray(start_states, dtype=np.float64).reshape(-1, 4)
    en = np.asarray(end_states, dtype=np.float64).reshape(-1, 4)
    wins, fields, _ = windowed_fields(grid, res, origin, st[:, :2], en[:, :2], r, margin)
    keys, field_of, whole = {}, np.full(len(en), -1, dtype=np.int32), []
    for q in range(len(en)):
        X0, Y0, WX, WY = (int(v) for v in wins[q])
        if WX == 0:
            continue
        key = (goal_cell(res, origin, en[q]), (X0, Y0, WX, WY))
        if key not in keys:
            keys[key] = len(whole)
            f = np.full(grid.shape, U, dtype=np.int32)
            f[Y0:Y0 + WY, X0:X0 + WX] = fields[q]
            whole.append(f)
        field_of[q] = keys[key]
    arr = np.stack(whole) if whole else np.full((1,) + grid.shape, U, dtype=np.int32)
    return dict(fields=np.ascontiguousarray(arr), field_of=field_of, unit=float(scale) * float(res) / 5.0)
