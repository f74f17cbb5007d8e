"""ctypes loader of the CPU yardstick of the goal field -- TEST INFRASTRUCTURE (goalfield_oracle.cpp).

Only tests/ and scripts/ import this."""
import ctypes as C
import math
import os

import numpy as np

from oracle_shared.loader import Loader


UNREACHED = 2147483647            # DFTPAV_FIELD_UNREACHED
AXIAL, DIAGONAL = 5, 7
DEFAULT_SCALE = 1.0 / math.sqrt(1.16)


def _declare(L):
    L.oracle_goal_threshold.restype = C.c_int
    L.oracle_goal_threshold.argtypes = [C.c_double, C.c_double]
    L.oracle_goal_field.restype = None
    L.oracle_goal_field.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p]


_load = Loader(os.path.dirname(os.path.abspath(__file__)), "libgoalfield_oracle.so",
               ("goalfield_oracle.cpp",), _declare)
build, lib = _load.build, _load.lib


def threshold(inflate_radius, resolution):
    """T = (int)floor(r * r / (resolution * resolution)): a cell is blocked iff d2 <= T"""
    return int(lib().oracle_goal_threshold(float(inflate_radius), float(resolution)))


def distance_field(grid, brute=False):
    """the squared cell distance to the nearest occupied cell: oracle_clearance's Meijster restatement, or its brute force"""
    from oracle_clearance import pyclearance as pc
    return (pc.field_brute if brute else pc.field)(grid)


def goal_field(grid, resolution, origin, goals_xy, inflate_radius=0.0, d2=None):
    """uint8 grid [size_y][size_x] (80 = occupied), goals [n][2] (x, y) -> dict(field int32 [n][size_y][size_x], n_reached [n],
    cell [n][2] -- the goal's cell (ix, iy), (-1, -1) outside the grid)"""
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    assert g.ndim == 2
    d2 = np.ascontiguousarray(distance_field(g) if d2 is None else d2, dtype=np.int32)
    assert d2.shape == g.shape
    xy = np.ascontiguousarray(goals_xy, dtype=np.float64).reshape(-1, 2)
    n = xy.shape[0]
    field = np.zeros((n,) + g.shape, dtype=np.int32)
    reached, cell = np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    lib().oracle_goal_field(d2.ctypes.data, g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), xy.ctypes.data, n,
                            float(inflate_radius), field.ctypes.data, reached.ctypes.data, cell.ctypes.data)
    return dict(field=field, n_reached=reached, cell=cell)


def search_fields(grid, resolution, origin, end_states, inflate_radius=0.0, scale=DEFAULT_SCALE):
    """what oracle_search.pysearch.kino_search takes for the heuristic of dftpav_set_search_heuristic: one field per distinct goal
    cell of end_states [n][4] -> dict(fields, field_of [n] (-1: the goal is outside the grid), unit)"""
    en = np.ascontiguousarray(end_states, dtype=np.float64).reshape(-1, 4)
    r = goal_field(grid, resolution, origin, en[:, :2], inflate_radius)
    keys, field_of, keep = {}, np.full(en.shape[0], -1, dtype=np.int32), []
    for q, (ix, iy) in enumerate(r["cell"]):
        if ix < 0:
            continue
        if (ix, iy) not in keys:
            keys[(ix, iy)] = len(keep)
            keep.append(q)
        field_of[q] = keys[(ix, iy)]
    fields = r["field"][keep] if keep else np.zeros((1,) + r["field"].shape[1:], dtype=np.int32)
    return dict(fields=np.ascontiguousarray(fields), field_of=field_of, unit=float(scale) * float(resolution) / 5.0)
