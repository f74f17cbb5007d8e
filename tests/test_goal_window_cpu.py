"""The window of a goal field (dftpav_goal_window, pure host code) against a numpy-free restatement of its rule; the three new names
in the header, in EXPORTS and in the library; the refusals that need no device; and, on the yardstick alone, what a window that cuts
the only route means: the cells behind the cut stay UNREACHED while the whole-map field reaches them."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import goal_window_cases as gw
from dftpav_amd import search_scenes as ss
from oracle_goalfield import pygoalfield as pg

NEW = ("dftpav_goal_window", "dftpav_set_search_heuristic_window", "dftpav_grid_goal_field_windowed")
RES, ORG = ss.FIELD_RES, ss.FIELD_ORIGIN
GRIDS = ((1, 1), (1, 130), (130, 1), (67, 35), (200, 200))
MARGINS = (0.0, 0.6, 1.0, 3.3, 1.0e4)          # 0; no multiple of 0.25; a multiple; more cells than a tile; larger than any of the maps


def _pairs(sx, sy):
    """(start, goal) points: the same cell, opposite corners both ways, cells round the tile borders, a start outside the grid on
    each side, a goal outside the grid"""
    c = lambda x, y: ss.cell_centre(x, y, RES, ORG)
    inside = [(0, 0), (sx - 1, sy - 1), (sx - 1, 0), (sx // 2, sy // 2), (min(63, sx - 1), min(31, sy - 1)), (min(64, sx - 1), min(32, sy - 1))]
    inside = list(dict.fromkeys(inside))
    pairs = [(c(*a), c(*b)) for a, b in itertools.product(inside, inside)]
    mid = c(sx // 2, sy // 2)
    pairs += [(c(-5, sy // 2), mid), (c(sx + 4, sy // 2), mid), (c(sx // 2, -7), mid), (c(sx // 2, sy + 9), mid), (c(-3, sy + 2), mid)]
    pairs += [(mid, c(-1, 0)), (mid, c(sx // 2, sy)), (mid, (ORG[0] + 1e4, ORG[1]))]
    return pairs


@pytest.mark.parametrize("size", GRIDS, ids=["%dx%d" % s for s in GRIDS])
def test_window_equals_the_rule(hiplib, size):
    sx, sy = size
    n_none = 0
    for margin in MARGINS:
        for st, go in _pairs(sx, sy):
            want = gw.window_rule(sx, sy, RES, ORG, st, go, margin)
            got = hiplib.goal_window(sx, sy, RES, ORG, st, go, margin)
            assert got == want, (size, margin, st, go, got, want)
            n_none += want is None
            if want is not None:
                X0, Y0, WX, WY = want
                assert X0 % 64 == 0 and Y0 % 32 == 0 and WX >= 1 and WY >= 1 and X0 + WX <= sx and Y0 + WY <= sy
                gx, gy = gw.goal_cell(RES, ORG, go)
                assert X0 <= gx < X0 + WX and Y0 <= gy < Y0 + WY
                if margin == 1.0e4:
                    assert want == (0, 0, sx, sy)
    assert n_none == 3 * len(MARGINS)


def test_points_off_the_cell_centres_round_as_the_goal_field_does(hiplib):
    """a goal half a cell short of a tile border and just beyond it; a start and a goal at the grid's outer half cell"""
    sx, sy = 200, 200
    for gx in (63.49, 63.51, 64.49, -0.49, 199.49):
        for gy in (31.49, 31.51, -0.49, 199.49):
            go = (ORG[0] + RES * gx, ORG[1] + RES * gy)
            st = (ORG[0] + RES * 70.2, ORG[1] + RES * 40.7)
            for margin in (0.0, 0.3):
                assert hiplib.goal_window(sx, sy, RES, ORG, st, go, margin) == gw.window_rule(sx, sy, RES, ORG, st, go, margin)


def test_the_names_are_declared_exported_and_present(hiplib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dftpav_hip.h")).read()
    declared = set(re.findall(r"\b(dftpav_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in hiplib.EXPORTS and getattr(hiplib.lib(), name) is not None, name


def test_refusals_without_a_device(hiplib):
    L = hiplib.lib()
    m = hiplib.GridMap(None, 67, 35, RES, ORG[0], ORG[1])
    xy, win = (C.c_double * 2)(0.0, 3.0), (C.c_int * 4)(7, 7, 7, 7)
    fn = L.dftpav_goal_window
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    assert fn(C.byref(m), xy, xy, 0.5, win) == 1 and tuple(win) == hiplib.goal_window(67, 35, RES, ORG, (0.0, 3.0), (0.0, 3.0), 0.5)
    for args in ((None, xy, xy, 0.5, win), (C.byref(m), None, xy, 0.5, win), (C.byref(m), xy, None, 0.5, win), (C.byref(m), xy, xy, 0.5, None),
                 (C.byref(m), xy, xy, -0.1, win), (C.byref(m), xy, xy, float("nan"), win), (C.byref(m), xy, xy, float("inf"), win)):
        assert fn(*args) == hiplib.E_INVALID, args[3:4]
    for bad in (hiplib.GridMap(None, 0, 35, RES, 0.0, 0.0), hiplib.GridMap(None, 67, -1, RES, 0.0, 0.0), hiplib.GridMap(None, 67, 35, 0.0, 0.0, 0.0),
                hiplib.GridMap(None, 67, 35, float("nan"), 0.0, 0.0)):
        assert fn(C.byref(bad), xy, xy, 0.5, win) == hiplib.E_INVALID
    with pytest.raises(hiplib.DftpavError) as e:
        hiplib.goal_window(67, 35, RES, ORG, (0.0, 3.0), (0.0, 3.0), -1.0)
    assert e.value.code == hiplib.E_INVALID
    # a NULL handle
    setw = L.dftpav_set_search_heuristic_window
    setw.argtypes = [C.c_void_p, C.c_double]
    assert setw(None, 1.0) == hiplib.E_INVALID and setw(None, -1.0) == hiplib.E_INVALID
    gfw = L.dftpav_grid_goal_field_windowed
    gfw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert gfw(None, xy, xy, 1, 0.0, 1.0, win, None, None, None) == hiplib.E_INVALID


def _cut(scene, start_cell, goal_cell, margin, r=0.0):
    """(the whole-map yardstick, the windowed yardstick pasted into the whole size, the window)"""
    name, g, res, org = scene
    go, st = ss.cell_centre(*goal_cell, res, org), ss.cell_centre(*start_cell, res, org)
    whole = pg.goal_field(g, res, org, np.array([go]), r)["field"][0]
    win = gw.window_rule(g.shape[1], g.shape[0], res, org, st, go, margin)
    F = gw.search_fields(g, res, org, np.array([[st[0], st[1], 0.0, 0.0]]), np.array([[go[0], go[1], 0.0, 0.0]]), r, margin)
    return whole, F["fields"][0], win


def test_a_window_that_cuts_the_only_route_leaves_the_cells_behind_it_unreached():
    """Yardstick only -- the documented meaning of a window.  Serpentine: start and goal in the left tile column, one wall apart; the
    wall between them is open at its right end only, in another tile column.  Pocket, 67 x 40 and inflated by 16 cells: the ring's
    inflation bars the upper tile row (rows 32 .. 39) from side to side and leaves row 0 free, so the way from the right side to
    the left runs below the ring, outside a window of the upper tile row."""
    whole, cut, win = _cut(ss.field_serpentine(), (5, 1), (5, 5), 0.0)
    assert win == (0, 0, 64, 32)
    assert whole[1, 5] != gw.U and whole[1, 5] > 5 * 2 * (130 - 5 - 5)          # out to the open end and back
    assert cut[1, 5] == gw.U and (cut[:3, :64] == gw.U).all()                  # the start's whole corridor, inside the window
    assert cut[5, 5] == 0 and cut[5, 63] == 5 * 58 and (cut[:, 64:] == gw.U).all() and (cut[32:] == gw.U).all()
    inside = cut != gw.U
    assert inside.any() and (cut[inside] >= whole[inside]).all()                # an upper bound where it has a value
    scene = ss.field_pocket(67, 40)
    r = 16 * scene[2]
    whole, cut, win = _cut(scene, (0, 36), (66, 36), 0.0, r)
    assert win == (0, 32, 67, 8)
    assert whole[36, 0] != gw.U and whole[0, 33] != gw.U                        # round the ring by row 0
    assert cut[36, 66] == 0 and cut[36, 60] == 30 and cut[36, 0] == gw.U and (cut[32:, :29] == gw.U).all()
    inside = cut != gw.U
    assert (cut[:32] == gw.U).all() and (cut[inside] >= whole[inside]).all()
