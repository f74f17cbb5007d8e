"""dftpav_grid_goal_field_windowed on the device against the yardstick of the cropped map (tests/goal_window_cases.py: oracle_goalfield
on the crop, blocked by the whole map's distance field), every cell and n_reached with it: the maps of test_gpu_goalfield.py; windows
of one tile, windows clipped by each border of the grid, windows whose last tile is partial, goals in a window's corner and on an
occupied cell, seeds on a tile border inside a window of several tiles, starts outside the grid, goals outside the grid; the radii
0, 0.5 m and one with d2 == T; an obstacle just outside the window; a margin that covers the map; shared and unshared fields."""
import functools

import numpy as np
import pytest

import goal_window_cases as gw
from dftpav_amd import search_scenes as ss
from oracle_goalfield import pygoalfield as pg

pytestmark = pytest.mark.gpu

U = pg.UNREACHED
RADII = (0.0, 0.5, ss.FIELD_EXACT_RADIUS)
MARGINS = (0.0, 1.1)          # the cells' own tiles; 5 cells more (no multiple of the resolution)


def _maze_map():
    name, g, res, org, st, en = ss.maze()
    return "maze-200x200", g, res, org


SCENES = {
    "1x1": lambda: ss.field_free(1, 1),
    "1x130": lambda: ss.field_random(1, 130, 0.05, 1),
    "130x1": lambda: ss.field_random(130, 1, 0.05, 2),
    "65x33-corner-pair": ss.field_corner_pair,
    "67x35-pocket": ss.field_pocket,
    "130x70-serpentine": ss.field_serpentine,
    "200x200-maze": _maze_map,
}


def _pairs(g, res, org):
    """(starts [n][2], goals [n][2]) as points, from cells (clipped to the map where it is smaller)"""
    sy, sx = g.shape
    cl = lambda x, y: (min(x, sx - 1), min(y, sy - 1))
    cells = [
        (cl(63, 31), cl(63, 31)), (cl(64, 32), cl(64, 32)), (cl(64, 31), cl(64, 31)), ((0, 0), (0, 0)),          # one tile, the goal in its corner
        ((sx - 1, sy - 1), (sx - 1, sy - 1)),                                                                  # the last tile, partial
        ((0, 0), cl(64, 32)), ((0, 0), cl(63, 31)), (cl(64, 32), (0, 0)), ((sx - 1, sy - 1), cl(64, 31)),      # a seed on a tile border inside
        ((0, sy - 1), (sx - 1, 0)), ((sx - 1, 0), (0, sy - 1)),                                                # opposite corners
        ((sx // 2, sy // 2), cl(127, 63)), (cl(128, 64), (sx // 2, sy // 2)), ((sx // 2, 0), cl(0, 32)),
    ]
    occ = np.argwhere(g == 80)
    if len(occ):          # a goal on an occupied cell
        o = (int(occ[len(occ) // 2][1]), int(occ[len(occ) // 2][0]))
        cells += [(o, o), ((0, 0), o)]
    cells = list(dict.fromkeys(cells))
    st = [ss.cell_centre(*a, res, org) for a, b in cells]
    go = [ss.cell_centre(*b, res, org) for a, b in cells]
    mid = ss.cell_centre(sx // 2, sy // 2, res, org)
    # starts outside the grid on each side; goals outside the grid
    st += [ss.cell_centre(-5, sy // 2, res, org), ss.cell_centre(sx + 70, sy + 40, res, org), ss.cell_centre(sx // 2, -9, res, org), mid, mid]
    go += [mid, mid, ss.cell_centre(sx - 1, sy - 1, res, org), ss.cell_centre(-1, 0, res, org), (org[0] + 1e4, org[1])]
    return np.array(st), np.array(go)


@functools.lru_cache(maxsize=None)
def _case(scene, r, margin):
    """(grid, res, org, starts, goals, the yardstick's (windows, fields, n_reached)), computed once and shared"""
    name, g, res, org = SCENES[scene]()
    st, go = _pairs(g, res, org)
    want = gw.windowed_fields(g, res, org, st, go, r, margin)
    for a in want[1]:
        a.setflags(write=False)
    return g, res, org, st, go, want


def _assert_equal(got, want, tag):
    (win, fields, reached), (wwin, wfields, wreached) = got, want
    assert np.array_equal(win, wwin), (tag, win.tolist(), wwin.tolist())
    bad = [q for q in range(len(wfields)) if fields[q].shape != wfields[q].shape or not np.array_equal(fields[q], wfields[q])]
    assert not bad, (tag, bad, [int((fields[q] != wfields[q]).sum()) for q in bad if fields[q].shape == wfields[q].shape])
    assert np.array_equal(reached, wreached), (tag, reached.tolist(), wreached.tolist())


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("scene", list(SCENES))
def test_windowed_field_equals_the_cropped_yardstick(hiplib, scene, r, margin):
    g, res, org, st, go, want = _case(scene, r, margin)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    got = h.goal_field_windowed(st, go, r, margin)
    h.close()
    _assert_equal(got, want, (scene, r, margin))
    assert (want[0][-2:] == 0).all() and (got[2][-2:] == 0).all() and got[1][-1].shape == (0, 0)          # the goals outside the grid


def test_the_cases_hold_what_they_are_for():
    """no device: windows of one tile and of several, partial last tiles, windows short of the grid on every side"""
    g, res, org, st, go, (win, fields, reached) = _case("200x200-maze", 0.0, 0.0)
    w = [tuple(int(v) for v in r) for r in win]
    assert (0, 0, 64, 32) in w and (64, 32, 64, 32) in w and (192, 192, 8, 8) in w and (0, 0, 128, 64) in w
    assert any(x0 > 0 and y0 > 0 and x0 + wx < 200 and y0 + wy < 200 for x0, y0, wx, wy in w)
    g, res, org, st, go, (win, fields, reached) = _case("1x130", 0.0, 0.0)
    w = [tuple(int(v) for v in r) for r in win]
    assert (0, 0, 1, 64) in w and (0, 128, 1, 2) in w          # a seed at rows 31 / 32 inside a window of two tiles: the 1 x 130 case
    g, res, org, st, go, (win, fields, reached) = _case("130x70-serpentine", 0.0, 1.1)
    assert any((f == U).any() and (f != U).any() for f in fields)          # windows that cut corridors off


def test_an_obstacle_one_cell_outside_the_window_inflates_into_it(hiplib):
    """fails if the blocked mask comes from the cropped occupancy map instead of the whole map's distance field"""
    name, g, res, org = ss.field_free(130, 70)
    g = g.copy()
    g[8:13, 64] = 80          # a block in the column just right of the window (0, 0, 64, 32)
    r = ss.FIELD_EXACT_RADIUS
    p = np.array([ss.cell_centre(55, 10, res, org)])
    win, fields, reached = gw.windowed_fields(g, res, org, p, p, r, 0.0)
    assert tuple(win[0]) == (0, 0, 64, 32)
    crop_only = pg.goal_field(np.ascontiguousarray(g[:32, :64]), res, org, p, r)
    assert crop_only["n_reached"][0] == 64 * 32 and reached[0] < 64 * 32 and fields[0][10, 63] == U and fields[0][10, 61] == U and fields[0][10, 60] == 25
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    got = h.goal_field_windowed(p, p, r, 0.0)
    h.close()
    _assert_equal(got, (win, fields, reached), "outside-block")


def test_a_margin_that_covers_the_map_gives_the_whole_map_field(hiplib):
    name, g, res, org = ss.field_random(67, 35, 0.2, 3)
    st, go = _pairs(g, res, org)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    whole, n_whole = h.goal_field(go, 0.5)
    win, fields, reached = h.goal_field_windowed(st, go, 0.5, 1.0e3)
    h.close()
    assert np.array_equal(reached, n_whole)
    for q in range(len(go)):
        if fields[q].size:
            assert tuple(win[q]) == (0, 0, 67, 35) and np.array_equal(fields[q], whole[q]), q
        else:
            assert (whole[q] == U).all()


def test_nine_queries_share_a_field_only_with_the_same_cell_and_window(hiplib):
    name, g, res, org = ss.field_random(130, 70, 0.2, 5)
    c = lambda x, y: ss.cell_centre(x, y, res, org)
    # queries 0, 3, 6: goal cell (5, 5) and the window (0, 0, 64, 32) from three starts; 1 and 7: the goal cell (70, 40) from starts in
    # other tiles, so two windows
    pairs = [((2, 2), (5, 5)), ((66, 34), (70, 40)), ((40, 20), (100, 60)), ((60, 30), (5, 5)), ((63, 31), (64, 32)), ((0, 69), (0, 34)),
             ((5, 5), (5, 5)), ((10, 10), (70, 40)), ((129, 0), (33, 1))]
    st, go = np.array([c(*a) for a, b in pairs]), np.array([c(*b) for a, b in pairs])
    go[3] += (0.1 * res, -0.2 * res)          # the same cell from another point of it
    want = gw.windowed_fields(g, res, org, st, go, 0.0, 0.0)
    assert all(tuple(want[0][q]) == (0, 0, 64, 32) for q in (0, 3, 6)) and tuple(want[0][1]) != tuple(want[0][7])
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    got = h.goal_field_windowed(st, go, 0.0, 0.0)
    assert h.goal_field_last_ms() > 0.0
    h.close()
    _assert_equal(got, want, "nine")
    assert np.array_equal(got[1][0], got[1][3]) and np.array_equal(got[1][0], got[1][6]) and got[1][1].shape != got[1][7].shape


def test_two_calls_in_a_row_then_a_new_map(hiplib):
    g1, res, org, st1, go1, want1 = _case("130x70-serpentine", 0.5, 1.1)
    g2, res2, org2, st2, go2, want2 = _case("67x35-pocket", 0.5, 1.1)
    g3, res3, org3, st3, go3, want3 = _case("200x200-maze", 0.5, 1.1)
    h = hiplib.Handle()
    h.set_grid_map(g1, res, org)
    a = h.goal_field_windowed(st1, go1, 0.5, 1.1)
    b = h.goal_field_windowed(st1, go1, 0.5, 1.1)
    _assert_equal(a, want1, "first")
    _assert_equal(b, want1, "second")
    h.set_grid_map(g2, res2, org2)          # a smaller map
    _assert_equal(h.goal_field_windowed(st2, go2, 0.5, 1.1), want2, "smaller")
    h.set_grid_map(g3, res3, org3)          # a larger one: the workspace grows
    _assert_equal(h.goal_field_windowed(st3, go3, 0.5, 1.1), want3, "larger")
    assert np.array_equal(h.goal_field(go3[:2], 0.5)[0], pg.goal_field(g3, res3, org3, go3[:2], 0.5)["field"])          # and the whole-map call after it
    h.close()


def test_argument_checks_leave_the_handle_usable(hiplib):
    g, res, org, st, go, want = _case("67x35-pocket", 0.0, 0.0)
    h = hiplib.Handle()
    for call in (lambda: h.set_search_heuristic_window(1.0), lambda: h.goal_field_windowed(st, go, 0.0, 0.0)):          # no map
        with pytest.raises(hiplib.DftpavError) as e:
            call()
        assert e.value.code == hiplib.E_INVALID
    h.set_grid_map(g, res, org)
    bad = (lambda: h.goal_field_windowed(st, go, 0.0, -1.0), lambda: h.goal_field_windowed(st, go, 0.0, float("nan")),
           lambda: h.goal_field_windowed(st, go, 0.0, float("inf")), lambda: h.goal_field_windowed(st, go, -0.5, 0.0),
           lambda: h.set_search_heuristic_window(float("nan")), lambda: h.set_search_heuristic_window(float("inf")))
    for call in bad:
        with pytest.raises(hiplib.DftpavError) as e:
            call()
        assert e.value.code == hiplib.E_INVALID
    _assert_equal(h.goal_field_windowed(st, go, 0.0, 0.0), want, "after the refusals")
    h.close()
