"""dftpav_grid_goal_field on the device against the Dijkstra yardstick (oracle_goalfield/), cell for cell and n_reached with it: maps
whose sides are no multiple of the 64 x 32 tile (1 x 1, 1 x 130, 130 x 1, 65 x 33, 67 x 35, 200 x 200), a map with no occupied
cell, an enclosed pocket, two occupied cells touching at a corner, a serpentine that drives the only path through every tile several
times; goals in a tile corner, on the border, outside the grid and on an occupied cell; the radii 0, 0.5 m and one with d2 == T."""
import functools

import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from oracle_goalfield import pygoalfield as pg

pytestmark = pytest.mark.gpu

U = pg.UNREACHED
RADII = (0.0, 0.5, ss.FIELD_EXACT_RADIUS)


def _maze_map():
    name, g, res, org, st, en = ss.maze()
    return "maze-200x200", g, res, org


SCENES = {
    "1x1": lambda: ss.field_free(1, 1),
    "1x130": lambda: ss.field_random(1, 130, 0.05, 1),
    "130x1": lambda: ss.field_random(130, 1, 0.05, 2),
    "65x33-free": lambda: ss.field_free(65, 33),
    "65x33-corner-pair": ss.field_corner_pair,
    "67x35-pocket": ss.field_pocket,
    "67x35-random": lambda: ss.field_random(67, 35, 0.2, 3),
    "130x70-serpentine": ss.field_serpentine,
    "200x200-maze": _maze_map,
}


def _goals(g, res, org):
    """cells in the corners of the 64 x 32 tiles, on the grid's border, on an occupied cell; points outside the grid"""
    sy, sx = g.shape
    cells = [(0, 0), (sx - 1, sy - 1), (sx - 1, 0), (sx // 2, sy - 1), (63, 31), (64, 32), (64, 31), (127, 63), (128, 64), (0, 32)]
    cells = [(x, y) for x, y in dict.fromkeys(cells) if x < sx and y < sy]
    occ = np.argwhere(g == 80)
    if len(occ):
        cells.append((int(occ[len(occ) // 2][1]), int(occ[len(occ) // 2][0])))
    xy = [ss.cell_centre(x, y, res, org) for x, y in cells]
    xy += [ss.cell_centre(-1, 0, res, org), ss.cell_centre(sx // 2, sy, res, org), (org[0] + 1e4, org[1])]
    return np.array(xy)


@functools.lru_cache(maxsize=None)
def _case(scene, r):
    """(grid, res, org, goals, the oracle's result), computed once and shared"""
    name, g, res, org = SCENES[scene]()
    xy = _goals(g, res, org)
    o = pg.goal_field(g, res, org, xy, r)
    for a in o.values():
        a.setflags(write=False)
    return g, res, org, xy, o


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("scene", list(SCENES))
def test_field_equals_the_oracle(hiplib, scene, r):
    g, res, org, xy, o = _case(scene, r)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    field, reached = h.goal_field(xy, r)
    h.close()
    bad = [i for i in range(len(xy)) if not np.array_equal(field[i], o["field"][i])]
    assert not bad, (scene, r, bad, [int((field[i] != o["field"][i]).sum()) for i in bad])
    assert np.array_equal(reached, o["n_reached"])
    outside = o["cell"][:, 0] < 0
    assert outside.sum() == 3 and (field[outside] == U).all()


def test_the_scenes_hold_what_they_are_for():
    """the serpentine's far end is many tile crossings away; the pocket is unreached; d2 == T occurs on the random map"""
    g, res, org, xy, o = _case("130x70-serpentine", 0.0)
    f = o["field"][0]
    assert f[f != U].max() > 5 * 130 * 15 and o["n_reached"][0] == (g != 80).sum()
    g, res, org, xy, o = _case("67x35-pocket", 0.0)
    assert o["field"][0][35 // 2, 67 // 2] == U
    g, res, org, xy, o = _case("67x35-random", ss.FIELD_EXACT_RADIUS)
    assert (pg.distance_field(g) == pg.threshold(ss.FIELD_EXACT_RADIUS, res)).any()


def test_nine_goals_of_which_three_share_a_cell(hiplib):
    name, g, res, org = ss.field_random(67, 35, 0.2, 3)
    cells = [(5, 5), (66, 34), (40, 20), (5, 5), (63, 31), (0, 34), (5, 5), (64, 32), (33, 1)]
    xy = np.array([ss.cell_centre(x, y, res, org) for x, y in cells])
    xy[3] += (0.1 * res, -0.2 * res)          # the same cell from another point of it
    o = pg.goal_field(g, res, org, xy, 0.0)
    assert (o["cell"][[0, 3, 6]] == (5, 5)).all()
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    field, reached = h.goal_field(xy, 0.0)
    assert np.array_equal(field, o["field"]) and np.array_equal(reached, o["n_reached"])
    assert np.array_equal(field[0], field[3]) and np.array_equal(field[0], field[6])
    # n_reached alone, nothing fetched
    assert np.array_equal(h.goal_field(xy, 0.0, fetch=False), o["n_reached"])
    assert h.goal_field_last_ms() > 0.0
    h.close()


def test_two_calls_in_a_row_give_the_same_bits(hiplib):
    g, res, org, xy, o = _case("130x70-serpentine", 0.0)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    a = h.goal_field(xy, 0.0)
    b = h.goal_field(xy, 0.0)
    h.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], o["field"])


def test_a_new_map_gives_the_new_maps_field(hiplib):
    g1, res, org, xy1, o1 = _case("67x35-pocket", 0.5)
    g2, res2, org2, xy2, o2 = _case("67x35-random", 0.5)
    g3, res3, org3, xy3, o3 = _case("130x70-serpentine", 0.5)
    h = hiplib.Handle()
    h.set_grid_map(g1, res, org)
    assert np.array_equal(h.goal_field(xy1, 0.5)[0], o1["field"])
    h.set_grid_map(g2, res2, org2)          # the same size, other cells
    assert np.array_equal(h.goal_field(xy2, 0.5)[0], o2["field"])
    h.set_grid_map(g3, res3, org3)          # a larger map: the workspace grows
    f, n = h.goal_field(xy3, 0.5)
    assert np.array_equal(f, o3["field"]) and np.array_equal(n, o3["n_reached"])
    h.close()
