"""oracle_render, the numpy yardstick of the rendered map (dftpav_grid_render), against dftpav_amd.scenarios.fill_polygons -- whose bytes
are normative: it made the default map every other test stands on -- and against hand counts for what fill_polygons does not draw
(discs, points, the background)."""
import os

import numpy as np
import pytest

from dftpav_amd import scenarios as sc
from oracle_render import pyrender as pr
from oracle_render import scenes as rsc

SX, SY, RES, ORG = rsc.SX, rsc.SY, rsc.RES, rsc.ORG


def _fill(polys, size_x=SX, size_y=SY, res=RES, org=ORG, background=127):
    g = np.full((size_y, size_x), background, dtype=np.uint8)
    xy, off = rsc.pack(polys)
    return sc.fill_polygons(g, org, res, xy, off)


def _render(polys, **kw):
    xy, off = rsc.pack(polys)
    return pr.render(SX, SY, RES, ORG, 127, xy, off, **kw)


def test_unit_square_of_the_default_map_test():
    xy = np.array([[2.0, 2.0], [4.0, 2.0], [4.0, 4.0], [2.0, 4.0], [2.0, 2.0]])
    got = pr.render(20, 20, 0.5, (0.0, 0.0), 127, xy, np.array([0, 5]))
    want = np.full((20, 20), 127, np.uint8)
    want[4:9, 4:9] = 80
    assert np.array_equal(got, want)
    assert np.array_equal(got, sc.fill_polygons(np.full((20, 20), 127, np.uint8), (0.0, 0.0), 0.5, xy, np.array([0, 5])))


def test_whole_default_arena():
    grid, origin, res, _ = sc.default_sim_map()
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "default_map.npz"))
    assert len(z["poly_off"]) - 1 == 36 and grid.shape == (1500, 1500)
    got = pr.render(1500, 1500, res, origin, 127, z["poly_xy"], z["poly_off"])
    assert np.array_equal(got, grid), np.argwhere(got != grid)[:8]
    assert pr.origin_centred(z["ego_init"][0], z["ego_init"][1], 1500 * res, 1500 * res) == origin == (-202.0, -120.0)


def test_named_shapes_equal_fill_polygons():
    for name, polys in rsc.named().items():
        if any(len(p) == 0 for p in polys):
            continue                                            # (fill_polygons takes no polygon without vertices)
        got, want = _render(polys), _fill(polys)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8])
    sq = _render(rsc.named()["square on integers"])
    assert (sq == 80).sum() == 26 * 21 and (sq[10:31, 20:46] == 80).all()
    assert (_render(rsc.named()["wholly outside"]) == 127).all()
    two = _render(rsc.named()["two vertices"])
    assert 44 <= (two == 80).sum() <= 2 * 44 and two[5, 5] == 80 and two[31, 48] == 80   # two outlines of max(43, 26) + 1 steps
    assert (_render(rsc.named()["a span over the whole row"])[5:26] == 80).all()


def test_random_polygons_equal_fill_polygons():
    scenes = rsc.random_polygons(11, 200)
    kinds = {k for _, k in scenes}
    assert len(kinds) == 15, kinds                              # every kind in every place
    n_cells = 0
    for poly, kind in scenes:
        got, want = _render([poly]), _fill([poly])
        assert np.array_equal(got, want), (kind, poly.tolist(), np.argwhere(got != want)[:8])
        n_cells += int((got == 80).sum())
    assert n_cells > 200 * 50
    polys = [p for p, _ in scenes[:40]]                         # and forty of them in one set
    assert np.array_equal(_render(polys), _fill(polys))


def test_invariant_to_polygon_order_and_idempotent():
    polys = [p for p, _ in rsc.random_polygons(5, 12)]
    a = _render(polys)
    assert np.array_equal(a, _render(polys[::-1]))
    assert np.array_equal(a, _render(polys + polys))            # the same set twice over
    assert np.array_equal(a, _render(polys))


@pytest.mark.parametrize("r,count", [(0, 1), (1, 5), (5, 81)])
def test_disc_hand_counts(r, count):
    """the lattice points of dx^2 + dy^2 <= r^2: 1, 5, and for r = 5: 11 + 2 * (9 + 9 + 9 + 7 + 1) = 81"""
    c = rsc.world([(30, 20)])[0]
    got = pr.render(SX, SY, RES, ORG, 0, circles=[[c[0], c[1], (r + 0.5) * RES]])       # r = (int)(radius / resolution): truncated
    assert (got == 80).sum() == count and set(np.unique(got)) <= {0, 80}
    ys, xs = np.nonzero(got == 80)
    assert ((xs - 30) ** 2 + (ys - 20) ** 2 <= r * r).all() and got[20, 30 + r] == 80 and got[20 - r, 30] == 80
    if r:
        assert got[20, 30 + r + 1] == 0 and got[20 + r, 30 + 1] == 0


def test_disc_across_a_border_and_radius_truncation():
    c = rsc.world([(0, 0)])[0]
    got = pr.render(SX, SY, RES, ORG, 127, circles=[[c[0], c[1], 5.5 * RES]])
    assert (got == 80).sum() == 26                             # the quarter x >= 0, y >= 0 of the 81: rows dy = 0..5 hold 6, 5, 5, 5, 4, 1
    c = rsc.world([(69, 39)])[0]
    assert (pr.render(SX, SY, RES, ORG, 127, circles=[[c[0], c[1], 1.0 * RES]]) == 80).sum() == 3
    c = rsc.world([(30, 20)])[0]
    assert (pr.render(SX, SY, RES, ORG, 127, circles=[[c[0], c[1], 0.99 * RES]]) == 80).sum() == 1      # (int)0.99 == 0
    assert (pr.render(SX, SY, RES, ORG, 127, circles=[[500.0, 500.0, 1.0]]) == 127).all()              # wholly outside


def test_points_inside_on_the_last_cell_and_outside():
    pts = rsc.world([(3, 4), (69, 39), (0, 0), (70, 39), (69, 40), (-1, 5), (5, -1), (69.4, 38.6), (69.6, 10)])
    got = pr.render(SX, SY, RES, ORG, 127, points=pts)
    want = np.full((SY, SX), 127, np.uint8)
    for x, y in ((3, 4), (69, 39), (0, 0)):                     # (69.4, 38.6) snaps to the last cell as well, (69.6, 10) to ix = 70: outside
        want[y, x] = 80
    assert np.array_equal(got, want)


def test_snapping_is_half_to_even():
    assert pr.snap([0.5, 1.5, 2.5, -0.5, -1.5], 0.0, 1.0).tolist() == [0, 2, 2, 0, -2]


@pytest.mark.parametrize("background", [0, 127])
def test_background(background):
    empty = pr.render(SX, SY, RES, ORG, background)
    assert empty.dtype == np.uint8 and empty.shape == (SY, SX) and (empty == background).all()
    xy, off = rsc.pack(rsc.named()["triangle"])
    got = pr.render(SX, SY, RES, ORG, background, xy, off, circles=[[1.0, 2.0, 0.5]], points=[[0.0, 1.0]])
    assert set(np.unique(got)) == {background, 80}
    assert np.array_equal(got == 80, pr.covered(SX, SY, RES, ORG, xy, off, [[1.0, 2.0, 0.5]], [[0.0, 1.0]]))


def test_overlap_is_the_union():
    xy, off = rsc.pack(rsc.named()["triangle"] + rsc.named()["L"])
    circ, pts = [[1.0, 2.0, 0.8], [4.0, 3.0, 0.35]], rsc.world([(12, 7), (60, 35)])
    got = pr.covered(SX, SY, RES, ORG, xy, off, circ, pts)
    parts = pr.covered(SX, SY, RES, ORG, xy, off) | pr.covered(SX, SY, RES, ORG, circles=circ) | pr.covered(SX, SY, RES, ORG, points=pts)
    assert np.array_equal(got, parts) and got.sum() > 500
