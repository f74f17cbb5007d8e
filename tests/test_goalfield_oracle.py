"""The CPU yardstick of the goal field (oracle_goalfield/): Dijkstra with a binary heap against a numpy Bellman-Ford run to its fixed
point, on random maps with goals at corners, on borders, on an occupied cell and outside the grid, at the radii 0, one cell and one
with r^2 / res^2 an exact integer; then the cases small enough to check by hand."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from oracle_goalfield import pygoalfield as pg

U = pg.UNREACHED
RES, ORG = ss.FIELD_RES, ss.FIELD_ORIGIN


def brute_field(grid, T, cell, d2):
    """Bellman-Ford over whole arrays until nothing changes.  int64; a cell takes F[n] + w from its neighbour n when the cell itself
    is not blocked and, for a diagonal, neither of the two cells between them is."""
    sy, sx = grid.shape
    big = np.int64(1) << 40
    F = np.full((sy + 2, sx + 2), big, dtype=np.int64)          # a frame of unreached cells round the grid
    B = np.ones((sy + 2, sx + 2), dtype=bool)                   # ... that are blocked
    B[1:-1, 1:-1] = d2 <= T
    if cell[0] >= 0:
        F[cell[1] + 1, cell[0] + 1] = 0
    inner = (slice(1, -1), slice(1, -1))
    free = ~B[inner]

    def sh(a, dy, dx):
        return a[1 + dy:sy + 1 + dy, 1 + dx:sx + 1 + dx]
    while True:
        best = F[inner].copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not dx and not dy:
                    continue
                cand = sh(F, dy, dx) + (7 if dx and dy else 5)
                ok = free.copy()
                if dx and dy:
                    ok &= ~sh(B, dy, 0) & ~sh(B, 0, dx)
                best = np.where(ok & (cand < best), cand, best)
        if np.array_equal(best, F[inner]):
            break
        F[inner] = best
    out = F[inner]
    return np.where(out >= big, U, out).astype(np.int32)


def _goals(sx, sy, grid):
    cells = [(0, 0), (sx - 1, 0), (0, sy - 1), (sx - 1, sy - 1), (sx // 2, 0), (0, sy // 2), (sx - 1, sy // 3), (sx // 3, sy // 2)]
    occ = np.argwhere(grid == 80)
    if len(occ):
        cells.append((int(occ[len(occ) // 2][1]), int(occ[len(occ) // 2][0])))
    xy = [ss.cell_centre(ix, iy) for ix, iy in cells]
    xy += [ss.cell_centre(-1, 0), ss.cell_centre(sx, sy // 2), ss.cell_centre(2, sy), (ORG[0] - 100.0, ORG[1])]   # outside the grid
    return np.array(xy)


@pytest.mark.parametrize("density", [0.0, 0.1, 0.35])
def test_dijkstra_equals_the_brute_force(density):
    n = 0
    for k, (sx, sy) in enumerate(((24, 17), (1, 1), (1, 13), (11, 1), (9, 16))):
        name, g, res, org = ss.field_random(sx, sy, density, seed=100 * k + int(100 * density))
        d2 = pg.distance_field(g, brute=True)
        assert np.array_equal(d2, pg.distance_field(g))
        xy = _goals(sx, sy, g)
        for r in (0.0, res, ss.FIELD_EXACT_RADIUS):
            T = pg.threshold(r, res)
            o = pg.goal_field(g, res, org, xy, r)
            for i in range(len(xy)):
                b = brute_field(g, T, o["cell"][i], d2)
                assert np.array_equal(o["field"][i], b), (name, r, i)
                assert o["n_reached"][i] == (b != U).sum()
                n += 1
            outside = o["cell"][:, 0] < 0
            assert outside.sum() == 4 and (o["field"][outside] == U).all() and (o["n_reached"][outside] == 0).all()
    assert n >= 5 * 3 * 12


def test_thresholds_and_the_exact_radius():
    assert pg.threshold(0.0, RES) == 0 and pg.threshold(RES, RES) == 1 and pg.threshold(ss.FIELD_EXACT_RADIUS, RES) == 9
    assert pg.threshold(0.74, RES) == 8 and pg.threshold(1e30, RES) == 2147483646
    # d2 == T occurs and blocks: one occupied cell, radius 0.75 -> the cells at the cell distance 3 exactly are blocked, those with 10 not
    g = np.full((9, 9), 127, dtype=np.uint8)
    g[4, 4] = 80
    f = pg.goal_field(g, RES, ORG, [ss.cell_centre(0, 0)], ss.FIELD_EXACT_RADIUS)["field"][0]
    assert f[4, 1] == U and f[4, 7] == U and f[1, 4] == U and f[7, 4] == U        # d2 = 9 = T
    assert f[2, 2] == U and f[6, 6] == U                                           # d2 = 8 < T
    assert f[1, 3] != U and f[3, 1] != U and f[7, 5] != U and f[5, 7] != U        # d2 = 10 > T
    assert f[4, 0] != U                                                            # d2 = 16
    # a map without an occupied cell blocks nothing, whatever the radius
    name, g, res, org = ss.field_free(7, 5)
    assert (pg.goal_field(g, res, org, [ss.cell_centre(3, 2)], 1e6)["field"] != U).all()


def test_three_by_three_free_map_by_hand():
    name, g, res, org = ss.field_free(3, 3)
    o = pg.goal_field(g, res, org, [ss.cell_centre(0, 0), ss.cell_centre(1, 1)])
    assert o["field"][0].tolist() == [[0, 5, 10], [5, 7, 12], [10, 12, 14]]
    assert o["field"][1].tolist() == [[7, 5, 7], [5, 0, 5], [7, 5, 7]]
    assert o["n_reached"].tolist() == [9, 9]


def test_no_diagonal_between_two_cells_touching_at_a_corner():
    g = np.full((3, 3), 127, dtype=np.uint8)
    g[0, 1] = 80
    g[1, 0] = 80
    o = pg.goal_field(g, RES, ORG, [ss.cell_centre(0, 0), ss.cell_centre(1, 1)])
    # the goal (0, 0) sits behind the pair: its only ways out are the diagonal (not taken) and the two occupied cells
    assert o["field"][0].tolist() == [[0, U, U], [U, U, U], [U, U, U]] and o["n_reached"][0] == 1
    # from (1, 1) everything free is reached but (0, 0); (2, 0) and (0, 2) lie beside an occupied cell: no diagonal, 5 + 5
    assert o["field"][1].tolist() == [[U, U, 10], [U, 0, 5], [10, 5, 7]] and o["n_reached"][1] == 6
    # the scene the device test uses: the same pair across a tile corner
    name, g, res, org = ss.field_corner_pair()
    f = pg.goal_field(g, res, org, [ss.cell_centre(63, 32)])["field"][0]
    assert f[32, 63] == 0 and f[31, 64] == 6 * 5        # not the diagonal's 7: six axial steps round (63, 31), no diagonal past it
    assert f[30, 62] == 3 * 5 and f[32, 62] == 5 and f[31, 62] == 10


def test_enclosed_pocket_stays_unreached():
    name, g, res, org = ss.field_pocket()
    sy, sx = g.shape
    inside = (sx // 2, sy // 2)
    o = pg.goal_field(g, res, org, [ss.cell_centre(0, 0), ss.cell_centre(*inside)])
    pocket = np.zeros(g.shape, dtype=bool)
    pocket[sy // 2 - 2:sy // 2 + 3, sx // 2 - 3:sx // 2 + 4] = True
    assert (g[pocket] != 80).all() and pocket.sum() == 35
    assert (o["field"][0][pocket] == U).all() and (o["field"][0][~pocket & (g != 80)] != U).all()
    assert (o["field"][1][pocket] != U).all() and (o["field"][1][~pocket] == U).all() and o["n_reached"][1] == 35


def test_a_blocked_goal_cell_is_seeded():
    g = np.full((5, 5), 127, dtype=np.uint8)
    g[2, 2] = 80
    o = pg.goal_field(g, RES, ORG, [ss.cell_centre(2, 2)])
    f = o["field"][0]
    assert f[2, 2] == 0 and f[2, 1] == 5 and f[1, 1] == 7 and f[0, 0] == 14 and o["n_reached"][0] == 25
    # ... and nothing enters it: from elsewhere it stays unreached
    assert pg.goal_field(g, RES, ORG, [ss.cell_centre(0, 0)])["field"][0][2, 2] == U
    # inflated by one cell the goal's whole neighbourhood is blocked: the seed alone
    o = pg.goal_field(g, RES, ORG, [ss.cell_centre(2, 2)], RES)
    assert o["n_reached"][0] == 1 and o["field"][0][2, 2] == 0 and (np.delete(o["field"][0].ravel(), 12) == U).all()
