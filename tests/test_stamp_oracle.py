"""The CPU yardstick of the stamps (oracle_stamp/) held to the definition in include/dftpav_hip.h by hand: a count worked out on
paper, the closed edge, a rigid motion of the grid, the coverage the inflation is there for, idempotence and the boxes that stamp
nothing.  tests/test_gpu_stamp.py holds the device to this yardstick byte for byte."""
import numpy as np

from oracle_stamp import pystamp as ps

NAN = float("nan")


def _box(cx, cy, deg):
    a = np.radians(deg)
    return [cx, cy, np.cos(a), np.sin(a)]


def test_hand_count_of_an_axis_aligned_box():
    """70 x 40 cells of 0.1 m from the origin, the default vehicle (4.88 x 1.90) about (3.0, 2.0) along x: |0.1 ix - 3.0| <= 2.44 holds
    for ix = 6 .. 54 (0.5 and 5.5 are 2.5 away), |0.1 iy - 2.0| <= 0.95 for iy = 11 .. 29 (1.0 and 3.0 are 1.0 away): 49 x 19 cells,
    none of them nearer than 0.04 m to the decision"""
    m = ps.covered([[3.0, 2.0, 1.0, 0.0]], 70, 40, 0.1, (0.0, 0.0))
    want = np.zeros((40, 70), dtype=bool)
    want[11:30, 6:55] = True
    assert m.sum() == 49 * 19 == 931 and np.array_equal(m, want)
    # the same box a quarter turn on: 19 x 49, about (3.0, 2.0) still -- 2.0 - 2.44 < 0, so the grid cuts it: iy = 0 .. 39
    t = ps.covered([[3.0, 2.0, 0.0, 1.0]], 70, 40, 0.1, (0.0, 0.0))
    want = np.zeros((40, 70), dtype=bool)
    want[0:40, 21:40] = True                                    # |0.1 ix - 3.0| <= 0.95: ix = 21 .. 39
    assert np.array_equal(t, want)
    # inflate grows every side: 0.1 more is one more cell on every side that the grid holds, the decision 0.04 m away as before
    g = ps.covered([[3.0, 2.0, 1.0, 0.0]], 70, 40, 0.1, (0.0, 0.0), inflate=0.1)
    assert g.sum() == 51 * 21


def test_a_cell_centre_on_the_edge_is_covered():
    """every number a binary fraction, so the comparison is with equality itself: a 2.0 x 1.0 vehicle about (2.0, 1.0) on cells of
    0.5 m reaches x = 1.0 and 3.0, y = 0.5 and 1.5 exactly"""
    veh = (1.0, 2.0)
    m = ps.covered([[2.0, 1.0, 1.0, 0.0]], 10, 6, 0.5, (0.0, 0.0), veh=veh)
    want = np.zeros((6, 10), dtype=bool)
    want[1:4, 2:7] = True
    assert np.array_equal(m, want)
    m = ps.covered([[2.0, 1.0, 0.0, 1.0]], 10, 6, 0.5, (0.0, 0.0), veh=veh)          # a quarter turn, cs = 0 and sn = 1 exactly
    want = np.zeros((6, 10), dtype=bool)
    want[0:5, 3:6] = True                                       # x = 1.5 .. 2.5, y = 0.0 .. 2.0
    assert np.array_equal(m, want)
    eps = ps.covered([[2.0, 1.0, 1.0, 0.0]], 10, 6, 0.5, (0.0, 0.0), inflate=0.0, veh=(np.nextafter(1.0, 0.0), np.nextafter(2.0, 0.0)))
    assert eps.sum() == 3 * 1                                   # one ulp less and the edge cells are out


def test_a_grid_shifted_by_whole_cells_gives_the_shifted_set():
    """resolution 0.25 and origins that are binary fractions: the cell centres of the two grids are the same doubles"""
    boxes = [_box(6.1, 4.3, 30.0), _box(9.7, 2.2, 137.0)]
    a = ps.covered(boxes, 60, 40, 0.25, (0.0, 0.0))
    b = ps.covered(boxes, 60, 40, 0.25, (-0.75, 0.5))           # three cells to the left, two up
    assert a.sum() > 200
    assert np.array_equal(a[2:, :57], b[:38, 3:])
    assert not a[:, 57:].any() and not b[38:, :].any()          # nothing of the set lies in the strips one grid has alone


def test_inflation_by_half_a_diagonal_covers_every_cell_the_recheck_can_name():
    """grid_occupied names the cell round((p - origin) / resolution) for a point p: its centre is at most half a cell from p on either
    axis, resolution / sqrt(2) in all.  10 000 seeded points inside 20 rotated uninflated boxes"""
    rng = np.random.default_rng(424)
    res, origin = 0.1, (-1.3, 0.7)
    W, L = ps.VEH
    n_in = 0
    for _ in range(20):
        cx, cy, deg = rng.uniform(4.0, 9.0), rng.uniform(5.0, 9.0), rng.uniform(0.0, 360.0)
        box = _box(cx, cy, deg)
        a, b = rng.uniform(-0.5 * L, 0.5 * L, 500), rng.uniform(-0.5 * W, 0.5 * W, 500)
        a[:4], b[:4] = (0.5 * L, 0.5 * L, -0.5 * L, -0.5 * L), (0.5 * W, -0.5 * W, 0.5 * W, -0.5 * W)   # the corners among them
        px, py = cx + a * box[2] - b * box[3], cy + a * box[3] + b * box[2]
        m = ps.covered([box], 140, 140, res, origin, inflate=res / np.sqrt(2.0) + 1e-9)
        ix, iy = ps.occupied_cell(px, py, res, origin)
        assert ((ix >= 0) & (ix < 140) & (iy >= 0) & (iy < 140)).all()
        assert m[iy, ix].all()
        n_in += len(ix)
        bare = ps.covered([box], 140, 140, res, origin)
        assert not bare[iy, ix].all()                           # without the inflation some of those cells are missed
    assert n_in == 10000


def test_stamping_twice_changes_nothing_and_other_bytes_stay():
    rng = np.random.default_rng(7)
    base = rng.choice(np.array([0, 0, 0, 80, 1, 79, 255], dtype=np.uint8), size=(40, 70))
    boxes = [_box(3.0, 2.0, 30.0), _box(4.0, 2.5, 90.0)]
    once = ps.stamp(base, boxes, 0.1, (0.0, 0.0), inflate=0.07)
    twice = ps.stamp(once, boxes, 0.1, (0.0, 0.0), inflate=0.07)
    assert np.array_equal(once, twice)
    m = ps.covered(boxes, 70, 40, 0.1, (0.0, 0.0), inflate=0.07)
    assert (once[m] == 80).all() and np.array_equal(once[~m], base[~m])
    assert ps.n_stamped(once, base) == int((m & (base != 80)).sum()) > 0
    one_by_one = ps.stamp(ps.stamp(base, boxes[:1], 0.1, (0.0, 0.0), inflate=0.07), boxes[1:], 0.1, (0.0, 0.0), inflate=0.07)
    assert np.array_equal(one_by_one, once)                     # stamps accumulate


def test_boxes_that_stamp_nothing():
    base = np.zeros((40, 70), dtype=np.uint8)
    for box in ([NAN, 2.0, 1.0, 0.0], [3.0, NAN, 1.0, 0.0], [3.0, 2.0, NAN, 0.0], [3.0, 2.0, 1.0, NAN], [float("inf"), 2.0, 1.0, 0.0],
                [3.0, 2.0, float("inf"), 0.0], _box(-5.0, 2.0, 0.0), _box(3.0, 30.0, 45.0), _box(12.0, 8.0, 137.0)):
        assert not ps.covered([box], 70, 40, 0.1, (0.0, 0.0), inflate=0.5).any(), box
    assert np.array_equal(ps.stamp(base, np.zeros((0, 4)), 0.1, (0.0, 0.0)), base)
    poses = np.full((3, 5, 4), NAN)                             # the slot form: empty slots are NaN rows, unselected slots are dropped
    poses[:, 1] = _box(3.0, 2.0, 0.0)
    poses[:, 3] = _box(3.0, 2.0, 90.0)
    assert ps.slot_boxes(poses).shape == (15, 4)
    only1 = ps.covered(ps.slot_boxes(poses, [0, 1, 0, 0, 0]), 70, 40, 0.1, (0.0, 0.0))
    assert np.array_equal(only1, ps.covered([_box(3.0, 2.0, 0.0)], 70, 40, 0.1, (0.0, 0.0)))
    assert not ps.covered(ps.slot_boxes(poses, [0] * 5), 70, 40, 0.1, (0.0, 0.0)).any()
