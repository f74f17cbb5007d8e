"""The rendered map on the device (render.hip): the map after dftpav_grid_render equals oracle_render byte for byte through
dftpav_grid_read_cells -- with and without the bit map, across the grid's borders, for every named shape where a kernel can go wrong
and on the default arena --, every consumer of the map sees a rendered handle as it sees a handle given the rendered bytes, the
stamps sit on a rendered map as on an uploaded one, and every refusal leaves the map as it was."""
import ctypes as C
import os

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import scenarios as sc
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import LayoutSpec
from oracle_render import pyrender as pr
from oracle_render import scenes as rsc
from oracle_stamp import pystamp as ps

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SX, SY, RES, ORG = rsc.SX, rsc.SY, rsc.RES, rsc.ORG


def _expect(h, want):
    got, n = h.read_cells()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert n == 0                                               # a rendered map has no stamps
    return got


def _both(h, size_x, size_y, res, org, background, polys=(), circles=None, points=None):
    """renders on the device and with the oracle; the device's bytes equal the oracle's"""
    xy, off = rsc.pack(list(polys))
    h.render_map(size_x, size_y, res, org, background, xy, off, circles, points)
    want = pr.render(size_x, size_y, res, org, background, xy, off, circles, points)
    _expect(h, want)
    assert h.render_last_ms() > 0.0
    return want


@pytest.fixture(scope="module")
def small(hiplib):
    h = hiplib.Handle()
    yield h
    h.close()


@pytest.mark.parametrize("name", sorted(rsc.named()))
def test_named_shapes_on_the_small_map(small, name):
    """70 x 40 at 0.1 m: a bit map, and no row of it word-aligned"""
    polys = rsc.named()[name]
    want = _both(small, SX, SY, RES, ORG, 127, polys)
    assert ((want == 80).sum() > 0) == (name != "wholly outside")
    if all(len(p) for p in polys):                              # and fill_polygons' bytes, which are the normative ones
        xy, off = rsc.pack(polys)
        assert np.array_equal(want, sc.fill_polygons(np.full((SY, SX), 127, np.uint8), ORG, RES, xy, off))


def test_empty_set_and_backgrounds(small):
    for background in (0, 127, 80, 255):
        want = _both(small, SX, SY, RES, ORG, background)
        assert (want == background).all()
    small.render_map(SX, SY, RES, ORG, 3, np.zeros((0, 2)), np.zeros(1, dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 2)))
    _expect(small, np.full((SY, SX), 3, np.uint8))
    _both(small, 33, 1, RES, ORG, 9)                             # fewer cells than a word of the bit map and a 16-byte store hold, and
    _both(small, 1, 47, RES, ORG, 9, [rsc.world([(-3, 2), (5, 20), (0, 40)])])     # a single column


def test_overlapping_polygons_circles_and_points(small):
    n = rsc.named()
    polys = n["triangle"] + n["L"] + n["bow-tie"] + n["left border"] + n["far corner"]
    c = rsc.world([(30, 20), (0, 0), (69, 39), (50, 10), (35, -8), (200, 20)])
    circles = [[c[0][0], c[0][1], 5.5 * RES], [c[1][0], c[1][1], 5.5 * RES], [c[2][0], c[2][1], 1.0 * RES], [c[3][0], c[3][1], 0.0],
               [c[4][0], c[4][1], 12.3 * RES], [c[5][0], c[5][1], 100.0 * RES + 1e-3], [c[5][0], c[5][1], 3.0 * RES]]
    points = rsc.world([(3, 4), (69, 39), (0, 0), (70, 39), (69, 40), (-1, 5), (5, -1), (69.4, 38.6), (69.6, 10), (22.5, 11.5), (23.5, 12.5)])
    for background in (127, 0):
        want = _both(small, SX, SY, RES, ORG, background, polys, circles, points)
    assert want[39, 69] == 80 and want[0, 0] == 80
    alone = _both(small, SX, SY, RES, ORG, 0, (), circles[:4])
    assert (alone == 80).sum() == 81 + 26 + 3 + 1              # the hand counts of the oracle's own test
    _both(small, SX, SY, RES, ORG, 0, (), None, points)
    _both(small, SX, SY, RES, ORG, 0, polys[::-1] + polys, circles[::-1], points[::-1])       # order and repetition do not show
    _expect(small, want)


def test_random_polygons(small):
    scenes = rsc.random_polygons(11, 200)
    for k in range(0, 200, 8):                                  # eight to a render
        _both(small, SX, SY, RES, ORG, 127, [p for p, _ in scenes[k:k + 8]])
    _both(small, SX, SY, RES, ORG, 127, [p for p, _ in scenes])


def test_large_map_without_bits(hiplib):
    """700 x 500 = 350 000 cells: beyond the bit map's 327 680; spans that start, end and run across ix = 63 | 64 and 127 | 128"""
    h = hiplib.Handle()
    org = (5.0, -3.0)
    polys = [rsc.world(p, 0.25, org) for p in ([(60, 10), (70, 12), (66, 40), (58, 30)], [(120, 50), (135, 60), (125, 90)],
                                               [(10, 100), (300, 110), (650, 130), (640, 300), (30, 280)], [(63, 320), (128, 320), (128, 340), (63, 340)],
                                               [(64, 360), (127, 360), (127, 380), (64, 380)], [(690, 480), (720, 490), (705, 520)])]
    c = rsc.world([(64, 450), (699, 0)], 0.25, org)
    want = _both(h, 700, 500, 0.25, org, 127, polys, [[c[0][0], c[0][1], 40 * 0.25], [c[1][0], c[1][1], 64 * 0.25]], rsc.world([(699, 499)], 0.25, org))
    assert want[330, 63] == 80 and want[330, 64] == 80 and want[330, 128] == 80 and want[330, 129] == 127
    assert want[370, 63] == 127 and want[370, 64] == 80 and want[370, 127] == 80 and want[370, 128] == 127
    assert want[200, 63] == 80 and want[200, 64] == 80 and want[200, 127] == 80 and want[200, 128] == 80
    h.close()


@pytest.fixture(scope="module")
def arena():
    grid, origin, res, ego = sc.default_sim_map()
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "default_map.npz"))
    return dict(grid=grid, origin=origin, res=res, ego=ego, xy=z["poly_xy"], off=z["poly_off"])


def test_default_arena(hiplib, arena):
    """36 polygons on 1500 x 1500: the bytes of scenarios.default_sim_map, the map every other test of the arena stands on"""
    h = hiplib.Handle()
    origin = hiplib.origin_centred(arena["ego"][0], arena["ego"][1], 1500 * arena["res"], 1500 * arena["res"])
    assert origin == arena["origin"] == (-202.0, -120.0)
    h.render_map(1500, 1500, arena["res"], origin, 127, arena["xy"], arena["off"])
    _expect(h, arena["grid"])
    print("default arena: render %.4f ms, %d cells set" % (h.render_last_ms(), int((arena["grid"] == 80).sum())))
    h.close()


def test_origin_centred(hiplib):
    for args in ((-52.0, 30.0, 300.0, 300.0), (0.5, -0.5, 0.0, 0.0), (1.5, 2.5, 0.0, 0.0), (-2.5, 7.49, 10.0, 3.0), (100.3, -7.7, 33.3, 0.1)):
        assert hiplib.origin_centred(*args) == pr.origin_centred(*args), args
    assert hiplib.origin_centred(0.5, -0.5, 0.0, 0.0) == (1.0, -1.0)        # C's round: halves away from zero
    fn = hiplib.lib().dftpav_grid_origin_centred
    fn.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    out = (C.c_double * 2)(7.0, 7.0)
    assert fn(0.0, 0.0, 1.0, 1.0, None) == hiplib.E_INVALID
    for bad in ((NAN, 0.0, 1.0, 1.0), (0.0, INF, 1.0, 1.0), (0.0, 0.0, NAN, 1.0), (0.0, 0.0, 1.0, -INF)):
        assert fn(*bad, out) == hiplib.E_INVALID and tuple(out) == (7.0, 7.0)


# ---- every consumer of the map sees the rendered bytes
def _validate(hiplib, h, plan):
    """dftpav_batch_validate of one plan uploaded as a batch of its layout (test hook dftpav_debug_batch_set_coeffs)"""
    lay = LayoutSpec([int(v) for v in plan["piece_nums"]], [int(v) for v in plan["singul"]], 4)
    bt = hiplib.Batch(h, lay, 1)
    fn = hiplib.lib().dftpav_debug_batch_set_coeffs
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    co = np.ascontiguousarray(plan["coeffs"][:lay.n_pieces], dtype=np.float64)
    dt = np.ascontiguousarray(plan["coeff_dt"][:lay.M], dtype=np.float64)
    assert fn(bt._b, co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p)) == 0
    col, first = bt.validate(sample_dt=0.05, vertex_res=0.1)
    bt.close()
    return int(col[0]), int(first[0])


def _consumers(hiplib, h, plan):
    states = np.array([[3.0, 5.0, 0.0], [8.5, 1.2, 0.4], [13.5, 5.0, 1.2], [8.5, 8.9, 0.0], [6.2, 5.0, -0.3]])
    search = h.kino_search([[2.0, 5.0, 0.0, 0.0]], [[15.0, 5.0, 0.0, 0.0]])
    return dict(rect=h.corridor_rectangles(states), dist=h.distance_field(), validate=np.array(_validate(hiplib, h, plan)),
                **{"search_" + k: v for k, v in search.items()})


def _same_consumers(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_consumers_see_a_rendered_handle_as_one_given_the_rendered_bytes(hiplib, oracle):
    """70 x 40 cells of 0.25 m (the bit map's path of the corridor): walls along the long sides, a post, a block across the straight
    line from (2, 5) to (15, 5)"""
    res, org = 0.25, (0.0, 0.0)
    polys = [np.array(p, dtype=np.float64) for p in ([(0.0, 0.0), (17.25, 0.0)], [(0.0, 9.75), (17.25, 9.75)],
                                                     [(1.0, 8.5), (1.25, 8.5), (1.25, 9.0), (1.0, 9.0)],
                                                     [(7.5, 3.5), (9.5, 4.0), (9.0, 6.5), (7.75, 6.0)])]
    circles, points = [[13.0, 1.5, 0.6]], [[5.0, 8.0]]
    xy, off = rsc.pack(polys)
    want = pr.render(70, 40, res, org, 0, xy, off, circles, points)
    free = pr.render(70, 40, res, org, 0, xy[:4], off[:3])       # the walls alone
    plan = cs._run(oracle.minco_generate, (2.0, 5.0), (15.0, 5.0), 0.0)
    A, B, Cb = hiplib.Handle(), hiplib.Handle(), hiplib.Handle()
    A.set_grid_map(free, res, org)
    A.distance_field()                                          # A has built its distance field on another map: it must go stale
    A.render_map(70, 40, res, org, 0, xy, off, circles, points)
    _expect(A, want)
    B.set_grid_map(want, res, org)
    Cb.set_grid_map(free, res, org)
    a, b, c = _consumers(hiplib, A, plan), _consumers(hiplib, B, plan), _consumers(hiplib, Cb, plan)
    _same_consumers(a, b)
    assert a["validate"][0] == 1 and c["validate"][0] == 0      # the plan runs through the block, and the block is what stops it
    for k in ("rect", "dist", "search_paths"):
        assert np.asarray(a[k]).tobytes() != np.asarray(c[k]).tobytes(), k      # (no comparison above was between two unchanged things)
    Cb.render_map(70, 40, res, org, 0, xy, off, circles, points)                 # and a render over an uploaded map of the same size
    _same_consumers(_consumers(hiplib, Cb, plan), b)
    for h in (A, B, Cb):
        h.close()


def test_search_on_a_search_scene_rebuilt_from_its_boxes(hiplib):
    """search_scenes.wall_gap, its two boxes given as polygons: the same bytes, and the same search as on the uploaded scene"""
    name, grid, res, origin, start, goal = ss.wall_gap()
    boxes = ((5.0, -20.0, 6.0, 3.0), (5.0, 9.0, 6.0, 20.0))
    polys = [np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)]) for x0, y0, x1, y1 in boxes]
    xy, off = rsc.pack(polys)
    want = pr.render(ss.SIZE, ss.SIZE, res, origin, 127, xy, off)
    assert np.array_equal(want, grid)
    A, B = hiplib.Handle(), hiplib.Handle()
    A.render_map(ss.SIZE, ss.SIZE, res, origin, 127, xy, off)
    _expect(A, want)
    B.set_grid_map(want, res, origin)
    a, b = A.kino_search(start[None], goal[None]), B.kino_search(start[None], goal[None])
    assert a["status"][0] == hiplib.SEARCH_REACH_END and a["iters"][0] > 0
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    A.close()
    B.close()


# ---- state transitions
def _box(cx, cy, deg):
    a = np.radians(deg)
    return [cx, cy, np.cos(a), np.sin(a)]


def test_render_stamp_clear_and_render_over_stamps(small):
    n = rsc.named()
    xy, off = rsc.pack(n["L"])
    h = small
    h.render_map(SX, SY, RES, ORG, 127, xy, off)
    base = pr.render(SX, SY, RES, ORG, 127, xy, off)
    boxes = [_box(ORG[0] + 4.0, ORG[1] + 2.0, 30.0)]
    h.stamp_poses(boxes, 0.0)
    work = ps.stamp(base, boxes, RES, ORG, 0.0)
    got, ns = h.read_cells()
    assert np.array_equal(got, work) and ns == ps.n_stamped(work, base) > 0
    states = np.array([[ORG[0] + 5.5, ORG[1] + 2.0, 0.3]])
    rect_stamped = h.corridor_rectangles(states)                # (the bit map follows the stamp on a rendered map too)
    h.clear_stamps()
    _expect(h, base)                                            # render, stamp, clear: the rendered map
    rect_base = h.corridor_rectangles(states)
    assert rect_stamped.tobytes() != rect_base.tobytes()
    h.stamp_poses(boxes, 0.0)
    xy2, off2 = rsc.pack(n["triangle"])
    h.render_map(SX, SY, RES, ORG, 0, xy2, off2)                # a render over a stamped map drops the stamps
    base2 = pr.render(SX, SY, RES, ORG, 0, xy2, off2)
    _expect(h, base2)
    h.clear_stamps()
    _expect(h, base2)                                           # and the base the stamps kept is gone with them
    h.stamp_poses(boxes, 0.0)
    got, ns = h.read_cells()
    work2 = ps.stamp(base2, boxes, RES, ORG, 0.0)
    assert np.array_equal(got, work2) and ns == ps.n_stamped(work2, base2)
    h.clear_stamps()
    _expect(h, base2)


def test_render_upload_render_with_another_size(hiplib):
    n = rsc.named()
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError):
        h.render_last_ms()                                      # before any render
    a = _both(h, SX, SY, RES, ORG, 127, n["triangle"])
    up = np.random.default_rng(4).choice(np.array([0, 127, 80, 3], dtype=np.uint8), size=(50, 90))
    h.set_grid_map(up, 0.5, (1.0, 2.0))
    got, ns = h.read_cells()
    assert np.array_equal(got, up) and ns == 0
    b = _both(h, 700, 500, 0.25, ORG, 0, [rsc.world([(50, 50), (600, 80), (300, 450)], 0.25)])      # larger, no bit map, another resolution
    assert h.distance_field().shape == (500, 700)
    c = _both(h, SX, SY, RES, ORG, 127, n["L"])                 # smaller again, with one; twice with different sets
    d = _both(h, SX, SY, RES, ORG, 127, n["triangle"])
    assert np.array_equal(a, d) and not np.array_equal(c, d) and (b == 80).sum() > 1000
    d2 = h.distance_field()
    assert d2.shape == (SY, SX) and ((d2 == 0) == (d == 80)).all()
    states = np.array([[ORG[0] + 5.5, ORG[1] + 2.0, 0.3]])
    fresh = hiplib.Handle()
    fresh.set_grid_map(d, RES, ORG)
    assert h.corridor_rectangles(states).tobytes() == fresh.corridor_rectangles(states).tobytes()     # the line table is RES's again
    fresh.close()
    h.close()


# ---- refusals
def test_refusals_change_nothing(hiplib, small):
    h = small
    tri = rsc.named()["triangle"]
    want = _both(h, SX, SY, RES, ORG, 127, tri)
    L = hiplib.lib()
    fn = L.dftpav_grid_render
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_ubyte, C.c_void_p]
    bad = hiplib.E_INVALID
    xy, off = rsc.pack(tri)
    circ, pts = [[1.0, 2.0, 0.5]], [[1.0, 2.0]]

    def call(hh=h._h, sx=SX, sy=SY, res=RES, ox=ORG[0], oy=ORG[1], obs=None, **kw):
        o = obs if obs is not None else hiplib.obstacle_set(kw.get("xy", xy), kw.get("off", off), kw.get("circ", circ), kw.get("pts", pts))
        return fn(hh, sx, sy, res, ox, oy, 0, C.byref(o))

    def with_xy(i, j, v):
        a = xy.copy()
        a[i, j] = v
        return a

    assert call(hh=None) == bad
    for kw in (dict(sx=0), dict(sx=-1), dict(sy=0), dict(sy=-5), dict(res=0.0), dict(res=-0.1), dict(res=NAN), dict(res=INF),
               dict(ox=NAN), dict(ox=INF), dict(oy=-INF), dict(oy=NAN)):
        assert call(**kw) == bad, kw
    for v in (NAN, INF, -INF, 1.2e8, -1.2e8):                    # not finite; a snapped coordinate beyond 2^30 (1.2e9 cells)
        assert call(xy=with_xy(1, 0, v)) == bad and call(xy=with_xy(2, 1, v)) == bad, v
        assert call(circ=[[v, 2.0, 0.5]]) == bad and call(circ=[[1.0, v, 0.5]]) == bad, v
        assert call(pts=[[1.0, 2.0], [v, 2.0]]) == bad and call(pts=[[1.0, v]]) == bad, v
    for r in (NAN, INF, -INF, -0.1, -1e-300, 1.2e8):
        assert call(circ=[[1.0, 2.0, 0.5], [1.0, 2.0, r]]) == bad, r
    for o in ([1, 4], [0, 3, 2], [0, 2, 1, 3], [-1, 3]):        # not from 0; not non-decreasing
        assert call(off=np.array(o, dtype=np.int32)) == bad, o
    ring = rsc.world([(35 + 14 * np.cos(a), 20 + 12 * np.sin(a)) for a in np.linspace(0.0, 2.0 * np.pi, 65, endpoint=False)])
    assert call(xy=ring, off=np.array([0, 65], dtype=np.int32)) == bad                       # 65 vertices
    _expect(h, want)
    assert call(xy=ring[:64], off=np.array([0, 64], dtype=np.int32)) == hiplib.OK            # (64 are taken)
    want = _both(h, SX, SY, RES, ORG, 127, tri)
    for field, value in (("n_poly", -1), ("n_circle", -1), ("n_point", -1), ("poly_off", None), ("poly_xy", None), ("circles", None),
                         ("points", None)):
        o = hiplib.obstacle_set(xy, off, circ, pts)
        setattr(o, field, value)                                # a negative count; a count with its array NULL
        assert call(obs=o) == bad, field
    ms = C.c_float(-1.0)
    fm = L.dftpav_render_last_ms
    fm.argtypes = [C.c_void_p, C.c_void_p]
    assert fm(None, C.byref(ms)) == bad and fm(h._h, None) == bad and ms.value == -1.0
    _expect(h, want)                                            # the map is the one of the last good render
    states = np.array([[ORG[0] + 5.5, ORG[1] + 2.0, 0.3]])
    fresh = hiplib.Handle()
    fresh.set_grid_map(want, RES, ORG)
    assert h.corridor_rectangles(states).tobytes() == fresh.corridor_rectangles(states).tobytes()
    assert h.distance_field().tobytes() == fresh.distance_field().tobytes()
    fresh.close()
    nomap = hiplib.Handle()                                     # a refusal on a handle without a map leaves it without one
    assert call(hh=nomap._h, sx=0) == bad and call(hh=nomap._h, xy=with_xy(0, 0, NAN)) == bad
    fr = L.dftpav_grid_read_cells
    fr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert fr(nomap._h, None, None) == bad
    assert fn(nomap._h, SX, SY, RES, ORG[0], ORG[1], 5, None) == hiplib.OK                   # obs NULL: the empty set
    nomap._map_shape = (SY, SX)
    _expect(nomap, np.full((SY, SX), 5, np.uint8))
    nomap.close()
