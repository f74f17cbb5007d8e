"""The stamps on the device (stamp.hip): the working map after dftpav_grid_stamp_poses / dftpav_planner_stamp_slots equals
oracle_stamp byte for byte through dftpav_grid_read_cells -- with and without the bit map, across the grid's borders, for NaN rows
and repeated calls -- every consumer of the map sees a stamped handle as it sees a handle given the stamped bytes, the clear puts
the uploaded bytes back, and a second vehicle planned against a stamped one goes round it."""
import ctypes as C

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from dftpav_amd.pods import LayoutSpec
from oracle_conflict import pyconflict as pc
from oracle_stamp import pystamp as ps

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")
RES, ORG = 0.25, (0.0, 0.0)            # the small map: 70 x 40 cells, 17.5 m x 10 m; 70 % 32 != 0, so no row of bits is word-aligned
DIAG = RES / np.sqrt(2.0)
DEGS = (0.0, 30.0, 90.0, 137.0)


def _box(cx, cy, deg):
    a = np.radians(deg)
    return [cx, cy, np.cos(a), np.sin(a)]


def _base(shape, seed):
    """a map with bytes other than 0 and 80, a tenth of it occupied"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 127, 1, 79, 81, 255, 80], dtype=np.uint8), size=shape, p=[0.4, 0.3, 0.05, 0.05, 0.05, 0.05, 0.1])


def _expect(h, work, base):
    got, n = h.read_cells()
    assert got.dtype == np.uint8 and got.shape == work.shape
    assert np.array_equal(got, work), np.argwhere(got != work)[:8]
    assert n == ps.n_stamped(work, base)
    return n


@pytest.fixture(scope="module")
def small(hiplib):
    base = _base((40, 70), 1)
    h = hiplib.Handle()
    h.set_grid_map(base, RES, ORG)
    yield dict(h=h, base=base)
    h.close()


def test_a_handle_that_never_stamped_reads_the_uploaded_bytes(hiplib):
    base = _base((40, 70), 2)
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError):
        h.read_cells()                                          # no map
    h.set_grid_map(base, RES, ORG)
    got, n = h.read_cells()
    assert np.array_equal(got, base) and n == 0
    assert h.stamp_last_ms() == (0.0, 0.0)
    h.clear_stamps()                                            # a clear before any stamp is OK
    got, n = h.read_cells()
    assert np.array_equal(got, base) and n == 0
    h.close()


@pytest.mark.parametrize("inflate", [0.0, DIAG])
@pytest.mark.parametrize("deg", DEGS)
def test_one_box_on_the_small_map(small, deg, inflate):
    h, base = small["h"], small["base"]
    h.clear_stamps()
    box = _box(8.6, 5.1, deg)
    h.stamp_poses([box], inflate)
    n = _expect(h, ps.stamp(base, [box], RES, ORG, inflate), base)
    assert n > 100
    ms = h.stamp_last_ms()
    assert ms[0] == 0.0 and ms[1] > 0.0


def test_borders_corner_outside_nan_rows_and_repeats(small):
    h, base = small["h"], small["base"]
    h.clear_stamps()
    work = base.copy()
    calls = [[_box(0.3, 5.0, 30.0)],                            # across the left border
             [_box(17.2, 4.0, 137.0)],                          # the right
             [_box(9.0, 0.2, 90.0)],                            # the lower
             [_box(6.0, 9.8, 0.0)],                             # the upper
             [_box(17.3, 9.7, 30.0)],                           # across a corner
             [_box(-0.2, -0.1, 137.0)],                         # the corner at the origin, the centre outside the grid
             [_box(40.0, 5.0, 30.0)], [_box(8.0, -30.0, 0.0)], [_box(-1e300, 5.0, 0.0)],    # wholly outside
             [_box(3.0, 3.0, 0.0), [NAN, 3.0, 1.0, 0.0], _box(12.0, 7.0, 90.0), [5.0, 5.0, NAN, NAN], [5.0, INF, 1.0, 0.0]],   # NaN rows among finite ones
             [_box(7.0, 5.0, 30.0), _box(8.0, 5.5, 137.0)],     # two that overlap
             [[9.0, 5.0, 0.5, 0.0]]]                            # (cs, sn) not a unit vector: the definition as it stands
    for boxes in calls:
        for inflate in (0.0, DIAG):
            h.stamp_poses(boxes, inflate)
            work = ps.stamp(work, boxes, RES, ORG, inflate)
            _expect(h, work, base)
    before = work.copy()
    h.stamp_poses(calls[-2], DIAG)                              # the same call again
    _expect(h, before, base)
    h.stamp_poses(np.zeros((0, 4)), 0.0)                        # n = 0
    _expect(h, before, base)
    h.clear_stamps()
    _expect(h, base, base)


def test_large_map_without_bits(hiplib):
    """700 x 500 = 350 000 cells: beyond the bit map's 327 680; one box straddles ix = 63 | 64 (x = 15.875)"""
    base = _base((500, 700), 3)
    h = hiplib.Handle()
    h.set_grid_map(base, RES, ORG)
    boxes = [_box(15.875, 60.0, 90.0), _box(15.875, 20.0, 0.0)] + [_box(40.0 + 30.0 * i, 30.0 + 25.0 * i, d) for i, d in enumerate(DEGS)]
    boxes += [_box(174.9, 124.9, 30.0), _box(0.1, 100.0, 137.0)]                      # the far corner, the left border
    work = base
    for inflate in (0.0, DIAG):
        h.stamp_poses(boxes, inflate)
        work = ps.stamp(work, boxes, RES, ORG, inflate)
        n = _expect(h, work, base)
    assert n > 8 * 100 and work[240, 63] == 80 and work[240, 64] == 80
    h.clear_stamps()
    _expect(h, base, base)
    h.close()


def test_clear_puts_every_byte_back_and_a_new_map_has_no_stamps(small):
    h, base = small["h"], small["base"]
    h.clear_stamps()
    boxes = [_box(5.0, 5.0, 30.0), _box(12.0, 4.0, 137.0)]
    h.stamp_poses(boxes, DIAG)
    work = ps.stamp(base, boxes, RES, ORG, DIAG)
    assert _expect(h, work, base) > 0 and len(np.unique(base[work != base])) > 2        # bytes other than 0 lie under the stamps
    h.clear_stamps()
    assert _expect(h, base, base) == 0
    h.stamp_poses(boxes, DIAG)
    other = _base((40, 70), 9)
    h.set_grid_map(other, RES, ORG)                             # after stamps: the new map is the base, no stamps remain
    assert _expect(h, other, other) == 0
    h.clear_stamps()
    assert _expect(h, other, other) == 0
    h.stamp_poses(boxes[:1], 0.0)
    _expect(h, ps.stamp(other, boxes[:1], RES, ORG, 0.0), other)
    h.set_grid_map(base, RES, ORG)                              # (the module's map again)
    _expect(h, base, base)


def test_refusals_change_nothing(hiplib, small, oracle):
    h, base = small["h"], small["base"]
    h.clear_stamps()
    boxes = np.array([_box(5.0, 5.0, 30.0)])
    h.stamp_poses(boxes, 0.0)
    work = ps.stamp(base, boxes, RES, ORG, 0.0)
    L = hiplib.lib()
    fp, fs, fc, fr = L.dftpav_grid_stamp_poses, L.dftpav_planner_stamp_slots, L.dftpav_grid_clear_stamps, L.dftpav_grid_read_cells
    fp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    fs.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double]
    fc.argtypes = [C.c_void_p]
    fr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    ptr = boxes.ctypes.data_as(C.c_void_p)
    bad = hiplib.E_INVALID
    assert fp(None, ptr, 1, 0.0) == bad and fp(h._h, None, 1, 0.0) == bad and fp(h._h, ptr, -1, 0.0) == bad
    for inflate in (-0.1, NAN, INF, -INF):
        assert fp(h._h, ptr, 1, inflate) == bad, inflate
    assert fc(None) == bad and fr(None, None, None) == bad and fs(None, None, 0.0, 0.1, 1, 0.0) == bad
    assert L.dftpav_stamp_last_ms(None, None, None) == bad
    _expect(h, work, base)
    pl = hiplib.Planner(h, 3, 1)
    assert fs(pl._p, None, 0.0, 0.1, 1, 0.0) == bad            # a planner whose table was never filled
    _install(pl, dict(slots=[cs._run(oracle.minco_generate, (3.0, 5.0), (12.0, 5.0), 0.0), None, None]))
    ok = dict(t0=0.0, dt=0.1, K=2, inflate=0.0)
    for b in (dict(K=0), dict(K=-1), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN),
              dict(inflate=-0.1), dict(inflate=NAN), dict(inflate=INF)):
        a = dict(ok, **b)
        assert fs(pl._p, None, a["t0"], a["dt"], a["K"], a["inflate"]) == bad, b
    _expect(h, work, base)
    nomap = hiplib.Handle()                                     # no map
    pl2 = hiplib.Planner(nomap, 3, 1)
    _install(pl2, dict(slots=[cs._run(oracle.minco_generate, (3.0, 5.0), (12.0, 5.0), 0.0), None, None]))
    assert fp(nomap._h, ptr, 1, 0.0) == bad and fc(nomap._h) == bad and fr(nomap._h, None, None) == bad
    assert fs(pl2._p, None, 0.0, 0.1, 1, 0.0) == bad
    pl2.close()
    nomap.close()
    assert fs(pl._p, None, 0.0, 0.1, 2, 0.0) == hiplib.OK      # and the good call stamps
    _expect(h, ps.stamp(work, ps.slot_boxes(pl.sample_poses(0.0, 0.1, 2)), RES, ORG, 0.0), base)
    pl.close()
    h.clear_stamps()


# ---- the slot form
def _install(pl, scene):
    pad = rs.padded(scene, cs.MAX_SEG, cs.MAX_PIECES)
    for k in range(len(pad["slots"])):
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])


def _oracle_poses(pl, t0, dt, K):
    tab = pc.from_executing([pl.executing(s) for s in range(pl.max_queries)])
    return pc.poses(*tab, t0, dt, K, order=2)


def _state(pl, t0, dt):
    S = pl.max_queries
    return ([pl.executing(s) for s in range(S)], [pl.publisher_state(s) for s in range(S)], pl.sample_poses(t0, dt, 3))


def _same_state(a, b):
    for x, y in zip(a[0], b[0]):
        assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in EXEC_KEYS)
    for x, y in zip(a[1], b[1]):
        assert x["exe_index"] == y["exe_index"] and x["have_hist"] == y["have_hist"] and x["hist"].tobytes() == y["hist"].tobytes()
    assert a[2].tobytes() == b[2].tobytes()


SLOT_RES, SLOT_ORG = 0.5, (-30.0, -10.0)   # 120 x 440 cells over the scene's first two groups (slots 0, 1, 2, 4, 5): the others lie outside


@pytest.fixture(scope="module")
def crafted(hiplib, oracle):
    sc = cs.crafted(oracle.minco_generate)
    base = _base((440, 120), 4)
    h = hiplib.Handle()
    h.set_grid_map(base, SLOT_RES, SLOT_ORG)
    pl = hiplib.Planner(h, cs.N_SLOTS, 1)
    _install(pl, sc)
    yield dict(sc=sc, h=h, pl=pl, base=base)
    pl.close()
    h.close()


@pytest.mark.parametrize("K", [1, 3, 7])
def test_slot_form_on_the_crafted_scene(crafted, K):
    sc, h, pl, base = crafted["sc"], crafted["h"], crafted["pl"], crafted["base"]
    dt = 1.3
    before = _state(pl, sc["t0"], dt)
    poses = _oracle_poses(pl, sc["t0"], dt, K)
    assert np.isnan(poses[:, 3]).all() and np.isfinite(poses[:, 4]).all()       # empty slots in between
    subset = np.zeros(cs.N_SLOTS, dtype=np.uint8)
    subset[[1, 3, 5, 10]] = 1                                   # one on the map per group, an empty one, one outside the map
    for select, inflate in ((None, 0.0), (subset, SLOT_RES / np.sqrt(2.0)), (np.zeros(cs.N_SLOTS, dtype=np.uint8), 0.3), (None, 0.3)):
        h.clear_stamps()
        pl.stamp_slots(sc["t0"], dt, K, inflate, select=select)
        work = ps.stamp(base, ps.slot_boxes(poses, select), SLOT_RES, SLOT_ORG, inflate)
        n = _expect(h, work, base)
        assert (n > 0) == (select is None or select.any())
        ms = h.stamp_last_ms()
        assert ms[0] > 0.0 and ms[1] > 0.0
    h.stamp_poses(ps.slot_boxes(poses), 0.3)                    # the same boxes from the host: nothing new
    _expect(h, work, base)
    _same_state(before, _state(pl, sc["t0"], dt))
    h.clear_stamps()


def test_slot_form_over_three_tiles(hiplib, oracle):
    """130 slots: S_pad = 192, three tiles of the pose kernel; the seeded runs of conflict_scenes over a square of 200 m, a map of
    150 m x 130 m in its middle"""
    rng = np.random.default_rng(130)
    plans = cs.straight_plans(oracle.minco_generate, rng, 130, 200.0)
    plans[64], plans[129] = None, None
    res, org = 0.5, (-75.0, -65.0)
    base = _base((260, 300), 5)
    h = hiplib.Handle()
    h.set_grid_map(base, res, org)
    pl = hiplib.Planner(h, 130, 1)
    pad = rs.padded(dict(slots=plans), cs.MAX_SEG, cs.MAX_PIECES)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=0.0)
    before = _state(pl, 0.0, 2.5)
    poses = _oracle_poses(pl, 0.0, 2.5, 3)
    select = (np.arange(130) % 3 != 1).astype(np.uint8)
    for sel in (None, select):
        h.clear_stamps()
        pl.stamp_slots(0.0, 2.5, 3, 0.4, select=sel)
        n = _expect(h, ps.stamp(base, ps.slot_boxes(poses, sel), res, org, 0.4), base)
        assert n > 1000
    _same_state(before, _state(pl, 0.0, 2.5))
    pl.close()
    h.close()


def test_a_slot_under_its_own_stamp(hiplib, oracle):
    """the lanes of the crafted scene's slots 4 and 5 on open ground: stamped where it stands, slot 5 collides at its first sample"""
    sc = cs.crafted(oracle.minco_generate)
    h = hiplib.Handle()
    h.set_grid_map(np.zeros((40, 120), dtype=np.uint8), 0.5, (-30.0, cs.GROUP - 10.0))
    pl = hiplib.Planner(h, cs.N_SLOTS, 1)
    _install(pl, sc)
    t_now = sc["t0"] + 1.0
    before = pl.check(t_now)
    assert before["collision"].sum() == 0 and before["occupied"].sum() == 24
    sel = np.zeros(cs.N_SLOTS, dtype=np.uint8)
    sel[5] = 1
    pl.stamp_slots(t_now, 0.1, 1, 0.5 / np.sqrt(2.0), select=sel)
    got = pl.check(t_now)
    assert got["collision"][5] == 1 and got["first_sample"][5] == 0
    assert got["collision"].sum() == 1                          # its neighbour 3 m to the side stays clear
    h.clear_stamps()
    after = pl.check(t_now)
    assert set(after) == set(before) and all(np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes() for k in before)
    pl.close()
    h.close()


# ---- every consumer of the map sees the stamps
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


def test_consumers_see_a_stamped_handle_as_one_given_the_stamped_bytes(hiplib, oracle):
    base = np.zeros((40, 70), dtype=np.uint8)
    base[0, :] = base[-1, :] = 80                               # walls along the long sides, a post; bytes other than 0 and 80
    base[34:37, 4:6] = 80
    base[5:8, 20:30] = 127
    boxes = [_box(8.5, 3.0, 90.0), _box(13.8, 8.4, 30.0)]       # the first stands across the straight line from (2, 5) to (15, 5)
    plan = cs._run(oracle.minco_generate, (2.0, 5.0), (15.0, 5.0), 0.0)
    stamped = ps.stamp(base, boxes, RES, ORG, DIAG)
    A, B, Cb = hiplib.Handle(), hiplib.Handle(), hiplib.Handle()
    A.set_grid_map(base, RES, ORG)
    B.set_grid_map(stamped, RES, ORG)
    Cb.set_grid_map(base, RES, ORG)
    A.distance_field()                                          # A has built its distance field before the stamp: it must go stale
    A.stamp_poses(boxes, DIAG)
    _expect(A, stamped, base)
    a, b, c = _consumers(hiplib, A, plan), _consumers(hiplib, B, plan), _consumers(hiplib, Cb, plan)
    _same_consumers(a, b)
    assert a["validate"][0] == 1 and c["validate"][0] == 0      # the plan runs through the stamp, and the stamp is what stops it
    for k in ("rect", "dist", "search_paths"):
        assert np.asarray(a[k]).tobytes() != np.asarray(c[k]).tobytes(), k      # (no comparison above was between two unchanged things)
    A.clear_stamps()
    _same_consumers(_consumers(hiplib, A, plan), c)
    for h in (A, B, Cb):
        h.close()


# ---- end to end: B planned against A's swept footprint goes round it
def test_a_second_vehicle_plans_round_a_stamped_one(hiplib, oracle):
    """40 m x 40 m of open ground (cells of 0.2 m).  Slot 0, A, creeps east along y = 0 from x = 5 to x = 7 in 30 s, its box over
    x = 3.6 .. 10.4 on B's line all the while; B is to drive from (-4, 0) to (16, 0), straight through it, and has to pull out by
    some 2.2 m to pass."""
    res, org = 0.2, (-20.0, -20.0)
    h = hiplib.Handle()
    h.set_grid_map(np.full((200, 200), 127, dtype=np.uint8), res, org)
    pl = hiplib.Planner(h, 2, 4)
    pp = hiplib.default_plan_params()
    pp.seed = 7
    pad = rs.padded(dict(slots=[cs._run(oracle.minco_generate, (5.0, 0.0), (7.0, 0.0), 0.0, seconds=30.0), None]), pp.max_seg, pp.max_pieces)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"],
               t_start=0.0)                                     # (in the padding of the plans that will be adopted beside it)
    S, E = np.array([[-4.0, 0.0, 0.0, 0.0]]), np.array([[16.0, 0.0, 0.0, 0.0]])
    t0, dt, K = 0.0, 0.25, 121                                  # the 30 s of A's plan
    # control: on the base map B's plan runs into A at a common clock
    out = pl.plan(S, E, pp=pp)
    assert out["plan_status"][0] == hiplib.PLAN_OK and out["winner"][0] >= 0
    assert pl.adopt([0], [1], t_start=0.0)[0] == 1
    ctl = pl.check_conflicts(t0, dt, K, 0.0, 20.0)
    print("control: min_sep", ctl["min_sep"], "sample", ctl["sep_sample"])
    assert ctl["min_sep"][1] == 0.0 and ctl["sep_partner"][1] == 0
    # with A stamped over the horizon
    pl.clear([1])
    pl.stamp_slots(t0, dt, K, res / np.sqrt(2.0))
    assert h.read_cells()[1] > 0
    out = pl.plan(S, E, pp=pp)
    w = int(out["winner"][0])
    print("stamped: status", out["plan_status"], "winner", w, "r_collision", out["r_collision"])
    assert out["plan_status"][0] == hiplib.PLAN_OK and w >= 0 and out["r_collision"][0, w] == 0
    assert pl.adopt([0], [1], t_start=0.0)[0] == 1
    got = pl.check_conflicts(t0, dt, K, 0.0, 20.0)
    print("stamped: min_sep", got["min_sep"], "sample", got["sep_sample"])
    assert got["min_sep"][1] > 0.0 and got["min_sep"][0] > 0.0
    pl.close()
    h.close()
