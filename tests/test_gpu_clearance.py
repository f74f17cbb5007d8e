"""The distance field of the grid map (distfield.hip), the clearance of solved and executing plans (clearance.hip) and the clearance
filter of dftpav_plan_queries -- every cell and every field equal to oracle_clearance in order 2 (tests/limits_cases.py holds the
chain of CPU oracles the filter is held against)."""
import ctypes as C

import numpy as np
import pytest

import limits_cases as lc
import terms_cases as tc
from dftpav_amd import replan_scenes as rs
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import LayoutSpec
from oracle_clearance import pyclearance as pc

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
FAR = pc.FAR
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")
RES, ORG = 0.2, (-3.0, -2.0)

# Both field passes run workgroups of 64 x 4 threads (kDistTileX, kDistTileY): a wave takes 64 cells of a row (the row pass carries
# its scan from one chunk of 64 to the next), a workgroup four rows.  The sizes the issue names, then each side of those boundaries:
# 63 / 64 / 65 and 127 / 128 / 129 cells along x (one chunk, exactly one, a carry into a second and a third), 3 / 4 / 5 and 8 / 9
# rows (one workgroup, exactly one, two and three).
SIZES = [(1, 1), (1, 7), (7, 1), (33, 17), (64, 64), (65, 63), (257, 3),
         (63, 4), (64, 5), (65, 3), (127, 8), (128, 9), (129, 5)]                # (size_x, size_y)


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in pc.FIELDS)


def _fills(rng, sx, sy):
    corner = np.zeros((sy, sx), dtype=np.uint8)
    corner[sy - 1, sx - 1] = 80
    return dict(empty=np.zeros((sy, sx), dtype=np.uint8), corner=corner, full=np.full((sy, sx), 80, dtype=np.uint8),
                d01=np.where(rng.random((sy, sx)) < 0.01, 80, 0).astype(np.uint8),
                d30=np.where(rng.random((sy, sx)) < 0.30, 80, 0).astype(np.uint8))


@pytest.mark.parametrize("sx,sy", SIZES)
def test_field_equals_the_oracle_in_every_cell(hiplib, sx, sy):
    rng = np.random.default_rng(1000 * sx + sy)
    h = hiplib.Handle()
    for name, g in _fills(rng, sx, sy).items():
        h.set_grid_map(g, RES, ORG)                             # (each a second dftpav_set_grid_map of the handle: the field follows)
        got, ref = h.distance_field(), pc.field(g)
        assert got.shape == (sy, sx) and np.array_equal(got, ref), (name, np.argwhere(got != ref)[:5])
        if name == "empty":
            assert (got == FAR).all()
        if name == "full":
            assert not got.any()
        if name == "corner":
            assert got[0, 0] == (sx - 1) ** 2 + (sy - 1) ** 2
    h.close()


def test_field_of_the_default_arena_and_of_a_second_map(hiplib):
    grid, res, org, _, _ = ss.arena()
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError) as e:
        h.distance_field(fetch=False)                           # no map yet
    assert e.value.code == hiplib.E_INVALID
    assert h.clearance_last_ms() == (0.0, 0.0)
    h.set_grid_map(grid, res, org)
    assert h.clearance_last_ms() == (0.0, 0.0)                  # dftpav_set_grid_map built nothing
    h.distance_field(fetch=False)                               # build only
    ms = h.clearance_last_ms()
    got = h.distance_field()                                    # (no second build: the map did not change)
    assert h.clearance_last_ms() == ms and ms[0] > 0.0 and ms[1] == 0.0
    ref = pc.field(grid)
    print("arena", grid.shape, "field build ms", ms[0], "largest d2", int(ref.max()))
    assert np.array_equal(got, ref) and np.array_equal(got == 0, grid == 80)
    # a second, smaller map on the same handle: the field is that of the new map
    g2 = np.zeros((37, 91), dtype=np.uint8)
    g2[5, 70] = g2[30, 2] = 80
    h.set_grid_map(g2, 0.5, (0.0, 0.0))
    assert np.array_equal(h.distance_field(), pc.field(g2))
    # and back to a larger one
    h.set_grid_map(grid[:300, :1100], res, org)
    assert np.array_equal(h.distance_field(), pc.field(grid[:300, :1100]))
    # a side above 16384 cells: refused, whichever side
    for shape in ((1, 16385), (16385, 1)):
        h.set_grid_map(np.zeros(shape, dtype=np.uint8), res, org)
        with pytest.raises(hiplib.DftpavError) as e:
            h.distance_field()
        assert e.value.code == hiplib.E_UNSUPPORTED
    line = np.zeros((1, 16384), dtype=np.uint8)                  # the largest side allowed: the largest distances of the field
    line[0, 0] = 80
    h.set_grid_map(line, res, org)
    assert np.array_equal(h.distance_field()[0], np.arange(16384, dtype=np.int64) ** 2)
    h.close()


def _set_coeffs(hiplib, bt, co, dt):
    fn = hiplib.lib().dftpav_debug_batch_set_coeffs
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    co, dt = np.ascontiguousarray(co, dtype=np.float64), np.ascontiguousarray(dt, dtype=np.float64)
    assert fn(bt._b, co.ctypes.data_as(C.c_void_p), dt.ctypes.data_as(C.c_void_p)) == 0


def _crafted(hiplib, h, scene, piece_nums, singuls, co, dt, check_dt):
    """device and oracle rows of coefficients [B][Ntot][6][2] / piece durations [B][M] on the map scene = (grid, res, org); the
    device's collision re-check of the same batch beside them"""
    grid, res, org = scene
    co = np.ascontiguousarray(co, dtype=np.float64)
    bt = hiplib.Batch(h, LayoutSpec(list(piece_nums), list(singuls), 4), co.shape[0])
    _set_coeffs(hiplib, bt, co, dt)
    got = bt.check_clearance(check_dt)
    col, first = bt.validate(sample_dt=check_dt, vertex_res=0.1)
    bt.close()
    ref = pc.check_batch(grid, res, org, singuls, piece_nums, co, dt, check_dt, order=2)
    assert _same(got, ref), (got, ref)
    assert np.array_equal(got["min_d2"] == 0, col != 0) and np.array_equal(got["arg"][col != 0], first[col != 0])
    return got, ref


def straight(x0, y0, speed, n_pieces, dT, direction=1.0):
    co = np.zeros((n_pieces, 6, 2))
    for p in range(n_pieces):
        co[p, 0] = (x0 + direction * speed * dT * p, y0)
        co[p, 1, 0] = direction * speed
    return co


@pytest.fixture(scope="module")
def arena(hiplib, oracle):
    """the fourteen arena queries, a handle with their map, and the outputs of a planner that never had a filter"""
    grid, res, org, S, E = lc.chain()["scene"]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, len(E), lc.R)
    plain = pl0.plan(S, E, pp=_pp(hiplib))
    yield dict(h=h, scene=(grid, res, org), S=S, E=E, Q=len(E), plain=plain, pl0=pl0, n_batches=pl0.info()["n_batches"])
    pl0.close()
    h.close()


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    return pp


_CHAIN_CLR = None


def chain_clearance():
    """the clearance oracle (order 2) on every restart of the chain: dict of [Q][R] rows, (FAR, -1, inf) where nothing was solved"""
    global _CHAIN_CLR
    if _CHAIN_CLR is None:
        ch = lc.chain()
        grid, res, org, _, _ = ch["scene"]
        Q = len(ch["per"])
        out = dict(min_d2=np.full((Q, lc.R), FAR, np.int32), arg=np.full((Q, lc.R), -1, np.int32), clearance=np.full((Q, lc.R), INF),
                   n_samples=np.zeros((Q, lc.R), np.int32))
        for q, e in enumerate(ch["per"]):
            if e is not None:
                r = pc.check_batch(grid, res, org, e["layout"].singuls, e["layout"].piece_nums, e["coeffs"], e["dts"], lc.CHECK_DT, order=2)
                for k in out:
                    out[k][q] = r[k]
        _CHAIN_CLR = out
    return _CHAIN_CLR


def test_batch_clearance_on_the_chain(hiplib, arena):
    """the chain's solved coefficients through dftpav_debug_batch_set_coeffs: all three fields equal the oracle, min_d2 == 0 exactly
    where dftpav_batch_validate reports a collision and arg is then its first sample; plans of more than 256 samples and
    gear-shift plans are among them"""
    ch, ref = lc.chain(), chain_clearance()
    n, more, gears, hits = 0, 0, 0, 0
    for q, e in enumerate(ch["per"]):
        if e is None:
            continue
        lay = e["layout"]
        for dt in (lc.CHECK_DT, 0.0371):                        # the second divides no duration
            got, r = _crafted(hiplib, arena["h"], arena["scene"], lay.piece_nums, lay.singuls, e["coeffs"], e["dts"], dt)
            if dt == lc.CHECK_DT:
                assert all(np.array_equal(got[k], ref[k][q]) for k in pc.FIELDS), q
                assert np.array_equal(got["min_d2"] == 0, e["collision"] != 0), q
            more += int((r["n_samples"] > 256).sum())
            hits += int((got["min_d2"] == 0).sum())
        gears += len(lay.singuls) > 1 and -1 in list(lay.singuls)
        n += 1
    print("queries", n, "rows of more than 256 samples", more, "gear-shift layouts", gears, "colliding rows", hits)
    assert n >= 10 and more >= 2 and gears >= 1 and hits >= 2
    assert arena["h"].clearance_last_ms()[1] > 0.0


def test_batch_clearance_of_crafted_plans(hiplib, arena, oracle):
    h, scene = arena["h"], arena["scene"]
    y = rs.LANES[1]
    # exactly 256 and 257 samples: check_dt 2^-4 and durations of 16 and 16 + 2^-4 s are exact, so t_256 = 16.0 is the first
    # sample that is not < 16.0, and is < 16.0625; thread 0 of the workgroup then takes a second sample
    for dT, want in ((4.0, 256), (4.015625, 257)):
        got, ref = _crafted(hiplib, h, scene, [4], [1], straight(-64.0, y, 1.0, 4, dT)[None], [[dT]], 0.0625)
        assert ref["n_samples"][0] == want and 0 < got["min_d2"][0] < FAR and got["arg"][0] >= 0
    # a plan shorter than one sample step: a single sample at t = 0
    got, ref = _crafted(hiplib, h, scene, [2], [1], straight(-64.0, y, 1.0, 2, 0.01)[None], [[0.01]], 0.05)
    assert ref["n_samples"][0] == 1 and got["arg"][0] == 0 and got["min_d2"][0] < FAR
    # translated wholly off the grid: every probe is skipped
    got, ref = _crafted(hiplib, h, scene, [4], [1], straight(1.0e4, y, 1.0, 4, 1.0)[None], [[1.0]], 0.05)
    assert got["min_d2"][0] == FAR and got["arg"][0] == -1 and np.isposinf(got["clearance"][0]) and ref["n_samples"][0] > 0
    # partly off the grid (it leaves across the map's edge): the probes inside count
    grid, res, org = scene
    x_edge = org[0] + res * grid.shape[1]
    got, ref = _crafted(hiplib, h, scene, [4], [1], straight(x_edge - 6.0, y, 2.0, 4, 1.0)[None], [[1.0]], 0.05)
    assert got["min_d2"][0] < FAR
    # two segments, the second in reverse (replan_scenes.plan_b)
    pb = rs.plan_b(oracle.minco_generate, 2)
    got, ref = _crafted(hiplib, h, scene, pb["piece_nums"], pb["singul"], pb["coeffs"][None], pb["coeff_dt"][None], 0.05)
    assert 0 < got["min_d2"][0] < FAR
    # the pointers of dftpav_clearance_out may be NULL, one by one
    bt = hiplib.Batch(h, LayoutSpec([4], [1], 4), 1)
    _set_coeffs(hiplib, bt, straight(-64.0, y, 1.0, 4, 1.0)[None], [[1.0]])
    full = bt.check_clearance(0.05)
    out = hiplib.ClearanceOut(1)
    out.c.min_d2 = None
    out.c.clearance = None
    fn = hiplib.lib().dftpav_batch_check_clearance
    fn.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    assert fn(bt._b, 0.05, C.byref(out.c)) == 0
    assert out.a["arg"][0] == full["arg"][0] and out.a["min_d2"][0] == 0 and out.a["clearance"][0] == 0.0
    bt.close()


def test_collision_and_an_empty_map(hiplib, oracle):
    """the map of the replan scene (a box dropped onto lane 0): the plan through it has min_d2 0 at validate's first sample; the
    same plans on an empty map: FAR, -1, +inf"""
    scene = rs.crafted(oracle.minco_generate)
    m = (scene["grid"], scene["resolution"], scene["origin"])
    h = hiplib.Handle()
    h.set_grid_map(*m)
    pa = [rs.plan_a(oracle.minco_generate, lane) for lane in (0, 1)]
    co = np.stack([p["coeffs"] for p in pa])
    dts = np.stack([p["coeff_dt"] for p in pa])
    got, _ = _crafted(hiplib, h, m, [6], [1], co, dts, 0.05)
    assert got["min_d2"][0] == 0 and got["clearance"][0] == 0.0 and got["arg"][0] > 0 and got["min_d2"][1] > 0
    empty = (np.zeros_like(m[0]), m[1], m[2])
    h.set_grid_map(*empty)
    got, _ = _crafted(hiplib, h, empty, [6], [1], co, dts, 0.05)
    assert (got["min_d2"] == FAR).all() and (got["arg"] == -1).all() and np.isposinf(got["clearance"]).all()
    h.close()


def test_table_variant(hiplib, oracle):
    scene = rs.crafted(oracle.minco_generate)
    grid, res, org = scene["grid"], scene["resolution"], scene["origin"]
    Q = rs.N_SLOTS + 2
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, lc.R)
    empty = pl.check_clearance(0.05)                            # before the table was filled once
    assert (empty["min_d2"] == FAR).all() and (empty["arg"] == -1).all() and np.isposinf(empty["clearance"]).all()
    pad = rs.padded(scene)
    for k in range(len(pad["slots"])):
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])
    for dt in (0.05, 0.0371):
        ex = [pl.executing(s) for s in range(Q)]
        ref = pc.check_table(grid, res, org, [e["n_seg"] for e in ex], [e["singul"] for e in ex], [e["piece_nums"] for e in ex],
                             [e["coeff_dt"] for e in ex], np.array([e["coeffs"] for e in ex]), dt, order=2)
        got = pl.check_clearance(dt)
        assert _same(got, ref), (dt, got, ref)
        after = [pl.executing(s) for s in range(Q)]             # the table is unchanged, byte for byte
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for a, b in zip(ex, after) for k in EXEC_KEYS)
    occupied = np.array([e["n_seg"] > 0 for e in ex])
    assert occupied.sum() == 9
    assert (got["min_d2"][~occupied] == FAR).all() and (got["arg"][~occupied] == -1).all() and np.isposinf(got["clearance"][~occupied]).all()
    assert (got["arg"][occupied] >= 0).all() and got["min_d2"][3] == 0 and (got["min_d2"][occupied] == 0).sum() == 1   # slot 3: the box on its lane
    assert any(e["n_seg"] >= 2 and -1 in e["singul"][:e["n_seg"]] for e in ex)     # gear-shift plans among them
    pl.close()
    h.close()


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_filter_off_is_a_planner_without_one(hiplib, arena):
    pl = hiplib.Planner(arena["h"], arena["Q"], lc.R)
    pl.set_clearance_filter(None)                               # off before it was ever on
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    pl.set_clearance_filter(0.5, lc.CHECK_DT)
    pl.set_clearance_filter(-1.0)
    off = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    _same_outputs(off, arena["plain"])
    assert pl.info()["n_batches"] == arena["n_batches"]
    for planner in (pl, arena["pl0"]):
        with pytest.raises(hiplib.DftpavError) as e:
            planner.last_clearance(arena["Q"])                  # that call ran without the filter
        assert e.value.code == hiplib.E_INVALID
    pl.close()


# The two thresholds come from the oracle chain's own clearances (chain_clearance(), 0.2 m cells): the unfiltered winners lie
# between 0.2 m and 2.41 m.  0.5 m (min_d2 >= 7) lies between those and moves at least one query to a dearer restart; 1.0 m is
# larger and leaves queries without a restart.  The test asserts these properties of the thresholds from the oracle rows.
MIN_1, MIN_2 = 0.5, 1.0


def _filter_case(hiplib, arena, pl, min_clearance, extra_reject=None):
    """plan() with the clearance filter at min_clearance against the selection rule over the oracle flags; returns per solved query
    (w0, w1), the device outputs and the last rows"""
    ch, ref, plain = lc.chain(), chain_clearance(), arena["plain"]
    Q = arena["Q"]
    pl.set_clearance_filter(min_clearance, lc.CHECK_DT)
    out = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    last = pl.last_clearance(Q)
    wins = {}
    for q, c in enumerate(ch["per"]):
        if c is None or out["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            assert out["winner"][q] == -1 and (last["min_d2"][q] == FAR).all() and (last["arg"][q] == -1).all(), q
            assert np.isposinf(last["clearance"][q]).all(), q
            continue
        assert all(np.array_equal(last[k][q], ref[k][q]) for k in pc.FIELDS), (q, last["min_d2"][q], ref["min_d2"][q])
        r = c["solve"]
        rej = (~(ref["clearance"][q] >= min_clearance)).astype(np.int32)
        if extra_reject is not None:
            rej = rej | extra_reject[q]
        w0 = lc.select(r["final_cost"], r["success"], c["collision"])
        w1 = lc.select(r["final_cost"], r["success"], c["collision"] | rej)
        print(q, "min", min_clearance, "winner", w0, "->", w1, "device", plain["winner"][q], "->", out["winner"][q], "clearance",
              last["clearance"][q].tolist())
        assert plain["winner"][q] == w0 and out["winner"][q] == w1, q
        assert out["plan_status"][q] == (hiplib.PLAN_OK if w1 >= 0 else hiplib.PLAN_NO_VALID_RESTART), q
        assert np.array_equal(out["r_collision"][q], c["collision"]) and np.array_equal(out["r_first_sample"][q], c["first"]), q
        for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
            assert np.array_equal(out[k][q], plain[k][q]), (q, k)
        if w1 >= 0:
            assert out["final_cost"][q] == r["final_cost"][w1] and np.array_equal(out["coeffs"][q, :c["layout"].n_pieces], c["coeffs"][w1]), q
        else:
            assert not out["coeffs"][q].any(), q
        wins[q] = (w0, w1)
    return wins, out, last


def test_filter_on(hiplib, arena):
    ch, ref = lc.chain(), chain_clearance()
    w_clr = [ref["clearance"][q, lc.select(c["solve"]["final_cost"], c["solve"]["success"], c["collision"])]
             for q, c in enumerate(ch["per"]) if c is not None and lc.select(c["solve"]["final_cost"], c["solve"]["success"], c["collision"]) >= 0]
    assert min(w_clr) < MIN_1 < max(w_clr) and MIN_2 > MIN_1
    pl = hiplib.Planner(arena["h"], arena["Q"], lc.R)
    wins, out, last = _filter_case(hiplib, arena, pl, MIN_1)
    changed = [q for q, (w0, w1) in wins.items() if w1 >= 0 and w1 != w0]
    assert changed, wins                                        # at least one query's winner differs from the unfiltered one
    for q in changed:
        r = ch["per"][q]["solve"]
        assert r["final_cost"][wins[q][1]] > r["final_cost"][wins[q][0]] and last["clearance"][q, wins[q][1]] >= MIN_1 > last["clearance"][q, wins[q][0]]
    # a refused change of the filter leaves it as it is
    for bad_min, bad_dt in ((NAN, 0.05), (INF, 0.05), (MIN_1, 0.0), (MIN_1, -0.05), (MIN_1, NAN), (MIN_1, INF)):
        with pytest.raises(hiplib.DftpavError) as e:
            pl.set_clearance_filter(bad_min, bad_dt)
        assert e.value.code == hiplib.E_INVALID
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), out)
    assert _same(pl.last_clearance(arena["Q"]), last)
    # the larger threshold: queries without a valid restart
    wins2, out2, _ = _filter_case(hiplib, arena, pl, MIN_2)
    none = [q for q, (w0, w1) in wins2.items() if w0 >= 0 and w1 == -1]
    assert none and all(out2["plan_status"][q] == hiplib.PLAN_NO_VALID_RESTART for q in none), wins2
    # 0.0 is legal and rejects nothing that does not already collide
    wins0, out0, _ = _filter_case(hiplib, arena, pl, 0.0)
    assert all(w0 == w1 for w0, w1 in wins0.values())
    _same_outputs(out0, arena["plain"])
    pl.set_clearance_filter(None)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    pl.close()


def test_composition_with_the_limit_and_penalty_filters(hiplib, arena):
    """all three filters on: the winners equal the rule over the OR of the three oracle flags, whichever subset is set"""
    Q = arena["Q"]
    T, _ = tc.chain_terms()
    caps = hiplib.PenaltyCaps(**tc.CAPS)
    pen_rej = tc.gate_rule(T.reshape(-1, 5), caps, np.zeros(Q * lc.R, np.int32))[1].reshape(Q, lc.R)
    lim = hiplib.default_limits()
    lim.max_forward_vel, lim.max_backward_vel, lim.max_forward_cur, lim.max_backward_cur = 5.01, 2.01, 1.01, 1.01   # tests/test_gpu_limits.py: FILTER
    lim_rej = 1 - lc.chain_limits(lim)["feasible"]
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    low = 0.25                                                   # (between one and two cells: rejects the restarts that pass one cell from a wall)
    pl.set_limit_filter(lim, lc.CHECK_DT)
    wins_l, _, _ = _filter_case(hiplib, arena, pl, low, extra_reject=lim_rej)
    pl.set_penalty_filter(caps)
    wins_all, out_all, last = _filter_case(hiplib, arena, pl, low, extra_reject=lim_rej | pen_rej)
    lrows = pl.last_limits(Q)
    _, prej = pl.last_cost_terms(Q)
    assert np.array_equal(prej, pen_rej) and np.array_equal(lrows["feasible"], 1 - lim_rej)
    pl.set_limit_filter(None)
    wins_p, _, _ = _filter_case(hiplib, arena, pl, low, extra_reject=pen_rej)
    pl1 = hiplib.Planner(arena["h"], Q, lc.R)
    only, _, _ = _filter_case(hiplib, arena, pl1, low)
    pl1.close()
    assert len({tuple(sorted(w.items())) for w in (wins_l, wins_all, wins_p, only)}) >= 2     # the other filters add rejections of their own
    # a refused call leaves the filter state as it was
    with pytest.raises(hiplib.DftpavError):
        pl.set_clearance_filter(NAN, lc.CHECK_DT)
    with pytest.raises(hiplib.DftpavError):
        pl.set_penalty_filter(hiplib.PenaltyCaps(-1.0, INF, INF))
    wins_again, _, _ = _filter_case(hiplib, arena, pl, low, extra_reject=pen_rej)
    assert wins_again == wins_p
    pl.close()


def test_filter_rows_do_not_leak_between_calls(hiplib, arena):
    """all three filters on: after a call of Q queries, a call of the first Q // 2 on the same planner leaves the rows and the plans
    of a fresh planner given that second call alone; a read-out of a filter the latest call ran without is refused"""
    Q, S, E = arena["Q"], arena["S"], arena["E"]
    n = Q // 2
    caps = hiplib.PenaltyCaps(**tc.CAPS)
    lim = hiplib.default_limits()
    lim.max_forward_vel, lim.max_backward_vel, lim.max_forward_cur, lim.max_backward_cur = 5.01, 2.01, 1.01, 1.01   # tests/test_gpu_limits.py: FILTER

    def planner():
        pl = hiplib.Planner(arena["h"], Q, lc.R)
        pl.set_limit_filter(lim, lc.CHECK_DT)
        pl.set_clearance_filter(0.25, lc.CHECK_DT)
        pl.set_penalty_filter(caps)
        return pl

    def rows(pl):
        terms, rej = pl.last_cost_terms(n)
        return dict(limits=pl.last_limits(n), clearance=pl.last_clearance(n), terms=dict(terms=terms, rejected=rej))

    pl, fresh = planner(), planner()
    whole = pl.plan(S, E, pp=_pp(hiplib))
    assert (pl.last_limits(Q)["feasible"][n:] != 0).any() and np.isfinite(pl.last_clearance(Q)["clearance"][n:]).any()   # rows behind n were written
    second, alone = pl.plan(S[:n], E[:n], pp=_pp(hiplib)), fresh.plan(S[:n], E[:n], pp=_pp(hiplib))
    _same_outputs(second, alone)
    for k in whole:
        assert np.array_equal(second[k], whole[k][:n], equal_nan=True), k
    got, ref = rows(pl), rows(fresh)
    for name in ref:
        assert set(got[name]) == set(ref[name])
        for k in ref[name]:
            assert np.array_equal(got[name][k], ref[name][k], equal_nan=True), (name, k)
    assert np.isin(second["plan_status"], (hiplib.PLAN_OK, hiplib.PLAN_NO_VALID_RESTART)).any()
    fresh.close()
    # the latest call ran without a filter: its rows are not there to read, whatever an earlier call left
    reads = dict(limits=lambda: pl.last_limits(n), terms=lambda: pl.last_cost_terms(n), clearance=lambda: pl.last_clearance(n))
    for off, name in ((lambda: pl.set_limit_filter(None), "limits"), (lambda: pl.set_penalty_filter(None), "terms"),
                      (lambda: pl.set_clearance_filter(None), "clearance")):
        off()
        pl.plan(S[:n], E[:n], pp=_pp(hiplib))
        with pytest.raises(hiplib.DftpavError) as e:
            reads[name]()
        assert e.value.code == hiplib.E_INVALID, name
    pl.close()


def test_refusals_leave_outputs_untouched(hiplib, oracle):
    h = hiplib.Handle()
    bt = hiplib.Batch(h, LayoutSpec([4], [1], 4), 2)
    fb = hiplib.lib().dftpav_batch_check_clearance
    fb.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    fp = hiplib.lib().dftpav_planner_check_clearance
    fp.argtypes = [C.c_void_p, C.c_double, C.c_void_p]

    def untouched(fn, obj, n, dt):
        out = hiplib.ClearanceOut(n)
        for a in out.a.values():
            a[...] = 77
        assert fn(obj, dt, C.byref(out.c)) == hiplib.E_INVALID
        assert all((a == 77).all() for a in out.a.values())

    co = np.stack([straight(-64.0, rs.LANES[1], 1.0, 4, 1.0)] * 2)
    pl = hiplib.Planner(h, 3, 2)
    untouched(fb, bt._b, 2, 0.05)                               # no map, nothing solved
    _set_coeffs(hiplib, bt, co, [[1.0], [1.0]])
    untouched(fb, bt._b, 2, 0.05)                               # coefficients, but no grid map installed
    untouched(fp, pl._p, 3, 0.05)
    grid, res, org, _, _ = ss.arena()
    h.set_grid_map(grid, res, org)
    bt2 = hiplib.Batch(h, LayoutSpec([4], [1], 4), 2)
    untouched(fb, bt2._b, 2, 0.05)                              # a map, but no solved coefficients
    good = bt.check_clearance(0.05)
    for dt in (0.0, -0.05, NAN, INF):
        untouched(fb, bt._b, 2, dt)
        untouched(fp, pl._p, 3, dt)
    assert fb(bt._b, 0.05, None) == hiplib.E_INVALID and fp(pl._p, 0.05, None) == hiplib.E_INVALID
    assert _same(bt.check_clearance(0.05), good)                # and the batch is as it was
    with pytest.raises(hiplib.DftpavError) as e:
        pl.last_clearance(1)                                    # no call to read
    assert e.value.code == hiplib.E_INVALID
    pl.close()
    bt2.close()
    bt.close()
    h.close()
