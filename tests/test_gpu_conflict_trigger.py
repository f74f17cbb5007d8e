"""The conflict trigger on the device (conflict_trigger.hip): every row of dftpav_planner_check_yield, dftpav_debug_conflict_trigger
and the trigger of dftpav_replan_tick identical to oracle_conflict/pytrigger.py -- on the crafted scene, across tile edges, for
sample counts that do not fill the four waves -- the read-out writes nothing, and the tick with the trigger replans the union of the
check's flags and the trigger's yields exactly as a separate dftpav_plan_queries call does."""
import ctypes as C
import itertools

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from dftpav_amd import search_scenes as ss
from dftpav_amd import trigger_scenes as ts
from oracle_conflict import pyconflict as pc
from oracle_conflict import pytrigger as pt
from oracle_replan import pyreplan as pr

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")
CHECK_KEYS = pr.INTS + ("desired", "start_state", "start_ctrl")
YIELD_ARGTYPES = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]


def _install(pl, scene, max_seg=cs.MAX_SEG, max_pieces=cs.MAX_PIECES):
    pad = rs.padded(scene, max_seg, max_pieces)
    for k in range(len(pad["slots"])):
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])
    for s, p in enumerate(scene["slots"]):
        if p is not None and p.get("hist") is not None:
            pl.set_history([s], [p["hist"][0]], [p["hist"][1]])


def _table(pl):
    """the table as the device holds it, read back slot by slot: the oracle's arguments, and the ends of the last segments"""
    ex = [pl.executing(s) for s in range(pl.max_queries)]
    return pc.from_executing(ex), np.array([e["end_time"][e["n_seg"] - 1] if e["n_seg"] > 0 else 0.0 for e in ex])


def _oracle(tab, ends, t_now, t0, dt, K, margin, rng, stats=None):
    ref = pt.check_yield(*tab, t_now, t0, dt, K, margin, rng, order=2, stats=stats)
    assert np.array_equal(pt.end_times(tab[0], tab[2], tab[3], tab[5]), ends)     # the oracle chains the ends the table holds
    return ref


def _same(got, ref):
    for k in pt.FIELDS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:8], a[a != b][:8], b[a != b][:8])


def _empty(r, idx=slice(None)):
    return (r["yield"][idx] == 0).all() and (r["yield_sample"][idx] == -1).all() and (r["yield_partner"][idx] == -1).all()


def _exec_same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in EXEC_KEYS)


@pytest.fixture(scope="module")
def crafted(hiplib, oracle):
    sc = ts.crafted(oracle.minco_generate)
    h = hiplib.Handle()
    pl = hiplib.Planner(h, ts.N_SLOTS, 1)
    fresh = pl.check_yield(sc["t0"], sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)      # never filled
    _install(pl, sc)
    tab, ends = _table(pl)
    yield dict(sc=sc, h=h, pl=pl, tab=tab, ends=ends, fresh=fresh)
    pl.close()
    h.close()


def test_a_never_filled_planner_gives_the_empty_rows(hiplib, crafted):
    assert _empty(crafted["fresh"]) and crafted["fresh"]["yield"].shape == (ts.N_SLOTS,)
    with pytest.raises(hiplib.DftpavError) as e:
        crafted["pl"].last_trigger()                            # no tick ran with the trigger
    assert e.value.code == hiplib.E_INVALID


@pytest.mark.parametrize("case", ts.CASES)
def test_read_out_equals_the_oracle_on_the_scene(crafted, case):
    sc, pl = crafted["sc"], crafted["pl"]
    seen = []
    for t_now in sc["t_nows"]:
        got = pl.check_yield(t_now, sc["t0"], sc["dt"], sc["K"], *case)
        ref = _oracle(crafted["tab"], crafted["ends"], t_now, sc["t0"], sc["dt"], sc["K"], *case)
        _same(got, ref)
        seen.append(got)
        ms = crafted["h"].trigger_last_ms()
        assert ms[0] > 0.0 and ms[1] > 0.0
    a, b = seen                                                 # slot 21's plan ends between the two clocks: who yields flips
    assert (a["yield"][20], a["yield"][21]) == (0, 1) and (b["yield"][20], b["yield"][21]) == (1, 0)
    assert a["yield"][1] == 1 and a["yield_partner"][1] == 0 and a["yield"][0] == 0 and a["yield_sample"][0] == -1
    assert a["yield"][3] == 1 and a["yield_partner"][3] == 4 and a["yield"][4] == 0 and a["yield_partner"][4] == 3


@pytest.mark.parametrize("K", [1, 2, 3, 7, 257])
def test_sample_counts(crafted, K):
    sc, pl = crafted["sc"], crafted["pl"]
    dt = 10.0 / 256 if K == 257 else 0.4                        # 257 clocks over the scene's 10 s: exactly representable steps
    hits = 0
    for t0 in (sc["t0"], sc["t0"] + 4.0):                       # the second window starts next to the crossings
        for t_now in sc["t_nows"]:
            got = pl.check_yield(t_now, t0, dt, K, 0.5, 60.0)
            _same(got, _oracle(crafted["tab"], crafted["ends"], t_now, t0, dt, K, 0.5, 60.0))
            hits += int(got["yield"].sum())
    assert hits >= 4                                            # the overlapping pairs conflict at every clock


def test_nothing_is_written(crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    S = ts.N_SLOTS
    grid = np.zeros((40, 120), dtype=np.uint8)                  # dftpav_replan_check needs a map; the trigger's read-out does not
    grid[20:22, 70:72] = 80
    crafted["h"].set_grid_map(grid, 0.5, (-30.0, cs.GROUP - 10.0))

    def state():
        ex = [pl.executing(s) for s in range(S)]
        pub = [pl.publisher_state(s) for s in range(S)]
        chk = pl.check(sc["t0"] + 1.0)
        cnf = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
        return ex, pub, chk, cnf

    ex0, pub0, chk0, cnf0 = state()
    for t_now in sc["t_nows"]:
        pl.check_yield(t_now, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    ex1, pub1, chk1, cnf1 = state()
    assert all(_exec_same(a, b) for a, b in zip(ex0, ex1))
    for a, b in zip(pub0, pub1):
        assert a["exe_index"] == b["exe_index"] and a["have_hist"] == b["have_hist"] and a["hist"].tobytes() == b["hist"].tobytes()
    assert chk0["occupied"].sum() == 17
    assert set(chk0) == set(chk1) and all(np.asarray(chk0[k]).tobytes() == np.asarray(chk1[k]).tobytes() for k in chk0)
    assert set(cnf0) == set(cnf1) and all(np.asarray(cnf0[k]).tobytes() == np.asarray(cnf1[k]).tobytes() for k in cnf0)


def test_null_output_pointers(hiplib, crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    full = pl.check_yield(sc["t0"], sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    fn = hiplib.lib().dftpav_planner_check_yield
    fn.argtypes = YIELD_ARGTYPES
    n = 0
    for keep in itertools.product((False, True), repeat=3):
        if not any(keep):
            continue
        out = hiplib.YieldOut(ts.N_SLOTS)
        for a in out.a.values():
            a[...] = 77
        for k, on in zip(pt.FIELDS, keep):
            if not on:
                setattr(out.c, k, None)
        assert fn(pl._p, sc["t0"], sc["t0"], sc["dt"], sc["K"], 0.5, 60.0, C.byref(out.c)) == hiplib.OK
        for k, on in zip(pt.FIELDS, keep):
            assert np.array_equal(out.a[k], full[k]) if on else (out.a[k] == 77).all(), (keep, k)
        n += 1
    assert n == 7


def test_refusals_change_nothing(hiplib, crafted):
    sc, pl, h = crafted["sc"], crafted["pl"], crafted["h"]
    good = pl.check_yield(sc["t0"], sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    ms = h.trigger_last_ms()
    ex0 = [pl.executing(s) for s in range(ts.N_SLOTS)]
    fn = hiplib.lib().dftpav_planner_check_yield
    fn.argtypes = YIELD_ARGTYPES
    out = hiplib.YieldOut(ts.N_SLOTS)
    for a in out.a.values():
        a[...] = 77
    ok = dict(t_now=sc["t0"], t0=sc["t0"], dt=sc["dt"], K=2, margin=0.5, range=60.0)
    bad = [dict(K=0), dict(K=-1), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN),
           dict(t_now=INF), dict(t_now=-INF), dict(t_now=NAN), dict(margin=-0.1), dict(margin=NAN), dict(margin=61.0), dict(range=INF),
           dict(range=NAN), dict(margin=INF), dict(margin=INF, range=INF)]
    for b in bad:
        a = dict(ok, **b)
        assert fn(pl._p, a["t_now"], a["t0"], a["dt"], a["K"], a["margin"], a["range"], C.byref(out.c)) == hiplib.E_INVALID, b
    assert fn(pl._p, ok["t_now"], ok["t0"], ok["dt"], 2, 0.5, 60.0, None) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values())
    assert h.trigger_last_ms() == ms                            # nothing ran
    # the trigger's own configuration: a refusal leaves it off, and the last rows stay refused
    st = hiplib.lib().dftpav_planner_set_conflict_trigger
    st.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int]
    for m, r, dt, K in ((NAN, 1.0, 0.1, 5), (0.5, 0.4, 0.1, 5), (0.5, INF, 0.1, 5), (0.5, NAN, 0.1, 5), (0.5, 1.0, 0.0, 5), (0.5, 1.0, NAN, 5),
                        (0.5, 1.0, 0.1, 0), (0.5, 1.0, 0.1, 4097), (INF, INF, 0.1, 5)):
        assert st(pl._p, m, r, dt, K) == hiplib.E_INVALID, (m, r, dt, K)
    lt = hiplib.lib().dftpav_planner_last_trigger
    lt.argtypes = [C.c_void_p, C.c_void_p]
    assert lt(pl._p, C.byref(out.c)) == hiplib.E_INVALID and all((a == 77).all() for a in out.a.values())
    # the debug hook
    dbg = hiplib.lib().dftpav_debug_conflict_trigger
    dbg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    poses, cy = np.zeros((2, 3, 4)), np.ones(3, dtype=np.int32)
    pp, cp = poses.ctypes.data_as(C.c_void_p), cy.ctypes.data_as(C.c_void_p)
    for args in ((None, 3, 2, pp, cp, 0.5, 1.0), (h._h, 0, 2, pp, cp, 0.5, 1.0), (h._h, 3, 0, pp, cp, 0.5, 1.0), (h._h, 3, 4097, pp, cp, 0.5, 1.0),
                 (h._h, 3, 2, None, cp, 0.5, 1.0), (h._h, 3, 2, pp, None, 0.5, 1.0), (h._h, 3, 2, pp, cp, -0.1, 1.0), (h._h, 3, 2, pp, cp, NAN, 1.0),
                 (h._h, 3, 2, pp, cp, 0.5, 0.4), (h._h, 3, 2, pp, cp, 0.5, INF)):
        assert dbg(*args, C.byref(out.c)) == hiplib.E_INVALID, args[1:3] + args[5:]
    assert all((a == 77).all() for a in out.a.values()) and h.trigger_last_ms() == ms
    ex1 = [pl.executing(s) for s in range(ts.N_SLOTS)]
    assert all(_exec_same(a, b) for a, b in zip(ex0, ex1))
    _same(pl.check_yield(sc["t0"], sc["t0"], sc["dt"], sc["K"], 0.5, 60.0), good)


# ---- tile edges: 130 slots are three tiles of the pair kernel (64 + 64 + 2), nine workgroups
N_EDGE, EDGE_T0, EDGE_DT, EDGE_K = 130, 0.0, 0.5, 21


def _edge_scene(generate):
    """seeded straight runs over a square of 400 m; slots 63 | 64 and 127 | 128 made neighbours in space (lanes 1.5 m apart: they
    overlap), and slots 0 and 129 partners (one following the other 4 m behind: they overlap)"""
    rng = np.random.default_rng(130)
    plans = cs.straight_plans(generate, rng, N_EDGE, 400.0, t_start=EDGE_T0)
    for a, b, y in ((63, 64, 1000.0), (127, 128, 1200.0)):
        plans[a] = cs._run(generate, (-10.0, y), (10.0, y), EDGE_T0)
        plans[b] = cs._run(generate, (-10.0, y + 1.5), (10.0, y + 1.5), EDGE_T0)
    plans[0] = cs._run(generate, (0.0, 1400.0), (20.0, 1400.0), EDGE_T0)
    plans[129] = cs._run(generate, (-4.0, 1400.0), (16.0, 1400.0), EDGE_T0)
    return dict(slots=plans)


@pytest.fixture(scope="module")
def edges(hiplib, oracle):
    sc = _edge_scene(oracle.minco_generate)
    h = hiplib.Handle()
    pl = hiplib.Planner(h, N_EDGE, 1)
    pad = rs.padded(sc, cs.MAX_SEG, cs.MAX_PIECES)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=EDGE_T0)
    tab, ends = _table(pl)
    poses = pc.poses(*tab, EDGE_T0, EDGE_DT, EDGE_K, order=2)
    yield dict(h=h, pl=pl, tab=tab, ends=ends, poses=poses)
    pl.close()
    h.close()


def _flags(name):
    f = np.ones(N_EDGE, dtype=np.int32)
    if name == "none":
        f[:] = 0
    elif name == "alternating":
        f[1::2] = 0
    elif name == "only_129_cannot":
        f[129] = 0
    return f


@pytest.mark.parametrize("flags", ["all", "none", "alternating", "only_129_cannot"])
def test_tile_edges_through_the_debug_hook(hiplib, edges, flags):
    h, P, f = edges["h"], edges["poses"], _flags(flags)
    for margin, rng in ((0.5, 20.0), (0.0, 0.0)):
        st = {}
        ref = pt.rows(P, f, margin, rng, stats=st)
        got = hiplib.debug_conflict_trigger(h, P, f, margin, rng)
        _same(got, ref)
        assert st["inside"] > 100 and 0 < st["narrow"] <= st["inside"]
        ms = h.trigger_last_ms()
        assert ms[0] == 0.0 and ms[1] > 0.0                     # no pose kernel
        assert got["yield_partner"][64] == 63 and got["yield_partner"][128] == 127 and got["yield_partner"][129] == 0
        if flags == "all":
            assert got["yield"][0] == 0 and got["yield_sample"][0] == -1 and got["yield"][129] == 1 and got["yield"][64] == 1 and got["yield"][63] == 0
        if flags == "none":
            assert got["yield"].sum() == 0 and got["yield_partner"][0] == 129 and got["yield_partner"][63] == 64
        if flags == "only_129_cannot":                          # slot 0 must yield to 129, across the whole table
            assert got["yield"][0] == 1 and got["yield_partner"][0] == 129 and got["yield_sample"][0] == 0 and got["yield"][129] == 0


def test_debug_hook_small_tables_and_empty_slots(hiplib, edges):
    h, P = edges["h"], edges["poses"]
    f = np.ones(N_EDGE, dtype=np.int32)
    Q = P.copy()
    Q[:, 1::2] = NAN                                            # every second slot emptied
    got = hiplib.debug_conflict_trigger(h, Q, f, 0.5, 20.0)
    _same(got, pt.rows(Q, f, 0.5, 20.0))
    assert _empty(got, np.arange(1, N_EDGE, 2)) and got["yield_partner"][64] == -1 and got["yield_partner"][128] != 127
    Q = np.full_like(P, NAN)                                    # a table that is all NaN
    assert _empty(hiplib.debug_conflict_trigger(h, Q, f, 0.5, 20.0)) and _empty(pt.rows(Q, f, 0.5, 20.0))
    for S, first in ((1, 63), (3, 62), (64, 1)):                # one slot; three (62, 63, 64: the overlapping pair); a whole tile
        sub, fs = np.ascontiguousarray(P[:, first:first + S]), np.ones(S, dtype=np.int32)
        for flags in (fs, 0 * fs):
            got = hiplib.debug_conflict_trigger(h, sub, flags, 0.5, 20.0)
            _same(got, pt.rows(sub, flags, 0.5, 20.0))
            assert got["yield"].shape == (S,)
        if S == 3:
            assert got["yield_partner"].tolist()[1:] == [2, 1]


def test_installed_plans_across_tiles(edges):
    pl = edges["pl"]
    for t_now in (EDGE_T0, EDGE_T0 + 10.5):                     # under way; every plan completed
        for margin, rng in ((0.5, 20.0), (0.0, 0.0)):
            got = pl.check_yield(t_now, EDGE_T0, EDGE_DT, EDGE_K, margin, rng)
            _same(got, _oracle(edges["tab"], edges["ends"], t_now, EDGE_T0, EDGE_DT, EDGE_K, margin, rng))
            assert got["yield"][129] == (1 if t_now == EDGE_T0 else 0) and got["yield_partner"][129] == 0
            assert got["yield_partner"][0] == (-1 if t_now == EDGE_T0 else 129)


def test_one_partial_tile(hiplib, oracle):
    """max_queries = 3: a single tile of which three lanes are slots"""
    h = hiplib.Handle()
    pl = hiplib.Planner(h, 3, 1)
    gen = oracle.minco_generate
    sc = dict(slots=[cs._run(gen, (-20.0, 0.0), (20.0, 0.0), 0.0), None, cs._run(gen, (0.0, -20.0), (0.0, 20.0), 0.0)])
    _install(pl, sc)
    tab, ends = _table(pl)
    for K in (1, 6, 101):
        for t_now in (0.0, 11.0):
            got = pl.check_yield(t_now, 0.0, 0.1, K, 0.3, 5.0)
            _same(got, _oracle(tab, ends, t_now, 0.0, 0.1, K, 0.3, 5.0))
    assert got["yield"].tolist() == [0, 0, 0] and got["yield_partner"].tolist() == [2, -1, 0]    # both completed: rows, no yield
    got = pl.check_yield(0.0, 0.0, 0.1, 101, 0.3, 5.0)
    assert got["yield"].tolist() == [0, 0, 1] and got["yield_partner"].tolist() == [-1, -1, 0]
    pl.close()
    h.close()


# ---- the tick
R = 2
SEED = 7
TRIGGER = dict(margin=0.4, range=2.0, dt=0.1, K=80)


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = SEED
    return pp


def _replan_table(scene, n):
    T = pr.Table(n)
    for s, p in enumerate(scene["slots"]):
        if p is None:
            continue
        T.install(s, p["singul"], p["piece_nums"], p["coeff_dt"], p["coeffs"], p["end_state"], p["t_start"])
        if p["hist"] is not None:
            T.set_history(s, *p["hist"])
    return T


def _same_tick(a, b):
    for k in CHECK_KEYS:
        assert np.array_equal(a["check"][k], b["check"][k]), k
    assert np.array_equal(a["query_slot"], b["query_slot"])
    assert set(a["plan"]) == set(b["plan"])
    for k in a["plan"]:
        assert np.array_equal(a["plan"][k], b["plan"][k], equal_nan=True), k


def test_tick_trigger_never_set_against_set_and_switched_off(hiplib, oracle):
    sc = rs.crafted(oracle.minco_generate)
    pp = _pp(hiplib)
    ticks, tables = [], []
    for mode in ("never", "off_again"):
        h = hiplib.Handle()
        h.set_grid_map(sc["grid"], sc["resolution"], sc["origin"])
        pl = hiplib.Planner(h, rs.N_SLOTS, R)
        if mode == "off_again":
            pl.set_conflict_trigger(**TRIGGER)
            pl.set_conflict_trigger(None)
        _install(pl, sc, pp.max_seg, pp.max_pieces)
        goals = np.array([p["end_state"] if p is not None else (-40.0, rs.LANES[0], 0.0, 0.0) for p in sc["slots"]])
        ticks.append(pl.tick(sc["t_now"], sc["budget"], end_states=goals, ego_states=sc["ego_states"], pp=pp))
        tables.append([pl.executing(s) for s in range(rs.N_SLOTS)])
        with pytest.raises(hiplib.DftpavError):
            pl.last_trigger()
        assert h.trigger_last_ms() == (0.0, 0.0)                # nothing of the trigger ran
        pl.close()
        h.close()
    _same_tick(ticks[0], ticks[1])
    assert ticks[0]["query_slot"].size >= 2
    assert all(_exec_same(a, b) for a, b in zip(*tables))


N_TICK = 6


def _tick_scene(generate):
    """the default arena, nothing dropped onto it.  Slots 0 and 1 head-on in lane 0, both 1 s into 12 s; slot 2 near its end with its
    goal 1 m aside (the check's own flag); slot 3 empty; slot 4 under way in lane 1 towards slot 5, whose plan ended 6 s ago"""
    grid, res, origin, _, _ = ss.arena()
    t_now = rs.T_NOW
    slots = [None] * N_TICK

    def put(s, plan, t_start):
        plan["t_start"], plan["hist"] = float(t_start), None
        slots[s] = plan

    y0, y1 = rs.LANES[0], rs.LANES[1]
    put(0, rs.plan_a(generate, 0), t_now - 1.0)
    put(1, rs._plan([rs._segment(generate, (-40.0, y0), (-64.0, y0), 6, 2.0, 1, 0.05, 0.05)]), t_now - 1.0)
    put(2, rs.plan_a(generate, 2, goal_offset=(0.0, 1.0)), t_now - 9.0)
    put(4, rs.plan_a(generate, 1), t_now - 1.0)
    put(5, rs._plan([rs._segment(generate, (-58.0, y1), (-50.0, y1), 4, 1.0, 1, 0.05, 0.05)]), t_now - 10.0)
    return dict(grid=grid, resolution=res, origin=origin, t_now=t_now, budget=rs.BUDGET, slots=slots)


def _oracle_tick(sc):
    """the oracle chain alone: the check's flags and start states, the trigger's rows at the adoption clock, the union"""
    chk = pr.replan_check(sc["grid"], sc["resolution"], sc["origin"], _replan_table(sc, N_TICK), sc["t_now"], sc["budget"], order=2)
    pad = rs.padded(sc, 8, 64)
    S = N_TICK
    n_seg, ts_ = np.zeros(S, np.int32), np.zeros(S)
    sg, pn, dt = np.zeros((S, 8), np.int32), np.zeros((S, 8), np.int32), np.zeros((S, 8))
    co = np.zeros((S, 8 * 64, 6, 2))
    for k, s in enumerate(pad["slots"]):
        n_seg[s], sg[s], pn[s], dt[s], co[s], ts_[s] = (pad[key][k] for key in ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "t_start"))
    trg = pt.check_yield(n_seg, sg, pn, dt, co, ts_, sc["t_now"], sc["t_now"] + sc["budget"], TRIGGER["dt"], TRIGGER["K"], TRIGGER["margin"],
                         TRIGGER["range"], order=2)
    union = np.flatnonzero((chk["replan"] != 0) | (trg["yield"] != 0))
    return chk, trg, union


@pytest.mark.parametrize("filtered", [False, True])
def test_tick_with_the_trigger(hiplib, oracle, filtered):
    sc = _tick_scene(oracle.minco_generate)
    chk, trg, union = _oracle_tick(sc)
    # before the device runs: the oracle flags exactly the intended slots
    assert np.flatnonzero(chk["replan"]).tolist() == [2] and np.flatnonzero(trg["yield"]).tolist() == [1, 4]
    assert trg["yield_partner"].tolist() == [-1, 0, -1, -1, 5, 4] and chk["complete"][5] == 1 and union.tolist() == [1, 2, 4]
    pp = _pp(hiplib)
    h = hiplib.Handle()
    h.set_grid_map(sc["grid"], sc["resolution"], sc["origin"])

    def planner():
        pl = hiplib.Planner(h, N_TICK, R)
        if filtered:
            pl.set_conflict_filter(0.5, 2.0, dt=0.1, K=80)
            pl.set_joint_selection(True)
        _install(pl, sc, pp.max_seg, pp.max_pieces)
        return pl

    pl = planner()
    pl.set_conflict_trigger(**TRIGGER)
    before = [pl.executing(s) for s in range(N_TICK)]
    tk = pl.tick(sc["t_now"], sc["budget"], pp=pp)
    for k in CHECK_KEYS:
        assert np.array_equal(tk["check"][k], chk[k]), k        # replan stays the check's own flag
    assert np.array_equal(tk["query_slot"], union)
    _same(pl.last_trigger(), trg)
    ms = h.trigger_last_ms()
    assert ms[0] > 0.0 and ms[1] > 0.0
    # the plans: a separate call with the oracle's start states and those own slots, on a planner of its own with the same table
    pl2 = planner()
    if filtered:
        pl2.set_own_slots(union)
    goals = np.array([sc["slots"][s]["end_state"] for s in union])
    sep = pl2.plan(chk["start_state"][union], goals, start_ctrl=chk["start_ctrl"][union], pp=pp, t_now=sc["t_now"] + sc["budget"])
    pl2.close()
    assert set(sep) == set(tk["plan"])
    for k in sep:
        assert np.array_equal(tk["plan"][k], sep[k], equal_nan=True), k
    new_ok = (sep["plan_status"] == hiplib.PLAN_OK) & (sep["winner"] >= 0)
    print("plan_status of the tick:", sep["plan_status"].tolist(), "trigger ms:", ms, "tick ms:", pl.replan_last_ms())
    stamp = sc["t_now"] + sc["budget"]
    for s in range(N_TICK):
        ex = pl.executing(s)
        k = np.flatnonzero(union == s)
        if k.size == 0 or not new_ok[k[0]]:
            assert _exec_same(ex, before[s]), s                 # not a query, or its planning failed: the old plan, byte for byte
            continue
        k = int(k[0])
        assert ex["n_seg"] == int(sep["n_seg"][k]) and np.array_equal(ex["coeffs"], sep["coeffs"][k]) and np.array_equal(ex["coeff_dt"], sep["coeff_dt"][k])
        assert ex["start_time"][0] == stamp and np.array_equal(ex["end_state"], sc["slots"][s]["end_state"])
        assert ex["have_hist"] == 1 and np.array_equal(ex["hist"], [stamp, chk["desired"][s, 3]])
    # a second identical tick on the restored table: the same bits, no new batch
    nb = pl.info()["n_batches"]
    pl.clear(np.arange(N_TICK))
    _install(pl, sc, pp.max_seg, pp.max_pieces)
    assert all(_exec_same(before[s], pl.executing(s)) for s in range(N_TICK))
    tk2 = pl.tick(sc["t_now"], sc["budget"], pp=pp)
    _same_tick(tk, tk2)
    _same(pl.last_trigger(), trg)
    assert pl.info()["n_batches"] == nb
    pl.close()
    h.close()


def test_a_larger_K_after_a_smaller_one(hiplib, oracle):
    """the trigger set for K = 4, a tick, then set for K = 40: the allocation is made again for the larger K, the rows of the last tick
    went with the old one, and the next tick's rows are the read-out's (and the oracle's) on the table that tick finds"""
    sc = _tick_scene(oracle.minco_generate)
    pp = _pp(hiplib)
    t_now, t0 = sc["t_now"], sc["t_now"] + sc["budget"]
    h = hiplib.Handle()
    h.set_grid_map(sc["grid"], sc["resolution"], sc["origin"])
    pl = hiplib.Planner(h, N_TICK, R)
    _install(pl, sc, pp.max_seg, pp.max_pieces)
    rows = []
    for K in (4, 40):
        pl.set_conflict_trigger(**dict(TRIGGER, K=K))
        if rows:
            with pytest.raises(hiplib.DftpavError) as e:
                pl.last_trigger()                               # until the next tick
            assert e.value.code == hiplib.E_INVALID
        clocks = (t_now, t0, TRIGGER["dt"], K, TRIGGER["margin"], TRIGGER["range"])
        want = pl.check_yield(*clocks)                          # the read-out writes nothing: the table is the one the tick finds
        _same(want, _oracle(*_table(pl), *clocks))
        pl.tick(t_now, sc["budget"], pp=pp)
        rows.append(pl.last_trigger())
        _same(rows[-1], want)
    assert _empty(rows[0])                                      # nothing within four clocks; the rows of K = 40 lie beyond them
    assert rows[1]["yield"].any() and (rows[1]["yield_sample"][rows[1]["yield"] != 0] >= 4).all()
    pl.close()
    h.close()
