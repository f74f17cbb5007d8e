"""Candidate plans against the executing table on the device (cand_conflict.hip): the candidates' poses and all five rows bit-equal
to oracle_conflict/candidate_oracle.cpp in order 2 and to the install construction on the device itself, across tile edges, with own
slots; the conflict filter of dftpav_plan_queries against the chain of CPU oracles of tests/limits_cases.py; own slots through
dftpav_replan_tick."""
import ctypes as C
import itertools

import numpy as np
import pytest

import limits_cases as lc
from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import LayoutSpec
from oracle_conflict import pycandidate as pcand
from oracle_conflict import pyconflict as pc

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
EXEC_KEYS = ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "duration", "start_time", "end_time", "end_state", "hist", "have_hist")


def _install(pl, scene):
    pad = rs.padded(scene, cs.MAX_SEG, cs.MAX_PIECES)
    for k in range(len(pad["slots"])):
        sl = slice(k, k + 1)
        pl.install(pad["slots"][sl], pad["n_seg"][sl], pad["singul"][sl], pad["piece_nums"][sl], pad["coeff_dt"][sl], pad["coeffs"][sl],
                   pad["end_states"][sl], t_start=pad["t_start"][k])


def _install_plan(pl, s, plan, t_start):
    _install(pl, dict(slots=[None] * s + [dict(plan, t_start=t_start)]))


def _table(pl):
    return pc.from_executing([pl.executing(s) for s in range(pl.max_queries)])


def _same(got, ref, ig=slice(None), ir=slice(None)):
    for k in pc.FIELDS:
        a, b = np.asarray(got[k][ig]), np.asarray(ref[k][ir])
        same = np.array_equal(a.view(np.int64), b.view(np.int64)) if k == "min_sep" else np.array_equal(a, b)
        assert same, (k, a, b)


def _empty(r, idx=slice(None)):
    return np.isposinf(r["min_sep"][idx]).all() and all((r[k][idx] == -1).all() for k in pc.FIELDS[1:])


def _moved(plan, dx, dy):
    return dict(plan, coeffs=plan["coeffs"] + np.array([dx, dy]) * (np.arange(6) == 0)[None, :, None])


def _batch_of(hiplib, h, plans):
    """plans of one layout as a batch with their coefficients set; -> (batch, the oracle's batch arguments)"""
    lay = LayoutSpec([int(v) for v in plans[0]["piece_nums"]], [int(v) for v in plans[0]["singul"]], 4)
    co, dt = np.stack([p["coeffs"] for p in plans]), np.stack([p["coeff_dt"] for p in plans])
    bt = hiplib.Batch(h, lay, len(plans))
    bt.set_coeffs(co, dt)
    return bt, (plans[0]["singul"], plans[0]["piece_nums"], dt, co)


@pytest.fixture(scope="module")
def crafted(hiplib, oracle):
    sc = cs.crafted(oracle.minco_generate)
    h = hiplib.Handle()
    pl = hiplib.Planner(h, cs.N_SLOTS, 1)
    occupied = [p for p in sc["slots"] if p is not None]
    shift = next(p for p in occupied if len(p["piece_nums"]) == 2)       # forward, then back: two segments, the second reverse
    # the gear-shift plan where it is (on its own old plan), one group up (beside the held vehicles), and on the crossing
    two = [shift, _moved(shift, 3.0, cs.GROUP + 1.0), _moved(shift, 8.0, -5 * cs.GROUP + 2.0)]
    one = [p for p in occupied if len(p["piece_nums"]) == 1 and p["piece_nums"][0] == 5]     # every straight run of five pieces
    assert shift["singul"][1] == -1 and len(one) >= 10
    b2, a2 = _batch_of(hiplib, h, two)
    b1, a1 = _batch_of(hiplib, h, one)
    fresh = b1.check_conflicts(pl, 48.0, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)      # never filled
    _install(pl, sc)
    yield dict(sc=sc, h=h, pl=pl, tab=_table(pl), fresh=fresh, batches=((b2, a2), (b1, a1)), one=one, shift=shift)
    b1.close()
    b2.close()
    pl.close()
    h.close()


# t_start = 52.5 with t0 = 50: held before the start for 25 clocks; the runs of 10 s end at 62.5, the clocks of K = 257 run to 75.6
T_START = 52.5


@pytest.mark.parametrize("K", [1, 2, 3, 7, 257])
def test_poses_and_rows_equal_the_oracle(crafted, K):
    sc, pl = crafted["sc"], crafted["pl"]
    dt = 0.1 if K == 257 else 1.5                                # 7 clocks of 1.5 s: 50 .. 59; both holds occur from K = 3 on / at 257
    for bt, args in crafted["batches"]:
        got = bt.sample_poses(T_START, sc["t0"], dt, K)
        ref = pcand.poses(*args, T_START, sc["t0"], dt, K, order=2)
        assert got.shape == ref.shape == (K, bt.B, 4) and np.isfinite(got).all()
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), np.argwhere(got.view(np.int64) != ref.view(np.int64))[:8]
        assert (got[0] == got[min(1, K - 1)]).all()              # held still before t_start
        if K == 257:
            assert (got[-1] == got[-20]).all() and not (got[-1] == got[100]).all()      # held still after the end
        assert crafted["h"].batch_conflicts_last_ms()[0] > 0.0 and crafted["h"].batch_conflicts_last_ms()[1] == 0.0
        for case in sc["cases"]:
            rows = bt.check_conflicts(pl, T_START, sc["t0"], dt, K, *case)
            _same(rows, pcand.conflicts(*args, T_START, crafted["tab"], sc["t0"], dt, K, *case, order=2))
        ms = crafted["h"].batch_conflicts_last_ms()
        assert ms[0] > 0.0 and ms[1] > 0.0


def test_rows_on_the_scene_clocks(crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    clocks = (sc["t0"], sc["dt"], sc["K"])
    hits = 0
    for bt, args in crafted["batches"]:
        for case in sc["cases"]:
            for t_start in (sc["t0"], T_START):
                got = bt.check_conflicts(pl, t_start, *clocks, *case)
                _same(got, pcand.conflicts(*args, t_start, crafted["tab"], *clocks, *case, order=2))
                hits += int((got["conflict_sample"] >= 0).sum())
                if case == sc["cases"][0]:                       # range None is margin
                    _same(bt.check_conflicts(pl, t_start, *clocks, case[0]), got)
    assert hits > 20
    assert _empty(crafted["fresh"]) and crafted["fresh"]["min_sep"].shape == (len(crafted["one"]),)


def test_install_construction_on_the_device(hiplib, crafted):
    """a candidate's poses and row are those of the slot it is installed in: a free slot (3) and a replaced one (its own old slot)"""
    sc, h = crafted["sc"], crafted["h"]
    clocks = (sc["t0"], sc["dt"], sc["K"])
    pl = hiplib.Planner(h, cs.N_SLOTS, 1)
    _install(pl, sc)
    for (bt, _), plans in zip(crafted["batches"], ([crafted["shift"]], crafted["one"][:3])):
        poses = bt.sample_poses(T_START, *clocks)
        for c, plan in enumerate(plans):
            src = next(s for s, p in enumerate(sc["slots"]) if p is plan)
            for s in (3, src):
                own = np.full(bt.B, -1, np.int32)
                own[c] = s
                row = bt.check_conflicts(pl, T_START, *clocks, 0.5, 60.0, own=own)
                before = pl.executing(s)
                _install_plan(pl, s, plan, T_START)
                slot_poses = pl.sample_poses(*clocks)[:, s]
                assert np.array_equal(poses[:, c].view(np.int64), slot_poses.view(np.int64)), (c, s)
                _same(row, pl.check_conflicts(*clocks, 0.5, 60.0), slice(c, c + 1), slice(s, s + 1))
                pl.clear([s])                                    # the table as it was
                if before["n_seg"]:
                    pl.install([s], [before["n_seg"]], before["singul"][None], before["piece_nums"][None], before["coeff_dt"][None],
                               before["coeffs"][None], before["end_state"][None], t_start=before["start_time"][0])
    pl.close()


def test_nothing_is_written(crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    S = cs.N_SLOTS
    grid = np.zeros((40, 120), dtype=np.uint8)
    grid[20:22, 70:72] = 80
    crafted["h"].set_grid_map(grid, 0.5, (-30.0, cs.GROUP - 10.0))
    bt, _ = crafted["batches"][0]

    def state():
        return [pl.executing(s) for s in range(S)], [pl.publisher_state(s) for s in range(S)], pl.check(sc["t0"] + 1.0)

    ex0, pub0, chk0 = state()
    co0 = bt.sample_poses(T_START, sc["t0"], sc["dt"], 3)
    bt.check_conflicts(pl, T_START, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0, own=np.zeros(bt.B, np.int32))
    bt.sample_poses(T_START, sc["t0"], sc["dt"], sc["K"])
    ex1, pub1, chk1 = state()
    for a, b in zip(ex0, ex1):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in EXEC_KEYS)
    for a, b in zip(pub0, pub1):
        assert a["exe_index"] == b["exe_index"] and a["have_hist"] == b["have_hist"] and a["hist"].tobytes() == b["hist"].tobytes()
    assert chk0["occupied"].sum() == 24
    assert set(chk0) == set(chk1) and all(np.asarray(chk0[k]).tobytes() == np.asarray(chk1[k]).tobytes() for k in chk0)
    assert bt.sample_poses(T_START, sc["t0"], sc["dt"], 3).tobytes() == co0.tobytes()        # the batch neither


CHECK_ARGS = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]


def test_null_output_pointers(hiplib, crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    bt, _ = crafted["batches"][1]
    full = bt.check_conflicts(pl, T_START, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    fn = hiplib.lib().dftpav_batch_check_conflicts
    fn.argtypes = CHECK_ARGS
    n = 0
    for keep in itertools.product((False, True), repeat=5):
        if not any(keep):
            continue
        out = hiplib.ConflictOut(bt.B)
        for a in out.a.values():
            a[...] = 77
        for k, on in zip(pc.FIELDS, keep):
            if not on:
                setattr(out.c, k, None)
        assert fn(bt._b, pl._p, T_START, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0, None, C.byref(out.c)) == hiplib.OK
        for k, on in zip(pc.FIELDS, keep):
            assert np.array_equal(out.a[k], full[k]) if on else (out.a[k] == 77).all(), (keep, k)
        n += 1
    assert n == 31


def test_refusals_change_nothing(hiplib, crafted):
    sc, pl, h = crafted["sc"], crafted["pl"], crafted["h"]
    bt, _ = crafted["batches"][1]
    good = bt.check_conflicts(pl, T_START, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    ms = h.batch_conflicts_last_ms()
    fn, fp = hiplib.lib().dftpav_batch_check_conflicts, hiplib.lib().dftpav_batch_sample_poses
    fn.argtypes = CHECK_ARGS
    fp.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    out = hiplib.ConflictOut(bt.B)
    for a in out.a.values():
        a[...] = 77
    poses = np.full((2, bt.B, 4), 77.0)
    own = np.full(bt.B, -1, np.int32)
    ok = dict(b=bt._b, p=pl._p, t_start=T_START, t0=sc["t0"], dt=sc["dt"], K=2, margin=0.5, range=60.0, own=own)
    h2 = hiplib.Handle()
    other = hiplib.Planner(h2, 3, 1)                            # a planner on another handle
    unsolved = hiplib.Batch(h, LayoutSpec([5], [1], 4), 2)      # no coefficients
    bad = [dict(K=0), dict(K=-1), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN),
           dict(t_start=INF), dict(t_start=NAN), dict(margin=NAN), dict(margin=61.0), dict(range=INF), dict(range=NAN), dict(margin=INF),
           dict(margin=INF, range=INF), dict(b=None), dict(p=None), dict(p=other._p), dict(b=unsolved._b),
           dict(own=np.full(bt.B, cs.N_SLOTS, np.int32)), dict(own=np.full(bt.B, -2, np.int32))]
    for b in bad:
        a = dict(ok, **b)
        assert fn(a["b"], a["p"], a["t_start"], a["t0"], a["dt"], a["K"], a["margin"], a["range"], a["own"].ctypes.data_as(C.c_void_p),
                  C.byref(out.c)) == hiplib.E_INVALID, b
        if not set(b) & {"margin", "range", "own", "p"}:
            assert fp(a["b"], a["t_start"], a["t0"], a["dt"], a["K"], poses.ctypes.data_as(C.c_void_p)) == hiplib.E_INVALID, b
    assert fn(bt._b, pl._p, T_START, sc["t0"], sc["dt"], 2, 0.5, 60.0, None, None) == hiplib.E_INVALID
    assert fp(bt._b, T_START, sc["t0"], sc["dt"], 2, None) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and (poses == 77.0).all()
    assert h.batch_conflicts_last_ms() == ms                    # nothing ran
    for bad_filter in ((NAN, 1.0, 0.1, 10), (0.5, 0.4, 0.1, 10), (0.5, INF, 0.1, 10), (0.5, 1.0, 0.0, 10), (0.5, 1.0, NAN, 10), (0.5, 1.0, 0.1, 0),
                       (0.5, 1.0, 0.1, 4097)):
        with pytest.raises(hiplib.DftpavError) as e:
            pl.set_conflict_filter(*bad_filter)
        assert e.value.code == hiplib.E_INVALID
    for bad_own in ([cs.N_SLOTS], [-2], [0] * (cs.N_SLOTS + 1)):
        with pytest.raises(hiplib.DftpavError):
            pl.set_own_slots(bad_own)
    with pytest.raises(hiplib.DftpavError):
        pl.last_conflicts(1)                                    # no call ran with the filter
    _same(bt.check_conflicts(pl, T_START, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0), good)
    assert bt.check_conflicts(pl, T_START, sc["t0"], sc["dt"], sc["K"], -1.0, 60.0)["conflict_sample"].max() == -1   # a negative margin is legal
    unsolved.close()
    other.close()
    h2.close()


# ---- tile edges: 130 slots are three J-tiles (64 + 64 + 2); 130 candidates three workgroups
N_EDGE, EDGE_T0, EDGE_DT, EDGE_K = 130, 0.0, 0.5, 21


def _edge_plans(generate, seed):
    rng = np.random.default_rng(seed)
    plans = cs.straight_plans(generate, rng, N_EDGE, 400.0, t_start=EDGE_T0)
    for p in plans:
        p["t_start"] = EDGE_T0
    return plans


@pytest.fixture(scope="module")
def edges(hiplib, oracle):
    gen = oracle.minco_generate
    slots = _edge_plans(gen, 130)
    cands = _edge_plans(gen, 131)
    run = lambda p0, p1: cs._run(gen, p0, p1, EDGE_T0, n_pieces=4)
    # slots 0 and 129 far from the rest, 40 m apart; candidate 0 runs beside slot 0 (nearer) and in range of slot 129, candidate 129
    # the other way round
    slots[0] = run((0.0, 1400.0), (20.0, 1400.0))
    slots[129] = run((0.0, 1406.5), (20.0, 1406.5))
    cands[0] = run((0.0, 1402.8), (20.0, 1402.8))
    cands[129] = run((0.0, 1403.6), (20.0, 1403.6))
    # candidates 63 | 64 and 127 | 128 beside slots 63 | 64 and 127 | 128
    for a, y in ((63, 1000.0), (127, 1200.0)):
        slots[a], slots[a + 1] = run((-10.0, y), (10.0, y)), run((-10.0, y + 6.0), (10.0, y + 6.0))
        cands[a], cands[a + 1] = run((-10.0, y + 2.8), (10.0, y + 2.8)), run((-10.0, y + 3.3), (10.0, y + 3.3))
    h = hiplib.Handle()
    pl = hiplib.Planner(h, N_EDGE, 1)
    pad = rs.padded(dict(slots=slots), cs.MAX_SEG, cs.MAX_PIECES)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=EDGE_T0)
    bt, args = _batch_of(hiplib, h, cands)
    yield dict(h=h, pl=pl, bt=bt, args=args, cands=cands)
    bt.close()
    pl.close()
    h.close()


def _edge_case(hiplib, edges, cleared):
    pl, bt, args = edges["pl"], edges["bt"], edges["args"]
    tab = _table(pl)
    clocks = (EDGE_T0, EDGE_DT, EDGE_K)
    none = bt.check_conflicts(pl, EDGE_T0, *clocks, 0.5, 20.0)
    _same(none, pcand.conflicts(*args, EDGE_T0, tab, *clocks, 0.5, 20.0, order=2))
    _same(bt.check_conflicts(pl, EDGE_T0, *clocks, 0.0, 0.0), pcand.conflicts(*args, EDGE_T0, tab, *clocks, 0.0, 0.0, order=2))
    if not cleared:
        assert none["sep_partner"][0] == 0 and none["sep_partner"][129] == 129 and none["sep_partner"][63] == 63 and none["sep_partner"][64] == 64
        assert none["sep_partner"][127] == 127 and none["sep_partner"][128] == 128
    else:
        assert none["sep_partner"][129] == 0 and none["sep_partner"][63] == 64 and none["sep_partner"][127] == 128
    # own: the slot that would otherwise be the nearest partner, and one that would not
    own = np.full(N_EDGE, -1, np.int32)
    own[[0, 129, 63, 64, 127, 128]] = [0, 0, 63, 63, 128, 128]
    got = bt.check_conflicts(pl, EDGE_T0, *clocks, 0.5, 20.0, own=own)
    _same(got, pcand.conflicts(*args, EDGE_T0, tab, *clocks, 0.5, 20.0, own=own, order=2))
    assert got["sep_partner"][63] == 64
    if not cleared:
        assert got["sep_partner"][0] == 129 and got["sep_partner"][128] == 127
    else:                                                       # slots 129 and 127 are gone, 0 and 128 are their own
        assert _empty(got, [0, 128])
    assert got["sep_partner"][129] == 129 if not cleared else _empty(got, [129])
    # a batch of 1 and of 3 candidates
    for n in (1, 3):
        b, a = _batch_of(hiplib, edges["h"], edges["cands"][127:127 + n])
        _same(b.check_conflicts(pl, EDGE_T0, *clocks, 0.5, 20.0, own=own[127:127 + n]),
              pcand.conflicts(*a, EDGE_T0, tab, *clocks, 0.5, 20.0, own=own[127:127 + n], order=2))
        b.close()


def test_tile_edges(hiplib, edges):
    _edge_case(hiplib, edges, cleared=False)


def test_tile_edges_with_every_second_slot_cleared(hiplib, edges):
    """(runs after test_tile_edges: it changes the module's table)"""
    edges["pl"].clear(np.arange(1, N_EDGE, 2))
    _edge_case(hiplib, edges, cleared=True)
    edges["pl"].clear(np.arange(0, N_EDGE, 2))                  # an all-empty table
    assert _empty(edges["bt"].check_conflicts(edges["pl"], EDGE_T0, EDGE_T0, EDGE_DT, EDGE_K, 0.5, 20.0))


def test_one_partial_tile(hiplib, oracle):
    """max_queries = 3: a single J-tile of which three lanes are slots"""
    gen = oracle.minco_generate
    h = hiplib.Handle()
    pl = hiplib.Planner(h, 3, 1)
    _install(pl, dict(slots=[cs._run(gen, (-20.0, 0.0), (20.0, 0.0), 0.0), None, cs._run(gen, (0.0, -20.0), (0.0, 20.0), 0.0)]))
    bt, args = _batch_of(hiplib, h, [cs._run(gen, (-20.0, 2.5), (20.0, 2.5), 0.0), cs._run(gen, (20.0, -30.0), (-20.0, -30.0), 0.0)])
    for K in (1, 6, 101):
        for own in (None, [0, 2], [2, -1]):
            _same(bt.check_conflicts(pl, 0.0, 0.0, 0.1, K, 0.3, 5.0, own=own), pcand.conflicts(*args, 0.0, _table(pl), 0.0, 0.1, K, 0.3, 5.0, own=own, order=2))
    got = bt.check_conflicts(pl, 0.0, 0.0, 0.1, 101, 0.3, 5.0)
    assert got["min_sep"][0] == 0.0 and got["sep_partner"][0] == 2 and got["conflict_partner"][0] == 2 and _empty(got, [1])
    bt.close()
    pl.close()
    h.close()


# ---- the filter, on the fourteen arena queries of tests/limits_cases.py
F_DT, F_K, F_RANGE = 0.25, 48, 2.0
# A vehicle parked beside the first metres of the path of query 0, heading 0.  The oracle's min_sep of that query's four restarts is
# 0.375, 0.422, 0.424, 0.120 m: restart 0 wins unfiltered; a margin of 0.40 m lies between it and restarts 1 and 2, and 1.0 m above all
# four.  The test asserts these properties from the oracle rows.
BLOCKER, FAR_AWAY = (-55.0, 35.6), (5000.0, 5000.0)
M_1, M_2 = 0.40, 1.0
BLOCK_SLOT, FAR_SLOT = 13, 5


def _pp(hiplib):
    pp = hiplib.default_plan_params()
    pp.seed = lc.SEED
    return pp


@pytest.fixture(scope="module")
def arena(hiplib, oracle):
    grid, res, org, S, E = lc.chain()["scene"]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl0 = hiplib.Planner(h, len(E), lc.R)
    plain = pl0.plan(S, E, pp=_pp(hiplib))
    yield dict(h=h, S=S, E=E, Q=len(E), plain=plain, pl0=pl0, n_batches=pl0.info()["n_batches"], gen=oracle.minco_generate)
    pl0.close()
    h.close()


def _park(arena, pl, slot, where):
    _install_plan(pl, slot, cs._held(arena["gen"], where, 0.0, -15.0), -18.0)


def _chain_rows(tab, margin, own=None):
    """the candidate oracle (order 2) on every restart of the chain, t_start = t0 = 0: dict of [Q][R] rows"""
    ch = lc.chain()
    Q = len(ch["per"])
    out = dict(min_sep=np.full((Q, lc.R), INF), **{k: np.full((Q, lc.R), -1, np.int32) for k in pc.FIELDS[1:]})
    for q, e in enumerate(ch["per"]):
        if e is not None:
            r = pcand.conflicts(e["layout"].singuls, e["layout"].piece_nums, e["dts"], e["coeffs"], 0.0, tab, 0.0, F_DT, F_K, margin, F_RANGE,
                                own=None if own is None else [own[q]] * lc.R, order=2)
            for k in pc.FIELDS:
                out[k][q] = r[k]
    return out


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _wins(ref, extra=None):
    ch = lc.chain()
    w = {}
    for q, c in enumerate(ch["per"]):
        if c is None:
            continue
        rej = (ref["conflict_sample"][q] >= 0).astype(np.int32) | (0 if extra is None else extra[q])
        r = c["solve"]
        w[q] = (lc.select(r["final_cost"], r["success"], c["collision"]), lc.select(r["final_cost"], r["success"], c["collision"] | rej))
    return w


def _filter_case(hiplib, arena, pl, margin, wins, ref):
    ch, plain, Q = lc.chain(), arena["plain"], arena["Q"]
    pl.set_conflict_filter(margin, F_RANGE, F_DT, F_K)
    out = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    last = pl.last_conflicts(Q)
    for q, c in enumerate(ch["per"]):
        if c is None or out["plan_status"][q] == hiplib.PLAN_LAYOUT_UNSUPPORTED:
            assert out["winner"][q] == -1 and _empty(last, q), q
            continue
        _same(last, ref, q, q)
        w0, w1 = wins[q]
        print(q, "margin", margin, "winner", w0, "->", w1, "device", plain["winner"][q], "->", out["winner"][q], "min_sep", last["min_sep"][q].tolist())
        assert plain["winner"][q] == w0 and out["winner"][q] == w1, q
        assert out["plan_status"][q] == (hiplib.PLAN_OK if w1 >= 0 else hiplib.PLAN_NO_VALID_RESTART), q
        for k in ("r_final_cost", "r_status", "r_success", "r_iters", "r_evals", "r_collision", "r_first_sample"):
            assert np.array_equal(out[k][q], plain[k][q]), (q, k)
        if w1 >= 0:
            assert out["final_cost"][q] == c["solve"]["final_cost"][w1] and np.array_equal(out["coeffs"][q, :c["layout"].n_pieces], c["coeffs"][w1]), q
        else:
            assert not out["coeffs"][q].any(), q
    return out, last


def test_filter_off_is_a_planner_without_one(hiplib, arena):
    pl = hiplib.Planner(arena["h"], arena["Q"], lc.R)
    _park(arena, pl, BLOCK_SLOT, BLOCKER)
    pl.set_conflict_filter(None)                                # off before it was ever on
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    pl.set_conflict_filter(M_2, F_RANGE, F_DT, F_K)
    pl.set_conflict_filter(-1.0)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    assert pl.info()["n_batches"] == arena["n_batches"]
    for planner in (pl, arena["pl0"]):
        with pytest.raises(hiplib.DftpavError) as e:
            planner.last_conflicts(arena["Q"])                  # that call ran without the filter
        assert e.value.code == hiplib.E_INVALID
    pl.close()


def test_filter_on(hiplib, arena):
    ch, Q = lc.chain(), arena["Q"]
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    # a table never filled: nothing is rejected, every row empty
    pl.set_conflict_filter(M_2, F_RANGE, F_DT, F_K)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    assert _empty(pl.last_conflicts(Q))
    # (c) a vehicle parked far from every path changes nothing
    _park(arena, pl, FAR_SLOT, FAR_AWAY)
    ref_far = _chain_rows(_table(pl), M_2)
    assert _empty(ref_far) and all(w0 == w1 for w0, w1 in _wins(ref_far).values())
    out_far, _ = _filter_case(hiplib, arena, pl, M_2, _wins(ref_far), ref_far)
    _same_outputs(out_far, arena["plain"])
    # (a) the blocker with the smaller margin: a winner moves to a dearer restart
    _park(arena, pl, BLOCK_SLOT, BLOCKER)
    tab = _table(pl)
    ref1, ref2 = _chain_rows(tab, M_1), _chain_rows(tab, M_2)
    wins1, wins2 = _wins(ref1), _wins(ref2)
    moved = [q for q, (w0, w1) in wins1.items() if w1 >= 0 and w1 != w0]
    none = [q for q, (w0, w1) in wins2.items() if w0 >= 0 and w1 == -1]
    assert moved and none, (wins1, wins2)                       # (a) and (b), from the oracle rows alone
    for q in moved:
        r = ch["per"][q]["solve"]
        assert r["final_cost"][wins1[q][1]] > r["final_cost"][wins1[q][0]] and ref1["min_sep"][q, wins1[q][1]] > M_1 >= ref1["min_sep"][q, wins1[q][0]]
    out1, last1 = _filter_case(hiplib, arena, pl, M_1, wins1, ref1)
    # rows do not leak between calls: the same call again, then (b) the larger margin, then the first again
    out1b, last1b = _filter_case(hiplib, arena, pl, M_1, wins1, ref1)
    _same_outputs(out1b, out1)
    out2, _ = _filter_case(hiplib, arena, pl, M_2, wins2, ref2)
    assert all(out2["plan_status"][q] == hiplib.PLAN_NO_VALID_RESTART for q in none)
    _same_outputs(_filter_case(hiplib, arena, pl, M_1, wins1, ref1)[0], out1)
    # a call of fewer queries: the rows are those of its own queries
    pl.set_conflict_filter(M_1, F_RANGE, F_DT, F_K)
    sub = pl.plan(arena["S"][:2], arena["E"][:2], pp=_pp(hiplib))
    assert np.array_equal(sub["winner"], out1["winner"][:2])
    _same(pl.last_conflicts(2), ref1, slice(0, 2), slice(0, 2))
    # own slots: used by one call and gone on the next.  Every query owning the blocker's slot sees the far vehicle alone
    pl.set_own_slots([BLOCK_SLOT] * Q)
    owned = pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    _same_outputs(owned, arena["plain"])
    assert _empty(pl.last_conflicts(Q))
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), out1)
    pl.set_own_slots([BLOCK_SLOT] * 3)                          # for another number of queries: refused, and consumed
    with pytest.raises(hiplib.DftpavError):
        pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), out1)
    # a refused change of the filter leaves it as it is
    with pytest.raises(hiplib.DftpavError):
        pl.set_conflict_filter(NAN, F_RANGE, F_DT, F_K)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), out1)
    pl.set_conflict_filter(None)
    _same_outputs(pl.plan(arena["S"], arena["E"], pp=_pp(hiplib)), arena["plain"])
    pl.close()


def test_composition_with_the_limit_filter(hiplib, arena):
    """both filters on: the winners equal the rule over the OR of the two oracle flags"""
    Q = arena["Q"]
    lim = hiplib.default_limits()
    lim.max_forward_vel, lim.max_backward_vel, lim.max_forward_cur, lim.max_backward_cur = 5.01, 2.01, 1.01, 1.01   # tests/test_gpu_limits.py: FILTER
    lim_rej = 1 - lc.chain_limits(lim)["feasible"]
    pl = hiplib.Planner(arena["h"], Q, lc.R)
    _park(arena, pl, BLOCK_SLOT, BLOCKER)
    ref = _chain_rows(_table(pl), M_1)
    both, alone = _wins(ref, lim_rej), _wins(ref)
    pl.set_limit_filter(lim, lc.CHECK_DT)
    _filter_case(hiplib, arena, pl, M_1, both, ref)
    assert np.array_equal(pl.last_limits(Q)["feasible"], 1 - lim_rej)
    pl.set_limit_filter(None)
    _filter_case(hiplib, arena, pl, M_1, alone, ref)
    print("both", both, "alone", alone)
    pl.close()


def test_a_larger_K_after_a_smaller_one(hiplib, arena):
    """the filter set for K = 4, a call, then set for K = F_K: the poses are allocated again for the larger K, and the rows of the next
    call are the oracle's at F_K, bit for bit"""
    pl = hiplib.Planner(arena["h"], arena["Q"], lc.R)
    _park(arena, pl, BLOCK_SLOT, BLOCKER)
    ref = _chain_rows(_table(pl), M_1)
    assert (ref["conflict_sample"] >= 4).any() and (ref["sep_sample"] >= 4).any()     # clocks that the first allocation has no poses for
    pl.set_conflict_filter(M_1, F_RANGE, F_DT, 4)
    pl.plan(arena["S"], arena["E"], pp=_pp(hiplib))
    small = pl.last_conflicts(arena["Q"])
    assert (small["sep_sample"] < 4).all() and (small["conflict_sample"] < 4).all()
    _filter_case(hiplib, arena, pl, M_1, _wins(ref), ref)       # (sets F_K)
    pl.close()


def test_own_slots_through_the_tick(hiplib, oracle):
    """one adopted plan with an obstacle dropped on it replans in a tick with the filter on: its own old plan does not reject it; a
    vehicle parked on the start of its new path does, and it keeps its plan; plan_out is a separate call's with set_own_slots"""
    grid, res, org, S, E = ss.arena_plan_queries()
    Q, R = len(E), 2
    pp = hiplib.default_plan_params()
    pp.seed = 7
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    pl = hiplib.Planner(h, Q, R)
    out = pl.plan(S, E, pp=pp)
    ok = np.flatnonzero((out["plan_status"] == hiplib.PLAN_OK) & (out["winner"] >= 0))
    xs, ys = org[0] + np.arange(grid.shape[1]) * res, org[1] + np.arange(grid.shape[0]) * res
    pl.set_conflict_filter(0.3, 2.0, 0.25, 48)
    pl2 = hiplib.Planner(h, Q, R)
    pl2.set_conflict_filter(0.3, 2.0, 0.25, 48)
    budget, found = 0.5, False
    # the scene: the first adopted plan that, with an obstacle dropped two thirds down its path, is flagged by the check and replans
    # well from its desired state (the separate call below: a planner with the same table and filter, the query's own slot set)
    for a in (int(q) for q in ok):
        pl.clear(np.arange(Q))
        pl2.clear(np.arange(Q))
        h.set_grid_map(grid, res, org)
        pl.plan(S, E, pp=pp)
        pl.adopt([a], [a], t_start=0.0, pp=pp)
        mine = pl.executing(a)
        na = int(out["piece_nums"][a, :out["n_seg"][a]].sum())
        t_now = 0.2 * float(mine["end_time"][mine["n_seg"] - 1])
        after = grid.copy()
        mid = out["coeffs"][a, (2 * na) // 3, 0]                # where a piece two thirds down the plan starts
        after[np.ix_((ys >= mid[1] - 0.4) & (ys <= mid[1] + 0.4), (xs >= mid[0] - 0.4) & (xs <= mid[0] + 0.4))] = 80
        h.set_grid_map(after, res, org)
        chk = pl.check(t_now, budget)
        if chk["replan"][a] != 1:
            continue
        pl2.install([a], [mine["n_seg"]], mine["singul"][None], mine["piece_nums"][None], mine["coeff_dt"][None], mine["coeffs"][None],
                    mine["end_state"][None], t_start=0.0)
        pl2.set_own_slots([a])
        sep = pl2.plan(chk["start_state"][[a]], E[[a]], start_ctrl=chk["start_ctrl"][[a]], pp=pp, t_now=t_now + budget)
        print("slot", a, "replans with status", sep["plan_status"].tolist())
        if sep["plan_status"][0] == hiplib.PLAN_OK:
            found = True
            break
    assert found and chk["replan"].sum() == 1
    assert _empty(pl2.last_conflicts(1))                        # nothing but its own old plan is there
    not_own = pl2.plan(chk["start_state"][[a]], E[[a]], start_ctrl=chk["start_ctrl"][[a]], pp=pp, t_now=t_now + budget)   # consumed: none now
    rows = pl2.last_conflicts(1)
    assert (rows["conflict_sample"][0] == 0).all() and (rows["conflict_partner"][0] == a).all() and not_own["plan_status"][0] == hiplib.PLAN_NO_VALID_RESTART
    tk = pl.tick(t_now, budget, pp=pp)
    assert np.array_equal(tk["query_slot"], [a])
    for k in sep:
        assert np.array_equal(tk["plan"][k], sep[k], equal_nan=True), k
    assert sep["plan_status"][0] == hiplib.PLAN_OK and _empty(pl.last_conflicts(1))
    new = pl.executing(a)
    assert new["start_time"][0] == t_now + budget and np.array_equal(new["coeffs"], sep["coeffs"][0])
    # the table restored, a vehicle parked a metre beside the start of the new path: every restart is rejected at the first clock
    pl.clear([a])
    pl.install([a], [mine["n_seg"]], mine["singul"][None], mine["piece_nums"][None], mine["coeff_dt"][None], mine["coeffs"][None],
               mine["end_state"][None], t_start=0.0)
    st = chk["start_state"][a]
    b = (a + 1) % Q
    park = cs._held(oracle.minco_generate, (st[0] - 1.0 * np.sin(st[2]), st[1] + 1.0 * np.cos(st[2])), np.degrees(st[2]), -15.0)
    pad = rs.padded(dict(slots=[park]), pp.max_seg, pp.max_pieces)
    pl.install([b], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=-18.0)
    before = pl.executing(a)
    tk2 = pl.tick(t_now, budget, pp=pp)
    rows = pl.last_conflicts(1)
    assert np.array_equal(tk2["query_slot"], [a]) and tk2["plan"]["plan_status"][0] == hiplib.PLAN_NO_VALID_RESTART
    assert (rows["conflict_sample"][0] == 0).all() and (rows["conflict_partner"][0] == b).all()
    assert all(np.asarray(before[k]).tobytes() == np.asarray(pl.executing(a)[k]).tobytes() for k in EXEC_KEYS)   # it keeps its plan
    pl2.close()
    pl.close()
    h.close()
