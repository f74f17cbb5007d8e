"""Footprint conflicts between the executing plans on the device (conflict.hip): the poses and all five outputs bit-equal to
oracle_conflict in order 2 -- on the crafted scene, across tile edges, with cleared slots, for sample counts that do not fill the
four waves -- and the calls leave the table and the publisher as they found them."""
import ctypes as C
import itertools

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
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


def _table(pl):
    """the table as the device holds it, read back slot by slot, in the oracle's arguments"""
    return pc.from_executing([pl.executing(s) for s in range(pl.max_queries)])


def _same(got, ref):
    for k in pc.FIELDS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        same = np.array_equal(a.view(np.int64), b.view(np.int64)) if k == "min_sep" else np.array_equal(a, b)
        assert same, (k, np.flatnonzero(a != b)[:8], a[a != b][:8], b[a != b][:8])


def _empty(r, idx=slice(None)):
    return np.isposinf(r["min_sep"][idx]).all() and all((r[k][idx] == -1).all() for k in pc.FIELDS[1:])


@pytest.fixture(scope="module")
def crafted(hiplib, oracle):
    sc = cs.crafted(oracle.minco_generate)
    h = hiplib.Handle()
    pl = hiplib.Planner(h, cs.N_SLOTS, 1)
    fresh = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0), pl.sample_poses(sc["t0"], sc["dt"], 3)   # never filled
    _install(pl, sc)
    yield dict(sc=sc, h=h, pl=pl, tab=_table(pl), fresh=fresh)
    pl.close()
    h.close()


def test_a_never_filled_planner_gives_the_empty_rows(crafted):
    rows, poses = crafted["fresh"]
    assert _empty(rows) and rows["min_sep"].shape == (cs.N_SLOTS,)
    assert poses.shape == (3, cs.N_SLOTS, 4) and np.isnan(poses).all()


@pytest.mark.parametrize("K", [1, 5, 257])
def test_poses_equal_the_oracle(crafted, K):
    sc, pl = crafted["sc"], crafted["pl"]
    dt = 10.0 / 256 if K == 257 else sc["dt"]                   # 257 clocks over the same 10 s: exactly representable steps
    got = pl.sample_poses(sc["t0"], dt, K)
    ref = pc.poses(*crafted["tab"], sc["t0"], dt, K, order=2)
    assert got.shape == ref.shape == (K, cs.N_SLOTS, 4)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64)), np.argwhere(got.view(np.int64) != ref.view(np.int64))[:8]
    occupied = np.array([p is not None for p in sc["slots"]])
    assert np.isnan(got[:, ~occupied]).all() and np.isfinite(got[:, occupied]).all()
    assert crafted["h"].conflicts_last_ms()[0] > 0.0 and crafted["h"].conflicts_last_ms()[1] == 0.0


@pytest.mark.parametrize("case", cs.CASES)
def test_rows_equal_the_oracle_on_the_scene(crafted, case):
    sc, pl = crafted["sc"], crafted["pl"]
    got = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], *case)
    ref = pc.conflicts(*crafted["tab"], sc["t0"], sc["dt"], sc["K"], *case, order=2)
    _same(got, ref)
    assert ref["inside"] > 0 and (got["min_sep"] == 0.0).sum() == 4 and (got["conflict_sample"] >= 0).sum() >= 4
    ms = crafted["h"].conflicts_last_ms()
    assert ms[0] > 0.0 and ms[1] > 0.0
    if case == cs.CASES[0]:                                     # range None is margin
        _same(pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], case[0]), ref)


@pytest.mark.parametrize("K", [1, 2, 3, 7])
def test_sample_counts_that_do_not_fill_the_waves(crafted, K):
    sc, pl = crafted["sc"], crafted["pl"]
    for t0 in (sc["t0"], sc["t0"] + 4.0):                       # the second window starts next to the crossing
        _same(pl.check_conflicts(t0, 0.4, K, 0.5, 60.0), pc.conflicts(*crafted["tab"], t0, 0.4, K, 0.5, 60.0, order=2))


def test_mirrored_pairs_on_the_device_rows(crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    r = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    seen = 0
    for i in range(cs.N_SLOTS):
        j = r["sep_partner"][i]
        if j < 0:
            continue
        seen += 1
        mine = (r["min_sep"][i], r["sep_sample"][i], i)         # what j sees of i: the same bits, so j's minimum is no larger
        assert (r["min_sep"][j], r["sep_sample"][j], r["sep_partner"][j]) <= mine, (i, j)
        c = r["conflict_partner"][i]
        if c >= 0:
            assert (r["conflict_sample"][c], r["conflict_partner"][c]) <= (r["conflict_sample"][i], i)
    assert seen >= 20


def test_nothing_is_written(crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    S = cs.N_SLOTS
    # dftpav_replan_check needs a map (the conflict calls do not: the tests before this one ran without): open ground round the
    # lanes of slots 4 and 5, a box on the first lane
    grid = np.zeros((40, 120), dtype=np.uint8)
    grid[20:22, 70:72] = 80
    crafted["h"].set_grid_map(grid, 0.5, (-30.0, cs.GROUP - 10.0))

    def state():
        ex = [pl.executing(s) for s in range(S)]
        pub = [pl.publisher_state(s) for s in range(S)]
        chk = pl.check(sc["t0"] + 1.0)
        return ex, pub, chk

    ex0, pub0, chk0 = state()
    pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    pl.sample_poses(sc["t0"], sc["dt"], sc["K"])
    ex1, pub1, chk1 = state()
    for a, b in zip(ex0, ex1):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in EXEC_KEYS)
    for a, b in zip(pub0, pub1):
        assert a["exe_index"] == b["exe_index"] and a["have_hist"] == b["have_hist"] and a["hist"].tobytes() == b["hist"].tobytes()
    assert chk0["collision"][4] == 1 and chk0["occupied"].sum() == 24
    assert set(chk0) == set(chk1) and all(np.asarray(chk0[k]).tobytes() == np.asarray(chk1[k]).tobytes() for k in chk0)


def test_null_output_pointers(hiplib, crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    full = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    fn = hiplib.lib().dftpav_planner_check_conflicts
    fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    n = 0
    for keep in itertools.product((False, True), repeat=5):
        if not any(keep):
            continue
        out = hiplib.ConflictOut(cs.N_SLOTS)
        for a in out.a.values():
            a[...] = 77
        for k, on in zip(pc.FIELDS, keep):
            if not on:
                setattr(out.c, k, None)
        assert fn(pl._p, sc["t0"], sc["dt"], sc["K"], 0.5, 60.0, C.byref(out.c)) == hiplib.OK
        for k, on in zip(pc.FIELDS, keep):
            assert np.array_equal(out.a[k], full[k]) if on else (out.a[k] == 77).all(), (keep, k)
        n += 1
    assert n == 31


def test_refusals_change_nothing(hiplib, crafted):
    sc, pl = crafted["sc"], crafted["pl"]
    good = pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0)
    ms = crafted["h"].conflicts_last_ms()
    ex0 = [pl.executing(s) for s in range(cs.N_SLOTS)]
    fn, fp = hiplib.lib().dftpav_planner_check_conflicts, hiplib.lib().dftpav_planner_sample_poses
    fn.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    fp.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    out = hiplib.ConflictOut(cs.N_SLOTS)
    for a in out.a.values():
        a[...] = 77
    poses = np.full((2, cs.N_SLOTS, 4), 77.0)
    ok = dict(t0=sc["t0"], dt=sc["dt"], K=2, margin=0.5, range=60.0)
    bad = [dict(K=0), dict(K=-1), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN),
           dict(margin=-0.1), dict(margin=NAN), dict(margin=61.0), dict(range=INF), dict(range=NAN), dict(margin=INF), dict(margin=INF, range=INF)]
    for b in bad:
        a = dict(ok, **b)
        assert fn(pl._p, a["t0"], a["dt"], a["K"], a["margin"], a["range"], C.byref(out.c)) == hiplib.E_INVALID, b
        if "margin" not in b and "range" not in b:
            assert fp(pl._p, a["t0"], a["dt"], a["K"], poses.ctypes.data_as(C.c_void_p)) == hiplib.E_INVALID, b
    assert fn(pl._p, ok["t0"], ok["dt"], 2, 0.5, 60.0, None) == hiplib.E_INVALID
    assert fp(pl._p, ok["t0"], ok["dt"], 2, None) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and (poses == 77.0).all()
    assert crafted["h"].conflicts_last_ms() == ms               # nothing ran
    ex1 = [pl.executing(s) for s in range(cs.N_SLOTS)]
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for a, b in zip(ex0, ex1) for k in EXEC_KEYS)
    _same(pl.check_conflicts(sc["t0"], sc["dt"], sc["K"], 0.5, 60.0), good)


# ---- tile edges: 130 slots are three tiles of the pair kernel (64 + 64 + 2), nine workgroups
N_EDGE, EDGE_T0, EDGE_DT, EDGE_K = 130, 0.0, 0.5, 21


def _edge_scene(generate):
    """seeded straight runs over a square of 400 m; slots 63 | 64 and 127 | 128 made neighbours in space (lanes 3 m apart), and slots
    0 and 129 partners (one following the other)"""
    rng = np.random.default_rng(130)
    plans = cs.straight_plans(generate, rng, N_EDGE, 400.0, t_start=EDGE_T0)
    for a, b, y in ((63, 64, 1000.0), (127, 128, 1200.0)):
        plans[a] = cs._run(generate, (-10.0, y), (10.0, y), EDGE_T0)
        plans[b] = cs._run(generate, (-10.0, y + 3.0), (10.0, y + 3.0), EDGE_T0)
    plans[0] = cs._run(generate, (0.0, 1400.0), (20.0, 1400.0), EDGE_T0)
    plans[129] = cs._run(generate, (-7.0, 1400.0), (13.0, 1400.0), EDGE_T0)
    return dict(slots=plans)


@pytest.fixture(scope="module")
def edges(hiplib, oracle):
    sc = _edge_scene(oracle.minco_generate)
    h = hiplib.Handle()
    pl = hiplib.Planner(h, N_EDGE, 1)
    pad = rs.padded(sc, cs.MAX_SEG, cs.MAX_PIECES)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=EDGE_T0)
    yield dict(h=h, pl=pl)
    pl.close()
    h.close()


def test_tile_edges(edges):
    pl = edges["pl"]
    for margin, rng in ((0.5, 20.0), (0.0, 0.0)):
        ref = pc.conflicts(*_table(pl), EDGE_T0, EDGE_DT, EDGE_K, margin, rng, order=2)
        got = pl.check_conflicts(EDGE_T0, EDGE_DT, EDGE_K, margin, rng)
        _same(got, ref)
        assert got["sep_partner"][63] == 64 and got["sep_partner"][64] == 63 and got["sep_partner"][127] == 128 and got["sep_partner"][128] == 127
        if rng > 0.0:                                           # one follows the other 7 m behind: outside the broad phase of range 0
            assert got["sep_partner"][0] == 129 and got["sep_partner"][129] == 0
        assert (got["min_sep"] == 0.0).sum() >= 2 and ref["inside"] > 100   # the seeded runs meet one another too


def test_tile_edges_with_every_second_slot_cleared(edges):
    """(runs after test_tile_edges: it changes the module's table)"""
    pl = edges["pl"]
    pl.clear(np.arange(1, N_EDGE, 2))
    ref = pc.conflicts(*_table(pl), EDGE_T0, EDGE_DT, EDGE_K, 0.5, 20.0, order=2)
    got = pl.check_conflicts(EDGE_T0, EDGE_DT, EDGE_K, 0.5, 20.0)
    _same(got, ref)
    assert _empty(got, np.arange(1, N_EDGE, 2)) and not _empty(got, np.arange(0, N_EDGE, 2))
    assert got["sep_partner"][0] != 129 and got["sep_partner"][64] != 63
    poses = pl.sample_poses(EDGE_T0, EDGE_DT, 2)
    assert np.isnan(poses[:, 1::2]).all() and np.isfinite(poses[:, 0::2]).all()


def test_one_partial_tile(hiplib, oracle):
    """max_queries = 3: a single tile of which three lanes are slots"""
    h = hiplib.Handle()
    pl = hiplib.Planner(h, 3, 1)
    gen = oracle.minco_generate
    sc = dict(slots=[cs._run(gen, (-20.0, 0.0), (20.0, 0.0), 0.0), None, cs._run(gen, (0.0, -20.0), (0.0, 20.0), 0.0)])
    _install(pl, sc)
    for K in (1, 6, 101):
        ref = pc.conflicts(*_table(pl), 0.0, 0.1, K, 0.3, 5.0, order=2)
        got = pl.check_conflicts(0.0, 0.1, K, 0.3, 5.0)
        _same(got, ref)
    assert got["min_sep"][0] == 0.0 and got["sep_partner"][0] == 2 and got["conflict_partner"][2] == 0 and _empty(got, [1])
    got = pl.sample_poses(0.0, 0.1, 6)
    assert np.array_equal(got.view(np.int64), pc.poses(*_table(pl), 0.0, 0.1, 6, order=2).view(np.int64))
    pl.close()
    h.close()
