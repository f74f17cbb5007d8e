"""The CPU yardstick of the conflict trigger (oracle_conflict/pytrigger.py) held to the cases its scene is there for, to the two
properties of the definition against the conflict check's oracle, to hand values, and to its own symmetries; and what the new entry
points refuse without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from dftpav_amd import trigger_scenes as ts
from oracle_conflict import pyconflict as pc
from oracle_conflict import pytrigger as pt

INF, NAN = float("inf"), float("nan")
NEW = ("dftpav_planner_check_yield", "dftpav_planner_set_conflict_trigger", "dftpav_planner_last_trigger", "dftpav_trigger_last_ms",
       "dftpav_debug_conflict_trigger")


def table_of(scene, max_seg=cs.MAX_SEG, max_pieces=cs.MAX_PIECES):
    """the scene's slots as the full padded table the oracles take (empty slots: n_seg 0)"""
    pad = rs.padded(scene, max_seg, max_pieces)
    S = len(scene["slots"])
    n_seg, t0 = np.zeros(S, np.int32), np.zeros(S)
    sg, pn, dt = np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg))
    co = np.zeros((S, max_seg * max_pieces, 6, 2))
    for k, s in enumerate(pad["slots"]):
        n_seg[s], sg[s], pn[s], dt[s], co[s], t0[s] = (pad[key][k] for key in ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "t_start"))
    return n_seg, sg, pn, dt, co, t0


@pytest.fixture(scope="module")
def scene(oracle):
    sc = ts.crafted(oracle.minco_generate)
    tab = table_of(sc)
    clocks = (sc["t0"], sc["dt"], sc["K"])
    rows, stats = {}, {}
    for case in sc["cases"]:
        for t_now in sc["t_nows"]:
            stats[case, t_now] = {}
            rows[case, t_now] = pt.check_yield(*tab, t_now, *clocks, *case, order=2, stats=stats[case, t_now])
    check = {case: pc.conflicts(*tab, *clocks, *case, order=2) for case in sc["cases"]}
    return dict(sc=sc, tab=tab, clocks=clocks, rows=rows, stats=stats, check=check, poses=pc.poses(*tab, *clocks, order=2))


def _slots(sc, case):
    return [s for s, c in sc["expect"].items() if c == case]


def _row(r, s):
    return int(r["yield"][s]), int(r["yield_sample"][s]), int(r["yield_partner"][s])


def test_every_case_of_the_scene_occurs(scene):
    sc, rows = scene["sc"], scene["rows"]
    early, late = sc["t_nows"]
    tight, mid, wide = sc["cases"]                              # (0, 0), (0.5, 0.5), (0.5, 60)
    occupied = np.array([p is not None for p in sc["slots"]])
    assert occupied.sum() == 17 and (~occupied).sum() == 7
    for r in rows.values():                                     # an empty slot: 0, -1, -1
        assert (r["yield"][~occupied] == 0).all() and (r["yield_sample"][~occupied] == -1).all() and (r["yield_partner"][~occupied] == -1).all()
    for case in sc["cases"]:
        r, chk = rows[case, early], scene["check"][case]
        a, b = _slots(sc, "precedes_all")[0], _slots(sc, "crossing_yields")[0]
        assert a < b and _row(r, a) == (0, -1, -1) and chk["conflict_partner"][a] == b     # in conflict, but only with a slot it precedes
        assert _row(r, b) == (1, chk["conflict_sample"][b], a) and r["yield_sample"][b] > 0
        a, b = _slots(sc, "drives_into_parked")[0], _slots(sc, "parked_on_path")[0]
        assert a < b and _row(r, a)[0] == 1 and r["yield_partner"][a] == b                   # the LOWER slot yields to a completed plan
        assert _row(r, b) == (0, r["yield_sample"][a], a)                                    # which names it, and cannot yield
        a, b = _slots(sc, "both_completed")
        assert _row(r, a) == (0, 0, b) and _row(r, b) == (0, 0, a)                           # neither yields, both rows name a partner
        lo, me, hi = (_slots(sc, c)[0] for c in ("late_partner", "two_partners", "early_partner"))
        assert lo < me < hi and _row(r, lo) == (0, -1, -1) and r["yield"][me] == 1 and r["yield"][hi] == 1
        assert (chk["conflict_sample"][me], chk["conflict_partner"][me]) == (r["yield_sample"][hi], hi)   # the check: the early partner
        assert r["yield_partner"][me] == lo and r["yield_sample"][me] > chk["conflict_sample"][me]       # the trigger: the one that precedes
        a, b = _slots(sc, "at_k0")
        assert _row(r, a) == (0, -1, -1) and _row(r, b) == (1, 0, a)
        a, b = _slots(sc, "range_cut")
        assert _row(r, a) == (0, -1, -1) and _row(r, b) == (0, -1, -1)
    a, b = _slots(sc, "range_cut")                              # the pair alone: outside the broad phase of range 0, inside that of 0.5
    alone = scene["poses"][:, [a, b]]
    for (margin, rng), n in ((tight, 0), (mid, 2 * sc["K"])):
        st = {}
        pt.rows(alone, [1, 1], margin, rng, stats=st)
        assert st["inside"] == n and st["narrow"] == n // 2
    a, b = _slots(sc, "at_k_last")                              # closing to 0.3 m at the last clock
    assert _row(rows[tight, early], b) == (0, -1, -1)
    for case in (mid, wide):
        assert _row(rows[case, early], a) == (0, -1, -1) and _row(rows[case, early], b) == (1, sc["K"] - 1, a)
    a, b = _slots(sc, "meets_ending")[0], _slots(sc, "ends_early")[0]
    for case in sc["cases"]:                                    # can_yield flips between the two clocks, and who yields with it
        r0, r1 = rows[case, early], rows[case, late]
        assert a < b and _row(r0, a) == (0, -1, -1) and r0["yield"][b] == 1 and r0["yield_partner"][b] == a
        assert _row(r1, a) == (1, r0["yield_sample"][b], b) and _row(r1, b) == (0, r0["yield_sample"][b], a)
        assert scene["stats"][case, late]["narrow"] > scene["stats"][case, early]["narrow"]
        assert scene["stats"][case, late]["inside"] == scene["stats"][case, early]["inside"] == scene["check"][case]["inside"]


def test_the_two_properties_against_the_conflict_check(scene):
    sc, tab = scene["sc"], scene["tab"]
    ends = pt.end_times(tab[0], tab[2], tab[3], tab[5])
    for case in sc["cases"]:
        chk = scene["check"][case]
        for t_now in sc["t_nows"]:
            r = scene["rows"][case, t_now]
            cy = pt.can_yield(tab[0], ends, t_now)
            for i in range(ts.N_SLOTS):
                if tab[0][i] == 0:
                    continue
                # every partner of i that conflicts at all, from the pairwise separations
                partners = [j for j in range(ts.N_SLOTS) if j != i and tab[0][j] > 0 and any(
                    np.hypot(*(scene["poses"][k, i, :2] - scene["poses"][k, j, :2])) <= case[1] + 5.3 and
                    pc.sep(scene["poses"][k, i], scene["poses"][k, j]) <= case[0] for k in range(0, sc["K"]))]
                if partners and all((not cy[j]) or j < i for j in partners):   # all of them precede i: the check's own rows
                    assert (r["yield_sample"][i], r["yield_partner"][i]) == (chk["conflict_sample"][i], chk["conflict_partner"][i]), i
                if not partners:
                    assert r["yield_sample"][i] == -1 and chk["conflict_sample"][i] == -1
    # with every slot able to yield, the lowest slot of a conflicting set never yields and its highest always does
    under_way = [s for s in range(ts.N_SLOTS) if sc["expect"].get(s) in ("precedes_all", "crossing_yields", "late_partner", "two_partners",
                                                                          "early_partner", "at_k0")]
    P = scene["poses"][:, under_way]
    r = pt.rows(P, [1] * len(under_way), 0.5, 60.0)
    c = pc.conflicts(*[np.asarray(a)[under_way] for a in tab], *scene["clocks"], 0.5, 60.0, order=2)
    assert r["yield"][0] == 0 and r["yield_sample"][0] == -1 and c["conflict_sample"][0] >= 0
    assert r["yield"].tolist() == [0, 1, 0, 1, 1, 0, 1]
    comp = list(range(len(under_way)))                          # the conflicting sets: the components of the check's partner edges
    for _ in comp:
        for i in np.flatnonzero(c["conflict_sample"] >= 0):
            comp[i] = comp[c["conflict_partner"][i]] = min(comp[i], comp[c["conflict_partner"][i]])
    groups = [[i for i in range(len(comp)) if comp[i] == g] for g in set(comp)]
    assert sorted(len(g) for g in groups) == [2, 2, 3]
    for g in groups:
        assert r["yield"][max(g)] == 1 and r["yield"][min(g)] == 0


def _pose(x, y, deg=0.0):
    return [x, y, np.cos(np.radians(deg)), np.sin(np.radians(deg))]


def test_hand_made_tables():
    far = 1000.0
    # three slots in a row along x, 5.0 m apart nose to tail (gap 0.12): 0 - 1 - 2; K = 2, the second sample 100 m apart
    near = [_pose(0.0, 0.0), _pose(5.0, 0.0), _pose(10.0, 0.0)]
    apart = [_pose(0.0, 0.0), _pose(0.0, far), _pose(far, 0.0)]
    r = pt.rows([apart, near], [1, 1, 1], 0.2, 1.0)
    assert r["yield"].tolist() == [0, 1, 1] and r["yield_sample"].tolist() == [-1, 1, 1] and r["yield_partner"].tolist() == [-1, 0, 1]
    r = pt.rows([apart, near], [1, 1, 0], 0.2, 1.0)             # slot 2 cannot yield: slot 1 names slot 0 still (the lower j at the same k)
    assert r["yield"].tolist() == [0, 1, 0] and r["yield_partner"].tolist() == [-1, 0, 1]
    r = pt.rows([apart, near], [1, 0, 1], 0.2, 1.0)             # slot 1 cannot: both neighbours yield to it
    assert r["yield"].tolist() == [1, 0, 1] and r["yield_partner"].tolist() == [1, 0, 1] and r["yield_sample"].tolist() == [1, 1, 1]
    r = pt.rows([apart, near], [1, 1, 1], 0.1, 1.0)             # a margin below the gap: nothing
    assert r["yield"].tolist() == [0, 0, 0] and (r["yield_sample"] == -1).all()
    # four slots: 0 and 3 overlap at k = 0; 1 and 3 overlap at k = 1; 2 is a NaN row (empty)
    k0 = [_pose(0.0, 0.0), _pose(0.0, far), [NAN] * 4, _pose(1.0, 0.5, 30.0)]
    k1 = [_pose(far, 0.0), _pose(0.0, far), [NAN] * 4, _pose(1.0, far + 0.5, 30.0)]
    r = pt.rows([k0, k1], [1, 1, 1, 1], 0.0, 0.0)
    assert r["yield"].tolist() == [0, 0, 0, 1] and r["yield_sample"].tolist() == [-1, -1, -1, 0] and r["yield_partner"].tolist() == [-1, -1, -1, 0]
    r = pt.rows([k0, k1], [1, 1, 1, 0], 0.0, 0.0)               # slot 3 completed: 0 yields at k = 0, 1 at k = 1
    assert r["yield"].tolist() == [1, 1, 0, 0] and r["yield_sample"].tolist() == [0, 1, -1, 0] and r["yield_partner"].tolist() == [3, 3, -1, 0]
    # five slots, a chain of overlaps 0 - 1 - 2 - 3 - 4 at one clock: everybody but slot 0 yields to the one below
    chain = [[_pose(3.0 * s, 0.0) for s in range(5)]]
    r = pt.rows(chain, [1] * 5, 0.0, 0.0)
    assert r["yield"].tolist() == [0, 1, 1, 1, 1] and r["yield_partner"].tolist() == [-1, 0, 1, 2, 3]
    r = pt.rows(chain, [1, 1, 0, 1, 1], 0.0, 0.0)
    assert r["yield"].tolist() == [0, 1, 0, 1, 1] and r["yield_partner"].tolist() == [-1, 0, 1, 2, 3]
    r = pt.rows(chain, [0] * 5, 0.0, 0.0)
    assert r["yield"].sum() == 0 and r["yield_partner"].tolist() == [1, 0, 1, 2, 3]


def test_orders_agree_on_every_index(scene):
    sc = scene["sc"]
    for case in sc["cases"]:
        for t_now in sc["t_nows"]:
            r0 = pt.check_yield(*scene["tab"], t_now, *scene["clocks"], *case, order=0)
            for k in pt.FIELDS:
                assert np.array_equal(r0[k], scene["rows"][case, t_now][k]), (case, t_now, k)


def test_swapping_two_slots_swaps_who_yields(scene):
    sc = scene["sc"]
    for a, b in (_slots(sc, "precedes_all") + _slots(sc, "crossing_yields"), _slots(sc, "at_k0"), _slots(sc, "at_k_last")):
        perm = np.arange(ts.N_SLOTS)
        perm[[a, b]] = perm[[b, a]]
        tab = [np.asarray(x)[perm] for x in scene["tab"]]
        r0 = scene["rows"][sc["cases"][2], sc["t_nows"][0]]
        r1 = pt.check_yield(*tab, sc["t_nows"][0], *scene["clocks"], *sc["cases"][2], order=2)
        # the plan that did not yield sits in the higher slot now, and yields there: the rows are a matter of the indices alone
        assert np.array_equal(tab[4][b], scene["tab"][4][a]) and not np.array_equal(tab[4][b], scene["tab"][4][b])
        assert r0["yield"][a] == 0 and r0["yield"][b] == 1 and r1["yield"][a] == 0 and r1["yield"][b] == 1
        assert r1["yield_partner"][b] == a and r1["yield_sample"][b] == r0["yield_sample"][b] and r1["yield_sample"][a] == -1
        rest = [s for s in range(ts.N_SLOTS) if s not in (a, b)]
        assert all(np.array_equal(r0[k][rest], r1[k][rest]) for k in pt.FIELDS)


def test_the_names_are_declared_exported_and_present(hiplib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dftpav_hip.h")).read()
    declared = set(re.findall(r"\b(dftpav_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in hiplib.EXPORTS and getattr(hiplib.lib(), name) is not None, name
    assert C.sizeof(hiplib._YieldOutC) == 24 and hiplib.YieldOut.KEYS == pt.FIELDS
    assert "There is no trigger" not in hdr


REFUSED = [dict(K=0), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN), dict(t_now=INF),
           dict(t_now=NAN), dict(margin=-0.1), dict(margin=NAN), dict(margin=1.0, range=0.5), dict(range=INF), dict(range=NAN),
           dict(margin=INF), dict(margin=INF, range=INF)]


def test_python_entry_points_refuse_without_a_library_call(hiplib):
    good = dict(t_now=1.0, t0=0.0, dt=0.1, K=5, margin=0.5, range=None)
    assert hiplib.yield_args(**good) == (1.0, 0.0, 0.1, 5, 0.5, 0.5) and pt.check_args(**good) == (0.5, 0.5)
    pl = hiplib.Planner.__new__(hiplib.Planner)                 # no handle, no planner behind it: a library call would fail otherwise
    pl._p, pl.handle, pl.max_queries = None, None, 3
    for bad in REFUSED:
        kw = dict(good, **bad)
        with pytest.raises(hiplib.DftpavError) as e:
            hiplib.yield_args(**kw)
        assert e.value.code == hiplib.E_INVALID
        with pytest.raises(hiplib.DftpavError) as e:
            pl.check_yield(**kw)
        assert e.value.code == hiplib.E_INVALID
        with pytest.raises(ValueError):
            pt.check_args(**kw)


def test_entry_points_refuse_a_null_planner(hiplib):
    """no planner, no handle: DFTPAV_E_INVALID from each of the new calls, outputs untouched"""
    Lb = hiplib.lib()
    out = hiplib.YieldOut(3)
    for a in out.a.values():
        a[...] = 77
    ms = (C.c_float(7.0), C.c_float(7.0))
    poses, cy = np.zeros((2, 3, 4)), np.ones(3, dtype=np.int32)
    Lb.dftpav_planner_check_yield.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    Lb.dftpav_planner_set_conflict_trigger.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int]
    Lb.dftpav_planner_last_trigger.argtypes = [C.c_void_p, C.c_void_p]
    Lb.dftpav_trigger_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    Lb.dftpav_debug_conflict_trigger.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    assert Lb.dftpav_planner_check_yield(None, 0.0, 0.0, 0.1, 2, 0.0, 0.0, C.byref(out.c)) == hiplib.E_INVALID
    assert Lb.dftpav_planner_set_conflict_trigger(None, 0.5, 1.0, 0.1, 5) == hiplib.E_INVALID
    assert Lb.dftpav_planner_set_conflict_trigger(None, -1.0, 1.0, 0.1, 5) == hiplib.E_INVALID
    assert Lb.dftpav_planner_last_trigger(None, C.byref(out.c)) == hiplib.E_INVALID
    assert Lb.dftpav_trigger_last_ms(None, C.byref(ms[0]), C.byref(ms[1])) == hiplib.E_INVALID
    assert Lb.dftpav_debug_conflict_trigger(None, 3, 2, poses.ctypes.data_as(C.c_void_p), cy.ctypes.data_as(C.c_void_p), 0.5, 1.0,
                                            C.byref(out.c)) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and ms[0].value == 7.0 and ms[1].value == 7.0
