"""The CPU yardstick of the candidate conflict check (oracle_conflict/candidate_oracle.cpp) held to the install construction within
the oracle alone -- a candidate's row equals the row of its slot on a table with the candidate installed there -- to hand values,
to the agreement of its two orders on every index; and what the new entry points refuse without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from oracle_conflict import pycandidate as pcand
from oracle_conflict import pyconflict as pc

INF, NAN = float("inf"), float("nan")
NEW = ("dftpav_batch_check_conflicts", "dftpav_batch_sample_poses", "dftpav_batch_conflicts_last_ms", "dftpav_planner_set_conflict_filter",
       "dftpav_planner_set_own_slots", "dftpav_planner_last_conflicts")


def table_of(scene, max_seg=cs.MAX_SEG, max_pieces=cs.MAX_PIECES):
    """the scene's slots as the full padded table the oracle takes (empty slots: n_seg 0)"""
    pad = rs.padded(scene, max_seg, max_pieces)
    S = len(scene["slots"])
    n_seg, ts = np.zeros(S, np.int32), np.zeros(S)
    sg, pn, dt = np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg))
    co = np.zeros((S, max_seg * max_pieces, 6, 2))
    for k, s in enumerate(pad["slots"]):
        n_seg[s], sg[s], pn[s], dt[s], co[s], ts[s] = (pad[key][k] for key in ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "t_start"))
    return n_seg, sg, pn, dt, co, ts


def installed(tab, s, plan, t_start):
    """a copy of the table with `plan` in slot s, started at t_start"""
    n_seg, sg, pn, dt, co, ts = (a.copy() for a in tab)
    M = len(plan["piece_nums"])
    n_seg[s], ts[s] = M, t_start
    sg[s], pn[s], dt[s], co[s] = 0, 0, 0.0, 0.0
    sg[s, :M], pn[s, :M], dt[s, :M] = plan["singul"], plan["piece_nums"], plan["coeff_dt"]
    co[s, :plan["coeffs"].shape[0]] = plan["coeffs"]
    return n_seg, sg, pn, dt, co, ts


def as_batch(plan):
    """one plan as a batch of one candidate: singul, piece_nums, piece_dt [1][M], coeffs [1][Ntot][6][2]"""
    return plan["singul"], plan["piece_nums"], plan["coeff_dt"][None], plan["coeffs"][None]


def same(a, b, ia=slice(None), ib=slice(None)):
    return all((np.array_equal(np.asarray(a[k][ia]).view(np.int64), np.asarray(b[k][ib]).view(np.int64)) if k == "min_sep"
                else np.array_equal(a[k][ia], b[k][ib])) for k in pc.FIELDS)


@pytest.fixture(scope="module")
def scene(oracle):
    sc = cs.crafted(oracle.minco_generate)
    return dict(sc=sc, tab=table_of(sc), clocks=(sc["t0"], sc["dt"], sc["K"]))


def _slots(sc, case):
    return [s for s, c in sc["expect"].items() if c == case]


@pytest.mark.parametrize("order", [0, 2])
def test_install_construction(scene, order):
    """every plan of the scene as a candidate: into its own slot (a replaced slot) and into a free one.  The existing oracle's row of
    slot s on a table with the candidate installed in s equals the candidate's row with own = s, indices included."""
    sc, tab = scene["sc"], scene["tab"]
    free = [s for s, p in enumerate(sc["slots"]) if p is None]
    seen = 0
    for case in sc["cases"]:
        for src, plan in enumerate(sc["slots"]):
            if plan is None:
                continue
            for s in (src, free[src % len(free)]):
                for t_start in (plan["t_start"], sc["t0"] + 2.5):
                    ref = pc.conflicts(*installed(tab, s, plan, t_start), *scene["clocks"], *case, order=order)
                    got = pcand.conflicts(*as_batch(plan), t_start, tab, *scene["clocks"], *case, own=[s], order=order)
                    assert same(got, ref, slice(0, 1), slice(s, s + 1)), (case, src, s, t_start, {k: (got[k][0], ref[k][s]) for k in pc.FIELDS})
                    seen += got["sep_partner"][0] >= 0
                    if s != src and t_start == plan["t_start"]:    # installed beside itself: the twin overlaps it from the first clock on
                        assert got["min_sep"][0] == 0.0 and got["sep_partner"][0] <= src and got["conflict_sample"][0] == 0
    assert seen > 100
    # the poses too: the candidate's are the installed slot's
    plan = sc["slots"][_slots(sc, "gear_shift")[0]]
    a = pcand.poses(*as_batch(plan), 47.5, *scene["clocks"], order=order)
    b = pc.poses(*installed(tab, free[0], plan, 47.5), *scene["clocks"], order=order)
    assert np.array_equal(a[:, 0].view(np.int64), b[:, free[0]].view(np.int64))


def test_own_slot_takes_no_part(scene):
    sc, tab = scene["sc"], scene["tab"]
    a, b = _slots(sc, "lanes")
    plan = sc["slots"][a]
    none = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], 0.5, 60.0, own=None)
    assert none["min_sep"][0] == 0.0 and none["sep_partner"][0] == a and none["conflict_sample"][0] == 0    # its own old plan
    minus = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], 0.5, 60.0, own=[-1])
    assert same(none, minus)
    own = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], 0.5, 60.0, own=[a])
    assert own["sep_partner"][0] == b and own["conflict_sample"][0] == -1
    other = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], 0.5, 60.0, own=[b])
    assert same(other, none)                                    # excluding a slot that is not the nearest changes nothing here


def test_hand_values(scene):
    """the 1.10 m lane gap: the lower lane's plan as a candidate for its own slot sees the upper lane 1.10 m away at every clock, so
    the first clock has it; with a margin of 1.2 m that clock conflicts, with 1.0 m none does"""
    sc, tab = scene["sc"], scene["tab"]
    a, b = _slots(sc, "lanes")
    plan = sc["slots"][a]
    for margin, first in ((1.0, -1), (1.2, 0)):
        r = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], margin, 2.0, own=[a])
        assert abs(r["min_sep"][0] - 1.10) < 1e-9 and abs(r["min_sep"][0] - cs.LANE_GAP) < 1e-9
        assert r["sep_sample"][0] == 0 and r["sep_partner"][0] == b and r["conflict_sample"][0] == first and r["conflict_partner"][0] == (b if first == 0 else -1)
    # started 4 s late it is held at its start while the other drives on: the gap is 1.10 m only at the first clock
    late = pcand.conflicts(*as_batch(plan), plan["t_start"] + 4.0, tab, *scene["clocks"], 0.5, 60.0, own=[a])
    assert abs(late["min_sep"][0] - 1.10) < 1e-9 and late["sep_sample"][0] == 0
    # a negative margin is legal and never conflicts, an overlap included
    r = pcand.conflicts(*as_batch(plan), plan["t_start"], tab, *scene["clocks"], -1.0, 2.0)
    assert r["min_sep"][0] == 0.0 and r["conflict_sample"][0] == -1
    # far from everything, and against an empty table: +inf, -1
    far = dict(plan, coeffs=plan["coeffs"] + np.array([0.0, 5000.0]) * (np.arange(6) == 0)[None, :, None])
    for t in (tab, tuple(np.zeros_like(x) for x in tab)):
        r = pcand.conflicts(*as_batch(far if t is tab else plan), plan["t_start"], t, *scene["clocks"], 0.5, 60.0)
        assert np.isposinf(r["min_sep"][0]) and all(r[k][0] == -1 for k in pc.FIELDS[1:])


def test_orders_agree_on_every_index(scene):
    sc, tab = scene["sc"], scene["tab"]
    plans = [p for p in sc["slots"] if p is not None and len(p["piece_nums"]) == 1 and p["piece_nums"][0] == 5]
    batch = (plans[0]["singul"], plans[0]["piece_nums"], np.stack([p["coeff_dt"] for p in plans]), np.stack([p["coeffs"] for p in plans]))
    assert len(plans) >= 10
    for case in sc["cases"]:
        r0 = pcand.conflicts(*batch, sc["t0"] + 1.0, tab, *scene["clocks"], *case, order=0)
        r2 = pcand.conflicts(*batch, sc["t0"] + 1.0, tab, *scene["clocks"], *case, order=2)
        for k in pc.FIELDS[1:]:
            assert np.array_equal(r0[k], r2[k]), (case, k)
        assert np.allclose(r0["min_sep"], r2["min_sep"], rtol=0.0, atol=1e-9) and (r2["sep_partner"] >= 0).sum() >= 10


def test_the_names_are_declared_exported_and_present(hiplib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dftpav_hip.h")).read()
    declared = set(re.findall(r"\b(dftpav_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in hiplib.EXPORTS and getattr(hiplib.lib(), name) is not None, name


REFUSED = [dict(K=0), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN), dict(t_start=INF),
           dict(t_start=NAN), dict(margin=NAN), dict(margin=1.0, range=0.5), dict(range=INF), dict(range=NAN), dict(margin=INF),
           dict(margin=INF, range=INF)]


def test_python_entry_points_refuse_without_a_library_call(hiplib):
    good = dict(t_start=1.0, t0=0.0, dt=0.1, K=5, margin=0.5, range=None)
    assert hiplib.candidate_conflict_args(**good) == (1.0, 0.0, 0.1, 5, 0.5, 0.5) and pcand.check_args(**good) == (0.5, 0.5)
    assert hiplib.candidate_conflict_args(**dict(good, margin=-1.0, range=0.0))[4] == -1.0
    for bad in REFUSED:
        kw = dict(good, **bad)
        with pytest.raises(hiplib.DftpavError) as e:
            hiplib.candidate_conflict_args(**kw)
        assert e.value.code == hiplib.E_INVALID
        with pytest.raises(ValueError):
            pcand.check_args(**kw)


def test_entry_points_refuse_a_null_planner_or_batch(hiplib):
    """no batch, no planner, no handle: DFTPAV_E_INVALID from each of the new calls, outputs untouched"""
    Lb = hiplib.lib()
    out = hiplib.ConflictOut(3)
    for a in out.a.values():
        a[...] = 77
    poses = np.full((2, 3, 4), 77.0)
    own = np.zeros(3, np.int32)
    ms = (C.c_float(7.0), C.c_float(7.0))
    vp, dbl = C.c_void_p, C.c_double
    Lb.dftpav_batch_check_conflicts.argtypes = [vp, vp, dbl, dbl, dbl, C.c_int, dbl, dbl, vp, vp]
    Lb.dftpav_batch_sample_poses.argtypes = [vp, dbl, dbl, dbl, C.c_int, vp]
    Lb.dftpav_batch_conflicts_last_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    Lb.dftpav_planner_set_conflict_filter.argtypes = [vp, dbl, dbl, dbl, C.c_int]
    Lb.dftpav_planner_set_own_slots.argtypes = [vp, vp, C.c_int]
    Lb.dftpav_planner_last_conflicts.argtypes = [vp, vp]
    assert Lb.dftpav_batch_check_conflicts(None, None, 0.0, 0.0, 0.1, 2, 0.0, 0.0, None, C.byref(out.c)) == hiplib.E_INVALID
    assert Lb.dftpav_batch_sample_poses(None, 0.0, 0.0, 0.1, 2, poses.ctypes.data_as(vp)) == hiplib.E_INVALID
    assert Lb.dftpav_batch_conflicts_last_ms(None, C.byref(ms[0]), C.byref(ms[1])) == hiplib.E_INVALID
    assert Lb.dftpav_planner_set_conflict_filter(None, 0.5, 1.0, 0.1, 10) == hiplib.E_INVALID
    assert Lb.dftpav_planner_set_own_slots(None, own.ctypes.data_as(vp), 3) == hiplib.E_INVALID
    assert Lb.dftpav_planner_last_conflicts(None, C.byref(out.c)) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and (poses == 77.0).all() and ms[0].value == 7.0 and ms[1].value == 7.0
