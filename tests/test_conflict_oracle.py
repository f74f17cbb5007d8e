"""The CPU yardstick of the conflict check between executing plans (oracle_conflict/) held to the cases it is there for, to hand
values, to its own symmetries and to an independent point sampling; and what the new entry points refuse without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dftpav_amd import conflict_scenes as cs
from dftpav_amd import replan_scenes as rs
from oracle_conflict import pyconflict as pc

INF, NAN = float("inf"), float("nan")
W, L, DCR = pc.VEH
NEW = ("dftpav_planner_check_conflicts", "dftpav_planner_sample_poses", "dftpav_conflicts_last_ms")


def table_of(scene, n_slots=None, max_seg=cs.MAX_SEG, max_pieces=cs.MAX_PIECES):
    """the scene's slots as the full padded table the oracle takes (empty slots: n_seg 0)"""
    pad = rs.padded(scene, max_seg, max_pieces)
    S = len(scene["slots"]) if n_slots is None else n_slots
    n_seg, ts = np.zeros(S, np.int32), np.zeros(S)
    sg, pn, dt = np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg), np.int32), np.zeros((S, max_seg))
    co = np.zeros((S, max_seg * max_pieces, 6, 2))
    for k, s in enumerate(pad["slots"]):
        n_seg[s], sg[s], pn[s], dt[s], co[s], ts[s] = (pad[key][k] for key in ("n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "t_start"))
    return n_seg, sg, pn, dt, co, ts


@pytest.fixture(scope="module")
def scene(oracle):
    sc = cs.crafted(oracle.minco_generate)
    tab = table_of(sc)
    clocks = (sc["t0"], sc["dt"], sc["K"])
    rows = {case: pc.conflicts(*tab, *clocks, *case, order=2) for case in sc["cases"]}
    return dict(sc=sc, tab=tab, clocks=clocks, rows=rows, poses=pc.poses(*tab, *clocks, order=2))


def _slots(sc, case):
    return [s for s, c in sc["expect"].items() if c == case]


def test_every_case_of_the_scene_occurs(scene):
    sc, rows = scene["sc"], scene["rows"]
    tight, mid, wide = (rows[c] for c in sc["cases"])          # (0, 0), (1, 1), (0.5, 60)
    occupied = np.array([p is not None for p in sc["slots"]])
    assert occupied.sum() == 24 and (~occupied).sum() == 11     # empty slots in between
    for r in rows.values():                                     # an empty slot: +inf, -1, -1, -1, -1
        assert np.isposinf(r["min_sep"][~occupied]).all() and all((r[k][~occupied] == -1).all() for k in pc.FIELDS[1:])
        e = _slots(sc, "beyond_range")[0]                       # a vehicle beyond range: the same
        assert np.isposinf(r["min_sep"][e]) and all(r[k][e] == -1 for k in pc.FIELDS[1:])
        # partners are mutual in every group of two
        for s in np.flatnonzero(occupied):
            j = r["sep_partner"][s]
            if j >= 0 and sc["expect"][s] not in ("tie_upper", "tie_middle", "tie_lower"):
                assert r["sep_partner"][j] == s and r["min_sep"][j] == r["min_sep"][s] and r["sep_sample"][j] == r["sep_sample"][s]
    a, b = _slots(sc, "crossing_hit")                           # the crossing reached together: overlap, with margin 0 too
    for r in rows.values():
        assert r["min_sep"][a] == 0.0 and r["sep_partner"][a] == b and r["conflict_partner"][a] == b and r["conflict_sample"][a] > 0
    assert tight["conflict_sample"][a] == tight["sep_sample"][a]   # margin 0: the first overlap is the first conflict
    assert mid["conflict_sample"][a] < tight["conflict_sample"][a]  # a margin of 1 m: earlier
    a, b = _slots(sc, "crossing_miss")                          # one t_start later: they miss
    assert np.isposinf(tight["min_sep"][a]) and wide["min_sep"][a] > 10.0 and wide["sep_partner"][a] == b and wide["conflict_sample"][a] == -1
    a, b = _slots(sc, "lanes")                                  # side by side: inside every broad phase (centres 3.0 m apart)
    for r in rows.values():
        assert abs(r["min_sep"][a] - cs.LANE_GAP) < 1e-9 and r["sep_sample"][a] == 0 and r["sep_partner"][a] == b and r["conflict_sample"][a] == -1
    a, b = _slots(sc, "lanes_staggered")                        # the same gap, the centres 5.49 m apart: range 0 cuts the pair off
    assert np.isposinf(tight["min_sep"][a]) and tight["sep_partner"][a] == -1
    assert abs(mid["min_sep"][a] - cs.LANE_GAP) < 1e-9 and mid["sep_partner"][a] == b and mid["conflict_sample"][a] == -1
    a, b = _slots(sc, "head_on")                                # closing to 1.09 m at the last clock
    assert np.isposinf(tight["min_sep"][a]) and abs(wide["min_sep"][a] - 1.09) < 1e-9 and wide["sep_sample"][a] == sc["K"] - 1
    a, b = _slots(sc, "ended_before")[0], _slots(sc, "drives_into_ended")[0]
    for r in rows.values():                                     # a plan that ended before t0 is held at its end, in another's way
        assert r["min_sep"][a] == 0.0 and r["sep_partner"][a] == b and r["conflict_partner"][b] == a
    assert (scene["poses"][:, a] == scene["poses"][0, a]).all() and np.array_equal(scene["poses"][0, a], [DCR, 5 * cs.GROUP, 1.0, 0.0])
    a, b = _slots(sc, "starts_after")[0], _slots(sc, "passes_waiting")[0]
    assert (scene["poses"][:, a] == scene["poses"][0, a]).all()  # a plan that starts after the last clock is held at its start
    assert abs(tight["min_sep"][a] - 0.595) < 1e-9 and tight["conflict_sample"][a] == -1
    assert mid["conflict_partner"][a] == b and 0 < mid["conflict_sample"][a] < mid["sep_sample"][a]
    a, b = _slots(sc, "reversing")[0], _slots(sc, "follows_reversing")[0]
    p = scene["poses"][10]                                      # the reversing vehicle faces +x: its centre is AHEAD of its rear axle in x
    assert p[a, 2] == 1.0 and p[b, 2] == -1.0 and abs((p[b, 0] - p[a, 0]) - (8.0 - 2 * DCR)) < 1e-9
    assert abs(mid["min_sep"][a] - (8.0 - 2 * DCR - L)) < 1e-9 and mid["sep_partner"][a] == b
    a, b = _slots(sc, "gear_shift")[0], _slots(sc, "ahead_of_shift")[0]
    assert wide["sep_partner"][a] == b and wide["sep_sample"][a] == 50 and abs(wide["min_sep"][a] - (6.5 - L)) < 1e-9   # the shift at t0 + 5
    assert scene["poses"][49, a, 2] == 1.0 and scene["poses"][52, a, 2] == 1.0       # forward, then backing: the nose still faces +x
    a, b = _slots(sc, "edge")[0], _slots(sc, "corner")[0]
    for r in rows.values():                                     # the corner of the box at 30 degrees over the other's flank
        hand = (3.5 + DCR * 0.5) - L / 2 * 0.5 - W / 2 * np.cos(np.radians(30.0)) - W / 2
        assert abs(r["min_sep"][a] - hand) < 1e-9 and r["sep_partner"][a] == b and r["sep_sample"][a] == 0
    up, mid_s, low = (_slots(sc, c)[0] for c in ("tie_upper", "tie_middle", "tie_lower"))
    for r in rows.values():                                     # mirror-image partners tie, bit for bit: the lower index
        assert pc.sep(scene["poses"][0, mid_s], scene["poses"][0, up]) == pc.sep(scene["poses"][0, mid_s], scene["poses"][0, low])
        assert r["sep_partner"][mid_s] == up < low and r["sep_partner"][up] == mid_s and r["sep_partner"][low] == mid_s


def test_hand_values(scene):
    sc, wide, P = scene["sc"], scene["rows"][scene["sc"]["cases"][2]], scene["poses"]
    a, b = _slots(sc, "lanes")
    assert abs(wide["min_sep"][a] - 1.10) < 1e-9 and abs(pc.sep(P[37, a], P[37, b]) - 1.10) < 1e-9
    a, b = _slots(sc, "head_on")
    assert abs(cs.HEAD_ON_K0 - 53.09) < 1e-12 and abs(pc.sep(P[0, a], P[0, b]) - cs.HEAD_ON_K0) < 1e-9


def _random_poses(rng, n, spread):
    th = rng.uniform(-np.pi, np.pi, n)
    return np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), np.cos(th), np.sin(th)], axis=1)


def test_separation_is_symmetric_in_bits():
    rng = np.random.default_rng(20250)
    A, B = _random_poses(rng, 2000, 4.0), _random_poses(rng, 2000, 4.0)
    ab = np.array([pc.sep(a, b) for a, b in zip(A, B)])
    ba = np.array([pc.sep(b, a) for a, b in zip(A, B)])
    assert np.array_equal(ab.view(np.int64), ba.view(np.int64))
    assert 200 < (ab == 0.0).sum() < 1800 and (ab >= 0.0).all()   # both branches are well populated


def _corners(p):
    c, s = p[2], p[3]
    return np.array([[p[0] + sx * L / 2 * c - sy * W / 2 * s, p[1] + sx * L / 2 * s + sy * W / 2 * c] for sx, sy in ((1, -1), (1, 1), (-1, 1), (-1, -1))])


def _penetration(a, b):
    """the smallest overlap of the two boxes' projections on the four axes (negative: that axis separates them)"""
    ca, cb = _corners(a), _corners(b)
    depth = INF
    for ax in ((a[2], a[3]), (-a[3], a[2]), (b[2], b[3]), (-b[3], b[2])):
        pa, pb = ca @ np.array(ax), cb @ np.array(ax)
        depth = min(depth, min(pa.max(), pb.max()) - max(pa.min(), pb.min()))
    return depth


def test_overlap_agrees_with_point_sampling():
    """200 x 200 points of one rectangle tested inside the other; pairs whose separation or penetration is below 0.05 m are excluded
    (sampling cannot decide them) and must stay under 10 % for this seed"""
    rng = np.random.default_rng(4711)
    n = 300
    A, B = _random_poses(rng, n, 3.0), _random_poses(rng, n, 3.0)
    u, v = np.meshgrid(np.linspace(-L / 2, L / 2, 200), np.linspace(-W / 2, W / 2, 200))
    excluded = hit = 0
    for a, b in zip(A, B):
        sep, pen = pc.sep(a, b), _penetration(a, b)
        if (sep > 0.0 and sep < 0.05) or (sep == 0.0 and pen < 0.05):
            excluded += 1
            continue
        px, py = b[0] + u * b[2] - v * b[3], b[1] + u * b[3] + v * b[2]          # the points of b
        lx, ly = a[2] * (px - a[0]) + a[3] * (py - a[1]), a[2] * (py - a[1]) - a[3] * (px - a[0])
        inside = bool(((np.abs(lx) <= L / 2) & (np.abs(ly) <= W / 2)).any())
        assert inside == (sep == 0.0), (a, b, sep, pen)
        assert (pen > 0.0) == (sep == 0.0)
        hit += inside
    assert excluded < 0.10 * n, excluded
    assert 50 < hit < n - 50


def test_separation_is_invariant_under_a_rigid_motion():
    rng = np.random.default_rng(99)
    A, B = _random_poses(rng, 500, 6.0), _random_poses(rng, 500, 6.0)
    for a, b in zip(A, B):
        phi, t = rng.uniform(-np.pi, np.pi), rng.uniform(-90.0, 90.0, 2)
        c, s = np.cos(phi), np.sin(phi)
        move = lambda p: np.array([c * p[0] - s * p[1] + t[0], s * p[0] + c * p[1] + t[1], c * p[2] - s * p[3], s * p[2] + c * p[3]])
        assert abs(pc.sep(a, b) - pc.sep(move(a), move(b))) < 1e-9


def test_orders_agree_on_every_index(scene):
    sc = scene["sc"]
    for case in sc["cases"]:
        lib0 = pc.conflicts(*scene["tab"], *scene["clocks"], *case, order=0)
        for k in pc.FIELDS[1:]:
            assert np.array_equal(lib0[k], scene["rows"][case][k]), (case, k)
        assert np.allclose(lib0["min_sep"], scene["rows"][case]["min_sep"], rtol=0.0, atol=1e-9)


def test_poses_are_the_states_oracles(scene, oracle):
    """the position and heading of a slot at a clock are Trajectory::GetState's at the same local time (oracle.sample_states, order 2);
    the pose is that state's box centre, formed by one multiplication and one addition.  (That oracle publishes nothing at or past
    the end of a plan, so the clocks here lie before it; the pose held at the end is checked in the scene's test.)"""
    sc, P = scene["sc"], scene["poses"]
    for case, ks in (("lanes", (0, 37, 99)), ("reversing", (10, 99)), ("starts_after", (0, 50)), ("gear_shift", (20, 49, 50, 52, 80))):
        s = _slots(sc, case)[0]
        plan = sc["slots"][s]
        ends = plan["t_start"] + np.cumsum(plan["piece_nums"] * plan["coeff_dt"])
        for k in ks:
            t = sc["t0"] + float(k) * sc["dt"]
            e = min(int(np.searchsorted(ends, t, side="right")), len(ends) - 1)        # the first segment with end_time > t
            p0 = int(plan["piece_nums"][:e].sum())
            start = plan["t_start"] if e == 0 else ends[e - 1]
            tt = min(max(t - start, 0.0), float(plan["piece_nums"][e] * plan["coeff_dt"][e]))
            st, nv = oracle.sample_states(plan["coeffs"][None, p0:p0 + plan["piece_nums"][e]], [[plan["coeff_dt"][e]]], [plan["piece_nums"][e]],
                                          [plan["singul"][e]], t0=tt, sample_dt=0.01, n_samples=1, filter_singularity=False, order=2)
            assert nv[0] == 1
            x, y, ang = st[0, 0, 1], st[0, 0, 2], st[0, 0, 3]
            cx, cy, c, s_ = P[k, s]
            assert abs(c - np.cos(ang)) < 4e-16 and abs(s_ - np.sin(ang)) < 4e-16
            assert cx == x + DCR * c and cy == y + DCR * s_, (case, k)


def test_the_names_are_declared_exported_and_present(hiplib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dftpav_hip.h")).read()
    declared = set(re.findall(r"\b(dftpav_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in hiplib.EXPORTS and getattr(hiplib.lib(), name) is not None, name
    assert "#define DFTPAV_CONFLICT_MAX_SAMPLES 4096" in hdr and hiplib.CONFLICT_MAX_SAMPLES == 4096 == pc.MAX_SAMPLES
    assert C.sizeof(hiplib._ConflictOutC) == 40 and hiplib.ConflictOut.KEYS == pc.FIELDS


REFUSED = [dict(K=0), dict(K=4097), dict(dt=0.0), dict(dt=-0.1), dict(dt=INF), dict(dt=NAN), dict(t0=INF), dict(t0=NAN),
           dict(margin=-0.1), dict(margin=NAN), dict(margin=1.0, range=0.5), dict(range=INF), dict(range=NAN), dict(margin=INF),
           dict(margin=INF, range=INF)]


def test_python_entry_points_refuse_without_a_library_call(hiplib):
    good = dict(t0=0.0, dt=0.1, K=5, margin=0.5, range=None)
    assert hiplib.conflict_args(**good) == (0.0, 0.1, 5, 0.5, 0.5) and pc.check_args(**good) == (0.5, 0.5)
    pl = hiplib.Planner.__new__(hiplib.Planner)                 # no handle, no planner behind it: a library call would fail otherwise
    pl._p, pl.handle, pl.max_queries = None, None, 3
    for bad in REFUSED:
        kw = dict(good, **bad)
        with pytest.raises(hiplib.DftpavError) as e:
            hiplib.conflict_args(**kw)
        assert e.value.code == hiplib.E_INVALID
        with pytest.raises(hiplib.DftpavError) as e:
            pl.check_conflicts(**kw)
        assert e.value.code == hiplib.E_INVALID
        with pytest.raises(ValueError):
            pc.check_args(**kw)
        if "margin" not in bad and "range" not in bad:
            with pytest.raises(hiplib.DftpavError):
                pl.sample_poses(kw["t0"], kw["dt"], kw["K"])


def test_entry_points_refuse_without_objects(hiplib):
    """no planner, no handle: DFTPAV_E_INVALID from each of the new calls, outputs untouched"""
    Lb = hiplib.lib()
    out = hiplib.ConflictOut(3)
    for a in out.a.values():
        a[...] = 77
    poses = np.full((2, 3, 4), 77.0)
    ms = (C.c_float(7.0), C.c_float(7.0))
    Lb.dftpav_planner_check_conflicts.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    Lb.dftpav_planner_sample_poses.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    Lb.dftpav_conflicts_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    assert Lb.dftpav_planner_check_conflicts(None, 0.0, 0.1, 2, 0.0, 0.0, C.byref(out.c)) == hiplib.E_INVALID
    assert Lb.dftpav_planner_sample_poses(None, 0.0, 0.1, 2, poses.ctypes.data_as(C.c_void_p)) == hiplib.E_INVALID
    assert Lb.dftpav_conflicts_last_ms(None, C.byref(ms[0]), C.byref(ms[1])) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and (poses == 77.0).all() and ms[0].value == 7.0 and ms[1].value == 7.0
