"""The CPU yardstick of the distance field and the clearance check (oracle_clearance/): the fast field against the literal brute
force, its symmetries, the clearance in orders 0 and 2 on the oracle chain's plans, its tie to the collision re-check, and the new
entry points' refusals without a device."""
import ctypes as C

import numpy as np
import pytest

import limits_cases as lc
from oracle_clearance import pyclearance as pc

FAR = pc.FAR


def _grid(rng, sy, sx, density):
    return np.where(rng.random((sy, sx)) < density, 80, 0).astype(np.uint8)


def test_fast_field_equals_the_brute_force():
    rng = np.random.default_rng(11)
    n = 0
    for sy, sx in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 40), (40, 3), (17, 33), (40, 40), (31, 29)):
        for density in (0.0, 0.01, 0.1, 0.3, 0.7, 1.0):
            g = _grid(rng, sy, sx, density)
            assert np.array_equal(pc.field(g), pc.field_brute(g)), (sy, sx, density)
            n += 1
        one = np.zeros((sy, sx), dtype=np.uint8)                  # a single occupied cell, at a corner and somewhere inside
        for iy, ix in ((0, 0), (sy - 1, sx - 1), (sy // 2, sx // 3)):
            one[...] = 0
            one[iy, ix] = 80
            f = pc.field(one)
            yy, xx = np.mgrid[0:sy, 0:sx]
            assert np.array_equal(f, (yy - iy) ** 2 + (xx - ix) ** 2), (sy, sx, iy, ix)
            assert np.array_equal(f, pc.field_brute(one))
    assert n == 54
    # values other than 80 are free (GridMapND::OCCUPIED alone counts)
    g = np.full((5, 6), 79, dtype=np.uint8)
    assert (pc.field(g) == FAR).all() and (pc.field_brute(g) == FAR).all()
    assert (pc.field(np.full((5, 6), 80, dtype=np.uint8)) == 0).all()


def test_field_is_symmetric_under_flips_and_transpose():
    rng = np.random.default_rng(12)
    for sy, sx, density in ((23, 37, 0.02), (40, 40, 0.2), (64, 65, 0.005)):
        g = _grid(rng, sy, sx, density)
        f = pc.field(g)
        assert np.array_equal(pc.field(g[::-1]), f[::-1])
        assert np.array_equal(pc.field(g[:, ::-1]), f[:, ::-1])
        assert np.array_equal(pc.field(np.ascontiguousarray(g.T)), f.T)


def test_clearance_orders_agree_and_zero_means_collision(oracle):
    """On the oracle chain's plans: orders 0 and 2 give the same min_d2 / arg (a plan where they do not is printed with its
    arguments, as tests/test_gpu_plan_queries.py does for atan2, and left to order 2); min_d2 == 0 exactly when the collision
    re-check reports a collision, and then arg is its first sample."""
    ch = lc.chain()
    grid, res, org, _, _ = ch["scene"]
    differ, seen, zero = [], 0, 0
    for q, e in enumerate(ch["per"]):
        if e is None:
            continue
        lay = e["layout"]
        r2 = pc.check_batch(grid, res, org, lay.singuls, lay.piece_nums, e["coeffs"], e["dts"], lc.CHECK_DT, order=2)
        r0 = pc.check_batch(grid, res, org, lay.singuls, lay.piece_nums, e["coeffs"], e["dts"], lc.CHECK_DT, order=0)
        for b in range(lc.R):
            seen += 1
            if r0["min_d2"][b] != r2["min_d2"][b] or r0["arg"][b] != r2["arg"][b]:
                differ.append((q, b, int(r0["min_d2"][b]), int(r0["arg"][b]), int(r2["min_d2"][b]), int(r2["arg"][b])))
        col, first = e["collision"], e["first"]                 # (oracle.validate_trajectories, order 2, the same samples)
        assert np.array_equal(r2["min_d2"] == 0, col != 0), q
        assert np.array_equal(r2["arg"][col != 0], first[col != 0]), q
        assert (r2["arg"] >= 0).all() and (r2["min_d2"] < FAR).all() and (r2["n_samples"] > 0).all()
        assert np.array_equal(r2["clearance"], res * np.sqrt(r2["min_d2"].astype(np.float64)))
        zero += int((r2["min_d2"] == 0).sum())
    print("restarts", seen, "colliding", zero, "orders 0 and 2 differ at (query, restart, d2_0, arg_0, d2_2, arg_2):", differ)
    assert seen >= 40 and len(differ) < seen


def test_clearance_of_crafted_plans():
    """a straight drive along +x beside a one-cell obstacle: the minimum and where it is first reached follow by hand"""
    res, org = 0.5, (-10.0, -10.0)
    g = np.zeros((40, 80), dtype=np.uint8)
    g[30, 40] = 80                                               # the cell centred at (10.0, 5.0)
    co = np.zeros((1, 2, 6, 2))
    for p in range(2):
        co[0, p, 0] = (2.0 * p, 0.0)
        co[0, p, 1] = (1.0, 0.0)                                 # 1 m/s along +x from (0, 0), two pieces of 2 s
    r = pc.check_batch(g, res, org, [1], [2], co, [[2.0]], 0.05)
    # outline: x in [px + 1.015 - 2.44, px + 1.015 + 2.44], y in [-0.95, 0.95]; the nearest outline cell row is y = 1.0 (iy 22), the
    # obstacle's row iy 30: 8 cells; the front reaches x = 10.0 (ix 40 from round((x + 10) / 0.5)) only past the plan's end
    t, k, xs = 0.0, 0, []
    while t < 4.0:
        xs.append(t + 1.015 + 2.44)
        t += 0.05
        k += 1
    assert r["n_samples"][0] == k
    best = min((40 - int(np.round((x + 10.0) / 0.5))) ** 2 + 64 for x in xs)
    first = next(i for i, x in enumerate(xs) if (40 - int(np.round((x + 10.0) / 0.5))) ** 2 + 64 == best)
    assert r["min_d2"][0] == best and r["arg"][0] == first and r["clearance"][0] == 0.5 * np.sqrt(float(best))
    # wholly off the grid, no segment, an empty map
    far = co.copy()
    far[0, :, 0, 0] += 1000.0
    r = pc.check_batch(g, res, org, [1], [2], far, [[2.0]], 0.05)
    assert r["min_d2"][0] == FAR and r["arg"][0] == -1 and np.isposinf(r["clearance"][0]) and r["n_samples"][0] == k
    r = pc.check_table(g, res, org, [0], [[0]], [[0]], [[0.0]], np.zeros((1, 2, 6, 2)), 0.05)
    assert r["min_d2"][0] == FAR and r["arg"][0] == -1 and np.isposinf(r["clearance"][0]) and r["n_samples"][0] == 0
    r = pc.check_batch(np.zeros_like(g), res, org, [1], [2], co, [[2.0]], 0.05)
    assert r["min_d2"][0] == FAR and r["arg"][0] == -1 and np.isposinf(r["clearance"][0])


def test_entry_points_refuse_without_objects(hiplib):
    """no handle, batch or planner: DFTPAV_E_INVALID from each of the new calls, outputs untouched; without a device no handle exists"""
    L = hiplib.lib()
    out = hiplib.ClearanceOut(3)
    for a in out.a.values():
        a[...] = 77
    d2 = np.full(4, 77, dtype=np.int32)
    ms = (C.c_float(7.0), C.c_float(7.0))
    L.dftpav_grid_distance_field.argtypes = [C.c_void_p, C.c_void_p]
    L.dftpav_batch_check_clearance.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.dftpav_planner_check_clearance.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.dftpav_planner_set_clearance_filter.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.dftpav_planner_last_clearance.argtypes = [C.c_void_p, C.c_void_p]
    L.dftpav_clearance_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    assert L.dftpav_grid_distance_field(None, d2.ctypes.data_as(C.c_void_p)) == hiplib.E_INVALID
    assert L.dftpav_batch_check_clearance(None, 0.05, C.byref(out.c)) == hiplib.E_INVALID
    assert L.dftpav_planner_check_clearance(None, 0.05, C.byref(out.c)) == hiplib.E_INVALID
    assert L.dftpav_planner_set_clearance_filter(None, 1.0, 0.05) == hiplib.E_INVALID
    assert L.dftpav_planner_set_clearance_filter(None, -1.0, 0.05) == hiplib.E_INVALID
    assert L.dftpav_planner_last_clearance(None, C.byref(out.c)) == hiplib.E_INVALID
    assert L.dftpav_clearance_last_ms(None, C.byref(ms[0]), C.byref(ms[1])) == hiplib.E_INVALID
    assert all((a == 77).all() for a in out.a.values()) and (d2 == 77).all() and ms[0].value == 7.0 and ms[1].value == 7.0
    assert hiplib.DIST_FAR == FAR == 2 ** 31 - 1
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(hiplib.DftpavError) as e:
            hiplib.Handle(hiplib.default_params())
        assert e.value.code == hiplib.E_NO_DEVICE
