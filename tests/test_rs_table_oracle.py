"""The Reeds-Shepp cost-to-go table of the search oracle (oracle_rs_table): what any such table must satisfy, every entry against the
independent Reeds-Shepp restatement, the three orders against each other, the lookup rule against a numpy restatement, and the
entry points' refusals that need no device."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle_search import pysearch as ps

GEOM = dict(n_yaw=8, extent=2.0, cell=0.5)          # 8 x 9 x 9 = 648 entries


@functools.lru_cache(maxsize=None)
def _table(rho, order=2):
    t = ps.rs_table(rho, order=order, **GEOM)
    t.setflags(write=False)
    return t


def _poses(n_yaw, extent, cell):
    half = int(np.ceil(extent / cell))
    n = 2 * half + 1
    k, j, i = np.meshgrid(np.arange(n_yaw), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([(i - half) * cell, (j - half) * cell, k * (2.0 * np.pi / n_yaw)], -1).astype(np.float64), half, n


@pytest.mark.parametrize("rho", [1.0, 2.5])
def test_table_properties(rho):
    T = _table(rho)
    P, half, n = _poses(**GEOM)
    ny = GEOM["n_yaw"]
    assert T.shape == (ny, n, n) and np.isfinite(T).all()
    assert T[0, half, half] == 0.0
    assert (T >= np.hypot(P[..., 0], P[..., 1]) - 1e-9).all()
    mirror = T[(ny - np.arange(ny)) % ny][:, ::-1, :]                  # T[(n_yaw - k) % n_yaw][n - 1 - j][i]
    assert np.abs(T - mirror).max() <= 1e-9
    assert np.abs(T[0, half, :] - np.abs(P[0, half, :, 0])).max() <= 1e-12     # straight ahead or straight back


def test_every_entry_against_the_independent_restatement(oracle):
    T = _table(1.0)
    P, half, n = _poses(**GEOM)
    fr = P.reshape(-1, 3)
    lit = oracle.reeds_shepp_literal(fr, np.zeros_like(fr), max_cur=1.0, checkl=0.2, max_samples=8)
    assert lit["n_valid"].min() >= 1
    rel = np.abs(T.reshape(-1) - lit["length"]) / np.maximum(1.0, lit["length"])
    assert rel.max() <= 1e-12
    for order in (0, 1):
        other = _table(1.0, order)
        assert (np.abs(other - T) / np.maximum(1.0, T)).max() <= 1e-12


def _numpy_slot(goal, poses, n_yaw, extent, cell):
    """the lookup rule restated: nearest cell in the goal's frame, nearest heading slice, round half away from zero"""
    rnd = lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)          # noqa: E731  (C's round)
    half = int(np.ceil(extent / cell))
    n = 2 * half + 1
    dth = 2.0 * np.pi / n_yaw
    c, s = np.cos(goal[2]), np.sin(goal[2])
    out = []
    for x, y, yaw in poses:
        ddx, ddy = x - goal[0], y - goal[1]
        fi = rnd((c * ddx + s * ddy) / cell) + half
        fj = rnd((c * ddy - s * ddx) / cell) + half
        if not (0 <= fi < n and 0 <= fj < n):
            out.append(-1)
            continue
        k = int(rnd((yaw - goal[2]) / dth)) % n_yaw
        out.append((k * n + int(fj)) * n + int(fi))
    return np.array(out, dtype=np.int64)


def test_lookup_rule():
    ny, ext, cell = 16, 3.0, 0.25
    half, n, dth = 12, 25, 2.0 * np.pi / 16
    goal = np.array([0.0, 0.0, 0.0])                # exact products below: cos 0 = 1, sin 0 = 0
    nan = float("nan")
    poses = np.array([
        [0.0, 0.0, 0.0], [1.0, -0.5, 0.3], [1.0, -0.5, -0.3],          # a negative heading difference
        [0.5, 0.5, 2 * np.pi + 0.4], [0.5, 0.5, -4 * np.pi - 0.4], [0.5, 0.5, 7.0], [0.5, 0.5, -7.0],   # beyond +-2 pi
        [0.125, 0.0, 0.0], [-0.125, 0.0, 0.0], [0.0, 0.375, 0.0], [0.0, -0.375, 0.0],    # exactly half a cell: away from zero
        [0.0, 0.0, 0.5 * dth], [0.0, 0.0, -0.5 * dth], [0.0, 0.0, 1.5 * dth],            # exactly half a slice
        [3.0, 0.0, 0.0], [3.25, 0.0, 0.0], [-3.0, 0.0, 0.0], [-3.25, 0.0, 0.0],          # the last cell and one outside, each side
        [0.0, 3.0, 0.0], [0.0, 3.25, 0.0], [0.0, -3.0, 0.0], [0.0, -3.25, 0.0],
        [3.124, 0.0, 0.0], [3.125, 0.0, 0.0],                                            # rounds in, rounds out
        [nan, 0.0, 0.0], [0.0, nan, 0.0], [0.0, 0.0, nan], [0.0, 0.0, float("inf")], [1e300, 0.0, 0.0],
    ])
    want = _numpy_slot(goal, poses[:-5], ny, ext, cell)
    got = ps.rs_slot(goal, poses, ny, ext, cell)
    assert np.array_equal(got[:-5], want)
    assert (got[-5:] == -1).all()                   # a NaN, an infinite heading, a point far outside: nothing is read
    # spelled out, so that the two restatements cannot be wrong together
    assert got[0] == half * n + half and got[7] == half * n + half + 1 and got[8] == half * n + half - 1
    assert got[2] == (15 * n + (half - 2)) * n + half + 4
    assert got[11] == (1 * n + half) * n + half and got[12] == (15 * n + half) * n + half
    assert got[15] == -1 and got[14] == half * n + 2 * half and got[23] == -1 and got[22] == got[14]
    # a rotated and shifted goal: the pose one cell ahead of the goal and one to its left, a quarter turn on
    g2 = np.array([2.0, -1.0, 0.5 * np.pi])
    p2 = np.array([[2.0 - 0.25, -1.0 + 0.25, np.pi]])
    assert ps.rs_slot(g2, p2, ny, ext, cell)[0] == (4 * n + half + 1) * n + half + 1
    assert np.array_equal(ps.rs_slot(g2, p2, ny, ext, cell), _numpy_slot(g2, p2, ny, ext, cell))
    # one heading slice: every heading reads slice 0; extent 0: one cell, read within half a cell of the goal
    assert ps.rs_slot(goal, [[0.25, 0.0, 2.0]], 1, ext, cell)[0] == half * n + half + 1
    assert ps.rs_slot(goal, [[0.1, -0.1, 0.5], [0.13, 0.0, 0.0], [0.0, -0.13, 0.0]], 4, 0.0, cell).tolist() == [0, -1, -1]
    assert ps.rs_table(1.0, 1, 0.0, 0.25).shape == (1, 1, 1)


def test_entry_points_refuse_without_a_handle(hiplib):
    L = hiplib.lib()
    gp = hiplib.default_rs_heuristic_params()
    assert (gp.enabled, gp.n_yaw, gp.extent, gp.cell, gp.scale) == (0, 72, 15.0, 0.25, 1.0)
    L.dftpav_set_search_rs_heuristic.argtypes = [C.c_void_p, C.c_void_p]
    L.dftpav_rs_table.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dftpav_rs_table_last_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    dims, ms = (C.c_int * 3)(), C.c_float(0.0)
    gp.enabled = 1
    assert L.dftpav_set_search_rs_heuristic(None, C.byref(gp)) == hiplib.E_INVALID
    assert L.dftpav_rs_table(None, 1.0, C.byref(gp), None, dims) == hiplib.E_INVALID
    assert L.dftpav_rs_table_last_ms(None, C.byref(ms), None) == hiplib.E_INVALID
    L.dftpav_default_rs_heuristic_params(None)      # a NULL is ignored
