"""The hybrid A* search with the obstacle-aware heuristic on (dftpav_set_search_heuristic): dftpav_kino_search bit for bit against
the search oracle's entry with the goal fields of oracle_goalfield/, in order 2; switched off again it is the search it was; a batch
equals its queries one by one; dftpav_plan_queries searches with it too; the argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_goalfield import pygoalfield as pg
from oracle_search import pysearch as ps

pytestmark = pytest.mark.gpu

SEARCH_COLS = ("search_status", "search_iters", "search_path_len")


def _compare(r, o):          # (tests/test_gpu_search.py::_compare)
    for k in o:
        assert np.array_equal(r[k], o[k]), k


def _scenes():
    return ss.small_scenes() + [ss.maze()]


def _sp(name):
    return SearchParams.default().copy(max_iters=ss.MAZE_MAX_ITERS) if name == "maze" else SearchParams.default()


@functools.lru_cache(maxsize=None)
def _oracle(idx, r):
    name, g, res, org, st, en = _scenes()[idx]
    F = pg.search_fields(g, res, org, en[None], inflate_radius=r)
    return ps.kino_search(g, res, org, st[None], en[None], sp=_sp(name), order=2, **F)


@pytest.mark.parametrize("r", [0.0, 0.5])
@pytest.mark.parametrize("idx", range(8), ids=[s[0] for s in _scenes()])
def test_search_with_the_heuristic_matches_the_oracle(hiplib, idx, r):
    name, g, res, org, st, en = _scenes()[idx]
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    h.set_search_heuristic(True, inflate_radius=r)
    got = h.kino_search(st[None], en[None], sp=_sp(name))
    h.close()
    _compare(got, _oracle(idx, r))
    if name == "maze":          # the behaviour this is for: inside the budget that the plain search runs out
        assert got["budget_hit"][0] == 0 and got["shot_success"][0] == 1


def test_off_again_is_the_search_that_never_had_it(hiplib):
    plain, toggled = hiplib.Handle(), hiplib.Handle()
    for name, g, res, org, st, en in ss.small_scenes():
        S, E = np.repeat(st[None], 3, 0), np.repeat(en[None], 3, 0)
        plain.set_grid_map(g, res, org)
        toggled.set_grid_map(g, res, org)
        toggled.set_search_heuristic(True, inflate_radius=0.5)
        toggled.kino_search(S, E)
        toggled.set_search_heuristic(False)
        a, b = plain.kino_search(S, E), toggled.kino_search(S, E)
        _compare(b, a)
        _compare(a, ps.kino_search(g, res, org, S, E, order=2))
    plain.close()
    toggled.close()


def test_a_batch_equals_its_queries_one_by_one(hiplib):
    grid, res, org, start, goals = ss.arena()
    E = goals[[0, 3, 4, 8]]
    S = np.repeat(start[None], len(E), 0)
    F = pg.search_fields(grid, res, org, E)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, **F)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_heuristic(True)
    batch = h.kino_search(S, E)
    _compare(batch, o)
    for q in range(len(E)):
        one = h.kino_search(S[q:q + 1], E[q:q + 1])
        for k in o:
            assert np.array_equal(one[k][0], o[k][q]) and np.array_equal(one[k][0], batch[k][q]), (q, k)
    h.close()


def test_plan_queries_searches_with_the_heuristic(hiplib):
    grid, res, org, S, E = ss.arena_plan_queries()
    S, E = S[[0, 3, 4, 8]], E[[0, 3, 4, 8]]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_heuristic(True, inflate_radius=0.5)
    s = h.kino_search(S, E)
    pl = hiplib.Planner(h, len(E), 2)
    a = pl.plan(S, E)
    assert pl.info()["stage_ms"][0] > 0.0
    b = pl.plan(S, E)
    pl.close()
    h.close()
    assert np.array_equal(a["search_status"], s["status"]) and np.array_equal(a["search_iters"], s["iters"])
    assert np.array_equal(a["search_path_len"], s["path_len"])
    F = pg.search_fields(grid, res, org, E, inflate_radius=0.5)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, **F)
    assert np.array_equal(s["iters"], o["iters"]) and np.array_equal(s["status"], o["status"])
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_argument_checks_leave_the_handle_usable(hiplib):
    name, g, res, org, st, en = ss.wall_gap()
    h = hiplib.Handle()
    for call in (lambda: h.set_search_heuristic(True), lambda: h.goal_field(en[None, :2], 0.0, fetch=False)):      # no map
        with pytest.raises(hiplib.DftpavError) as e:
            call()
        assert e.value.code == hiplib.E_INVALID
    h.set_grid_map(g, res, org)
    plain = h.kino_search(st[None], en[None])
    bad = (lambda: h.set_search_heuristic(True, inflate_radius=-0.1), lambda: h.set_search_heuristic(True, inflate_radius=float("inf")),
           lambda: h.set_search_heuristic(True, scale=float("nan")), lambda: h.set_search_heuristic(True, scale=-1.0),
           lambda: h.goal_field(en[None, :2], -1.0), lambda: h.goal_field(en[None, :2], float("nan")))
    for call in bad:
        with pytest.raises(hiplib.DftpavError) as e:
            call()
        assert e.value.code == hiplib.E_INVALID
    with pytest.raises(hiplib.DftpavError):
        h.goal_field_last_ms()                                  # nothing was built
    _compare(h.kino_search(st[None], en[None]), plain)          # the refused calls switched nothing on
    h.set_search_heuristic(True)
    F = pg.search_fields(g, res, org, en[None])
    _compare(h.kino_search(st[None], en[None]), ps.kino_search(g, res, org, st[None], en[None], order=2, **F))
    gp = hiplib.default_goal_field_params()
    assert gp.enabled == 0 and gp.inflate_radius == 0.0 and gp.scale == pg.DEFAULT_SCALE
    h.close()
