"""The hybrid A* search with windowed goal fields (dftpav_set_search_heuristic with dftpav_set_search_heuristic_window):
dftpav_kino_search bit for bit against the search oracle, which takes the windowed yardstick pasted into whole-size arrays of UNREACHED
(tests/goal_window_cases.py), in order 2; a margin whose window cuts the maze's detours off and one that holds both gaps; switched
off again it is the whole-map heuristic, and without the heuristic it is the plain search; a batch equals its queries one by one;
dftpav_plan_queries searches with it; together with the Reeds-Shepp table; the argument checks."""
import functools

import numpy as np
import pytest

import goal_window_cases as gw
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_goalfield import pygoalfield as pg
from oracle_search import pysearch as ps

pytestmark = pytest.mark.gpu

# The maze: start (-15, -5), goal (3, 0), walls at x = -8 .. -7 (open above y = 10) and x = -1 .. 0 (open below y = -10).  2 m: the
# window is cells (0, 64, 128, 64), y = -7.2 .. 5.4 -- neither gap; the start's cell is unreached, the term 0 there.  12 m: the window
# is cells (0, 0, 192, 192), y = -20 .. 18.2 -- both gaps.  The oracle, run on the CPU before these were fixed: 2 m ends on the budget
# (2000 pops, 5337 nodes, as the plain search), 12 m inside it (56 pops; 472 nodes at r = 0, 487 at r = 0.5).
MARGINS = (2.0, 12.0)


def _compare(r, o):          # (tests/test_gpu_search.py::_compare)
    for k in o:
        assert np.array_equal(r[k], o[k]), k


def _scenes():
    return ss.small_scenes() + [ss.maze()]


def _sp(name):
    budget = {"maze": ss.MAZE_MAX_ITERS, "parallel-slot": ss.PARALLEL_SLOT_MAX_ITERS}.get(name)
    return SearchParams.default().copy(max_iters=budget) if budget else SearchParams.default()


@functools.lru_cache(maxsize=None)
def _oracle(idx, r, margin):
    name, g, res, org, st, en = _scenes()[idx]
    F = gw.search_fields(g, res, org, st[None], en[None], r, margin)
    return ps.kino_search(g, res, org, st[None], en[None], sp=_sp(name), order=2, **F)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("r", [0.0, 0.5])
@pytest.mark.parametrize("idx", range(8), ids=[s[0] for s in _scenes()])
def test_search_with_windowed_fields_matches_the_oracle(hiplib, idx, r, margin):
    name, g, res, org, st, en = _scenes()[idx]
    o = _oracle(idx, r, margin)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    h.set_search_heuristic(True, inflate_radius=r)
    h.set_search_heuristic_window(margin)
    got = h.kino_search(st[None], en[None], sp=_sp(name))
    h.close()
    print(name, r, margin, "pops", int(got["iters"][0]), "nodes", int(got["nodes_used"][0]), "budget_hit", int(got["budget_hit"][0]))
    _compare(got, o)
    assert got["budget_hit"][0] == o["budget_hit"][0]
    if name == "maze":          # both branches: the small window leaves the search the plain one, the large one ends it early
        assert o["budget_hit"][0] == (1 if margin == MARGINS[0] else 0)
        assert got["shot_success"][0] == (0 if margin == MARGINS[0] else 1)


def test_off_again_is_what_it_was(hiplib):
    """margin -1 after a windowed search: the whole-map heuristic's bits; a window set with the heuristic off: the plain search's"""
    plain, whole, toggled, never_on = hiplib.Handle(), hiplib.Handle(), hiplib.Handle(), hiplib.Handle()
    for name, g, res, org, st, en in ss.small_scenes():
        S, E = np.repeat(st[None], 3, 0), np.repeat(en[None], 3, 0)
        for h in (plain, whole, toggled, never_on):
            h.set_grid_map(g, res, org)
        whole.set_search_heuristic(True, inflate_radius=0.5)
        toggled.set_search_heuristic(True, inflate_radius=0.5)
        toggled.set_search_heuristic_window(2.0)
        toggled.kino_search(S, E)
        toggled.set_search_heuristic_window(-1.0)
        never_on.set_search_heuristic_window(2.0)          # the heuristic itself stays off
        a, b = whole.kino_search(S, E), toggled.kino_search(S, E)
        _compare(b, a)
        _compare(a, ps.kino_search(g, res, org, S, E, order=2, **pg.search_fields(g, res, org, E, inflate_radius=0.5)))
        c, d = plain.kino_search(S, E), never_on.kino_search(S, E)
        _compare(d, c)
        _compare(c, ps.kino_search(g, res, org, S, E, order=2))
        with pytest.raises(hiplib.DftpavError):
            never_on.goal_field_last_ms()          # nothing was built
        toggled.set_search_heuristic(False)
    for h in (plain, whole, toggled, never_on):
        h.close()


def test_a_batch_equals_its_queries_one_by_one(hiplib):
    grid, res, org, start, goals = ss.arena()
    E = goals[[0, 3, 4, 8]]
    S = np.repeat(start[None], len(E), 0)
    F = gw.search_fields(grid, res, org, S, E, 0.0, 5.0)
    assert len(F["fields"]) == 4 and (F["fields"] != gw.U).any(axis=(1, 2)).all()
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, **F)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_heuristic(True)
    h.set_search_heuristic_window(5.0)
    batch = h.kino_search(S, E)
    _compare(batch, o)
    for q in range(len(E)):
        one = h.kino_search(S[q:q + 1], E[q:q + 1])
        for k in o:
            assert np.array_equal(one[k][0], o[k][q]) and np.array_equal(one[k][0], batch[k][q]), (q, k)
    h.close()


def test_plan_queries_searches_with_windowed_fields(hiplib):
    grid, res, org, S, E = ss.arena_plan_queries()
    S, E = S[[0, 3, 4, 8]], E[[0, 3, 4, 8]]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_heuristic(True, inflate_radius=0.5)
    h.set_search_heuristic_window(5.0)
    s = h.kino_search(S, E)
    pl = hiplib.Planner(h, len(E), 2)
    a = pl.plan(S, E)
    assert pl.info()["stage_ms"][0] > 0.0
    b = pl.plan(S, E)
    pl.close()
    h.close()
    assert np.array_equal(a["search_status"], s["status"]) and np.array_equal(a["search_iters"], s["iters"])
    assert np.array_equal(a["search_path_len"], s["path_len"])
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, **gw.search_fields(grid, res, org, S, E, 0.5, 5.0))
    assert np.array_equal(s["iters"], o["iters"]) and np.array_equal(s["status"], o["status"])
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_window_and_reeds_shepp_table_together(hiplib):
    name, g, res, org, st, en = ss.parallel_slot()
    tab = ps.rs_table(1.0 / SearchParams.default().max_frontend_cur, order=2, **ss.RS_SMALL)
    F = gw.search_fields(g, res, org, st[None], en[None], 0.0, 2.0)
    o = ps.kino_search(g, res, org, st[None], en[None], sp=_sp(name), order=2, rs_tab=tab, rs_extent=ss.RS_SMALL["extent"],
                       rs_cell=ss.RS_SMALL["cell"], **F)
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    h.set_search_rs_heuristic(True, **ss.RS_SMALL)
    h.set_search_heuristic(True, inflate_radius=0.0)
    h.set_search_heuristic_window(2.0)
    got = h.kino_search(st[None], en[None], sp=_sp(name))
    h.close()
    _compare(got, o)


def test_argument_checks_leave_the_handle_usable(hiplib):
    name, g, res, org, st, en = ss.wall_gap()
    h = hiplib.Handle()
    with pytest.raises(hiplib.DftpavError) as e:
        h.set_search_heuristic_window(2.0)          # no map
    assert e.value.code == hiplib.E_INVALID
    h.set_grid_map(g, res, org)
    h.set_search_heuristic(True)
    h.set_search_heuristic_window(2.0)
    for margin in (float("nan"), float("inf")):          # refused, and the margin in force stays
        with pytest.raises(hiplib.DftpavError) as e:
            h.set_search_heuristic_window(margin)
        assert e.value.code == hiplib.E_INVALID
    F = gw.search_fields(g, res, org, st[None], en[None], 0.0, 2.0)
    _compare(h.kino_search(st[None], en[None]), ps.kino_search(g, res, org, st[None], en[None], order=2, **F))
    h.set_search_heuristic_window(float("-inf"))          # any negative margin: off
    F = pg.search_fields(g, res, org, en[None])
    _compare(h.kino_search(st[None], en[None]), ps.kino_search(g, res, org, st[None], en[None], order=2, **F))
    h.close()
