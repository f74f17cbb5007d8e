"""The hybrid A* search with the Reeds-Shepp term on (dftpav_set_search_rs_heuristic): dftpav_kino_search bit for bit against the
search oracle's entry with oracle_rs_table's table, in order 2, alone and together with the goal field; switched off again it is
the search it was; a batch equals its queries one by one; dftpav_plan_queries searches with it too."""
import functools

import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_goalfield import pygoalfield as pg
from oracle_search import pysearch as ps

pytestmark = pytest.mark.gpu

GEOM = dict(rs_extent=ss.RS_SMALL["extent"], rs_cell=ss.RS_SMALL["cell"])


def _compare(r, o):          # (tests/test_gpu_search.py::_compare)
    for k in o:
        assert np.array_equal(r[k], o[k]), k


def _scenes():
    return ss.small_scenes() + [ss.maze(), ss.parallel_slot()]


def _sp(name):
    budget = {"maze": ss.MAZE_MAX_ITERS, "parallel-slot": ss.PARALLEL_SLOT_MAX_ITERS}.get(name)
    return SearchParams.default().copy(max_iters=budget) if budget else SearchParams.default()


@functools.lru_cache(maxsize=None)
def _table():
    t = ps.rs_table(1.0 / SearchParams.default().max_frontend_cur, order=2, **ss.RS_SMALL)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _oracle(idx, field):
    name, g, res, org, st, en = _scenes()[idx]
    F = pg.search_fields(g, res, org, en[None], inflate_radius=0.0) if field else {}
    return ps.kino_search(g, res, org, st[None], en[None], sp=_sp(name), order=2, rs_tab=_table(), **GEOM, **F)


@pytest.mark.parametrize("field", [False, True], ids=["table", "table+field"])
@pytest.mark.parametrize("idx", range(9), ids=[s[0] for s in _scenes()])
def test_search_with_the_table_matches_the_oracle(hiplib, idx, field):
    name, g, res, org, st, en = _scenes()[idx]
    h = hiplib.Handle()
    h.set_grid_map(g, res, org)
    h.set_search_rs_heuristic(True, **ss.RS_SMALL)
    if field:
        h.set_search_heuristic(True, inflate_radius=0.0)
    got = h.kino_search(st[None], en[None], sp=_sp(name))
    again = h.kino_search(st[None], en[None], sp=_sp(name))
    assert h.rs_table_last_ms()[1] == 1             # built in front of the first launch, kept for the second
    h.close()
    _compare(got, _oracle(idx, field))
    _compare(again, got)
    if name == "parallel-slot":                     # what this is for
        assert got["shot_success"][0] == 1 and got["budget_hit"][0] == 0


def test_off_again_is_the_search_that_never_had_it(hiplib):
    plain, toggled = hiplib.Handle(), hiplib.Handle()
    for name, g, res, org, st, en in ss.small_scenes():
        S, E = np.repeat(st[None], 3, 0), np.repeat(en[None], 3, 0)
        plain.set_grid_map(g, res, org)
        toggled.set_grid_map(g, res, org)
        toggled.set_search_rs_heuristic(True, **ss.RS_SMALL)
        toggled.kino_search(S, E)
        toggled.set_search_rs_heuristic(False)
        a, b = plain.kino_search(S, E), toggled.kino_search(S, E)
        _compare(b, a)
        _compare(a, ps.kino_search(g, res, org, S, E, order=2))
    with pytest.raises(hiplib.DftpavError):
        plain.rs_table_last_ms()                    # the handle that never had it built nothing
    plain.close()
    toggled.close()


def test_a_batch_equals_its_queries_one_by_one(hiplib):
    grid, res, org, start, goals = ss.arena()
    E = goals[[0, 3, 4, 8]]
    S = np.repeat(start[None], len(E), 0)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, rs_tab=_table(), **GEOM)
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_rs_heuristic(True, **ss.RS_SMALL)
    batch = h.kino_search(S, E)
    _compare(batch, o)
    for q in range(len(E)):
        one = h.kino_search(S[q:q + 1], E[q:q + 1])
        for k in o:
            assert np.array_equal(one[k][0], o[k][q]) and np.array_equal(one[k][0], batch[k][q]), (q, k)
    h.close()


def test_plan_queries_searches_with_the_table(hiplib):
    grid, res, org, S, E = ss.arena_plan_queries()
    S, E = S[[0, 3, 4, 8]], E[[0, 3, 4, 8]]
    h = hiplib.Handle()
    h.set_grid_map(grid, res, org)
    h.set_search_rs_heuristic(True, **ss.RS_SMALL)
    s = h.kino_search(S, E)
    pl = hiplib.Planner(h, len(E), 2)
    a = pl.plan(S, E)
    b = pl.plan(S, E)
    pl.close()
    assert h.rs_table_last_ms()[1] == 1
    h.close()
    assert np.array_equal(a["search_status"], s["status"]) and np.array_equal(a["search_iters"], s["iters"])
    assert np.array_equal(a["search_path_len"], s["path_len"])
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=4, rs_tab=_table(), **GEOM)
    assert np.array_equal(s["iters"], o["iters"]) and np.array_equal(s["status"], o["status"])
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
