"""The search oracle's entry with a goal field (oracle_kino_search_field): without a field, and with a field of zeros, it returns
the bits of oracle_kino_search; with the goal's field the maze that runs the plain search's budget out ends on a free shot."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_goalfield import pygoalfield as pg
from oracle_search import pysearch as ps


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("scene", ss.small_scenes(), ids=lambda s: s[0])
def test_no_field_and_a_field_of_zeros_change_nothing(scene):
    name, g, res, org, st, en = scene
    plain = ps.kino_search(g, res, org, st[None], en[None], order=2)
    _same(plain, ps.kino_search(g, res, org, st[None], en[None], order=2, field_entry=True))
    zeros = np.zeros((1,) + g.shape, dtype=np.int32)
    _same(plain, ps.kino_search(g, res, org, st[None], en[None], order=2, fields=zeros, unit=res * pg.DEFAULT_SCALE / 5.0))
    # a query without a field (field_of -1) beside one with: the first is the plain search
    both = ps.kino_search(g, res, org, np.stack([st, st]), np.stack([en, en]), order=2, fields=zeros, field_of=[-1, 0], unit=1.0)
    for k in plain:
        assert np.array_equal(both[k][:1], plain[k]), k


def test_the_field_brings_the_maze_inside_its_budget():
    name, g, res, org, st, en = ss.maze()
    sp = SearchParams.default().copy(max_iters=ss.MAZE_MAX_ITERS)
    plain = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2)
    assert plain["budget_hit"][0] == 1 and plain["iters"][0] == ss.MAZE_MAX_ITERS          # today's documented result
    F = pg.search_fields(g, res, org, en[None], inflate_radius=0.0)
    assert F["unit"] == pg.DEFAULT_SCALE * res / 5.0 and F["field_of"].tolist() == [0]
    with_field = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, **F)
    assert with_field["budget_hit"][0] == 0 and with_field["shot_success"][0] == 1 and with_field["status"][0] == 2
    assert with_field["iters"][0] < plain["iters"][0]
    # the path ends at the goal, not where the budget left the search
    n = int(with_field["path_len"][0])
    assert np.array_equal(with_field["paths"][0, n - 1, :2], en[:2])
    m = int(plain["path_len"][0])
    assert np.hypot(*(plain["paths"][0, m - 1, :2] - en[:2])) > 5.0


def test_search_fields_share_a_field_per_goal_cell():
    name, g, res, org, st, en = ss.wall_gap()
    ens = np.stack([en, en + [0.01, 0.0, 0.3, 0.0], en + [1.0, 0.0, 0.0, 0.0], [1e3, 0.0, 0.0, 0.0]])
    F = pg.search_fields(g, res, org, ens)
    assert F["field_of"].tolist() == [0, 0, 1, -1] and F["fields"].shape == (2,) + g.shape


def test_scale_bounds_the_field_term_by_the_straight_line_in_free_space():
    name, g, res, org = ss.field_free(41, 37)
    f = pg.goal_field(g, res, org, [ss.cell_centre(20, 18)])["field"][0].astype(np.float64)
    yy, xx = np.mgrid[0:37, 0:41]
    euclid = np.hypot(xx - 20, yy - 18) * res
    assert (f * (pg.DEFAULT_SCALE * res / 5.0) <= euclid * (1 + 1e-12)).all()
