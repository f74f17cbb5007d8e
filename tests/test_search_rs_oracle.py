"""The search oracle's entry with a Reeds-Shepp table (oracle_kino_search_heu): without a table, and with a table of zeros, it
returns the bits of oracle_kino_search_field; on the parallel slot the table brings the search to its free shot in fewer pops."""
import numpy as np
import pytest

from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import SearchParams
from oracle_goalfield import pygoalfield as pg
from oracle_search import pysearch as ps

GEOM = dict(rs_extent=ss.RS_SMALL["extent"], rs_cell=ss.RS_SMALL["cell"])


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _sp(name):
    budget = {"maze": ss.MAZE_MAX_ITERS, "parallel-slot": ss.PARALLEL_SLOT_MAX_ITERS}.get(name)
    return SearchParams.default().copy(max_iters=budget) if budget else SearchParams.default()


@pytest.mark.parametrize("scene", ss.small_scenes() + [ss.maze()], ids=lambda s: s[0])
def test_no_table_and_a_table_of_zeros_change_nothing(scene):
    name, g, res, org, st, en = scene
    sp = _sp(name)
    zeros = np.zeros((16, 25, 25))
    F = pg.search_fields(g, res, org, en[None], inflate_radius=0.0)
    for kw in (dict(field_entry=True), F):          # without a field, and with the goal's
        base = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, **kw)
        _same(base, ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, heu_entry=True, **kw))
        _same(base, ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, rs_tab=zeros, rs_scale=1.0, **GEOM, **kw))
    plain = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2)
    _same(plain, ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, heu_entry=True))


def test_the_table_brings_the_parallel_slot_to_its_shot_in_fewer_pops():
    name, g, res, org, st, en = ss.parallel_slot()
    sp = _sp(name)
    T = ps.rs_table(1.0 / sp.max_frontend_cur, **ss.RS_SMALL)
    plain = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2)
    with_table = ps.kino_search(g, res, org, st[None], en[None], sp=sp, order=2, rs_tab=T, **GEOM)
    print("parallel slot: pops", int(plain["iters"][0]), "->", int(with_table["iters"][0]), " nodes", int(plain["nodes_used"][0]), "->",
          int(with_table["nodes_used"][0]))
    assert plain["iters"][0] > 0                    # the shot from the start collides
    for r in (plain, with_table):
        assert r["status"][0] == 2 and r["shot_success"][0] == 1 and r["budget_hit"][0] == 0
        assert np.array_equal(r["paths"][0, int(r["path_len"][0]) - 1, :2], en[:2])
    assert with_table["iters"][0] < plain["iters"][0]
