"""dftpav_rs_table: the device's Reeds-Shepp cost-to-go table (rstable.hip) bit for bit against oracle_rs_table in order 2, at sizes
that end inside a wave and inside a workgroup, at two turning radii; one build per key; the refusals."""
import functools

import numpy as np
import pytest

from dftpav_amd.pods import SearchParams
from oracle_search import pysearch as ps

pytestmark = pytest.mark.gpu

GEOMS = [dict(n_yaw=1, extent=0.0, cell=0.25),       # one entry
         dict(n_yaw=4, extent=1.0, cell=0.5),        # 4 x 5 x 5
         dict(n_yaw=16, extent=3.0, cell=0.25),      # 16 x 25 x 25: rows of 25, 10 000 entries -- no multiple of 64 or of 256
         dict(n_yaw=7, extent=2.1, cell=0.3)]        # 7 x 15 x 15: extent no multiple of the cell
MAX_CURS = [SearchParams.default().max_frontend_cur, 0.3]


@functools.lru_cache(maxsize=None)
def _oracle(gi, ci):
    t = ps.rs_table(1.0 / MAX_CURS[ci], order=2, **GEOMS[gi])
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("ci", range(2), ids=["default-cur", "cur-0.3"])
@pytest.mark.parametrize("gi", range(4), ids=["one", "5x5x4", "25x25x16", "15x15x7"])
def test_table_is_bit_equal_to_the_oracle(hiplib, gi, ci):
    h = hiplib.Handle()
    assert h.rs_table(MAX_CURS[ci], fetch=False, **GEOMS[gi]) == _oracle(gi, ci).shape
    with pytest.raises(hiplib.DftpavError):
        h.rs_table_last_ms()                                    # the shape alone built nothing
    got = h.rs_table(MAX_CURS[ci], **GEOMS[gi])
    h.close()
    assert got.shape == _oracle(gi, ci).shape
    assert np.array_equal(got.view(np.uint64), _oracle(gi, ci).view(np.uint64))


def test_one_build_per_key(hiplib):
    h = hiplib.Handle()
    a = h.rs_table(MAX_CURS[0], **GEOMS[2])
    ms, builds = h.rs_table_last_ms()
    assert builds == 1 and ms > 0.0
    b = h.rs_table(MAX_CURS[0], **GEOMS[2])
    assert h.rs_table_last_ms()[1] == 1                         # kept
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    builds = 1
    for ci, geom in ((1, GEOMS[2]), (1, dict(GEOMS[2], n_yaw=8)), (1, dict(GEOMS[2], n_yaw=8, cell=0.5)),
                     (1, dict(GEOMS[2], n_yaw=8, cell=0.5, extent=2.0))):      # each part of the key
        t = h.rs_table(MAX_CURS[ci], **geom)
        builds += 1
        assert h.rs_table_last_ms()[1] == builds
    assert np.array_equal(t, ps.rs_table(1.0 / MAX_CURS[1], order=2, n_yaw=8, cell=0.5, extent=2.0))
    c = h.rs_table(MAX_CURS[0], **GEOMS[2])                     # back: built again, the same bits
    assert h.rs_table_last_ms()[1] == builds + 1 and np.array_equal(a.view(np.uint64), c.view(np.uint64))
    h.close()


def test_refusals_leave_the_handle_usable(hiplib):
    h = hiplib.Handle()
    inf, nan = float("inf"), float("nan")
    bad = [dict(n_yaw=0), dict(n_yaw=-3), dict(cell=0.0), dict(cell=-0.25), dict(cell=nan), dict(cell=inf), dict(extent=-1.0),
           dict(extent=nan), dict(extent=inf)]
    for kw in bad:
        for call in (lambda: h.rs_table(1.0, fetch=False, **kw), lambda: h.rs_table(1.0, **kw),
                     lambda: h.set_search_rs_heuristic(True, **kw)):
            with pytest.raises(hiplib.DftpavError) as e:
                call()
            assert e.value.code == hiplib.E_INVALID, kw
    for scale in (-1.0, nan, inf):
        with pytest.raises(hiplib.DftpavError) as e:
            h.set_search_rs_heuristic(True, scale=scale)
        assert e.value.code == hiplib.E_INVALID
    for cur in (0.0, -1.0, nan, inf):
        with pytest.raises(hiplib.DftpavError) as e:
            h.rs_table(cur, **GEOMS[1])
        assert e.value.code == hiplib.E_INVALID
    # 72 x 683 x 683 doubles are 256.2 MiB; 72 x 681 x 681 fit, and their shape is given without a build
    for call in (lambda: h.rs_table(1.0, n_yaw=72, extent=341.0, cell=1.0, fetch=False), lambda: h.set_search_rs_heuristic(True, extent=341.0, cell=1.0),
                 lambda: h.rs_table(1.0, n_yaw=72, extent=1e9, cell=1e-3, fetch=False)):
        with pytest.raises(hiplib.DftpavError) as e:
            call()
        assert e.value.code == hiplib.E_UNSUPPORTED
    assert h.rs_table(1.0, n_yaw=72, extent=340.0, cell=1.0, fetch=False) == (72, 681, 681)
    with pytest.raises(hiplib.DftpavError):
        h.rs_table_last_ms()                                    # nothing was built by any of this
    assert np.array_equal(h.rs_table(MAX_CURS[0], **GEOMS[1]), _oracle(1, 0))
    h.close()
