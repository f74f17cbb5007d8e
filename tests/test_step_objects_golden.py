"""The step oracles that stand on oracle_shared/ref_objects.h (replan check, publisher, limits, clearance, collision re-check, state
read-out) against tests/golden/step_objects.npz: the inputs recorded there replayed through the current oracles at orders 0, 1 and
2, every output array equal to the recorded one BYTE FOR BYTE (NaN and -0.0 count).  The fixture was written by the oracles as they
were before they shared that header (tests/golden/README.md): it pins them to themselves, not to the reference.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_golden_step_objects", os.path.join(GOLDEN, "make_golden_step_objects.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_output_of_the_step_oracles_is_byte_equal_to_the_recorded_one(oracle, maker):
    rec = dict(np.load(os.path.join(GOLDEN, "step_objects.npz")))
    want = maker.recorded(rec)
    got = maker.replay(rec)
    assert sorted(got) == sorted(want) and len(want) > 500
    for entry in ("replan", "publish", "limits", "clearance", "validate", "states"):
        for order in maker.ORDERS:
            assert any(k.startswith("out_" + entry) and "_o%d" % order in k for k in want), (entry, order)
    bad = [k for k in sorted(want)
           if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or np.ascontiguousarray(got[k]).tobytes() != want[k].tobytes()]
    assert not bad, bad
