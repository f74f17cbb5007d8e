"""The cost of a plan term by term (dftpav_batch_cost_terms) and the residual-penalty filter (dftpav_planner_set_penalty_filter),
the part that needs no device: the preconditions of the scenes tests/test_gpu_cost_terms.py evaluates -- by the oracle alone --,
the association of the cost's sum on the oracle, the gate rule restated on crafted arrays, the caps of the planner tests chosen
from the oracle chain's own numbers, and the refusals of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import limits_cases as lc
import terms_cases as tc


def _oracle_rows(p, s, x, idx):
    return [tc.oracle_terms(p, s, int(b), x[int(b)]) for b in idx]


@pytest.mark.parametrize("name", ["team", "gear", "sur", "generic", "wave", "quad"])
def test_scenes_exercise_the_terms(oracle, hiplib, name):
    """at every perturbed point a GPU test evaluates, on the trajectories it compares with the oracle: a trajectory with an active
    corridor term, one with an active feasibility term, and among the moving cars one with an active surround term; the smoothness
    and time terms are positive everywhere.  A scene that stops exercising a term fails here."""
    p, s, xs = tc.scene(name)
    moving = s.surround is not None
    want = {"team": 0, "gear": 0, "sur": 0, "generic": 0, "wave": 1, "quad": 3}[name]
    assert tc.reference_plan(s, p, 4 if moving else 0) == want
    assert moving == (name in ("sur", "wave"))
    idx = range(s.B) if s.B <= 4 else np.linspace(0, s.B - 1, 16).astype(int)
    sigmas = tc.SIGMAS if len(xs) == len(tc.SIGMAS) else (0.3,)
    for sg, x in zip(sigmas, xs):
        T = np.array([t for _, t in _oracle_rows(p, s, x, idx)])
        assert (T[:, tc.SMOOTH] > 0).all() and (T[:, tc.TIME] > 0).all() and np.isfinite(T).all()
        if not moving:
            assert not T[:, tc.SURROUND].any()
        if sg == 0.0:
            continue
        assert (T[:, tc.CORRIDOR] > 0).any(), (name, sg)
        assert (T[:, tc.FEAS] > 0).any(), (name, sg)
        if moving:
            assert (T[:, tc.SURROUND] > 0).any(), (name, sg)


@pytest.mark.parametrize("name", ["team", "sur", "generic"])
def test_the_terms_recompose_to_the_cost_on_the_oracle(oracle, hiplib, name):
    """sm + time + sum over the segments of ((c0 + c1) + c2) is the value eval returned -- the association the GPU tests reuse.
    (The oracle keeps the five chained sums, not a segment's operands: on the scenes of one gear segment the two are the same
    numbers, a chain of one term from 0.0.)"""
    p, s, xs = tc.scene(name)
    assert s.layout.M == 1
    for x in xs:
        for b in range(s.B):
            f, t = tc.oracle_terms(p, s, b, x[b])
            assert tc.recompose(t, t[None]) == f, (name, b)
            assert np.array_equal(tc.chained(t[None]), t)


def test_gear_terms_bound_the_cost_on_the_oracle(oracle, hiplib):
    """with a gear shift the penalty is chained segment by segment, so the five totals alone do not give the bits of the cost; they
    are still its terms: non-negative, and their plain sum within a few roundings of it"""
    p, s, xs = tc.scene("gear")
    assert s.layout.M == 2
    for x in xs:
        for b in range(s.B):
            f, t = tc.oracle_terms(p, s, b, x[b])
            assert (t >= 0).all() and abs(float(np.sum(t)) - f) <= 8 * np.spacing(f)


def test_gate_rule_on_crafted_arrays(hiplib):
    """the numpy restatement of the gate against the expectations written out by hand"""
    for caps, terms, flags_in, rejected in tc.gate_cases():
        fo, rj = tc.gate_rule(terms, caps, flags_in)
        assert np.array_equal(rj, rejected), (caps.corridor, rj)
        assert np.array_equal(fo, ((flags_in != 0) | (rejected != 0)).astype(np.int32))
    up = float(np.nextafter(2.5, np.inf))
    assert up > 2.5 and tc.gate_rule([[0, 0, up, 0, 0]], hiplib.PenaltyCaps(2.5, 0.0, 0.0), [0])[1][0] == 1
    assert tc.gate_rule([[0, 0, -0.0, -0.0, -0.0]], hiplib.PenaltyCaps(0.0, 0.0, 0.0), [0])[1][0] == 0


def _filtered(T, caps):
    return tc.gate_rule(T.reshape(-1, 5), caps, np.zeros(T.shape[0] * T.shape[1], np.int32))[1].reshape(T.shape[:2])


def test_caps_of_the_planner_tests_hit_the_three_cases(oracle, hiplib):
    """on the oracle chain's numbers alone: with CAPS some query changes its winner to a dearer restart, some query loses every
    restart, some query keeps its winner -- and the tables the GPU test reads are those"""
    ch = lc.chain()
    T, scen = tc.chain_terms()
    caps = hiplib.PenaltyCaps(**tc.CAPS)
    rej = _filtered(T, caps)
    changed, none, kept = {}, {}, {}
    for q, e in enumerate(ch["per"]):
        if e is None:
            assert scen[q] is None and not T[q].any()
            continue
        r = e["solve"]
        w0 = lc.select(r["final_cost"], r["success"], e["collision"])
        w1 = lc.select(r["final_cost"], r["success"], e["collision"] | rej[q])
        if w1 < 0 <= w0:
            none[q] = w0
        elif w1 != w0:
            assert r["final_cost"][w1] > r["final_cost"][w0]
            changed[q] = (w0, w1)
        else:
            kept[q] = w0
    assert changed == tc.CHANGED and none == tc.NO_VALID and kept == tc.KEPT
    assert changed and none and kept
    assert not T[:, :, tc.SURROUND].any()                       # no moving obstacles on that scene
    # all +inf rejects nothing: every term of the chain is finite
    assert np.isfinite(T).all() and not _filtered(T, hiplib.PenaltyCaps()).any()


def test_new_entry_points_refuse_null_and_need_a_device(hiplib):
    L = hiplib.lib()
    vp = C.c_void_p
    L.dftpav_batch_cost_terms.argtypes = [vp, vp, vp, vp]
    L.dftpav_planner_set_penalty_filter.argtypes = [vp, vp]
    L.dftpav_planner_last_cost_terms.argtypes = [vp, vp, vp]
    L.dftpav_debug_penalty_gate.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    buf = np.full(16, 77.0)
    ibuf = np.full(16, 77, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(vp)
    caps = hiplib.PenaltyCaps(1.0, 1.0, 1.0)
    assert L.dftpav_batch_cost_terms(None, ptr(buf), ptr(buf), ptr(buf)) == hiplib.E_INVALID
    assert L.dftpav_planner_set_penalty_filter(None, C.byref(caps)) == hiplib.E_INVALID
    assert L.dftpav_planner_set_penalty_filter(None, None) == hiplib.E_INVALID
    assert L.dftpav_planner_last_cost_terms(None, ptr(buf), ptr(ibuf)) == hiplib.E_INVALID
    assert L.dftpav_debug_penalty_gate(None, 1, ptr(buf), C.byref(caps), ptr(ibuf), ptr(ibuf), ptr(ibuf)) == hiplib.E_INVALID
    assert (buf == 77.0).all() and (ibuf == 77).all()
    assert hiplib.PenaltyCaps().corridor == float("inf") and C.sizeof(hiplib.PenaltyCaps) == 24
    assert (hiplib.TERM_SMOOTH, hiplib.TERM_TIME, hiplib.TERM_CORRIDOR, hiplib.TERM_SURROUND, hiplib.TERM_FEAS, hiplib.COST_TERMS) == (0, 1, 2, 3, 4, 5)
    for name in ("dftpav_batch_cost_terms", "dftpav_planner_set_penalty_filter", "dftpav_planner_last_cost_terms", "dftpav_debug_penalty_gate"):
        assert name in hiplib.EXPORTS
    # with a handle the hook also refuses NULL arrays, NULL caps and caps that are negative or NaN, before anything touches the device;
    # without a usable device no handle exists at all: dftpav_create is DFTPAV_E_NO_DEVICE, as tests/test_abi.py expects
    try:
        h = hiplib.Handle()
    except hiplib.DftpavError as e:
        assert e.code == hiplib.E_NO_DEVICE
        return
    gate = L.dftpav_debug_penalty_gate
    assert gate(h._h, 1, None, C.byref(caps), ptr(ibuf), ptr(ibuf), ptr(ibuf)) == hiplib.E_INVALID
    assert gate(h._h, 1, ptr(buf), None, ptr(ibuf), ptr(ibuf), ptr(ibuf)) == hiplib.E_INVALID
    assert gate(h._h, 1, ptr(buf), C.byref(caps), None, ptr(ibuf), ptr(ibuf)) == hiplib.E_INVALID
    assert gate(h._h, 1, ptr(buf), C.byref(caps), ptr(ibuf), None, ptr(ibuf)) == hiplib.E_INVALID
    for bad in (hiplib.PenaltyCaps(-1.0, 1.0, 1.0), hiplib.PenaltyCaps(1.0, float("nan"), 1.0), hiplib.PenaltyCaps(1.0, 1.0, -0.5)):
        assert gate(h._h, 1, ptr(buf), C.byref(bad), ptr(ibuf), ptr(ibuf), ptr(ibuf)) == hiplib.E_INVALID
    assert (buf == 77.0).all() and (ibuf == 77).all()
    h.close()
