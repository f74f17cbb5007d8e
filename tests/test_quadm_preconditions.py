"""What the cases of tests/test_gpu_quadm_instances.py need in order to mean anything, from the restatement alone (no GPU): the corridor
active with H = 3 and H = 5 and both differing from H = 4, help_eps moving the gradient, gear_opt = 0 leaving zero junction gradients
and unmoved junction variables, solves of more than 8 x memory iterations, a second scene whose
solves change with the first scene's half-planes, the plan's kind for every forced shape, the instance each layout selects, and the
term count of tests/quad_cases.py against the restatement's own costs."""
import numpy as np
import pytest

import quad_cases as qc
import test_gpu_quadm_instances as tq
from dftpav_amd import scenarios as sc


@pytest.mark.parametrize("case,what,seed,instance", tq.GENERIC)
def test_generic_cases_are_not_vacuous(hiplib, oracle, case, what, seed, instance):
    base, s = tq.generic_scene(case, what, seed)
    p = tq.params_of(hiplib, s)
    tq.generic_precondition(oracle, p, base, s, what, seed)
    assert qc.quadm_instance(s) == instance and qc.quadm_instance(base) == instance.replace("false", "true")


@pytest.mark.parametrize("case,seed,instance", tq.GEAR)
def test_gear_opt_off_cases_are_not_vacuous(hiplib, oracle, monkeypatch, case, seed, instance):
    for order in (2, 1):
        p, s, _, _, _ = tq.gear_reference(hiplib, oracle, case, seed, order)
    assert qc.quadm_instance(s) == instance
    for shape, kind in (("quad", 5), ("team", 0), ("wave", 1)):
        monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
        assert qc.plan_readout(hiplib, s, p)[:2] == [1, kind]


@pytest.mark.parametrize("mem", tq.MEMS)
@pytest.mark.parametrize("case,seed,instance", tq.SHORT)
def test_short_history_cases_wrap_the_ring(hiplib, oracle, monkeypatch, case, seed, instance, mem):
    p, s, _ = tq.short_reference(hiplib, oracle, case, seed, mem)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    assert qc.quadm_instance(s) == instance and qc.plan_readout(hiplib, s, p)[:2] == [1, 5]


def test_one_segment_with_a_short_memory_lands_in_the_several_segment_kernel(hiplib, oracle, monkeypatch):
    p, s, _ = tq.short_reference(hiplib, oracle, "8", 11, 3)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    assert qc.plan_readout(hiplib, s, p)[:2] == [1, 5]
    assert qc.plan_readout(hiplib, s, tq.params_of(hiplib, s))[:2] == [1, 3]
    monkeypatch.delenv("DFTPAV_REF_SHAPE")
    assert qc.plan_readout(hiplib, s, p)[1] == 0  # left alone a batch this small stays in the TEAM shape


def test_a_stale_corridor_copy_would_show(hiplib, oracle):
    tq.upload_reference(hiplib, oracle)


def test_workgroup_shape_cases(hiplib, oracle, monkeypatch):
    p, s, _ = tq.shapes_reference(hiplib, oracle)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    monkeypatch.setenv("DFTPAV_REF_SLOTS", "1")
    monkeypatch.setenv("DFTPAV_REF_SLICE", "5")
    for waves in (1, 2, 4):
        monkeypatch.setenv("DFTPAV_REF_QUAD_WAVES", str(waves))
        for B in (1, 2, 3, 5, 8):
            out = qc.plan_readout(hiplib, s, p, B=B)
            assert out[:3] == [1, 5, 64 * waves] and out[4] == 1 and out[5] == 5, out


def test_active_terms_over_several_segments_agree_with_the_restatements_costs(hiplib, oracle):
    """quad_cases.active_terms: no active term exactly where the restatement's corridor and feasibility costs are both zero; on one
    segment it is the count tests/test_gpu_quad_parked.py always used"""
    s = qc.gear_scene("3-2-4-3", 6, 7)
    p = tq.params_of(hiplib, s)
    x0, x1 = tq.points(oracle, p, s, 7)
    some = 0
    for x in (x0, x1):
        for b in range(s.B):
            cnt, (cor, feas) = qc.active_terms(oracle, p, s, b, x[b], order=2)
            assert cnt.shape == (12, 8) and (cnt.sum() == 0) == (cor == 0.0 and feas == 0.0), (b, cnt.sum(), cor, feas)
            some += int(cnt.sum() > 0)
    assert some > 0
    s1 = sc.make_scenario([8], [-1], 6, 9, 2, seed=49, n_obs=30)
    p1 = tq.params_of(hiplib, s1, max_backward_vel=0.5)
    cnt, (cor, feas) = qc.active_terms(oracle, p1, s1, 1, oracle.OracleProblem(p1, s1, 1).x0())
    assert cnt.sum() > 0 and feas > 0.0
