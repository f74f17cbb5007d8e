"""The QUAD shape for several gear segments (dftpav_amd/csrc/solver_ref4m.hip) on the instances and branches the gear-shift cases of
tests/test_gpu_reference_order.py leave out.  The kernel is built four times, ref4m_kernel<FAST, TAIL>: launch_solver_quad picks FAST =
(H == 4 && help_eps == 0), reference_order_plan TAIL = 1 when n == 33 and 16 otherwise; those cases run <true, 1> and <true, 16> with
gear_opt = 1 and an L-BFGS memory of 40 or the default.  Here:

  1. the two generic instances <false, 1> and <false, 16>: H = 3, H = 5, and help_eps = 1e-3 with H = 4;
  2. gear_opt = 0 (the junction gradients written as zeros) in the QUAD, TEAM and WAVE shapes and in device order;
  3. q4m_two_loop with histories of 3, 4, 5 and 9 pairs (below one register block of kMB = 4, no multiple of it, a ring that wraps many
     times), also with true divisions; one segment with a memory of 3, which the one-segment kernel refuses (M = 1 inside ref4m_kernel);
  4. a second upload on the same batch (the kernel's own corridor copy, q4m_corridor_kernel);
  5. workgroups of 1, 2 and 4 waves over batches that leave rows of a wave empty.

Bar: every evaluated cost and gradient, and every field of every solve (final_cost, x, status, iters, evals, hist_sum, success),
BIT-EQUAL to the restatement of the reference with correctly rounded cos / sin (oracle/pyoracle.py, order 2; order 0 for the one
segment, which calls neither).  Every case of kind 5 asserts that the plan says 5 (dftpav_debug_reference_plan), names the instance that
selects in its id (checked against quad_cases.quadm_instance), compares evaluations at x0 and at x0 + N(0, 0.3), then a solve with the
hand-over of the last trajectories to the WAVE shape and one without.

Shapes (quad_cases.gear_scene: K = 5, Kd = 7, 30 obstacles, at most 8 trajectories -- the smallest that still have every structure):
5-4-6 (n = 33: TAIL 1, no shared sweep tables), 6-5-5 (n = 35: TAIL 16, the tables of segments 1 and 2 shared), 3-2-4-3 (n = 29, four
segments, the tables of segments 0 and 3 shared).  What a case needs in order to mean anything -- an active corridor, a gradient that
help_eps moves, a ring that has wrapped, half-planes whose replacement shows -- is asserted from the restatement alone (the precondition functions below; tests/
test_quadm_preconditions.py runs them without a GPU).  The seeds were picked on the CPU for those assertions.
"""
import numpy as np
import pytest

import quad_cases as qc
from dftpav_amd import scenarios as sc
from quad_cases import KEYS

pytestmark = pytest.mark.gpu

SIGMA = 0.3  # the perturbed evaluation point: x0 + N(0, SIGMA^2), drawn by default_rng(the scene's seed)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def points(oracle, p, s, seed, order=2):
    """the restatement's x0 [B][n] and the perturbed point"""
    x0 = np.stack([oracle.OracleProblem(p, s, b, order=order).x0() for b in range(s.B)])
    return x0, x0 + np.random.default_rng(seed).normal(0.0, SIGMA, x0.shape)


def params_of(hiplib, s, **fields):
    p = hiplib.default_params()
    s.apply_resolution(p)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def junction0(s):
    """index of the first junction variable (positions, then angles: the last 3 (M - 1) entries of x)"""
    return s.layout.n_vars - 3 * (s.layout.M - 1)


def check_quadm(hiplib, oracle, monkeypatch, p, s, seed, instance, env=(), order=2, want=None, threads=None):
    """Kind 5 on the device against the restatement: the plan, the instance, evaluations at x0 and x0 + N(0, 0.3), a solve with the
    hand-over and one without.  Returns (the evaluations' gradients [2][B][n], the solve)."""
    assert qc.quadm_instance(s) == instance
    want = want if want is not None else oracle.solve_batch(p, s, nthreads=8, order=order)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    out = qc.plan_readout(hiplib, s, p)
    assert out[0] == 1 and out[1] == 5, "the plan did not pick the QUAD shape for several segments: %s" % out
    if threads is not None:
        assert out[2] == threads, out
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    grads = []
    for x in points(oracle, p, s, seed, order):
        f, g = bt.eval(x)
        print("f", f)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=order).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (b, f[b], fo, np.abs(g[b] - go).max())
        grads.append(g)
    for hand in (-1, 0):  # -1: a batch alone on the device leaves its last B / 2 trajectories to the WAVE shape; 0: the QUAD launch finishes all
        bt.set_hand_over(hand)
        r = bt.solve()
        print("hand-over", hand, "iters", r["iters"], "status", r["status"])
        for k in KEYS:
            assert np.array_equal(r[k], want[k]), (hand, k)
    bt.close()
    h.close()
    return grads, r


# ---- 1. the generic instances

# (layout, scene seed): the seeds at which the dropped plane (H = 3) and the added one (H = 5) are active at the perturbed point for
# every trajectory of the batch -- at most seeds the fourth plane of a rectangle is met by no trajectory, and H = 3 equals H = 4
GENERIC = [("5-4-6", "H3", 155, "<false, 1>"), ("5-4-6", "H5", 5, "<false, 1>"), ("5-4-6", "eps", 5, "<false, 1>"),
           ("6-5-5", "H3", 122, "<false, 16>"), ("6-5-5", "H5", 122, "<false, 16>"), ("6-5-5", "eps", 122, "<false, 16>")]
GENERIC_B = 5


def generic_scene(case, what, seed):
    base = qc.gear_scene(case, GENERIC_B, seed)
    if what == "H3":
        return base, qc.three_planes(base)
    if what == "H5":
        return base, qc.extra_planes(base, 5)
    s = qc.gear_scene(case, GENERIC_B, seed)
    s.help_eps = 1e-3
    return base, s


def generic_precondition(oracle, p, base, s, what, seed):
    """From the restatement: with H = 3 / H = 5 the corridor cost at the perturbed point is above 0 for every trajectory and the cost
    differs from the H = 4 scene's; with help_eps the gradient differs from the help_eps = 0 one."""
    _, x1 = points(oracle, p, base, seed)
    for b in range(s.B):
        o4, o = oracle.OracleProblem(p, base, b, order=2), oracle.OracleProblem(p, s, b, order=2)
        (f4, g4), (f, g) = o4.eval(x1[b]), o.eval(x1[b])
        if what == "eps":
            assert not np.array_equal(g, g4), b
        else:
            assert o.cost_terms()[2] > 0.0, (b, o.cost_terms())
            assert f != f4, (b, f)


@pytest.mark.parametrize("case,what,seed,instance", GENERIC, ids=["%s-%s-ref4m_kernel%s" % (c, w, i.replace(", ", ",")) for c, w, _, i in GENERIC])
def test_generic_instances(hiplib, oracle, monkeypatch, case, what, seed, instance):
    """ref4m_kernel<false, 1> (5-4-6) and <false, 16> (6-5-5): H as a run-time value (three half-planes: the fourth dropped; five: one
    added as tests/quad_cases.py: extra_planes adds it), 5 H + 4 terms per point, and help_eps = 1e-3 in the curvature term at H = 4."""
    base, s = generic_scene(case, what, seed)
    p = params_of(hiplib, s)
    generic_precondition(oracle, p, base, s, what, seed)
    check_quadm(hiplib, oracle, monkeypatch, p, s, seed, instance)


# ---- 2. gear_opt = 0

GEAR = [("5-4-6", 5, "<true, 1>"), ("3-2-4-3", 7, "<true, 16>")]
GEAR_B = 5


def gear_reference(hiplib, oracle, case, seed, order):
    """(p, s, x0, x1, solves) of a gear_opt = 0 case in `order`, and from the restatement: the junction entries of every gradient are
    exactly 0.0, the junction variables of the solved x those of x0 -- and with gear_opt = 1 neither holds"""
    def make():
        s = qc.gear_scene(case, GEAR_B, seed)
        p = params_of(hiplib, s, gear_opt=0)
        x0, x1 = points(oracle, p, s, seed, order)
        want = oracle.solve_batch(p, s, nthreads=8, order=order)
        j0 = junction0(s)
        for x in (x0, x1):
            for b in range(s.B):
                _, g = oracle.OracleProblem(p, s, b, order=order).eval(x[b])
                assert (g[j0:] == 0.0).all() and not np.signbit(g[j0:]).any(), (b, g[j0:])
                assert np.abs(g[:j0]).max() > 0.0
        assert np.array_equal(want["x"][:, j0:], x0[:, j0:])
        assert (want["iters"] >= 2).all(), want["iters"]
        p1 = params_of(hiplib, s)  # what the switch switches off
        _, g1 = oracle.OracleProblem(p1, s, 0, order=order).eval(x1[0])
        assert (g1[j0:] != 0.0).all(), g1[j0:]
        return p, s, x0, x1, want
    return _cached(("gear", case, seed, order), make)


def _junctions_untouched(s, grads, r, x0):
    j0 = junction0(s)
    for g in grads:
        assert (g[:, j0:] == 0.0).all() and not np.signbit(g[:, j0:]).any(), g[:, j0:]
    assert np.array_equal(r["x"][:, j0:], x0[:, j0:])


@pytest.mark.parametrize("case,seed,instance", GEAR, ids=["%s-ref4m_kernel%s" % (c, i.replace(", ", ",")) for c, _, i in GEAR])
def test_gear_opt_off_in_the_quad_shape(hiplib, oracle, monkeypatch, case, seed, instance):
    """solver_ref4m.hip: the else arm of `if (P.gear_opt)` -- the junction positions and angles keep a zero gradient, so no solve moves
    them."""
    p, s, x0, _, want = gear_reference(hiplib, oracle, case, seed, 2)
    grads, r = check_quadm(hiplib, oracle, monkeypatch, p, s, seed, instance, want=want)
    _junctions_untouched(s, grads, r, x0)


@pytest.mark.parametrize("shape,kind", [("team", 0), ("wave", 1)])
@pytest.mark.parametrize("case,seed,instance", GEAR, ids=[c for c, _, _ in GEAR])
def test_gear_opt_off_in_the_team_and_wave_shapes(hiplib, oracle, monkeypatch, case, seed, instance, shape, kind):
    """solver_ref.hip: `if (!P.gear_opt)` of the TEAM / WAVE kernel (the WAVE shape from the ring: one persistent workgroup, slices of 9
    evaluations), the same scenes and the same assertions; the plan says which shape ran."""
    p, s, x0, x1, want = gear_reference(hiplib, oracle, case, seed, 2)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", shape)
    if shape == "wave":
        monkeypatch.setenv("DFTPAV_REF_SLOTS", "1")
        monkeypatch.setenv("DFTPAV_REF_SLICE", "9")
    out = qc.plan_readout(hiplib, s, p)
    assert out[0] == 1 and out[1] == kind, out
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.set_order(hiplib.ORDER_REFERENCE)
    grads = []
    for x in (x0, x1):
        f, g = bt.eval(x)
        for b in range(s.B):
            fo, go = oracle.OracleProblem(p, s, b, order=2).eval(x[b])
            assert f[b] == fo and np.array_equal(g[b], go), (shape, b)
        grads.append(g)
    r = bt.solve()
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), (shape, k)
    _junctions_untouched(s, grads, r, x0)
    bt.close()
    h.close()


@pytest.mark.parametrize("case,seed,instance", GEAR, ids=[c for c, _, _ in GEAR])
def test_gear_opt_off_in_device_order(hiplib, oracle, case, seed, instance):
    """solver.hip: `if (P.gear_opt)` of the device-order kernel.  The bar of tests/test_gpu_parity.py for its gear-shift cases
    (test_eval_matches_oracle, cfg 2; test_solve_matches_oracle): evaluations bit-equal to the restatement in device order (order 1) and
    within 1e-11 (cost) / 1e-10 (gradient) relative of the literal one (order 0); whole solves bit-equal to order 1."""
    p, s, x0, x1, want = gear_reference(hiplib, oracle, case, seed, 1)
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, s.layout, s.B)
    bt.upload(s)
    grads = []
    for x in (x0, x1):
        f, g = bt.eval(x)
        for b in range(s.B):
            fd, gd = oracle.OracleProblem(p, s, b, order=1).eval(x[b])
            assert f[b] == fd and np.array_equal(g[b], gd), b
            fl, gl = oracle.OracleProblem(p, s, b, order=0).eval(x[b])
            assert abs(f[b] - fl) <= 1e-11 * abs(fl)
            assert np.abs(g[b] - gl).max() <= 1e-10 * np.abs(gl).max()
        grads.append(g)
    r = bt.solve()
    for k in KEYS:
        assert np.array_equal(r[k], want[k]), k
    _junctions_untouched(s, grads, r, x0)
    bt.close()
    h.close()


# ---- 3. short histories

MEMS = [3, 4, 5, 9]
SHORT = [("5-4-6", 5, "<true, 1>"), ("6-5-5", 122, "<true, 16>")]
SHORT_B = 5
RING = (("DFTPAV_REF_SLOTS", 1), ("DFTPAV_REF_QUAD_WAVES", 1), ("DFTPAV_REF_SLICE", 7))  # one persistent wave, slices of 7 evaluations


def short_reference(hiplib, oracle, case, seed, mem):
    """(p, s, solves) with lbfgs_mem_size = mem; from the restatement: some trajectory runs more than 8 x mem iterations (the ring of
    stored pairs has wrapped many times), every trajectory stores a pair"""
    def make():
        s = qc.gear_scene(case, SHORT_B, seed) if "-" in case else sc.make_scenario([int(case)], [1], 5, 7, SHORT_B, seed=seed, n_obs=30)
        p = params_of(hiplib, s, lbfgs_mem_size=mem)
        want = oracle.solve_batch(p, s, nthreads=8, order=2 if "-" in case else 0)
        assert want["iters"].max() > 8 * mem, (mem, want["iters"])
        assert (want["hist_sum"] > 0).all(), want["hist_sum"]
        return p, s, want
    return _cached(("short", case, seed, mem), make)


@pytest.mark.parametrize("exact_div", [0, 1], ids=["rcp", "exact_div"])
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("case,seed,instance", SHORT, ids=["%s-ref4m_kernel%s" % (c, i.replace(", ", ",")) for c, _, i in SHORT])
def test_short_histories(hiplib, oracle, monkeypatch, case, seed, instance, mem, exact_div):
    """q4m_two_loop reads the history in register blocks of kMB = 4 pairs, two blocks per trip, `jl` wrapping modulo the memory: 3 pairs
    (less than one block: a block holds a pair more than once), 4, 5 and 9 (a last block partly beyond the bound), at the one-element
    tail (5-4-6) and the 48-step chain (6-5-5).  One persistent wave with slices of 7 evaluations: the history and iSLOWDIV pass through
    a suspended record.  exact_div: the same with true divisions from the first iteration on (DFTPAV_REF_EXACT_DIV=1)."""
    p, s, want = short_reference(hiplib, oracle, case, seed, mem)
    env = RING + ((("DFTPAV_REF_EXACT_DIV", 1),) if exact_div else ())
    check_quadm(hiplib, oracle, monkeypatch, p, s, seed, instance, env=env, want=want)


def test_one_segment_with_a_memory_below_the_one_segment_kernels_block(hiplib, oracle, monkeypatch):
    """ref4m_kernel<true, 16> with M = 1: the one-segment kernel refuses lbfgs_mem_size < kQB = 8 (reference_order_quad_supported), so
    under DFTPAV_REF_SHAPE=quad one segment of 8 pieces with a memory of 3 falls through to the kernel for several segments -- no
    junction lanes, no neighbour segment.  Against order 0 (no junction angle, so no cos / sin); with the default memory the same layout
    takes kind 3."""
    seed = 11
    p, s, want = short_reference(hiplib, oracle, "8", seed, 3)
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    assert qc.plan_readout(hiplib, s, params_of(hiplib, s))[1] == 3
    check_quadm(hiplib, oracle, monkeypatch, p, s, seed, "<true, 16>", env=RING, order=0, want=want)


# ---- 4. a second upload on the same batch

UPLOAD_SEEDS, UPLOAD_B = (5, 155), 5


def upload_reference(hiplib, oracle):
    """(p, the two 5-4-6 scenes, their solves); from the restatement: with the first scene's half-planes left in place of the second's
    -- what a stale copy of the corridor would be -- every evaluation and every solve of the second scene comes out different"""
    def make():
        scenes = [qc.gear_scene("5-4-6", UPLOAD_B, sd) for sd in UPLOAD_SEEDS]
        p = params_of(hiplib, scenes[0])
        wants = [oracle.solve_batch(p, s, nthreads=8, order=2) for s in scenes]
        s2 = scenes[1]
        stale = sc.Scenario("stale", s2.layout, s2.K, s2.Kd, s2.B, s2.ini_states, s2.fin_states, s2.inner_pts, s2.init_Ts, scenes[0].corridor)
        for x in points(oracle, p, s2, UPLOAD_SEEDS[1]):
            for b in range(s2.B):
                assert oracle.OracleProblem(p, stale, b, order=2).eval(x[b])[0] != oracle.OracleProblem(p, s2, b, order=2).eval(x[b])[0], b
        assert (oracle.solve_batch(p, stale, nthreads=8, order=2)["final_cost"] != wants[1]["final_cost"]).all()
        return p, scenes, wants
    return _cached("upload", make)


def test_second_upload_reaches_the_corridor_copy(hiplib, oracle, monkeypatch):
    """ref4m_kernel<true, 1>: the kernel reads its own copy of the corridor, [B][4 H][Kmax + 1][16], made by q4m_corridor_kernel.  A
    second scene of the same layout (another seed: other half-planes, waypoints, boundary states) uploaded into the same batch: every
    evaluation and solve is the restatement's of the second scene, and none is the first scene's."""
    p, scenes, wants = upload_reference(hiplib, oracle)
    assert qc.quadm_instance(scenes[0]) == "<true, 1>"
    monkeypatch.setenv("DFTPAV_REF_SHAPE", "quad")
    assert qc.plan_readout(hiplib, scenes[0], p)[:2] == [1, 5]
    h = hiplib.Handle(p)
    bt = hiplib.Batch(h, scenes[0].layout, UPLOAD_B)
    seen = []
    for s, seed, want in zip(scenes, UPLOAD_SEEDS, wants):
        bt.upload(s)
        bt.set_order(hiplib.ORDER_REFERENCE)  # (the first time; the batch keeps its order and plan afterwards)
        fs = []
        for x in points(oracle, p, s, seed):
            f, g = bt.eval(x)
            for b in range(s.B):
                fo, go = oracle.OracleProblem(p, s, b, order=2).eval(x[b])
                assert f[b] == fo and np.array_equal(g[b], go), (seed, b)
            fs.append(f)
        rs = []
        for hand in (-1, 0):
            bt.set_hand_over(hand)
            r = bt.solve()
            for k in KEYS:
                assert np.array_equal(r[k], want[k]), (seed, hand, k)
            rs.append(r)
        seen.append((fs, rs))
    (f_a, r_a), (f_b, r_b) = seen
    for fa, fb in zip(f_a, f_b):
        assert (fa != fb).all()
    for ra, rb in zip(r_a, r_b):
        assert (ra["final_cost"] != rb["final_cost"]).all() and (ra["x"] != rb["x"]).any(axis=1).all()
    bt.close()
    h.close()


# ---- 5. workgroup shapes

SHAPES_SEED = 7


def shapes_reference(hiplib, oracle):
    """the 3-2-4-3 scene of eight trajectories and its solves; a batch of B < 8 is its first B trajectories (make_scenario draws
    trajectory b from (seed, b) alone at these sizes)"""
    def make():
        s = qc.gear_scene("3-2-4-3", 8, SHAPES_SEED)
        p = params_of(hiplib, s)
        want = oracle.solve_batch(p, s, nthreads=8, order=2)
        assert (want["iters"] > 5).all(), want["iters"]  # every trajectory is suspended and resumed at slices of 5
        return p, s, want
    return _cached("shapes", make)


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_workgroup_shapes(hiplib, oracle, monkeypatch, waves, B):
    """ref4m_kernel<true, 16>, 3-2-4-3: workgroups of 1, 2 and 4 waves (DFTPAV_REF_QUAD_WAVES; the plan's thread count says it was
    taken), ONE workgroup for the whole batch (DFTPAV_REF_SLOTS=1) with slices of 5 evaluations, so every row pops its trajectories from
    the ring; batches of 1, 2, 3, 5 and 8 leave rows of a wave, and whole waves of a workgroup, empty."""
    p, s8, want8 = shapes_reference(hiplib, oracle)
    s = s8.subset(np.arange(B))
    small = qc.gear_scene("3-2-4-3", B, SHAPES_SEED)
    assert all(np.array_equal(getattr(s, k), getattr(small, k)) for k in ("ini_states", "fin_states", "inner_pts", "init_Ts", "corridor"))
    want = {k: want8[k][:B] for k in KEYS}
    env = (("DFTPAV_REF_QUAD_WAVES", waves), ("DFTPAV_REF_SLOTS", 1), ("DFTPAV_REF_SLICE", 5))
    check_quadm(hiplib, oracle, monkeypatch, p, s, SHAPES_SEED, "<true, 16>", env=env, want=want, threads=64 * waves)
