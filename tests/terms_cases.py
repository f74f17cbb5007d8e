"""Shared by the cost-terms tests (not a test module): the scenes of tests/test_gpu_cost_terms.py with the points they are
evaluated at, the oracle's terms there (OracleProblem.eval + cost_terms, order 2), the association of the cost's sum, the gate
rule restated in numpy with its crafted arrays, and the terms of every restart of the oracle chain behind dftpav_plan_queries
(tests/limits_cases.py) with the caps the planner tests filter on."""
import ctypes as C

import numpy as np

from dftpav_amd import capi
from dftpav_amd import scenarios as sc
from dftpav_amd.pods import FrontendParams, LayoutSpec
from oracle import pyoracle as po

SMOOTH, TIME, CORRIDOR, SURROUND, FEAS = range(5)
INF, NAN = float("inf"), float("nan")
N_WAVE = 1281  # five trajectories per CU of a 256-CU device and one more: the smallest batch that leaves the TEAM shape

_SCENES = {}


def _two_pieces(B, moving, n_hyp=4):
    return sc.make_scenario([2], [1], 8, 8, B, seed=5, n_obs=150, n_hyp=n_hyp, with_moving=moving,
                            **(dict(start_centre=(-38.0, 5.0)) if moving else {}))


# x0 (where the seeded scenes have no active corridor term), and the two perturbed points the preconditions are asserted at
SIGMAS = (0.0, 0.3, 1.0)


def _build(name):
    if name == "team":        # one segment of 2 pieces
        return _two_pieces(4, False), SIGMAS
    if name == "gear":        # a gear shift, 3 + 2 pieces
        return sc.make_scenario([3, 2], [1, -1], 8, 8, 4, seed=5, n_obs=150, n_hyp=4), SIGMAS
    if name == "sur":         # the same 2 pieces among the four moving cars
        return _two_pieces(4, True), SIGMAS
    if name == "wave":        # the plan leaves the TEAM shape at N_WAVE; with moving obstacles it takes the WAVE shape there
        return _two_pieces(N_WAVE, True), (0.3,)
    if name == "quad":        # ... and the QUAD shape without
        return _two_pieces(N_WAVE, False), (0.3,)
    if name == "generic":     # six half-planes per point: the generic form of the kernel (tests/test_gpu_parity.py: six planes)
        base = _two_pieces(2, False, n_hyp=2)
        cor = np.zeros((2, base.n_points, 6, 4))
        cor[:, :, :4] = base.corridor
        cor[:, :, 4:] = base.corridor[:, :, :2]
        cor[:, :, 4:, 2:] -= 0.2 * base.corridor[:, :, :2, :2]
        cor[:, :, 4:, :2] *= 3.0
        lay = LayoutSpec(base.layout.piece_nums, base.layout.singuls, H=6)
        return sc.Scenario("six_planes", lay, base.K, base.Kd, 2, base.ini_states, base.fin_states, base.inner_pts, base.init_Ts,
                           np.ascontiguousarray(cor)), SIGMAS
    raise KeyError(name)


def scene(name):
    """(params, scenario, [x [B][n], ...]) of a named scene: x0 of the oracle, moved by N(0, sigma^2) per listed sigma"""
    if name not in _SCENES:
        s, sigmas = _build(name)
        p = capi.default_params()
        s.apply_resolution(p)
        x0 = np.stack([po.OracleProblem(p, s, b, order=2).x0() for b in range(s.B)])
        rng = np.random.default_rng(17)
        _SCENES[name] = (p, s, [x0 + (rng.normal(0.0, sg, x0.shape) if sg else 0.0) for sg in sigmas])
    return _SCENES[name]


def oracle_terms(p, s, b, x):
    """(f, terms [5]) of trajectory b at x [n]: the restatement in order 2"""
    o = po.OracleProblem(p, s, b, order=2)
    f, _ = o.eval(x)
    return f, o.cost_terms()


def recompose(terms, seg_terms):
    """the cost in the association of traj_optimizer.cpp:292-297, 328-344: total_smcost + total_timecost + penalty_cost, the penalty
    chained over the segments as (costs(0) + costs(1)) + costs(2); terms [5], seg_terms [M][5]"""
    penalty = 0.0
    for sg in np.asarray(seg_terms):
        penalty += (float(sg[CORRIDOR]) + float(sg[SURROUND])) + float(sg[FEAS])
    return float(terms[SMOOTH]) + float(terms[TIME]) + penalty


def chained(seg_terms):
    """every column of seg_terms [M][5] chained over the segments in order from 0.0"""
    acc = np.zeros(5)
    for sg in np.asarray(seg_terms):
        acc = acc + sg
    return acc


def reference_plan(s, p, n_obstacles=0, B=None):
    """the kind of launch shape dftpav_batch_set_order chooses for the scenario (or for B trajectories of its layout) on a 256-CU
    device (dftpav_debug_reference_plan): 0 TEAM, 1 WAVE, 3 QUAD, 5 QUAD for several segments"""
    fn = capi.lib().dftpav_debug_reference_plan
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 8)()
    assert fn(C.byref(s.layout.c_struct()), C.byref(p), int(n_obstacles), int(B or s.B), 256, out) == 0 and int(out[0]) == 1
    return int(out[1])


# ---- the gate
def gate_rule(terms, caps, flags_in):
    """(flags_out, rejected) of penalty_gate_kernel: rejected unless every penalty sum is <= its cap (so a NaN is rejected)"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1, 5)
    with np.errstate(invalid="ignore"):
        rej = ~(t[:, CORRIDOR] <= caps.corridor) | ~(t[:, SURROUND] <= caps.surround) | ~(t[:, FEAS] <= caps.feasibility)
    return ((np.asarray(flags_in) != 0) | rej).astype(np.int32), rej.astype(np.int32)


def gate_cases():
    """[(caps, terms [n][5], flags_in [n], rejected expected [n])]: a term at its cap and one ulp above it, +inf caps, a cap of 0.0
    against +0.0 / -0.0 / the smallest positive double, NaN terms, flags_in already set"""
    up = lambda v: float(np.nextafter(v, INF))
    row = lambda c=0.0, s=0.0, f=0.0: [11.0, 3.0, c, s, f]
    cases = []
    caps = capi.PenaltyCaps(2.5, 0.75, 1.0e-3)
    t = [row(2.5, 0.75, 1.0e-3), row(c=up(2.5)), row(s=up(0.75)), row(f=up(1.0e-3)), row(), row(2.5, 0.75, 1.0e-3), row(c=NAN), row(s=NAN),
         row(f=NAN), row(c=INF), [NAN, NAN, 0.0, 0.0, 0.0]]
    cases.append((caps, t, [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0]))
    caps = capi.PenaltyCaps()  # all +inf
    t = [row(1e300, 1e300, 1e300), row(c=INF), row(s=NAN), row(), row(f=-NAN)]
    cases.append((caps, t, [0, 0, 0, 7, 1], [0, 0, 1, 0, 1]))
    caps = capi.PenaltyCaps(0.0, 0.0, 0.0)
    t = [row(0.0, 0.0, 0.0), row(-0.0, -0.0, -0.0), row(c=5e-324), row(s=5e-324), row(f=5e-324), row(-0.0, 0.0, -0.0)]
    cases.append((caps, t, [0, 0, 0, 0, 0, 2], [0, 0, 1, 1, 1, 0]))
    return [(c, np.array(t), np.array(fi, dtype=np.int32), np.array(rj, dtype=np.int32)) for c, t, fi, rj in cases]


# ---- the planner's chain
# The caps and the queries they hit were chosen on the CPU from the terms of the oracle chain's own solutions (chain_terms()):
# corridor <= 1000 and feasibility <= 0.5 (no moving obstacles on that scene: surround is 0.0 and not judged).
CAPS = dict(corridor=1000.0, feasibility=0.5)
CHANGED = {0: (0, 1), 11: (0, 1)}                    # query: (winner without the filter, winner with it -- a dearer restart)
NO_VALID = {1: 1, 2: 0, 3: 1, 10: 0}                 # query: winner without the filter; with it every restart is rejected
KEPT = {4: 3, 5: 1, 6: 3, 7: 3, 8: 2, 9: 2}          # query: the winner either way

_CHAIN_TERMS = None


def chain_scenarios():
    """per query of limits_cases.chain(): None or the Scenario of its R restarts (rebuilt as tests/test_gpu_plan_queries.py does)"""
    import limits_cases as lc
    import test_gpu_plan_queries as tq
    ch = lc.chain()
    grid, res, org, S, E = ch["scene"]
    o = ch["search"]
    fp = FrontendParams.default(K=lc.K, Kd=lc.KD)
    out = [None] * len(E)
    for q, e in enumerate(ch["per"]):
        if e is None:
            continue
        n = int(o["path_len"][q])
        fe = po.frontend_resample(o["paths"][q:q + 1, :n].copy(), o["path_len"][q:q + 1].copy(), S[q:q + 1], E[q:q + 1], np.zeros((1, 2)), fp,
                                  order=2)
        lay = e["layout"]
        inner, durs, states = tq._hypothesis(fe, 0, lay)
        inner_r, durs_r = tq._restarts_of(po.sample_restarts, q, inner, durs)
        cor = po.corridor_rectangles(grid, res, org, states, order=2)
        out[q] = tq._scenario(lay, fe, 0, inner_r, durs_r, np.repeat(cor[None], lc.R, 0))
    return out


def chain_terms():
    """(terms [Q][R][5] of the chain's solutions, zero rows where nothing was solved; the scenarios per query); once per process"""
    global _CHAIN_TERMS
    if _CHAIN_TERMS is None:
        import limits_cases as lc
        ch = lc.chain()
        scen = chain_scenarios()
        p = capi.default_params()
        T = np.zeros((len(scen), lc.R, 5))
        for q, s in enumerate(scen):
            if s is None:
                continue
            for b in range(lc.R):
                f, T[q, b] = oracle_terms(p, s, b, ch["per"][q]["solve"]["x"][b])
                assert f == ch["per"][q]["solve"]["final_cost"][b]
        _CHAIN_TERMS = (T, scen)
    return _CHAIN_TERMS
