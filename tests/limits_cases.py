"""Shared by the limits tests (not a test module): the chain of CPU oracles behind dftpav_plan_queries on the fourteen arena
queries (search -> resample -> restarts -> rectangles -> solve -> collision re-check, all in order 2, as
tests/test_gpu_plan_queries.py builds it) with the limits oracle at its end, and the selection rule with the limit filter."""
import numpy as np

from dftpav_amd import capi
from dftpav_amd import search_scenes as ss
from dftpav_amd.pods import FrontendParams, LayoutSpec
from dftpav_amd.scenarios import Scenario
from oracle import pyoracle as po
from oracle_limits import pylimits as plim
from oracle_search import pysearch as ps

R = 4
SEED = 7
K, KD = 16, 32
CHECK_DT = 0.05
FIELDS = ("max_abs", "arg", "violated", "feasible")

_CHAIN = None


def same_rows(a, b):
    """every field of two limits results equal, NaN equal to NaN"""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=(k == "max_abs")) for k in FIELDS)


def chain():
    """per query None (no path / arrived / outside the padding) or dict(layout, solve, coeffs [R][Ntot][6][2], dts [R][M], collision,
    first); computed once per process"""
    global _CHAIN
    if _CHAIN is not None:
        return _CHAIN
    grid, res, org, S, E = ss.arena_plan_queries()
    p = capi.default_params()
    Q = len(E)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=8)
    arrived = np.hypot(E[:, 0] - S[:, 0], E[:, 1] - S[:, 1]) < 1.0
    fp = FrontendParams.default(K=K, Kd=KD)
    per = [None] * Q
    for q in range(Q):
        if arrived[q] or o["status"][q] != 2:
            continue
        n = int(o["path_len"][q])
        fe = po.frontend_resample(o["paths"][q:q + 1, :n].copy(), o["path_len"][q:q + 1].copy(), S[q:q + 1], E[q:q + 1], np.zeros((1, 2)), fp,
                                  order=2)
        M = int(fe["n_seg"][0])
        if not 1 <= M <= 8:
            continue
        lay = LayoutSpec([int(v) for v in fe["piece_nums"][0, :M]], [int(v) for v in fe["singul"][0, :M]], 4)
        pn = lay.piece_nums
        inner = np.concatenate([fe["inner_pts"][0, i, :pn[i] - 1].reshape(-1) for i in range(M)])
        durs = fe["piece_dt"][0, :M] * fe["piece_nums"][0, :M]
        states = np.concatenate([fe["states"][0, i, :fe["n_states"][0, i]] for i in range(M)])
        # the sampler keys its streams by (seed, hypothesis, restart); the hypothesis is the query's index in the call
        a, d = np.zeros((q + 1, inner.size)), np.ones((q + 1, durs.size))
        a[q], d[q] = inner, durs
        oi, od = po.sample_restarts(a, d, R, seed=SEED)
        inner_r, durs_r = oi[q * R:(q + 1) * R].copy(), od[q * R:(q + 1) * R].copy()
        cor = po.corridor_rectangles(grid, res, org, states, order=2)
        s = Scenario("plan", lay, K, KD, R, np.repeat(fe["ini_states"][0:1, :M], R, 0).copy(), np.repeat(fe["fin_states"][0:1, :M], R, 0).copy(),
                     inner_r, durs_r, np.repeat(cor[None], R, 0))
        r = po.solve_batch(p, s, nthreads=8, order=2)
        co, dts = [], []
        for b in range(R):
            pr = po.OracleProblem(p, s, b, order=2)
            pr.eval(r["x"][b])
            c, t = pr.coeffs()
            co.append(c)
            dts.append(t)
        co, dts = np.array(co), np.array(dts)
        col, first = po.validate_trajectories(grid, res, org, co, dts, lay.piece_nums, lay.singuls, order=2)
        per[q] = dict(layout=lay, solve=r, coeffs=co, dts=dts, collision=col, first=first)
    _CHAIN = dict(per=per, arrived=arrived, search=o, scene=(grid, res, org, S, E))
    return _CHAIN


def chain_limits(limits, check_dt=CHECK_DT):
    """the limits oracle (order 2) on every restart of the chain: dict of [Q][R] rows, zero with arg -1 where nothing was solved"""
    c = chain()
    Q = len(c["per"])
    out = dict(max_abs=np.zeros((Q, R, 5)), arg=np.full((Q, R, 5), -1, np.int32), violated=np.zeros((Q, R, 5), np.int32),
               feasible=np.zeros((Q, R), np.int32))
    for q, e in enumerate(c["per"]):
        if e is None:
            continue
        lay = e["layout"]
        r = plim.check_batch(lay.singuls, lay.piece_nums, e["coeffs"], e["dts"], check_dt, limits, order=2)
        for k in FIELDS:
            out[k][q] = r[k]
    return out


def select(cost, success, reject):
    """the selection rule: among restarts that succeeded and are not rejected the smallest cost; a NaN never wins; ties go to the
    lowest index; -1 if none qualifies"""
    cost = np.asarray(cost, dtype=np.float64)
    ok = (np.asarray(success) != 0) & (np.asarray(reject) == 0) & ~np.isnan(cost)
    idx = np.flatnonzero(ok)
    return int(idx[np.argmin(cost[idx])]) if idx.size else -1
