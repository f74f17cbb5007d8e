"""Scenes of a few boxes for joint selection (include/dftpav_hip.h, "joint selection"), and a brute-force restatement of its rule in
plain Python floats -- shared by tests/test_joint_oracle.py (the CPU oracle against it) and tests/test_gpu_joint_select.py (the
kernels against the oracle)."""
import math

import numpy as np

W, L, DCR = 1.90, 4.88, 1.015           # the default vehicle: a box 4.88 m long; two boxes on a line dx apart are dx - 4.88 m apart
INF = float("inf")
FIELDS = ("min_sep", "sep_sample", "sep_partner", "conflict_sample", "conflict_partner")
FAR = 100.0                             # spacing of candidates that take no part: beyond every broad phase used here


def _corners(p):
    x, y, c, s = p
    return [(x + 0.5 * L * c + 0.5 * W * s, y + 0.5 * L * s - 0.5 * W * c), (x + 0.5 * L * c - 0.5 * W * s, y + 0.5 * L * s + 0.5 * W * c),
            (x - 0.5 * L * c - 0.5 * W * s, y - 0.5 * L * s + 0.5 * W * c), (x - 0.5 * L * c + 0.5 * W * s, y - 0.5 * L * s - 0.5 * W * c)]


def _separates(own, other):
    x, y, c, s = own
    lx = [c * (px - x) + s * (py - y) for px, py in other]
    ly = [c * (py - y) - s * (px - x) for px, py in other]
    return all(v > L / 2 for v in lx) or all(v < -L / 2 for v in lx) or all(v > W / 2 for v in ly) or all(v < -W / 2 for v in ly)


def sep(a, b):
    """steps 2 and 3 of the conflict check for two poses (cx, cy, cs, sn)"""
    ca, cb = _corners(a), _corners(b)
    if not _separates(a, cb) and not _separates(b, ca):
        return 0.0
    m = INF
    for P, E in ((ca, cb), (cb, ca)):
        for px, py in P:
            for e in range(4):
                (ax, ay), (bx, by) = E[e], E[(e + 1) % 4]
                u = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / ((bx - ax) * (bx - ax) + (by - ay) * (by - ay))
                u = 0.0 if not u > 0.0 else (1.0 if u > 1.0 else u)
                ex, ey = px - (ax + u * (bx - ax)), py - (ay + u * (by - ay))
                m = min(m, ex * ex + ey * ey)
    return math.sqrt(m)


def pair_sample(a, b, rng):
    """sep of one pair-sample, or None where it contributes nothing"""
    if not (all(math.isfinite(v) for v in a) and all(math.isfinite(v) for v in b)):
        return None
    rad = math.sqrt(0.25 * L * L + 0.25 * W * W)
    R = rng + 2.0 * rad
    dx, dy = a[0] - b[0], a[1] - b[1]
    if not dx * dx + dy * dy <= R * R:
        return None
    return sep(a, b)


def brute(poses, cost, eligible, margin, rng):
    """the rule, restated: poses [K][Q][R][4], cost / eligible [Q][R] -> the dict of pyjoint.select"""
    poses = np.asarray(poses, dtype=np.float64)
    K, Q, R, _ = poses.shape
    P = poses.tolist()
    out = dict(winner=np.full(Q, -1, np.int32), blocked=np.zeros((Q, R), np.int32), min_sep=np.full((Q, R), INF),
               **{k: np.full((Q, R), -1, np.int32) for k in FIELDS[1:]})
    for q in range(Q):
        best = None
        for r in range(R):
            triples = []                                       # (sep, k, q') of every contributing pair-sample
            for qq in range(q):
                w = int(out["winner"][qq])
                if w < 0:
                    continue
                for k in range(K):
                    s = pair_sample(P[k][q][r], P[k][qq][w], rng)
                    if s is not None:
                        triples.append((s, k, qq))
            if triples:
                out["min_sep"][q, r], out["sep_sample"][q, r], out["sep_partner"][q, r] = min(triples)
            within = [(k, qq) for s, k, qq in triples if s <= margin]
            if within:
                out["conflict_sample"][q, r], out["conflict_partner"][q, r] = min(within)
            out["blocked"][q, r] = 1 if within else 0
            c = float(cost[q][r])
            if eligible[q][r] and not within and c == c and (best is None or c < best[0]):
                best = (c, r)
        out["winner"][q] = -1 if best is None else best[1]
    return out


def same(got, ref):
    for k in ("winner", "blocked") + FIELDS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        ok = np.array_equal(a.view(np.int64), b.view(np.int64)) if k == "min_sep" else np.array_equal(a, b)
        assert ok, (k, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def apart(K, Q, R):
    """every candidate alone: poses [K][Q][R][4] on a grid FAR apart, heading 0, standing still; cost r + 1, all eligible"""
    poses = np.zeros((K, Q, R, 4))
    poses[..., 0] = (np.arange(Q)[:, None] * FAR)[None]
    poses[..., 1] = 10000.0 + (np.arange(R)[None, :] * FAR)[None]
    poses[..., 2] = 1.0
    cost = np.tile(np.arange(1.0, R + 1.0), (Q, 1))
    return poses, cost, np.ones((Q, R), np.int32)


def put(poses, q, r, x, y, k=None, heading=0.0):
    poses[slice(None) if k is None else k, q, r] = (x, y, math.cos(heading), math.sin(heading))


def chain(K=1):
    """Only winners block.  q0's winner blocks q1's cheapest restart, q1 takes its dearer one, which blocks q2's cheapest; q1's cheapest
    would not have blocked it.  margin 0.5, range 2: winners 0, 1, 1; with q0 ineligible: -1, 0, 0."""
    poses, cost, elig = apart(K, 3, 2)
    put(poses, 0, 0, 0.0, 0.0)
    put(poses, 1, 0, 5.0, 0.0)          # 0.12 m in front of q0's winner
    put(poses, 1, 1, 0.0, 50.0)
    put(poses, 2, 0, 5.0, 50.0)         # 0.12 m in front of q1's dearer restart, 50 m from its cheapest
    return poses, cost, elig, 0.5, 2.0


def random_scene(seed, K, Q, R, spread=6.0):
    """candidates that drive straight through one another: many conflicts, ties in cost, ineligible restarts, NaN costs and NaN poses"""
    rng = np.random.default_rng(seed)
    C = Q * R
    side = spread * math.sqrt(C)
    p0 = rng.uniform(0.0, side, (Q, R, 2))
    yaw = rng.uniform(-math.pi, math.pi, (Q, R))
    v = rng.uniform(0.0, 4.0, (Q, R))
    poses = np.zeros((K, Q, R, 4))
    for k in range(K):
        poses[k, ..., 0] = p0[..., 0] + 0.5 * k * v * np.cos(yaw)
        poses[k, ..., 1] = p0[..., 1] + 0.5 * k * v * np.sin(yaw)
        poses[k, ..., 2] = np.cos(yaw)
        poses[k, ..., 3] = np.sin(yaw)
    cost = np.round(rng.uniform(0.0, 3.0, (Q, R)), 1)           # ties
    cost[rng.uniform(size=(Q, R)) < 0.05] = np.nan
    elig = (rng.uniform(size=(Q, R)) < 0.85).astype(np.int32)
    poses[:, rng.uniform(size=(Q, R)) < 0.04] = np.nan          # a candidate of NaN poses
    return poses, cost, elig


# ---- a planner scene with distinct starts, and the chain of CPU oracles behind dftpav_plan_queries on it (as tests/limits_cases.py
# builds it for the arena queries, which all start in one state and so cannot come NEAR one another without overlapping)
PLAN_R, PLAN_SEED = 4, 7
_PLAN_CHAIN = {}


def plan_scene():
    """(grid, resolution, origin, starts [2][4], goals [2][4]): the default arena; two vehicles stand side by side across the ego start's
    heading, 3.2 m apart (1.3 m between the flanks), and drive to two arena goals, so their first metres run close to one another"""
    from dftpav_amd import search_scenes as ss
    grid, res, org, S, E = ss.arena_plan_queries()
    s0 = S[0]
    n = np.array([-math.sin(s0[2]), math.cos(s0[2])])
    lanes, goals = (1.0, 0.0), (5, 0)
    starts = np.array([[s0[0] + 3.2 * a * n[0], s0[1] + 3.2 * a * n[1], s0[2], s0[3]] for a in lanes])
    return grid, res, org, starts, E[list(goals)].copy()


def plan_chain(scene=None, R=PLAN_R, seed=PLAN_SEED):
    """per query None (no path / arrived / outside the padding) or dict(layout, solve, coeffs [R][Ntot][6][2], dts [R][M], collision,
    first), all in order 2; computed once per process and scene"""
    import limits_cases as lc
    from dftpav_amd import capi
    from dftpav_amd.pods import FrontendParams, LayoutSpec
    from dftpav_amd.scenarios import Scenario
    from oracle import pyoracle as po
    from oracle_search import pysearch as ps
    if scene is None and "default" in _PLAN_CHAIN:
        return _PLAN_CHAIN["default"]
    grid, res, org, S, E = plan_scene() if scene is None else scene
    p = capi.default_params()
    Q = len(E)
    o = ps.kino_search(grid, res, org, S, E, order=2, nthreads=8)
    arrived = np.hypot(E[:, 0] - S[:, 0], E[:, 1] - S[:, 1]) < 1.0
    fp = FrontendParams.default(K=lc.K, Kd=lc.KD)
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
        oi, od = po.sample_restarts(a, d, R, seed=seed)
        inner_r, durs_r = oi[q * R:(q + 1) * R].copy(), od[q * R:(q + 1) * R].copy()
        cor = po.corridor_rectangles(grid, res, org, states, order=2)
        s = Scenario("plan", lay, lc.K, lc.KD, R, np.repeat(fe["ini_states"][0:1, :M], R, 0).copy(), np.repeat(fe["fin_states"][0:1, :M], R, 0).copy(),
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
    out = dict(per=per, scene=(grid, res, org, S, E))
    if scene is None:
        _PLAN_CHAIN["default"] = out
    return out
