"""Timing of dftpav_plan_queries against the same work through the separate public calls.

N default-arena queries (the ego start, goals drawn 6-14 m round it: the scene of scripts/search_time.py), R restarts each:
  (a) one call of dftpav_plan_queries;
  (b) kino_search -> frontend_resample -> host grouping -> per layout: sample_restarts, Batch.upload, corridor_from_states,
      reference-order solve, coeffs, validate -- on batches created beforehand, as (a)'s are after its warm-up.
Both on the same build, one warm-up, then `reps` runs each; wall time of the host call(s) and, for (a), the device time of its
stages from the planner's events (dftpav_planner_info); for (b), the stages between dftpav_mark markers.
Usage: python scripts/plan_time.py [--n 64] [--restarts 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dftpav_amd import capi, search_scenes as ss  # noqa: E402
from dftpav_amd.pods import FrontendParams, LayoutSpec  # noqa: E402
from dftpav_amd.scenarios import Scenario  # noqa: E402

K, KD = 16, 32


def separate_calls(h, S, E, R, seed, batches, stages):
    """(b): the chain through the public calls; `batches` caches one Batch per (layout, size); returns the winners"""
    Q = len(E)
    t = time.perf_counter()
    sr = h.kino_search(S, E)
    stages["search"] += time.perf_counter() - t
    arrived = np.hypot(E[:, 0] - S[:, 0], E[:, 1] - S[:, 1]) < 1.0
    use = np.flatnonzero((sr["status"] == 2) & ~arrived)
    winner = np.full(Q, -1, dtype=np.int32)
    if not len(use):
        return winner
    t = time.perf_counter()
    mp = int(sr["path_len"].max())
    fe = h.frontend_resample(sr["paths"][use, :mp].copy(), sr["path_len"][use].copy(), S[use], E[use], np.zeros((len(use), 2)),
                             FrontendParams.default(K=K, Kd=KD))
    g = capi.plan_group_layouts(np.full(len(use), 2, dtype=np.int32), fe["n_seg"], fe["singul"], fe["piece_nums"])
    stages["resample"] += time.perf_counter() - t
    t = time.perf_counter()
    for gi, f in enumerate(g["group_first"]):
        members = np.flatnonzero(g["group"] == gi)
        M = int(fe["n_seg"][f])
        lay = LayoutSpec(fe["piece_nums"][f, :M].tolist(), fe["singul"][f, :M].tolist(), 4)
        if lay.n_vars > 256:
            continue
        B = len(members) * R
        inner_r, durs_r, states = [], [], []
        for m in members:
            inner = np.concatenate([fe["inner_pts"][m, i, :lay.piece_nums[i] - 1].reshape(-1) for i in range(M)])
            durs = fe["piece_dt"][m, :M] * fe["piece_nums"][m, :M]
            q = int(use[m])
            a = np.zeros((q + 1, inner.size))
            d = np.ones((q + 1, M))
            a[q], d[q] = inner, durs
            oi, od = h.sample_restarts(a, d, R, seed=seed)
            inner_r.append(oi[q * R:(q + 1) * R])
            durs_r.append(od[q * R:(q + 1) * R])
            states.append(np.concatenate([fe["states"][m, i, :fe["n_states"][m, i]] for i in range(M)]))
        key = (tuple(lay.piece_nums.tolist()), tuple(lay.singuls.tolist()), B)
        if key not in batches:
            batches[key] = capi.Batch(h, lay, B)
            batches[key].set_order(capi.ORDER_REFERENCE)
        bt = batches[key]
        s = Scenario("plan-time", lay, K, KD, B, np.repeat(fe["ini_states"][members, :M], R, 0).copy(),
                     np.repeat(fe["fin_states"][members, :M], R, 0).copy(), np.concatenate(inner_r), np.concatenate(durs_r),
                     np.zeros((B, lay.n_points(K, KD), 4, 4)))
        bt.upload(s, with_corridor=False)
        bt.corridor_from_states(np.array(states), n_restarts=R)
        r = bt.solve()
        bt.coeffs()
        col, _ = bt.validate()
        ok = (r["success"] != 0) & (col == 0) & ~np.isnan(r["final_cost"])
        for k, m in enumerate(members):
            sl = slice(k * R, (k + 1) * R)
            idx = np.flatnonzero(ok[sl])
            if idx.size:
                winner[use[m]] = idx[np.argmin(r["final_cost"][sl][idx])]
    stages["groups"] += time.perf_counter() - t
    return winner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--restarts", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    grid, res, org, start, _ = ss.arena()
    rng = np.random.default_rng(a.seed)
    r = rng.uniform(6.0, 14.0, a.n)
    ang = rng.uniform(-np.pi, np.pi, a.n)
    E = np.stack([start[0] + r * np.cos(ang), start[1] + r * np.sin(ang), rng.uniform(-np.pi, np.pi, a.n), np.zeros(a.n)], 1)
    S = np.repeat(start[None], a.n, 0)
    h = capi.Handle()
    h.set_grid_map(grid, res, org)
    pp = capi.default_plan_params()
    pp.seed = a.seed
    pl = capi.Planner(h, a.n, a.restarts)
    out = pl.plan(S, E, pp=pp)  # warm-up: the batches of every layout are created here
    wall_a, stage_a = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        o2 = pl.plan(S, E, pp=pp)
        wall_a.append((time.perf_counter() - t) * 1e3)
        stage_a.append(pl.info()["stage_ms"].tolist())
        assert all(np.array_equal(out[k], o2[k], equal_nan=True) for k in out)
    info = pl.info()
    batches = {}
    separate_calls(h, S, E, a.restarts, a.seed, batches, dict(search=0.0, resample=0.0, groups=0.0))  # warm-up
    wall_b, stage_b, dev_b = [], [], []
    for _ in range(a.reps):
        st = dict(search=0.0, resample=0.0, groups=0.0)
        h.mark(0)
        t = time.perf_counter()
        w = separate_calls(h, S, E, a.restarts, a.seed, batches, st)
        wall_b.append((time.perf_counter() - t) * 1e3)
        h.mark(1)
        dev_b.append(h.elapsed_since(h, 0, 1))
        stage_b.append({k: v * 1e3 for k, v in st.items()})
    planned = np.isin(out["plan_status"], (capi.PLAN_OK, capi.PLAN_NO_VALID_RESTART))
    best = int(np.argmin(wall_a))
    res_ = dict(n=a.n, restarts=a.restarts, groups=len(info["group_sizes"]), group_sizes=info["group_sizes"].tolist(),
                plan_status_counts=np.bincount(out["plan_status"], minlength=6).tolist(),
                a_wall_ms=wall_a, a_best_ms=min(wall_a), a_stage_ms_search_resample_groups_all=stage_a[best],
                b_wall_ms=wall_b, b_best_ms=min(wall_b), b_spread_ms=max(wall_b) - min(wall_b), b_marks_ms=dev_b,
                b_stage_wall_ms=stage_b[int(np.argmin(wall_b))],
                same_winners=bool(np.array_equal(w[planned], out["winner"][planned])))
    print(json.dumps(res_))
    for bt in batches.values():
        bt.close()
    pl.close()
    h.close()


if __name__ == "__main__":
    main()
