"""Device time of the Reeds-Shepp table build (rstable.hip) for the default geometry and for the tests' small one, and mean pops,
budget hits and kernel time of scripts/search_time.py's workload (N default-arena queries from the ego start) with the Reeds-Shepp
term of the heuristic off and on (dftpav_set_search_rs_heuristic).  Best of 3 after a warm-up, the handle's own HIP events; the
search's time is the span round its launches, which holds the table build only in the call that builds it (the warm-up).

    python scripts/rs_heuristic_time.py [--n 1024] [--plain-only]

--plain-only: the search without the term alone (what a library from before it can run; name it with DFTPAV_LIB).
Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.21 only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, search_scenes as ss  # noqa: E402


def _search(h, starts, goals, reps=3):
    out = h.kino_search(starts, goals)              # warm-up (workspace, code object, the table)
    ms = []
    for _ in range(reps):
        o2 = h.kino_search(starts, goals)
        ms.append(h.corridor_last_ms())
        assert all(np.array_equal(out[k], o2[k]) for k in out)
    return dict(kernel_ms=min(ms), kernel_ms_all=ms, mean_pops=float(out["iters"].mean()), max_pops=int(out["iters"].max()),
                mean_nodes=float(out["nodes_used"].mean()), reach_end=int((out["status"] == 2).sum()),
                shot=int(out["shot_success"].sum()), budget_hit=int(out["budget_hit"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    grid, res, org, start, _ = ss.arena()
    rng = np.random.default_rng(a.seed)             # (the draws of scripts/search_time.py)
    r = rng.uniform(6.0, 14.0, a.n)
    ang = rng.uniform(-np.pi, np.pi, a.n)
    goals = np.stack([start[0] + r * np.cos(ang), start[1] + r * np.sin(ang), rng.uniform(-np.pi, np.pi, a.n), np.zeros(a.n)], 1)
    starts = np.repeat(start[None], a.n, 0)
    h = capi.Handle()
    h.set_grid_map(grid, res, org)
    out = dict(n=a.n, search_off=_search(h, starts, goals))
    if not a.plain_only:
        for label, geom in (("default", {}), ("small", ss.RS_SMALL)):
            ms = []
            for rep in range(4):                    # another key in between, so that every call builds
                h.rs_table(n_yaw=1, extent=0.0, cell=1.0)
                shape = h.rs_table(**geom).shape
                ms.append(h.rs_table_last_ms()[0])
            out["table_%s" % label] = dict(shape=list(shape), build_ms=min(ms[1:]), build_ms_all=ms)
            h.set_search_rs_heuristic(True, **geom)
            out["search_on_%s" % label] = _search(h, starts, goals)
            h.set_search_rs_heuristic(False)
        out["search_off_again"] = _search(h, starts, goals)
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
