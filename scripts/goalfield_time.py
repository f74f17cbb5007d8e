"""Device time of the goal-field build (goalfield.hip) for 1, 16 and 256 distinct goals on the default 1500 x 1500 arena and on the
200 x 200 maze of search_scenes.py, and iterations and device time of the hybrid A* search on ARENA_GOALS with the obstacle-aware
heuristic off and on (dftpav_set_search_heuristic).  Best of 3 after a warm-up, the handle's own HIP events; the search's time is
the span round its launches, which with the heuristic on holds the field builds -- they are given beside it.

With windowed fields (dftpav_set_search_heuristic_window, --margins, metres): per margin the same search on ARENA_GOALS (span, field
share, pops) and the windowed build for 1, 16 and 256 (start, goal) pairs on the arena, each goal a free cell and its start 10 m
from it, at (+8 m, +6 m), clamped into the map by the window rule.

    python scripts/goalfield_time.py [--plain-only] [--inflate 0.0] [--margins 2,5,10 | --no-window]

--plain-only: the search without the heuristic alone (what a library from before the heuristic can run; name it with DFTPAV_LIB).
--no-window: everything but the windowed part (what a library from before the window can run).
Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.20 and 4.22 only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, search_scenes as ss  # noqa: E402


def _free_goals(grid, res, org, n, seed):
    """n points at the centres of distinct free cells"""
    rng = np.random.default_rng(seed)
    free = np.argwhere(grid != 80)
    pick = free[rng.choice(len(free), size=n, replace=False)]
    return np.stack([org[0] + res * pick[:, 1], org[1] + res * pick[:, 0]], 1)


def _best(fn, reps=4):
    ms = [fn() for _ in range(reps)]
    return min(ms[1:])                             # the first is the warm-up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--inflate", type=float, default=0.0)
    ap.add_argument("--margins", default="2,5,10")
    ap.add_argument("--no-window", action="store_true")
    a = ap.parse_args()
    grid, res, org, start, goals = ss.arena()
    S = np.repeat(start[None], len(goals), 0)
    h = capi.Handle()
    h.set_grid_map(grid, res, org)
    out = dict(arena=list(grid.shape), inflate_radius=a.inflate)

    def search():
        r = h.kino_search(S, goals)
        search.last = r
        return h.corridor_last_ms()
    out["search_plain_ms"] = _best(search)
    out["search_plain_iters"] = [int(v) for v in search.last["iters"]]
    if not a.plain_only:
        h.set_search_heuristic(True, inflate_radius=a.inflate)
        fields = []

        def search_on():
            ms = search()
            fields.append(h.goal_field_last_ms())
            return ms
        out["search_heuristic_ms"] = _best(search_on)
        out["search_heuristic_fields_ms"] = min(fields[1:])
        out["search_heuristic_iters"] = [int(v) for v in search.last["iters"]]
        out["search_heuristic_status"] = [int(v) for v in search.last["status"]]
        for m in ([] if a.no_window else [float(v) for v in a.margins.split(",")]):
            h.set_search_heuristic_window(m)
            del fields[:]
            key = "search_window_%g" % m
            out[key + "_ms"] = _best(search_on)
            out[key + "_fields_ms"] = min(fields[1:])
            out[key + "_iters"] = [int(v) for v in search.last["iters"]]
            out[key + "_status"] = [int(v) for v in search.last["status"]]
            for n in (1, 16, 256):
                xy = _free_goals(grid, res, org, n, seed=n)
                st = xy + (8.0, 6.0)

                def build_windowed():
                    h.goal_field_windowed(st, xy, a.inflate, m, fetch=False)
                    return h.goal_field_last_ms()
                out["field_window_%g_arena_%d_ms" % (m, n)] = _best(build_windowed)
            h.set_search_heuristic_window(-1.0)
        h.set_search_heuristic(False)
        name, mg, mres, morg, _, _ = ss.maze()
        for label, (g, r_, o_) in (("arena", (grid, res, org)), ("maze", (mg, mres, morg))):
            h.set_grid_map(g, r_, o_)
            for n in (1, 16, 256):
                xy = _free_goals(g, r_, o_, n, seed=n)

                def build():
                    h.goal_field(xy, a.inflate, fetch=False)
                    return h.goal_field_last_ms()
                out["field_%s_%d_ms" % (label, n)] = _best(build)
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
