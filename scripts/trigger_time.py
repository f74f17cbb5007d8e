"""Device time of the conflict trigger's pair pass (dftpav_planner_check_yield, conflict_trigger.hip) beside the full conflict check's
(dftpav_planner_check_conflicts, conflict.hip) on the same table in the same session: the scene of scripts/conflict_time.py, 1 024
installed straight runs of 20 m across one another, K = 200 clocks at dt = 0.05, margin 0.5, range 2.0.  Two tables: every slot under
way, and every second slot installed 20 s earlier so that its plan has ended (it stands at its end and cannot yield).  pair_ms (pair
and reduce kernels together) are the handle's own HIP events, best of 3 after a warm-up, with the spread of the three.  Beside them,
from the device's poses by numpy: the share of the (I-tile, J-tile) pairs the trigger skips (no lane has a partner that precedes it),
and the share of the pair-samples of two occupied slots that reach the narrow phase, for the check and for the trigger.

    python scripts/trigger_time.py [--slots 1024] [--samples 200] [--dt 0.05] [--extent 75] [--margin 0.5] [--range 2.0]

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.29 only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, conflict_scenes as cs, replan_scenes as rs  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

TILE = 64


def shares(poses, can_yield, rng, veh=(1.90, 4.88)):
    """(tile pairs skipped, narrow share of the check, narrow share of the trigger) of poses [K][S][4]; no early exit is counted"""
    K, S = poses.shape[0], poses.shape[1]
    rad = np.sqrt(0.25 * veh[1] * veh[1] + 0.25 * veh[0] * veh[0])
    reach2 = (rng + 2.0 * rad) ** 2
    idx = np.arange(S)
    prec = (~can_yield[None, :]) | (idx[None, :] < idx[:, None])          # [i][j]: j precedes i
    np.fill_diagonal(prec, False)
    tiles = (S + TILE - 1) // TILE
    pad = np.zeros((tiles * TILE, tiles * TILE), dtype=bool)
    pad[:S, :S] = prec
    walked = pad.reshape(tiles, TILE, tiles, TILE).any(axis=(1, 3))
    inside = narrow = 0
    for k in range(K):
        dx = poses[k, :, None, 0] - poses[k, None, :, 0]
        dy = poses[k, :, None, 1] - poses[k, None, :, 1]
        m = (dx * dx + dy * dy) <= reach2
        np.fill_diagonal(m, False)
        inside += int(m.sum())
        narrow += int((m & prec).sum())
    examined = K * S * (S - 1)
    return 1.0 - walked.mean(), inside / examined, narrow / examined


def measure(h, pl, a, t_now):
    trig, full = [], []
    for _ in range(4):                          # the first of each is the warm-up; the two calls alternate
        y = pl.check_yield(t_now, 0.0, a.dt, a.samples, a.margin, a.range)
        trig.append(h.trigger_last_ms()[1])
        c = pl.check_conflicts(0.0, a.dt, a.samples, a.margin, a.range)
        full.append(h.conflicts_last_ms()[1])
    return y, c, trig[1:], full[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--extent", type=float, default=75.0)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--range", type=float, default=2.0)
    a = ap.parse_args()
    po.build()
    plans = cs.straight_plans(po.minco_generate, np.random.default_rng(1024), a.slots, a.extent, t_start=0.0)
    pad = rs.padded(dict(slots=plans), 1, 4)
    h = capi.Handle(capi.default_params())
    pl = capi.Planner(h, a.slots, 1)
    out = dict(slots=a.slots, samples=a.samples, dt=a.dt, extent=a.extent, margin=a.margin, range=a.range)
    for name in ("under_way", "half_completed"):
        keys = ("slots", "n_seg", "singul", "piece_nums", "coeff_dt", "coeffs", "end_states")
        if name == "under_way":
            pl.install(*[pad[k] for k in keys], t_start=0.0)
        else:                                   # every second slot again, 20 s earlier: ended at -10, held at its end
            pl.install(*[pad[k][1::2] for k in keys], t_start=-20.0)
        y, c, trig, full = measure(h, pl, a, 0.0)
        ends = np.array([pl.executing(s)["end_time"][0] for s in range(a.slots)])
        can_yield = ~(0.0 > ends)
        skipped, narrow_check, narrow_trigger = shares(pl.sample_poses(0.0, a.dt, a.samples), can_yield, a.range)
        # every conflicting partner of a slot that yields to nobody does not precede it; a yielding slot conflicts
        assert ((y["yield_sample"] >= 0) <= (c["conflict_sample"] >= 0)).all()
        out[name] = dict(completed=int((~can_yield).sum()), yielding=int(y["yield"].sum()), conflicting=int((c["conflict_sample"] >= 0).sum()),
                         trigger_pair_ms=min(trig), trigger_pair_ms_runs=trig, check_pair_ms=min(full), check_pair_ms_runs=full,
                         tile_pairs_skipped=skipped, narrow_share_check=narrow_check, narrow_share_trigger=narrow_trigger)
    print(json.dumps(out))
    pl.close()
    h.close()


if __name__ == "__main__":
    main()
