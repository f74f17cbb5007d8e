"""Device time of the distance field build (distfield.hip, both passes) on the default 1500 x 1500 arena, and of the clearance check
(dftpav_batch_check_clearance, clearance.hip) on a solved batch of BASELINE configs[2] beside dftpav_batch_validate of the same
batch -- the same walk over the same samples and outline points, so validate's time is the yardstick.  Best of 3 after a warm-up,
the handle's own HIP events.

    python scripts/clearance_time.py [--batch 4096] [--check-dt 0.05]

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.19 only."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, scenarios as sc, search_scenes as ss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--check-dt", type=float, default=0.05)
    a = ap.parse_args()
    grid, res, org, _, _ = ss.arena()
    p = capi.default_params()
    s = sc.baseline_config(3, B=a.batch)       # configs[2]
    s.apply_resolution(p)
    h = capi.Handle(p)
    bt = capi.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.solve()
    field_ms, clr_ms, val_ms = [], [], []
    for k in range(4):                          # the first is the warm-up
        h.set_grid_map(grid, res, org)          # marks the field stale: the next call builds it
        h.distance_field(fetch=False)
        field_ms.append(h.clearance_last_ms()[0])
        r = bt.check_clearance(a.check_dt)
        clr_ms.append(h.clearance_last_ms()[1])
        col, _ = bt.validate(sample_dt=a.check_dt, vertex_res=0.1)
        val_ms.append(h.corridor_last_ms())
    assert np.array_equal(r["min_d2"] == 0, col != 0)
    print(json.dumps(dict(map=list(grid.shape), batch=s.B, pieces=[int(v) for v in s.layout.piece_nums], check_dt=a.check_dt,
                          colliding=int((col != 0).sum()), off_grid=int((r["arg"] < 0).sum()), field_build_ms=min(field_ms[1:]),
                          clearance_kernel_ms=min(clr_ms[1:]), validate_kernel_ms=min(val_ms[1:]))))
    bt.close()
    h.close()


if __name__ == "__main__":
    main()
