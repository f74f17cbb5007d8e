"""Device time of the stamps (dftpav_planner_stamp_slots, stamp.hip): 1 024 installed plans, straight runs of 20 m, on the default
arena (1500 x 1500 cells of 0.2 m), K = 200 clocks at dt = 0.05, inflated by one cell diagonal.  pose_ms and stamp_ms are the
handle's own HIP events, the clear is timed between two marks on the handle's stream, the distance-field rebuild that follows is
dftpav_clearance_last_ms's; each the best of 3 after a warm-up.  Beside them, what a caller pays for the same working map without
the stamps: the boxes rasterised on the host by numpy on one core -- the definition over each box's own window of cells, whose
result must equal the device's bytes -- and the dftpav_set_grid_map of the result.  The yardstick itself (oracle_stamp, every cell
of the grid for every box) is timed on a few boxes and scaled, for scale only.

    python scripts/stamp_time.py [--slots 1024] [--samples 200] [--dt 0.05] [--extent 120] [--oracle-boxes 16]

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.24 only."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, conflict_scenes as cs, replan_scenes as rs, search_scenes as ss  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from oracle_stamp import pystamp as ps  # noqa: E402


def host_raster(base, boxes, res, origin, inflate, veh):
    """the definition evaluated on each box's own window of cells (its axis-aligned box and two cells more on every side)"""
    out = base.copy()
    size_y, size_x = base.shape
    hl, hw = 0.5 * veh[1] + inflate, 0.5 * veh[0] + inflate
    for cx, cy, c, s in boxes:
        if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(c) and np.isfinite(s)):
            continue
        ex, ey = abs(c) * hl + abs(s) * hw, abs(s) * hl + abs(c) * hw
        x0, x1 = int(np.floor((cx - ex - origin[0]) / res)) - 2, int(np.ceil((cx + ex - origin[0]) / res)) + 2
        y0, y1 = int(np.floor((cy - ey - origin[1]) / res)) - 2, int(np.ceil((cy + ey - origin[1]) / res)) + 2
        x0, x1, y0, y1 = max(x0, 0), min(x1, size_x - 1), max(y0, 0), min(y1, size_y - 1)
        if x0 > x1 or y0 > y1:
            continue
        dx = (origin[0] + np.arange(x0, x1 + 1, dtype=np.float64) * res)[None, :] - cx
        dy = (origin[1] + np.arange(y0, y1 + 1, dtype=np.float64) * res)[:, None] - cy
        m = (np.abs(c * dx + s * dy) <= hl) & (np.abs(c * dy - s * dx) <= hw)
        out[y0:y1 + 1, x0:x1 + 1][m] = 80
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--extent", type=float, default=120.0)
    ap.add_argument("--oracle-boxes", type=int, default=16)
    a = ap.parse_args()
    po.build()
    grid, res, origin, _, _ = ss.arena()
    size_y, size_x = grid.shape
    centre = np.array([origin[0] + 0.5 * size_x * res, origin[1] + 0.5 * size_y * res])
    rng = np.random.default_rng(1024)
    plans = []
    for _ in range(a.slots):                                    # conflict_scenes.straight_plans about the arena's centre
        p0 = centre + (rng.random(2) - 0.5) * a.extent
        ang = rng.random() * 2.0 * np.pi
        plans.append(cs._run(po.minco_generate, p0, p0 + 20.0 * np.array([np.cos(ang), np.sin(ang)]), 0.0, n_pieces=4))
    pad = rs.padded(dict(slots=plans), 1, 4)
    p = capi.default_params()
    h = capi.Handle(p)
    h.set_grid_map(grid, res, origin)
    pl = capi.Planner(h, a.slots, 1)
    pl.install(pad["slots"], pad["n_seg"], pad["singul"], pad["piece_nums"], pad["coeff_dt"], pad["coeffs"], pad["end_states"], t_start=0.0)
    inflate = res * np.sqrt(2.0)
    h.distance_field(fetch=False)
    pose_ms, stamp_ms, clear_ms, field_ms = [], [], [], []
    for _ in range(4):                                          # the first is the warm-up
        h.mark(0)
        h.clear_stamps()
        h.mark(1)
        pl.stamp_slots(0.0, a.dt, a.samples, inflate)
        ms = h.stamp_last_ms()
        h.distance_field(fetch=False)
        pose_ms.append(ms[0])
        stamp_ms.append(ms[1])
        clear_ms.append(h.elapsed_since(h))
        field_ms.append(h.clearance_last_ms()[0])
    got, n_stamped = h.read_cells()
    boxes = ps.slot_boxes(pl.sample_poses(0.0, a.dt, a.samples))
    veh = (p.veh_width, p.veh_length)
    t = time.perf_counter()
    want = host_raster(grid, boxes, res, origin, inflate, veh)
    host_s = time.perf_counter() - t
    same = bool(np.array_equal(got, want))
    t = time.perf_counter()
    h.set_grid_map(want, res, origin)
    upload_s = time.perf_counter() - t
    nb = max(1, min(a.oracle_boxes, len(boxes)))
    t = time.perf_counter()
    ps.covered(boxes[:nb], size_x, size_y, res, origin, inflate, veh)
    oracle_box_s = (time.perf_counter() - t) / nb
    print(json.dumps(dict(slots=a.slots, samples=a.samples, dt=a.dt, extent=a.extent, cells=[size_x, size_y], boxes=len(boxes),
                          inflate=inflate, n_stamped=n_stamped, pose_ms=min(pose_ms[1:]), stamp_ms=min(stamp_ms[1:]),
                          clear_ms=min(clear_ms[1:]), field_rebuild_ms=min(field_ms[1:]), host_numpy_one_core_s=host_s,
                          host_set_grid_map_s=upload_s, oracle_whole_grid_s_per_box=oracle_box_s,
                          oracle_whole_grid_scaled_s=oracle_box_s * len(boxes), equal_to_host_raster=same)))
    pl.close()
    h.close()
    assert same


if __name__ == "__main__":
    main()
