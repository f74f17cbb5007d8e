"""The CPU yardstick of the stamps (dftpav_grid_stamp_poses, dftpav_planner_stamp_slots) -- TEST INFRASTRUCTURE.

A plain numpy restatement of the definition in include/dftpav_hip.h ("the stamps"), evaluated over EVERY cell of the grid: no
bounding range, no header shared with the kernel, no build step.  numpy's elementwise fp64 operations are separate roundings (no
contraction), so every decision is the one the definition names, bit for bit.

Only tests/ and scripts/ import this."""
import numpy as np

VEH = (1.90, 4.88)            # veh_width, veh_length of the default parameters
OCCUPIED = 80


def covered(boxes, size_x, size_y, resolution, origin, inflate=0.0, veh=VEH):
    """boxes [n][4] = cx, cy, cs, sn -> bool [size_y][size_x]: the cells at least one box covers"""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    resolution, inflate = np.float64(resolution), np.float64(inflate)
    ox, oy = np.float64(origin[0]), np.float64(origin[1])
    X = (ox + np.arange(size_x, dtype=np.float64) * resolution)[None, :]
    Y = (oy + np.arange(size_y, dtype=np.float64) * resolution)[:, None]
    hl = np.float64(0.5) * np.float64(veh[1]) + inflate
    hw = np.float64(0.5) * np.float64(veh[0]) + inflate
    out = np.zeros((size_y, size_x), dtype=bool)
    for cx, cy, cs, sn in boxes:
        if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(cs) and np.isfinite(sn)):
            continue                                            # a box with a member that is not finite covers nothing
        dx, dy = X - cx, Y - cy
        lx = cs * dx + sn * dy
        ly = cs * dy - sn * dx
        out |= (np.abs(lx) <= hl) & (np.abs(ly) <= hw)
    return out


def stamp(cells, boxes, resolution, origin, inflate=0.0, veh=VEH):
    """the working map after the boxes were stamped into `cells` (uint8 [size_y][size_x], not changed): covered cells become 80"""
    cells = np.asarray(cells, dtype=np.uint8)
    out = cells.copy()
    out[covered(boxes, cells.shape[1], cells.shape[0], resolution, origin, inflate, veh)] = OCCUPIED
    return out


def slot_boxes(poses, select=None):
    """the boxes of the slot form: poses [K][slots][4] as oracle_conflict.pyconflict.poses gives them in order 2 (NaN rows for empty
    slots), select [slots] (0: the slot stamps nothing) or None -> [n][4]"""
    poses = np.asarray(poses, dtype=np.float64)
    if select is not None:
        poses = poses[:, np.asarray(select).reshape(-1) != 0]
    return poses.reshape(-1, 4)


def n_stamped(work, base):
    """the cells that are 80 in the working map and not 80 in the base"""
    return int(((np.asarray(work) == OCCUPIED) & (np.asarray(base) != OCCUPIED)).sum())


def occupied_cell(x, y, resolution, origin):
    """the cell grid_occupied (footprint.h) names for the point (x, y): coord = round((p - origin) / resolution), halves away from zero"""
    def rnd(v):                                                 # C's round(): v - trunc(v) is exact
        t = np.trunc(v)
        return t + np.sign(v) * (np.abs(v - t) >= 0.5)
    return rnd((np.asarray(x, dtype=np.float64) - origin[0]) / resolution).astype(np.int64), \
        rnd((np.asarray(y, dtype=np.float64) - origin[1]) / resolution).astype(np.int64)
