"""Device time of the rendered map (dftpav_grid_render, render.hip) on the default arena: 36 polygons on 1500 x 1500 cells of 0.2 m.
render_ms is the handle's own HIP events (dftpav_render_last_ms: the kernels, without the copy of the obstacle set), render_call_ms
the wall clock of the whole call, each the best of 3 after a warm-up.  Beside them, what a caller pays for the same map today, on
the same box: scenarios.fill_polygons (numpy, one core) and the dftpav_set_grid_map of the result, each the best of 3.  The device's
bytes must equal fill_polygons'.

    python scripts/render_time.py

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.25 only."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, scenarios as sc  # noqa: E402


def main():
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "default_map.npz"))
    size_x, size_y, res = int(z["map_meta"][0]), int(z["map_meta"][1]), float(z["map_meta"][2])
    origin = capi.origin_centred(z["ego_init"][0], z["ego_init"][1], size_y * res, size_x * res)
    h = capi.Handle(capi.default_params())
    render_ms, call_ms = [], []
    for _ in range(4):                                          # the first is the warm-up
        t = time.perf_counter()
        h.render_map(size_x, size_y, res, origin, 127, z["poly_xy"], z["poly_off"])
        call_ms.append(1e3 * (time.perf_counter() - t))
        render_ms.append(h.render_last_ms())
    got, _ = h.read_cells()
    fill_s, upload_s = [], []
    for _ in range(3):
        t = time.perf_counter()
        want = sc.fill_polygons(np.full((size_y, size_x), 127, dtype=np.uint8), origin, res, z["poly_xy"], z["poly_off"])
        fill_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        h.set_grid_map(want, res, origin)
        upload_s.append(time.perf_counter() - t)
    same = bool(np.array_equal(got, want))
    print(json.dumps(dict(cells=[size_x, size_y], polygons=len(z["poly_off"]) - 1, vertices=int(z["poly_off"][-1]), cells_set=int((got == 80).sum()),
                          render_ms=min(render_ms[1:]), render_call_ms=min(call_ms[1:]), host_fill_polygons_s=min(fill_s),
                          host_set_grid_map_s=min(upload_s), equal_to_fill_polygons=same)))
    h.close()
    assert same


if __name__ == "__main__":
    main()
