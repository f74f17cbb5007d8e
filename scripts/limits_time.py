"""Device time of the kinematic-limits check (dftpav_batch_check_limits, limits.hip) on 4096 trajectories of BASELINE configs[3],
beside the time of what it replaces on the host's side: dftpav_batch_sample_states (the kernel's events) plus the copy of its
64 B per sample back to the host (wall time of the call minus the kernel).  Best of 3 after a warm-up, the kernels' own HIP events.

    python scripts/limits_time.py [--batch 4096] [--check-dt 0.05]

Prints one JSON line.  Its figures are quoted in docs/NEXT_ROWS.md 4.17 only."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from dftpav_amd import capi, scenarios as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--check-dt", type=float, default=0.05)
    a = ap.parse_args()
    p = capi.default_params()
    s = sc.baseline_config(4, B=a.batch)       # configs[3]: 16 pieces forward, 4096 trajectories
    s.apply_resolution(p)
    h = capi.Handle(p)
    bt = capi.Batch(h, s.layout, s.B)
    bt.upload(s)
    bt.solve()
    lim = capi.default_limits(p)
    _, dts = bt.coeffs()
    n_samples = int(np.ceil(float(np.max(np.sum(dts * s.layout.piece_nums[None, :], axis=1))) / a.check_dt)) + 1
    lim_ms, st_ms, st_wall = [], [], []
    for k in range(4):                          # the first is the warm-up
        r = bt.check_limits(a.check_dt, lim)
        lim_ms.append(h.limits_last_ms())
        t0 = time.perf_counter()
        bt.sample_states(0.0, a.check_dt, n_samples, filter_singularity=False)
        st_wall.append(1e3 * (time.perf_counter() - t0))
        st_ms.append(h.corridor_last_ms())
    print(json.dumps(dict(batch=s.B, check_dt=a.check_dt, n_samples=n_samples, infeasible=int((r["feasible"] == 0).sum()),
                          limits_kernel_ms=min(lim_ms[1:]), sample_states_kernel_ms=min(st_ms[1:]),
                          sample_states_call_ms=min(st_wall[1:]), sample_states_bytes=int(s.B) * n_samples * 64)))
    bt.close()
    h.close()


if __name__ == "__main__":
    main()
