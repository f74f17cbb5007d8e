"""Developer script: in-kernel phase breakdown of the solve kernel (shader clocks of thread 0)."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dftpav_amd import capi, scenarios as sc

NAMES = ["E1 rhs", "E2 coeffs", "E3+E4 samples", "E4 reduce", "E5 adjoint", "E6 assemble", "line search misc",
         "history update", "two-loop", "x (experiments)", "init", "misc (experiments)"]
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
p = capi.default_params()
s = sc.baseline_config(cfg, B=B); s.apply_resolution(p)
h = capi.Handle(p); h.set_surround(s.surround)
bt = capi.Batch(h, s.layout, B); bt.upload(s)
if os.environ.get("ORDER") == "ref":   # the reference-order kernel (solver_ref.hip): slots 0..8 as its Prof says
    bt.set_order(capi.ORDER_REFERENCE)
bt.solve_async(); bt.sync()
ms0 = []
for _ in range(3):
    bt.solve_async(); bt.sync(); ms0.append(bt.last_solve_ms())
bt.profile(True)
bt.solve_async(); bt.sync(); ms1 = bt.last_solve_ms()
r = bt.results()
pri = bt.read_profile()
REF = os.environ.get("ORDER") == "ref"
# the QUAD shape (solver_ref4.hip) counts in the upper half of slot 11 the evaluations whose parked-term chain took the slow path (a row
# of the wave had more terms than its LDS pool holds); the lower half is the slot's own figure
slow = (pri[:, 11] >> 32) if REF else np.zeros(len(pri), dtype=np.int64)
# ... and in the upper half of slot 9 the flushes of its list of active terms (q4_eval: flush), each counted by the four rows of the wave.
# SLOT11=flush / emit names what a library built with -DDFTPAV_PROF_FLUSH_CYCLES / -DDFTPAV_PROF_EMIT_CYCLES keeps in slot 11: the cycles of
# the flushes / of the whole emission instead of the emit loop's trips; SLOT11=chain: built with -DDFTPAV_PROF_CHAIN_CYCLES, the cycles
# of "E4 reduce" (the parked-term chains) of the evaluations on the slow path alone
flushes = (pri[:, 9] >> 32) if REF else np.zeros(len(pri), dtype=np.int64)
SLOT11 = os.environ.get("SLOT11", "")
if REF:
    pri[:, 11] &= 0xffffffff
    pri[:, 9] &= 0xffffffff
pr = pri.astype(np.float64)
# the reference-order kernel keeps COUNTS in some slots (solver_ref.hip): slot 9 = active terms (both launch shapes); in the WAVE
# shape slots 10 / 11 = evaluations beyond the LDS window and their terms, in the TEAM shape they are cycles (numbering, the
# window's list).  Counts are kept out of the cycle totals and printed under their own names.
wave_counts = REF and bool((pr[:, 10] <= r["evals"]).all())
count_slots = ([9, 10, 11] if wave_counts else [9]) if REF else []
if REF:
    # slot 10: the TEAM shape's numbering; in a QUAD shape the time between a row's lbfgs_advance and its next evaluation, which it
    # spends masked off while other rows of its wave run their recursion
    quad = not wave_counts and flushes.sum() > 0  # (only a QUAD kernel counts flushes of its list)
    NAMES[9], NAMES[10], NAMES[11] = "(count) active terms", ("between passes, masked wait" if quad else "numbering") if not wave_counts else "(count)", ("list flushes" if SLOT11 == "flush" else "emission" if SLOT11 == "emit" else "E4 reduce, slow path" if SLOT11 == "chain" else "window list") if not wave_counts else "(count)"
cyc = pr.copy()
cyc[:, count_slots] = 0.0
tot = cyc.sum(axis=1)
print("cfg", cfg, "B", B, "kernel ms (no prof)", np.round(ms0, 3), "with prof", round(ms1, 3))
print("iters mean/max", r["iters"].mean(), r["iters"].max(), "evals mean/max", r["evals"].mean(), r["evals"].max(),
      "latency ms p50/max", np.median(r["latency_us"]) / 1e3, r["latency_us"].max() / 1e3)
ghz = tot / (r["latency_us"] * 1e3)
print("shader clock GHz (cycles/latency):", round(float(np.median(ghz)), 3))
ev, it = r["evals"].astype(float), r["iters"].astype(float)
for i, nm in enumerate(NAMES):
    if cyc[:, i].sum() == 0: continue
    per_eval = i < 6 or (REF and i in (10, 11)) or (not REF and i in (9, 11))
    per = cyc[:, i] / (ev if per_eval else it)
    print("%-18s %6.1f%%   %9.0f cycles per %s" % (nm, 100 * cyc[:, i].sum() / tot.sum(), np.median(per), "eval" if per_eval else "iter"))
hs = r["hist_sum"].astype(float)
if REF:
    print("reference order: active terms per evaluation, mean", round(float(pr[:, 9].sum() / ev.sum()), 1))
    if wave_counts:
        big = pr[:, 10].sum()
        print("   evaluations with more terms than the LDS window holds:", round(float(100 * big / ev.sum()), 1), "% of all, with",
              round(float(pr[:, 11].sum() / max(1.0, big)), 1), "active terms on average")
if REF and not wave_counts and flushes.sum() > 0:
    print("QUAD shape: flushes of the list of active terms per evaluation, mean", round(float(flushes.sum() / ev.sum()), 2),
          "-- active terms per flush of a wave (four rows):", round(float(4 * pr[:, 9].sum() / flushes.sum()), 1))
if REF and not wave_counts:
    print("QUAD shape: evaluations on the slow path of the parked-term chain:", int(slow.sum()), "=", round(float(100 * slow.sum() / ev.sum()), 2), "% of all")
if REF and not wave_counts and SLOT11 == "chain":
    # E4 reduce by arm, cycles per evaluation of a row: slot 3 is every evaluation's, slot 11 the slow path's; a pass: all cycle slots
    n_slow, n_fast = float(slow.sum()), float(ev.sum() - slow.sum())
    c_slow, c_all = float(pr[:, 11].sum()), float(pr[:, 3].sum())
    per_slow, per_fast = c_slow / max(1.0, n_slow), (c_all - c_slow) / max(1.0, n_fast)
    per_pass = float((tot.sum() - c_slow) / ev.sum())  # (slot 11 repeats part of slot 3)
    print("QUAD shape: E4 reduce per evaluation, slow path %.0f cycles (%d evaluations), dense chain %.0f cycles (%d); a pass %.0f cycles;"
          " slow share x (slow - dense) / pass = %.2f %%" % (per_slow, n_slow, per_fast, n_fast, per_pass,
                                                              100.0 * n_slow / ev.sum() * (per_slow - per_fast) / per_pass))
print("two-loop cycles per history step (2 per entry per iteration):", round(float(np.median(pr[:, 8] / (2 * hs))), 1),
      " mean depth", round(float((hs / it).mean()), 1))
print("solves/s (kernel)", B / (np.mean(ms0) * 1e-3))
