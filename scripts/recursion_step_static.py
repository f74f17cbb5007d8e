#!/usr/bin/env python3
"""Developer script (no GPU): static instruction counts of the QUAD kernel's history steps, from the compiler's assembly.

  hipcc <the flags of solver_ref4.o> --cuda-device-only -S solver_ref4.hip -o ref4.s
  scripts/recursion_step_static.py ref4.s [kernel symbol substring, default ref4_kernelILb1ELb1E]

One line per stretch of code between the starts of two sequential sums (a sum of 31 / 32 terms = two v_fmac_f64_dpp chains): a run
of equal lines is the unrolled history steps of a block of q4_first_steps / q4_second_steps.  Columns: line of the stretch's first
instruction in the function, all instructions, VALU, chain links, other fp64 arithmetic, DPP moves, instructions that write EXEC,
branches, s_waitcnt, LDS, vector loads, vector stores, other SALU.  Below the table: the runs of consecutive steps that hold no
EXEC write and no branch (the full-block bodies).
"""
import re
import sys

FP64 = ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_fmac_f64", "v_rcp_f64", "v_div_", "v_max_f64", "v_min_f64", "v_ldexp_f64", "v_frexp", "v_cmp")


def instructions(path, sym):
    out, infn = [], False
    for ln in open(path):
        if re.match(r"^[A-Za-z_.$][\w.$]*:", ln):
            if ln.startswith(".Lfunc_end"):
                infn = False
            elif not ln.startswith(".L"):
                infn = sym in ln
            continue
        if not infn:
            continue
        m = re.match(r"^\s+([vs]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|buffer_[a-z0-9_]+|flat_[a-z0-9_]+|scratch_[a-z0-9_]+)\b(.*)", ln)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def classes(op, rest):
    c = {"all": 1}
    if op.startswith("v_"):
        c["valu"] = 1
        if op == "v_fmac_f64_dpp" and "row_newbcast" in rest:
            c["chain"] = 1
        elif op.endswith("_dpp"):
            c["dpp"] = 1
        elif op.startswith(FP64):
            c["fp64"] = 1
        if op.startswith("v_cmpx"):  # (writes EXEC, named or not)
            c["exec"] = 1
    elif op.startswith("s_"):
        dst = rest.split(",")[0].strip()
        if op == "s_waitcnt":
            c["wait"] = 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["br"] = 1
        elif "saveexec" in op or dst.startswith("exec"):
            c["exec"] = 1
        else:
            c["salu"] = 1
    elif op.startswith("ds_"):
        c["lds"] = 1
    elif "load" in op:
        c["vmld"] = 1
    else:
        c["vmst"] = 1
    return c


COLS = ("all", "valu", "chain", "fp64", "dpp", "exec", "br", "wait", "lds", "vmld", "vmst", "salu")


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else "ref4_kernelILb1ELb1E"
    ins = instructions(path, sym)
    starts = [i for i, (op, rest) in enumerate(ins) if op == "v_fmac_f64_dpp" and "row_newbcast:0 " in rest + " "]
    # a sum's second chain also starts with row_newbcast:0: keep the starts that do not follow another chain within six instructions (the second chain of the same sum)
    sums = []
    for i in starts:
        prev = [j for j in range(max(0, i - 6), i) if ins[j][0] == "v_fmac_f64_dpp"]
        if not prev:
            sums.append(i)
    print("%d instructions in %s; %d sequential sums" % (len(ins), sym, len(sums)))
    print("%6s " % "pos" + " ".join("%5s" % c for c in COLS))
    rows = []
    for a, b in zip(sums, sums[1:] + [len(ins)]):
        tot = dict.fromkeys(COLS, 0)
        for op, rest in ins[a:b]:
            for k in classes(op, rest):
                tot[k] += 1
        rows.append((a, tot))
        print("%6d " % a + " ".join("%5d" % tot[c] for c in COLS))
    print("runs of four or more consecutive stretches of fewer than 100 instructions without an EXEC write or a branch (pos, stretches):")
    run = []
    for a, tot in rows + [(None, {"exec": 1, "br": 1, "all": 0})]:
        if a is not None and tot["exec"] == 0 and tot["br"] == 0 and tot["all"] < 100:
            run.append(a)
        else:
            if len(run) >= 4:
                print("  %6d  %d" % (run[0], len(run)))
            run = []


if __name__ == "__main__":
    main()
