#!/usr/bin/env python3
"""Vector-issue estimate of one kernel from its gfx950 assembly (no GPU needed).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only -S csrc/ks_step.hip -o ks_step.s
  python tools/ks_issue_count.py ks_step.s 'ks_env_step_kernelIfNS_10FftWave256IfEELb1ELb0ELb0ELb0ELb0E' --trip 30

Splits the kernel into basic blocks at its local labels, classifies every instruction, finds the loops (a branch back to an
earlier label) and prints the instructions one wave issues per launch: straight-line blocks once, the blocks of the loop
that holds the transforms (most lane-exchange instructions) --trip times (the CNAB2 sub-step loop: K = 30 in the shipped configurations), every other loop once per static
instruction (their trip counts are 1 or 2 at the shipped geometry: A = 64, S = 64 over 64 or 128 lanes).

Issue cycles, per wave-instruction (one wave's stream on one SIMD): plain VALU, DPP and v_pk_* 4, permlane swaps 4 (+ the s_nop in
front of them, counted as s_nop: 4 per `s_nop 0` issue slot), transcendental 8.  LDS and global instructions are listed, not priced:
they do not occupy the SIMD's FMA datapath, which is what the f32 MFMA passes compete for.
"""
import argparse
import collections
import re
import sys

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def classify(op, line):
    if op.startswith("v_permlane"):
        return "permlane"
    if op.startswith("v_pk_"):
        return "valu_pk"
    if op.startswith("v_"):
        if op.startswith(TRANS):
            return "valu_trans"
        if "_dpp" in op or " row_" in line or "quad_perm" in line:
            return "valu_dpp"
        if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
            return "valu_lane"
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_barrier"):
        return "s_barrier"
    if op.startswith(("s_cbranch", "s_branch")):
        return "s_branch"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return "other"


VECTOR = ("valu", "valu_pk", "valu_dpp", "valu_trans", "valu_lane", "permlane")
CYCLES = {"valu": 4, "valu_pk": 4, "valu_dpp": 4, "valu_lane": 4, "permlane": 4, "valu_trans": 8}


def kernel_body(text, needle):
    """lines between the kernel's entry label and its .Lfunc_end"""
    lines = text.splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^\w+:", l) and needle in l.split(":")[0]]
    if len(starts) != 1:
        sys.exit(f"{len(starts)} kernels match {needle!r}: " + ", ".join(lines[i][:120] for i in starts[:6]))
    out = []
    for l in lines[starts[0] + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        out.append(l)
    return lines[starts[0]].split(":")[0], out


def blocks_of(body):
    blocks, cur = [["entry", []]], None
    for l in body:
        s = l.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            blocks.append([m.group(1), []])
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        blocks[-1][1].append(s)
    return blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the mangled kernel name (must match one kernel)")
    ap.add_argument("--trip", type=int, default=30, help="trip count of the largest loop (the sub-step loop)")
    ap.add_argument("--blocks", action="store_true", help="print the per-block table")
    a = ap.parse_args()
    name, body = kernel_body(open(a.asm).read(), a.kernel)
    blocks = blocks_of(body)
    index = {b[0]: i for i, b in enumerate(blocks)}
    counts = []
    loops = []
    for i, (label, ins) in enumerate(blocks):
        c = collections.Counter()
        for s in ins:
            op = s.split()[0]
            k = classify(op, s)
            if k == "s_nop":      # s_nop n occupies n + 1 issue slots
                c["s_nop_slots"] += int(s.split()[1], 0) + 1
            c[k] += 1
            if k == "s_branch":
                t = s.split()[-1]
                if t in index and index[t] <= i:
                    loops.append((index[t], i))
        counts.append(c)
    vec = lambda c: sum(c[k] for k in VECTOR)
    size = lambda lp: sum(vec(counts[i]) for i in range(lp[0], lp[1] + 1))
    # the sub-step loop is the loop that holds the transforms: most lane-exchange instructions, then fewest blocks
    xch = lambda lp: sum(counts[i]["permlane"] + counts[i]["valu_dpp"] for i in range(lp[0], lp[1] + 1))
    main_loop = max(loops, key=lambda lp: (xch(lp), lp[0] - lp[1])) if loops else None
    weight = [1] * len(blocks)
    if main_loop:
        for i in range(main_loop[0], main_loop[1] + 1):
            weight[i] = a.trip
    if a.blocks:
        for i, (label, _) in enumerate(blocks):
            print(f"{label:12s} x{weight[i]:<3d} " + " ".join(f"{k}={v}" for k, v in sorted(counts[i].items())))
    tot, loop_c, rest_c = collections.Counter(), collections.Counter(), collections.Counter()
    for i, c in enumerate(counts):
        for k, v in c.items():
            tot[k] += v * weight[i]
            (loop_c if weight[i] > 1 else rest_c)[k] += v
    print(name)
    if main_loop:
        print("sub-step loop:", blocks[main_loop[0]][0], "..", blocks[main_loop[1]][0])
    if main_loop:
        print(f"sub-step loop body, one trip: " + " ".join(f"{k}={v}" for k, v in sorted(loop_c.items())))
    print("outside it, static:           " + " ".join(f"{k}={v}" for k, v in sorted(rest_c.items())))
    print(f"per launch (loop x{a.trip}):        " + " ".join(f"{k}={v}" for k, v in sorted(tot.items())))
    nvec = vec(tot)
    cyc = sum(tot[k] * CYCLES[k] for k in VECTOR)
    nop = 4 * tot["s_nop_slots"]
    print(f"vector instructions per wave and launch: {nvec}  (loop trip: {vec(loop_c)})")
    print(f"vector issue cycles: {cyc}  + s_nop slots {nop}  = {cyc + nop}  "
          f"({(cyc + nop) / 2400.0:.2f} us at 2.4 GHz)")


if __name__ == "__main__":
    main()
