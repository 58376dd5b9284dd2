#!/usr/bin/python3
"""Static instruction counts of the loops of every kernel in a `hipcc -S` listing, by class.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S pde_multigrid_amd/csrc/mgx_block3d.hip -o block3.s
    python tools/loop_counts.py block3.s [--kernel SUBSTRING] [--min-barriers 1]

A loop is the stretch of the listing from the target of a backward branch to that branch (the compiler lays a loop's blocks out in
one piece).  Printed per loop: its labels, the barriers in it (= plane iterations per trip) and the instructions per class:
scalar (s_* other than waits, nops, barriers and branches), vector ALU (v_*), vector memory (buffer_* / global_* / flat_* /
scratch_*), LDS (ds_*), branches, waits.  The kernel's VGPR / SGPR / scratch figures come from its .amdhsa block.
"""
import argparse
import collections
import re


def classify(op):
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--kernel", default="")
    ap.add_argument("--min-barriers", type=int, default=1)
    args = ap.parse_args()
    lines = open(args.listing).read().split("\n")
    name, body, kernels = None, [], []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            kernels.append((name, body))
            name = None
            continue
        body.append(ln)
    meta = collections.defaultdict(dict)
    cur = None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size)\s+(\d+)", ln)
        if m and cur:
            meta[cur][m.group(1)] = int(m.group(2))
    for name, body in kernels:
        if args.kernel not in name:
            continue
        insts, labels = [], {}
        for ln in body:
            s = ln.split(";")[0].strip()
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                labels[m.group(1)] = len(insts)
                continue
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            insts.append(s)
        print("%s\n  %s, %d instructions" % (name, meta.get(name, {}), len(insts)))
        for i, s in enumerate(insts):
            op = s.split()[0]
            if classify(op) != "branch":
                continue
            tgt = s.split()[-1]
            if tgt in labels and labels[tgt] <= i:
                c = collections.Counter(classify(x.split()[0]) for x in insts[labels[tgt]:i + 1])
                if c["barrier"] >= args.min_barriers:
                    waits = [x for x in insts[labels[tgt]:i + 1] if x.startswith("s_waitcnt") and "vmcnt" in x]
                    print("  loop %s..%d: %s; vmcnt waits: %s" % (tgt, i, dict(sorted(c.items())), waits))


if __name__ == "__main__":
    main()
