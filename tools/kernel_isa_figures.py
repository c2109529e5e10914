#!/usr/bin/env python3
"""What a refactor of a kernel must leave alone when its ISA differs: per kernel of two device
assemblies (see tools/kernel_isa_diff.py for how to make them), side by side, the resource block
that decides occupancy (next-free VGPR / SGPR, accum_offset = where the AGPRs start, LDS and
private segment sizes) and the counts of the instructions that are its memory and matrix traffic
(v_mfma_*, ds_*, global_load* with the LDS-DMA forms, global_store*, s_barrier), then the total
instruction count, which may differ.

    tools/kernel_isa_figures.py parent/X.s this/X.s [--only REGEX]

Exits 1 if any figure but the total differs."""
import argparse
import re
import sys

from kernel_isa_diff import demangle, kernels

RES = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size"]
OPS = ["v_mfma_", "ds_", "global_load", "global_store", "s_barrier"]


def figures(lines):
    f = {}
    for r in RES:
        f[r] = next((ln.split()[-1] for ln in lines if ln.strip().startswith(".amdhsa_" + r + " ")), "?")
    ins = [ln.split()[0] for ln in lines if ln.startswith("\t") and not ln.strip().startswith(".")]
    for o in OPS:
        f[o + "*" if o.endswith("_") or o.startswith("global") else o] = sum(i.startswith(o) for i in ins)
    f["instructions (may differ)"] = len(ins)
    return f


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--only", default=".", help="demangled-name regex of the kernels to compare")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.this)
    names = demangle(sorted(old))
    bad = 0
    for k in sorted(old):
        if not re.search(a.only, names[k]) or k not in new:
            continue
        fo, fn = figures(old[k]), figures(new[k])
        print("== %s" % names[k])
        print("   %-28s %10s %10s" % ("", "parent", "this"))
        for key in fo:
            differs = fo[key] != fn[key] and "may differ" not in key
            bad += differs
            print("   %-28s %10s %10s%s" % (key, fo[key], fn[key], "   DIFFERS" if differs else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
