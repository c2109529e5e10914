#!/usr/bin/env python3
"""Are the kernels of two device assemblies the same code?

    hipcc <the Makefile's CXXFLAGS_HIP> --cuda-device-only -S csrc/X.hip -o X.s     (once per commit)
    tools/kernel_isa_diff.py parent/X.s this/X.s [--only REGEX]

Per kernel (a .amdhsa_kernel symbol): everything from its label to its .Lfunc_end, which is its
instructions and its .amdhsa_kernel block (registers, LDS, scratch), compared as text after the parts that depend on where
a function stands in the file are made anonymous: local labels (.LBB12_3 -> .LBB_3, .Ltmp, .Lfunc_end)
and comment lines.  Prints one line per kernel of the first file -- same / DIFFERS / missing --, the
kernels only the second file has, and exits 1 if a kernel of the first file differs or is missing."""
import argparse
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.M | re.S)
        lines = []
        for ln in body.group(1).splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.L(tmp|func_end|func_begin)\d+", r".L\1", ln)
            lines.append(ln)
        out[name] = lines
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--only", default=".", help="demangled-name regex of the kernels to compare")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.this)
    names = demangle(sorted(set(old) | set(new)))
    bad = 0
    for k in sorted(old):
        if not re.search(a.only, names[k]):
            continue
        if k not in new:
            verdict = "missing"
        elif old[k] == new[k]:
            verdict = "same (%d lines)" % len(old[k])
        else:
            verdict = "DIFFERS"
        bad += verdict != "same (%d lines)" % len(old[k])
        print("%-10s %s" % (verdict.split()[0], names[k]) + ("  " + verdict.split(" ", 1)[1] if " " in verdict else ""))
    for k in sorted(set(new) - set(old)):
        print("%-10s %s" % ("new", names[k]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
