#!/usr/bin/env python3
"""Compare the device code of two builds of one translation unit, kernel by kernel.

    hipcc ... --save-temps=obj -c unit.hip -o A/unit.o     (and the same into B/)
    tools/isa_diff.py A/unit-hip-amdgcn-amd-amdhsa-gfx950.s B/unit-hip-amdgcn-amd-amdhsa-gfx950.s

For every function symbol of the two assembly files: "same" when the instruction text between the symbol's label and
its .Lfunc_end is identical once the function-local label numbers (.LBB<n>_<k>, .Lfunc_end<n>, which count the
functions of the file) are normalised, else "DIFFERS"; symbols in one file only are listed as added / removed. The
kernel descriptors' resource figures (.amdhsa_next_free_vgpr and the like) are compared as well. Exit status 1 when a
common symbol differs.
"""
import re
import sys


def functions(path):
    out, desc = {}, {}
    name, body = None, []
    kd = None
    for line in open(path):
        s = line.strip()
        if kd is not None:
            if s.startswith(".end_amdhsa_kernel"):
                kd = None
            elif s.startswith(".amdhsa_"):
                desc[kdname].append(s)
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            kd, kdname = True, m.group(1)
            desc[kdname] = []
            continue
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line.rstrip())
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not s or s.startswith(";") or s.startswith(".p2align") or s.startswith(".loc") or s.startswith(".cfi"):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"\s*;.*$", "", s)
        body.append(s)
    return out, desc


def main():
    a, da = functions(sys.argv[1])
    b, db = functions(sys.argv[2])
    bad = 0
    for n in sorted(set(a) | set(b)):
        if n not in b:
            print("removed  %s" % n)
        elif n not in a:
            print("added    %s (%d instructions)" % (n, len(b[n])))
        elif a[n] == b[n] and da.get(n) == db.get(n):
            print("same     %s (%d instructions)" % (n, len(a[n])))
        else:
            bad = 1
            print("DIFFERS  %s (%d -> %d instructions)" % (n, len(a[n]), len(b[n])))
    return bad


if __name__ == "__main__":
    sys.exit(main())
