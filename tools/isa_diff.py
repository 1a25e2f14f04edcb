#!/usr/bin/env python3
"""Compare the device code of two builds of one translation unit, kernel by kernel.

    hipcc ... --save-temps=obj -c unit.hip -o A/unit.o     (and the same into B/)
    tools/isa_diff.py [--map FILE] [--rename REGEX REPL] [--show] A/unit-hip-amdgcn-amd-amdhsa-gfx950.s B/...gfx950.s

For every function symbol of the two assembly files, comparing the instruction text between the symbol's label and its
.Lfunc_end once the function-local label numbers (.LBB<n>_<k>, .Lfunc_end<n>, which count the functions of the file)
are normalised, and the kernel descriptors' resource figures (.amdhsa_next_free_vgpr and the like):
  same       identical instruction text and resource figures;
  reordered  identical resource figures and the same multiset of normalised instructions, in another order: what moved
             is listed (--show prints the moved lines with their positions), and is for the reader to judge;
  DIFFERS    anything else.
Symbols in one file only are listed as added / removed. Exit status 1 when a common symbol DIFFERS.

A refactor that renames kernels (template arguments are part of the mangled name) says which old symbol became which
new one: --map FILE holds one `old new` pair of symbols per line (# starts a comment), and --rename REGEX REPL
(repeatable, applied in order, re.sub) rewrites the symbols of the first file. References to a renamed symbol inside
the instruction text are rewritten as well.
"""
import argparse
import collections
import difflib
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


def renamer(args):
    pairs = {}
    if args.map:
        for line in open(args.map):
            f = line.split("#")[0].split()
            if len(f) == 2:
                pairs[f[0]] = f[1]
            elif f:
                sys.exit("%s: expected `old new`, got %r" % (args.map, line))
    rules = [(re.compile(r), s) for r, s in args.rename or []]

    def rename(n):
        n = pairs.get(n, n)
        for r, s in rules:
            n = r.sub(s, n)
        return n

    return rename


def apply_rename(funcs, desc, rename):
    names = {n: rename(n) for n in set(funcs) | set(desc)}
    changed = {o: n for o, n in names.items() if o != n}
    if len(set(names.values())) != len(names):
        dup = [n for n, c in collections.Counter(names.values()).items() if c > 1]
        sys.exit("the rename maps several symbols to one: %s" % ", ".join(sorted(dup)))
    if changed:  # a symbol named inside an instruction (a call, a table address)
        pat = re.compile("|".join(sorted(map(re.escape, changed), key=len, reverse=True)))
        fix = lambda body: [pat.sub(lambda m: changed[m.group(0)], s) for s in body]
    else:
        fix = lambda body: body
    return {names[n]: fix(b) for n, b in funcs.items()}, {names[n]: d for n, d in desc.items()}


def moved(a, b):
    """the lines of a and b outside their longest common subsequence, as (tag, position, text)"""
    out = []
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        out += [("-", i, a[i]) for i in range(i1, i2)]
        out += [("+", j, b[j]) for j in range(j1, j2)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--map", help="file of `old new` symbol pairs, applied to the first file")
    ap.add_argument("--rename", nargs=2, action="append", metavar=("REGEX", "REPL"),
                    help="regular-expression rewrite of the first file's symbols (repeatable)")
    ap.add_argument("--show", action="store_true", help="print the moved / differing lines of every kernel not `same`")
    args = ap.parse_args()
    a, da = functions(args.a)
    b, db = functions(args.b)
    a, da = apply_rename(a, da, renamer(args))
    bad = 0
    for n in sorted(set(a) | set(b)):
        if n not in b:
            print("removed  %s" % n)
            continue
        if n not in a:
            print("added    %s (%d instructions)" % (n, len(b[n])))
            continue
        if a[n] == b[n] and da.get(n) == db.get(n):
            print("same     %s (%d instructions)" % (n, len(a[n])))
            continue
        if da.get(n) == db.get(n) and collections.Counter(a[n]) == collections.Counter(b[n]):
            mv = moved(a[n], b[n])
            kinds = collections.Counter(s.split()[0] for t, _, s in mv if t == "+")
            print("reordered %s (%d instructions; moved: %s)"
                  % (n, len(a[n]), ", ".join("%d %s" % (c, k) for k, c in sorted(kinds.items()))))
        else:
            bad = 1
            mv = moved(a[n], b[n])
            print("DIFFERS  %s (%d -> %d instructions%s)"
                  % (n, len(a[n]), len(b[n]), "" if da.get(n) == db.get(n) else "; resource figures differ"))
            if args.show:
                for x, y in zip(da.get(n, []), db.get(n, [])):
                    if x != y:
                        print("    %s -> %s" % (x, y))
        if args.show:
            for t, i, s in mv:
                print("    %s %5d  %s" % (t, i, s))
    return bad


if __name__ == "__main__":
    sys.exit(main())
