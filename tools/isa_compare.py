#!/usr/bin/env python3
"""Per-kernel comparison of two `hipcc --cuda-device-only -S` listings (tools/build_asm.sh), as profiles/*_isa.txt record it.
usage: isa_compare.py parent.s branch.s [substring of a demangled kernel name ...] [--lines]
A row per kernel the filter names (without a filter: per kernel whose text differs): tools/kernel_resources.py's columns
vgpr/accum_offset/sgpr/lds/scratch/occupancy on both sides, the instruction counts, the differing lines with the label numbers blanked and
the same with the register names blanked too; then the opcodes whose count changes; --lines prints the differing lines themselves."""
import collections
import difflib
import re
import subprocess
import sys


def kernels(path):
    """name -> (resource row, instruction lines) of every kernel in the listing"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"^[ \t]*\.amdhsa_kernel (\S+)(.*?)^[ \t]*\.end_amdhsa_kernel", text, re.S | re.M):
        get = lambda k: (re.search(r"\.amdhsa_%s (\S+)" % k, m.group(2)) or [None, "?"])[1]
        res[m.group(1)] = [get("next_free_vgpr"), get("accum_offset"), get("next_free_sgpr"), get("group_segment_fixed_size"),
                           get("private_segment_fixed_size"), "?"]
    out, name, body = {}, None, []
    for line in text.split("\n"):
        m = re.match(r"(\S+):\s*; @(\S+)", line)
        if m and m.group(2) in res:
            name, body = m.group(2), []
            continue
        if name is None:
            continue
        m = re.match(r"; Occupancy: (\d+)", line)
        if m:
            res[name][5] = m.group(1)
            out[name] = ("/".join(res[name]), body)
            name = None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t))
    return out


def blank(lines):
    return [re.sub(r"\b[vsa]\d+\b|\b[vsa]\[\d+:\d+\]", "R", l) for l in lines]


def changed(a, b):
    return [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))]


def main():
    args = [a for a in sys.argv[1:] if a != "--lines"]
    pa, br, keys = kernels(args[0]), kernels(args[1]), args[2:]
    names = sorted(set(pa) | set(br))
    nice = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    short = lambda n: re.sub(r"^void ", "", nice[n].replace("(anonymous namespace)::", "").split("(")[0])
    same, rows = 0, []
    for n in names:
        if n not in pa or n not in br:
            print("only in the %s: %s" % ("parent" if n in pa else "branch", short(n)))
            continue
        if pa[n] == br[n]:
            same += 1
        if (any(k in nice[n] for k in keys) if keys else pa[n] != br[n]):
            rows.append(n)
    print("%-46s %-26s %-26s %6s %6s %6s %6s" % ("kernel", "parent v/a0/s/lds/scr/occ", "branch", "insts", "insts", "lines", "noreg"))
    for n in rows:
        (ra, a), (rb, b) = pa[n], br[n]
        print("%-46s %-26s %-26s %6d %6d %6d %6d" % (short(n), ra, rb, len(a), len(b), len(changed(a, b)), len(changed(blank(a), blank(b)))))
    print("\nresource columns equal in all %d rows: %s;  kernels of identical text: %d of %d" %
          (len(rows), "yes" if all(pa[n][0] == br[n][0] for n in rows) else "NO", same, len(names)))
    print("\nOpcodes whose count changes (branch - parent):")
    for n in rows:
        oa, ob = (collections.Counter(l.split()[0] for l in x[n][1]) for x in (pa, br))
        print("  %-46s %s" % (short(n), "  ".join("%s %+d" % (k, ob[k] - oa[k]) for k in sorted(set(oa) | set(ob)) if oa[k] != ob[k]) or "none"))
    if "--lines" in sys.argv:
        for n in rows:
            d = changed(pa[n][1], br[n][1])
            if d:
                print("\n%s\n  %s" % (short(n), "\n  ".join(d)))


main()
