#!/usr/bin/env python3
"""Register / LDS / spill table of every kernel in a `hipcc --cuda-device-only -S` listing (what decides waves per SIMD).
usage: kernel_resources.py file.s [substring ...]        (tools/build_asm.sh writes /tmp/isa/so3proj.s)"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def main():
    text = open(sys.argv[1]).read()
    keys = sys.argv[2:]
    rows = []
    for m in re.finditer(r"^[ \t]*\.amdhsa_kernel (\S+)(.*?)^[ \t]*\.end_amdhsa_kernel", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        get = lambda k: (re.search(r"\.amdhsa_%s (\S+)" % k, body) or [None, "?"])[1]
        rows.append([name, get("next_free_vgpr"), get("accum_offset"), get("next_free_sgpr"), get("group_segment_fixed_size"), get("private_segment_fixed_size")])
    # the comment block after each function has the spill counts: one pass over the lines (a lazy multi-line pattern is quadratic on
    # the library's 16 MB listing)
    spills, current, info = {}, None, {}
    for line in text.split("\n"):
        m = re.match(r"(\S+):\s*; @(\S+)", line)
        if m:
            current, info = m.group(2), {}
            continue
        m = re.match(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", line)
        if m and current is not None:
            info[m.group(1)] = m.group(2)
            if m.group(1) == "Occupancy":
                spills[current] = (info.get("ScratchSize", "?"), info["Occupancy"], info.get("NumVgprs", "?"), info.get("NumAgprs", "?"))
    dm = demangle([r[0] for r in rows])
    print("%-6s %-6s %-6s %-7s %-8s %-4s  kernel" % ("vgpr", "agpr0", "sgpr", "lds", "scratch", "occ"))
    for r in rows:
        nice = dm.get(r[0], r[0])
        if keys and not any(k in nice for k in keys):
            continue
        sp = spills.get(r[0], ("?", "?"))
        print("%-6s %-6s %-6s %-7s %-8s %-4s  %s" % (r[1], r[2], r[3], r[4], r[5], sp[1], nice[:170]))


main()
