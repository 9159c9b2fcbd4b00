#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc -S --cuda-device-only) symbol by symbol.

    tools/isa_compare.py before.s after.s [--rename OLD NEW]

For every kernel of `before`: its instruction text, its .amdhsa_kernel block and its register / scratch metadata must be
the same in `after`.  Labels are numbered per translation unit (.LBB<function>_<block>), so the function number is
dropped before comparing (also in the loop comments); --rename replaces a piece of the mangled names of `after` first (a
trailing template argument with a default adds e.g. "Lb0E" to every instance's name without changing its code).  Prints one line per
kernel and the kernels only `after` has; exit status 1 when a kernel of `before` differs or is missing."""
import argparse
import re
import sys


def kernels(path, rename=None):
    text = open(path).read()
    if rename:
        text = text.replace(rename[0], rename[1])
    text = re.sub(r"BB\d+_", "BB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"\.Ltmp\d+", ".Ltmp", text)
    text = re.sub(r"[ \t]+;", " ;", text)  # comment columns move with the width of a label's number
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        out[m.group(1)] = {"hsa": m.group(2)}
    for name, k in out.items():
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        k["code"] = m.group(1) if m else None
        # the metadata entry of the kernel: registers, spills, scratch, LDS
        m = re.search(r"\.name:\s+%s\n(.*?)(?=^\s+- \.a|^amdhsa\.|\Z)" % re.escape(name), text, re.S | re.M)
        meta = m.group(1) if m else ""
        k["meta"] = sorted(l.strip() for l in meta.splitlines()
                           if re.search(r"sgpr_count|vgpr_count|agpr_count|spill_count|segment_fixed_size|kernarg_segment_size", l))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", nargs=2, metavar=("OLD", "NEW"))
    a = ap.parse_args()
    b, c = kernels(a.before), kernels(a.after, a.rename)
    bad = 0
    for name in sorted(b):
        if name not in c:
            print("MISSING  %s" % name)
            bad += 1
            continue
        same = [b[name][k] == c[name][k] and b[name][k] is not None for k in ("code", "hsa", "meta")]
        n = len(b[name]["code"].splitlines()) if b[name]["code"] else 0
        print("%s  %s  (%d lines; text %s, .amdhsa %s, registers %s)"
              % ("same    " if all(same) else "DIFFERS ", name, n, *("same" if s else "DIFFERS" for s in same)))
        bad += not all(same)
    new = sorted(set(c) - set(b))
    for name in new:
        print("new      %s  %s" % (name, " ".join(c[name]["meta"])))
    print("%d kernels before, %d identical, %d new" % (len(b), len(b) - bad, len(new)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
