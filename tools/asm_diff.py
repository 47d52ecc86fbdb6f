#!/usr/bin/env python3
"""Compare the kernels of two sets of gfx950 assembly files (hipcc ... --cuda-device-only -S).

    tools/asm_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]
    tools/asm_diff.py OLD_DIR NEW_DIR

Two directories (`make -C fia-kdd-19_amd/csrc asm OBJDIR=<dir>` of two trees writes <dir>/asm) are
compared unit by unit, a summary line per unit; a unit only one side has counts as a difference.

Per kernel, keyed by its demangled name: the instruction text from the kernel's label to its
.amdhsa_kernel block (comments dropped, the function number of local labels normalised) and the
.amdhsa_ resource lines.  Prints the kernels only one side has and the ones that differ; exit
status 1 if any kernel present on both sides differs.
"""
import os
import re
import subprocess
import sys


def kernels(paths):
    out = {}
    for path in paths.split(","):
        lines = open(path).read().split("\n")
        names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", l))]
        plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        for name, key in zip(names, plain):
            start = lines.index(next(l for l in lines if l.startswith(name + ":")))
            desc = next(i for i in range(start, len(lines)) if lines[i].strip() == ".amdhsa_kernel " + name)
            end = next(i for i in range(desc, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            text = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[start + 1:desc]]
            text = [l for l in text if l.strip() and not l.strip().startswith((".section", ".p2align"))]
            out[key] = (text, [l.strip() for l in lines[desc + 1:end]])
    return out


def compare(old_paths, new_paths, unit=""):
    old, new = kernels(old_paths), kernels(new_paths)
    only = sorted(set(old) ^ set(new))
    for k in only:
        print("only in old:" if k in old else "only in new:", k)
    both = sorted(set(old) & set(new))
    bad = 0
    for k in both:
        (ot, orr), (nt, nr) = old[k], new[k]
        if ot != nt or orr != nr:
            bad += 1
            print("DIFFERS:", k)
            for a, b in zip(orr, nr):
                if a != b:
                    print("   ", a, "->", b)
            if ot != nt:
                print("    instruction text: %d -> %d lines" % (len(ot), len(nt)))
    print("%s%d kernels on both sides, %d identical, %d differ" % (unit, len(both), len(both) - bad, bad))
    return bad, len(only)


def main():
    a, b = sys.argv[1], sys.argv[2]
    if not (os.path.isdir(a) and os.path.isdir(b)):
        return 1 if compare(a, b)[0] else 0
    units = [sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (a, b)]
    status = 0
    for f in sorted(set(units[0]) ^ set(units[1])):
        print("%s: only in %s" % (f, a if f in units[0] else b))
        status = 1
    for f in sorted(set(units[0]) & set(units[1])):
        bad, only = compare(os.path.join(a, f), os.path.join(b, f), f + ": ")
        status |= 1 if bad or only else 0
    return status


if __name__ == "__main__":
    sys.exit(main())
