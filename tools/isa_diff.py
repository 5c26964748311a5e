#!/usr/bin/env python3
"""Compare two ISA dumps of the library (tools/isa_dump.sh -> lsm2d.s), function by function: prints which kernels' texts are identical and which differ.

    python3 tools/isa_diff.py parent/lsm2d.s this_tree/lsm2d.s

A function's text is everything between its `; -- Begin function` and `; -- End function` lines (code, the resource comments behind it, its .amdhsa block);
local labels carry the function's ordinal in the file, which is the same on both sides as long as no kernel is added or removed."""
import re
import sys


def functions(path):
    out, name, buf = {}, None, []
    for line in open(path, errors="replace"):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, buf = m.group(1), []
        elif "; -- End function" in line and name:
            out[name] = "".join(buf)
            name = None
        elif name:
            buf.append(line)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = [n for n in a if n in b and a[n] == b[n]]
    differ = [n for n in a if n in b and a[n] != b[n]]
    print("%d functions on the left, %d on the right; %d identical" % (len(a), len(b), len(same)))
    for n in sorted(set(a) - set(b)):
        print("only left :", n)
    for n in sorted(set(b) - set(a)):
        print("only right:", n)
    for n in differ:
        la, lb = a[n].count("\n"), b[n].count("\n")
        print("DIFFERENT : %s (%d lines against %d)" % (n, la, lb))
    for n in sorted(same):
        print("identical : %s" % n)


if __name__ == "__main__":
    main()
